/*
 * bev_pair_grid_plan.h — the host's byte model and build groups of the pair calls' search grids sized to the cloud
 * (bev_set_pair_search_grid; bev_pair_grid.h).  Plain C++, no HIP: bev_capi_reg.hip lays its workspace out by it,
 * tests/pairgridcheck checks it against a restatement.  The rule of a grid's size is bevsubreg::grid_dim (bev_submap_reg_plan.h)
 * and is not restated here.
 *
 * A pair call has `slots` clouds of one uniform capacity (Pn records in the fine stage, stride rows in the coarse one), of which
 * the first `targets` are the ones some match names as a target (the fine stage numbers its slots that way under a cap; every
 * slot of the coarse stage is a target).  With the cap D:
 *   D == 0   nothing of this exists: every size is 0, and a slot keeps the fixed grid's offsets in the stage's own piece;
 *   D >= 1   a target owns grid_cells(capacity, D) + 1 offset words at its slot * (cells + 1): no base table.  The counters
 *            and the build's partial bounds and sums (kGridPartBytes per slot, 5 KiB) exist for ONE build group of at most
 *            kBuildGroup targets: the groups are built one behind the other on the stream in front of the ICP launches, and a
 *            group's counters are dead once it has scattered.  The point counts (a SubvoxHdr each) and the tables that
 *            k_subgrid_* read (a Map and a first-counter word per target) exist for every target.
 * kBuildGroup = 256 = kFineVoxelGroup: the voxel stage already holds sort keys and voxel starts for 256 slots, 8 Kn + 4 (Pn + 1)
 * bytes each, and cells <= ceil(sqrt(Pn))^2 < Pn + 2 sqrt(Pn) + 1, so a group's counters stay below half of that scratch; 256
 * targets of 2048-point parts fill the device's 256 CUs even for clouds of one part.  Without groups a call on 1000 HDL_64E
 * sweeps would carry 0.5 GB of dead counters; with them 0.13 GB at most.
 */
#ifndef BEV_PAIR_GRID_PLAN_H
#define BEV_PAIR_GRID_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "bev_submap_reg_plan.h"

namespace bevpair {

constexpr int kGridCapMax = bevsubreg::kGridCapMax; /* BEV_PAIR_SEARCH_GRID_MAX */
constexpr uint32_t kBuildGroup = 256;               /* targets whose grids are built together */
constexpr uint32_t kPartPoints = 2048;              /* points of a target that one workgroup of the build takes */
constexpr uint32_t kHdrBytes = 32, kMapBytes = 16, kCell0Bytes = 8; /* SubvoxHdr, bevsubreg::Map, a first-counter word */

struct Layout {
    uint64_t cells = 0;      /* the cells a target's offsets have room for */
    uint64_t off_words = 0;  /* offset words of one target: cells + 1 */
    uint32_t group = 0;      /* targets of a build group at most */
    /* device bytes, all 0 at D == 0 */
    uint64_t off_bytes = 0;    /* every target's offsets */
    uint64_t cnt_bytes = 0;    /* one group's counters */
    uint64_t bounds_bytes = 0; /* one group's partial bounds */
    uint64_t sums_bytes = 0;   /* one group's tile sums */
    uint64_t hdr_bytes = 0;    /* every target's point count */
    /* bytes of the upload table, 0 at D == 0 */
    uint64_t map_bytes = 0, cell0_bytes = 0;
    uint32_t parts = 0, tiles = 0; /* workgroups over a target's points and over its cells */
};

inline Layout layout(uint64_t targets, uint64_t capacity, int D)
{
    Layout l;
    if (D <= 0 || targets == 0) return l;
    l.cells = bevsubreg::grid_cells(capacity, D);
    l.off_words = l.cells + 1;
    l.group = (uint32_t)std::min<uint64_t>(targets, kBuildGroup);
    l.off_bytes = targets * l.off_words * 4;
    l.cnt_bytes = (uint64_t)l.group * l.off_words * 4;
    l.bounds_bytes = (uint64_t)l.group * bevsubreg::kGridParts * 16;
    l.sums_bytes = (uint64_t)l.group * bevsubreg::kGridScanParts * 4;
    l.hdr_bytes = targets * kHdrBytes;
    l.map_bytes = targets * kMapBytes;
    l.cell0_bytes = targets * kCell0Bytes;
    l.parts = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((capacity + kPartPoints - 1) / kPartPoints, 1), bevsubreg::kGridParts);
    l.tiles = (uint32_t)((l.cells + bevsubreg::kGridScanTile - 1) / bevsubreg::kGridScanTile);
    return l;
}

/* the first counter word of target t inside its build group */
inline uint64_t cell0(uint64_t t, const Layout &l) { return (t % l.group) * l.off_words; }

struct Group {
    uint32_t t0, n; /* targets [t0, t0 + n) */
};
inline std::vector<Group> groups(uint64_t targets, const Layout &l)
{
    std::vector<Group> g;
    for (uint64_t t = 0; l.group && t < targets; t += l.group)
        g.push_back(Group{(uint32_t)t, (uint32_t)std::min<uint64_t>(l.group, targets - t)});
    return g;
}

} /* namespace bevpair */

#endif /* BEV_PAIR_GRID_PLAN_H */
