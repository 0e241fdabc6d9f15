/*
 * bev_submap_reg_plan.h — the host plan of a scan-to-map registration call (bev_submap_registration_device_resident,
 * bev_submap_registration_batch): which frames get a voxel cloud, which voxel clouds under which matrices
 * make which map's target, which maps share a launch group and which matches run against them.  Plain C++, no HIP:
 * bev_capi_submap_reg.hip builds and uploads the plan, tests/submapregcheck builds it and checks its invariants.
 *
 *   slots    the distinct frames that a match's query or a used map's entry names, in the order of first appearance (the
 *            matches in their order, a match's query before its map's entries): one voxel cloud each;
 *   maps     the maps that a match names ("used"), ascending by map index; a map that no match names costs nothing.  A
 *            map's entries stay IN MAP ORDER (the index of a target point is its position in the concatenation, and ties
 *            of the search go to the lowest index), each with its slot and its matrix; its capacity is the sum of its
 *            entries' record counts, an upper bound of its voxel count (which only the device knows);
 *   groups   consecutive used maps whose workspace (map_bytes of each) fits the cap; a map above the cap is a group alone.
 *            A map's points lie at pt0 of the group's point arrays, its header and cell offsets at its index in the group;
 *   problems the matches of a group's maps, ascending by map and among equal maps in the order of the call; match m's
 *            result lands at index m whatever the grouping.
 * bev_submap_plan.h sorts a group's entries by frame (its rasters are order-free) and is not used here.
 *
 * A call is described by one Call (the frame table, the maps, the matches) and its Options:
 *
 * union_voxel: the maps are thinned by a second voxel grid over their union (bev_submap_vox.h), so a map also
 * owns its sort keys at key0 of the group's key array (bev_submap_vox_plan.h pads them), its voxel starts and the thinned
 * points, and map_bytes counts them.  all_maps: every map of the call is used, whatever the matches name
 * (bev_submap_voxel_cloud_device_resident has none).
 *
 * point_normal: the call is bev_submap_coarse_registration_device_resident's: the frames are PointNormal clouds
 * of `stride` rows each (frames.n[f] = stride, frames.off unused), a map's capacity is n_entries * stride rows and its bytes are
 * map_coarse_bytes; the caller makes two problems (the guesses) of every Problem.  Everything else is as above; with the
 * default Options every call plans exactly as before.
 *
 * point_normal with union_voxel: the PointNormal maps are thinned over their union and their normals recomputed
 * (bev_submap_pn_vox.h): a map owns its sort keys as under union_voxel, and its bytes are map_coarse_union_bytes.  With all_maps
 * as well: bev_submap_pn_cloud_device_resident.  Every other combination plans exactly as before.
 *
 * top_union, with point_normal and union_voxel: the call is bev_submap_top_part_coarse_registration_device_resident's
 * or, with all_maps, bev_submap_top_part_cloud_device_resident's: the frames are FULL clouds (frames.off, frames.n as in a fine
 * call), and a map is the top part over the union of its moved full clouds (bev_submap_top.h), thinned as above.  A map then has
 * two sizes: map_union_cap, the records of its union (the sum of its entries' record counts), whose keys lie at map_u0 of the
 * group's union keys; and map_cap, top_max_out of that: the rows its top part can have, which is what pt0, the sort keys and
 * everything of §6q are counted in.  An entry's pad words carry its first index in the union and its record count.  A map's
 * bytes are map_top_union_bytes.  Without top_union nothing of this is computed and every plan is what it was.
 *
 * grid_cap (bev_set_submap_search_grid): 0: a map's search grid is the one-workgroup build's, at most 128 x 128
 * (fine) or 64 x 64 (PointNormal) cells whose offsets lie at the map's index in the group, and every plan is what it was.
 * 1 .. kGridCapMax: the grid is built by bev_submap_grid.h with grid_dim(n, grid_cap) cells per axis, n the map's point count,
 * which only the device knows; grid_dim is monotone in n, so grid_cells(capacity, grid_cap) bounds a map's cells.  A map then
 * owns grid_cells + 1 offsets and as many counters at map_cell0 of the group's two arrays (a prefix inside its group), and the
 * byte models count them, with the build's partial bounds and sums, in place of the fixed grid.
 */
#ifndef BEV_SUBMAP_REG_PLAN_H
#define BEV_SUBMAP_REG_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/bev_mi355x.h" /* bev_match_t */
#include "bev_submap_vox_plan.h"

#if defined(__HIPCC__)
#define BEV_PLAN_HD __host__ __device__
#else
#define BEV_PLAN_HD
#endif

namespace bevsubreg {

/* ---- the size of a search grid (bev_reg_common.h's rule, here once for the host plan and for bev_submap_grid.h) ---- */
constexpr int kGridCapMax = 1024; /* the largest settable cap of cells per axis */
/* cells per axis of the grid of a target of n points (searchable or not) under the cap D >= 1 */
BEV_PLAN_HD inline int grid_dim(uint32_t n, int D)
{
    const int r = (int)ceilf(sqrtf((float)n));
    return r < 1 ? 1 : r > D ? D : r;
}
/* cells a target of at most cap points can have: grid_dim is monotone in n */
inline uint64_t grid_cells(uint64_t cap, int D)
{
    const uint64_t d = (uint64_t)grid_dim((uint32_t)std::min<uint64_t>(cap, 0xffffffffull), D);
    return d * d;
}
/* bev_submap_grid.h's partial results per map: kGridParts bounds of four floats, kGridScanParts sums of cell counts */
constexpr uint32_t kGridParts = 256, kGridScanTile = 4096;
constexpr uint32_t kGridScanParts = (uint32_t)kGridCapMax * kGridCapMax / kGridScanTile;
constexpr uint32_t kGridPartBytes = kGridParts * 16 + kGridScanParts * 4;
/* device bytes of a map's search grid besides its points: D == 0: the offsets of fixed_cells cells; else the offsets and the
 * counters of grid_cells(cap, D) cells and the partial results */
inline uint64_t grid_bytes(uint64_t cap, int D, uint32_t fixed_cells)
{
    return D == 0 ? (uint64_t)(fixed_cells + 1) * 4 : (grid_cells(cap, D) + 1) * 8 + kGridPartBytes;
}

constexpr uint32_t kGridCells = 128 * 128; /* kFineCells (bev_internal.h): cells of a map's search grid */
constexpr uint32_t kCoarseGridCells = 64 * 64; /* kIcpCells: cells of a PointNormal map's search grid */
constexpr uint32_t kCoarseRowBytes = 48 + 16;  /* ... a moved PointNormal row and its searchable copy */
/* ... of a PointNormal map thinned over its union, per row of capacity: the thinned row and its searchable copy,
 * the moved row, a voxel start, a voxel index, a thinned position */
constexpr uint32_t kCoarseUnionRowBytes = kCoarseRowBytes + 48 + 4 + 4 + 16;

/* of a map's top part over its union (bev_internal.h has the device's structures): the cells' counts, ranks,
 * prefixes and thresholds of the radix select and its three counters; its histograms, 64 digits per cell */
constexpr uint32_t kTopCellBytes = 100 * (3 * 4 + 2 * 8) + 16;
constexpr uint32_t kTopHistBytes = 100 * 64 * 4;
constexpr uint64_t kTopMaxUnion = (uint64_t)1 << 24; /* BEV_SUBMAP_TOP_MAX_UNION: the key has 25 bits for a union index */

struct Slot { /* FineSlot's layout (bev_internal.h): k_fine_voxel reads the slots */
    uint64_t off;
    uint32_t n, _pad;
};
struct alignas(64) Entry { /* one aligned 64-byte line per entry, read at a workgroup-uniform address */
    float m[12];   /* row-major 3 x 4 */
    uint32_t slot; /* whose voxel cloud it moves */
    uint32_t pad[3]; /* 0; top_union: its first index in the map's union, its record count, 0 */
};
struct Map {
    uint64_t pt0;         /* its first point in the group's point arrays */
    uint32_t ent0, n_ent; /* its entries: [ent0, ent0 + n_ent) of Plan::entries */
};
struct Problem {
    uint32_t src_slot; /* the query's slot */
    uint32_t map;      /* index into Plan::maps */
    uint32_t result;   /* the match's index in the call */
    uint32_t _pad;
};
static_assert(sizeof(Slot) == 16 && sizeof(Entry) == 64 && sizeof(Map) == 16 && sizeof(Problem) == 16, "the device reads these layouts");

struct Group {
    uint32_t map0 = 0, n_maps = 0;   /* [map0, map0 + n_maps) of Plan::maps */
    uint32_t prob0 = 0, n_probs = 0; /* [prob0, prob0 + n_probs) of Plan::probs */
    uint64_t pts = 0;                /* points its maps can hold together */
    uint64_t max_cap = 0;            /* the largest map_cap among its maps: it sizes the launches over a map's points */
    uint64_t bytes = 0;              /* sum of map_bytes over its maps */
    uint64_t keys = 0;               /* union_voxel: sort keys of its maps together (bevsubvox::key_slots of each) */
    uint64_t max_slots = 0;          /* union_voxel: the largest key array among its maps: it sizes the sort's launches */
    uint64_t union_pts = 0;          /* top_union: records of its maps' unions together */
    uint64_t max_union = 0;          /* top_union: the largest union among its maps: it sizes the select's launches */
    uint64_t cells = 0;              /* grid_cap > 0: grid_cells + 1 of its maps together */
    uint64_t max_cells = 0;          /* grid_cap > 0: the largest grid_cells among its maps: it sizes the scan's launches */
};
struct Plan {
    std::vector<Slot> slots;
    std::vector<int32_t> slot_frame; /* the call's frame index of a slot */
    std::vector<Entry> entries;
    std::vector<Map> maps;
    std::vector<int32_t> map_id;     /* the call's map index of a used map */
    std::vector<uint64_t> map_cap;   /* points a used map can hold */
    std::vector<uint64_t> map_key0;  /* union_voxel: a used map's first key in its group's key array */
    std::vector<Problem> probs;
    std::vector<Group> groups;
    size_t Pn = 1;                   /* the largest record count of a slot (at least 1) */
    uint64_t max_group_pts = 0;
    uint32_t max_group_maps = 0;
    uint64_t max_group_keys = 0;     /* union_voxel */
    std::vector<uint64_t> map_union_cap; /* top_union: records of a used map's union (map_cap: rows of its top part) */
    std::vector<uint64_t> map_u0;        /* top_union: a used map's first key in its group's union keys */
    uint64_t max_group_union = 0;        /* top_union */
    std::vector<uint64_t> map_cell0;     /* grid_cap > 0: a used map's first word in its group's offsets and counters */
    uint64_t max_group_cells = 0;        /* grid_cap > 0 */
};

/* what the union grid adds to a map that can hold cap points: the thinned points (16 bytes each), the padded sort keys
 * (8 bytes each), the voxel starts (cap + 1 words), the sort's header (32 bytes) */
inline uint64_t map_union_bytes(uint64_t cap) { return cap * 16 + bevsubvox::key_slots(cap) * 8 + (cap + 1) * 4 + 32; }

/* device bytes of a map that can hold cap points: the moved points and the searchable points by cell (16 bytes each),
 * the search grid (grid_bytes), the header; union_voxel: and map_union_bytes; a wide grid (D > 0) without it: the count's
 * header (32 bytes), since the concatenation is then bev_submap_vox.h's */
inline uint64_t map_bytes(uint64_t cap, bool union_voxel = false, int D = 0)
{
    return cap * 32 + grid_bytes(cap, D, kGridCells) + 32 + (union_voxel ? map_union_bytes(cap) : D ? 32 : 0);
}

/* device bytes of a PointNormal map of cap rows (bev_submap_coarse_registration_device_resident): the moved rows and the
 * searchable points by cell, the search grid (grid_bytes: D == 0, the 64 x 64 grid's cell offsets), the header; a wide grid: the
 * count's header too (the concatenation is then bev_submap_pn_vox.h's) */
inline uint64_t map_coarse_bytes(uint64_t cap, int D = 0)
{
    return cap * kCoarseRowBytes + grid_bytes(cap, D, kCoarseGridCells) + 32 + (D ? 32 : 0);
}

/* device bytes of a PointNormal map of cap rows that is thinned over its union (bev_submap_coarse_voxel_registration_device_resident,
 * bev_submap_pn_cloud_device_resident): kCoarseUnionRowBytes per row, the padded sort keys (8 bytes each), the last voxel start,
 * the search grid (grid_bytes) and its header, the sort's header */
inline uint64_t map_coarse_union_bytes(uint64_t cap, int D = 0)
{
    return cap * kCoarseUnionRowBytes + bevsubvox::key_slots(cap) * 8 + 4 + grid_bytes(cap, D, kCoarseGridCells) + 32 + 32;
}

/* rows the top part of n records can have: bev_regfront_max_out (sum over 100 cells of round(0.2f * n_c) <= n / 5 + 50) */
inline uint64_t top_max_out(uint64_t n) { return n / 5 + 51; }

/* device bytes of a map whose union holds c records and whose target is the thinned top part over it
 * (bev_submap_top_part_coarse_registration_device_resident, bev_submap_top_part_cloud_device_resident): a key per record of the
 * union (the moved records are not kept: a row is moved again from its entry and record), the cells' table and histograms, and
 * what a thinned PointNormal map of top_max_out(c) rows takes, its padded sort keys holding the padded selection first */
inline uint64_t map_top_union_bytes(uint64_t c, int D = 0)
{
    return c * 8 + kTopCellBytes + kTopHistBytes + map_coarse_union_bytes(top_max_out(c), D);
}

/* points the entries of map g can hold together: the sum of their frames' record counts */
inline uint64_t map_capacity(const uint64_t *frame_n, const uint64_t *map_offs, const int32_t *entry_frame, int g)
{
    uint64_t cap = 0;
    for (uint64_t e = map_offs[g]; e < map_offs[g + 1]; ++e) cap += frame_n[entry_frame[e]];
    return cap;
}

/* the frames of a call: frame f = n[f] records at off[f] of the caller's buffer */
struct FrameTable {
    std::vector<uint64_t> off, n;
    int size() const { return (int)n.size(); }
};
/* a call: map g owns entries [map_offs[g], map_offs[g + 1]); entry e names frame entry_frame[e] and the matrix at
 * entry_pose + 12 * e; match m registers frame matches[m].query_idx against map matches[m].match_idx (all indices checked by
 * the caller; the arrays are the caller's and outlive the struct's use) */
struct Call {
    FrameTable frames;
    int n_maps = 0;
    const uint64_t *map_offs = nullptr;
    const int32_t *entry_frame = nullptr;
    const float *entry_pose = nullptr;
    int n_matches = 0;
    const bev_match_t *matches = nullptr;
};
struct Options { /* see the head of the file */
    bool union_voxel = false, all_maps = false, point_normal = false, top_union = false;
    int grid_cap = 0; /* 0 .. kGridCapMax */
};

/* cap_bytes: the group cap */
inline Plan plan_call(const Call &call, const Options &opt, uint64_t cap_bytes)
{
    const int n_frames = call.frames.size(), n_maps = call.n_maps, n_matches = call.n_matches;
    const uint64_t *const frame_off = call.frames.off.data(), *const frame_n = call.frames.n.data(), *const map_offs = call.map_offs;
    const int32_t *const entry_frame = call.entry_frame;
    const bev_match_t *const mt = call.matches;
    Plan p;
    std::vector<int32_t> slot_of((size_t)std::max(n_frames, 0), -1), used((size_t)std::max(n_maps, 0), -1);
    auto slot = [&](int f) -> uint32_t {
        if (slot_of[f] < 0) {
            slot_of[f] = (int32_t)p.slots.size();
            p.slots.push_back(Slot{frame_off[f], (uint32_t)frame_n[f], 0u});
            p.slot_frame.push_back(f);
            p.Pn = std::max(p.Pn, (size_t)frame_n[f]);
        }
        return (uint32_t)slot_of[f];
    };
    /* slots in the order of first appearance; which maps are used */
    for (int m = 0; m < n_matches; ++m) {
        slot(mt[m].query_idx);
        const int g = mt[m].match_idx;
        if (used[g] >= 0) continue;
        used[g] = 0;
        for (uint64_t e = map_offs[g]; e < map_offs[g + 1]; ++e) slot(entry_frame[e]);
    }
    for (int g = 0; opt.all_maps && g < n_maps; ++g) {
        if (used[g] >= 0) continue;
        used[g] = 0;
        for (uint64_t e = map_offs[g]; e < map_offs[g + 1]; ++e) slot(entry_frame[e]);
    }
    /* the used maps, ascending, their entries in map order */
    for (int g = 0; g < n_maps; ++g) {
        if (used[g] < 0) continue;
        used[g] = (int32_t)p.maps.size();
        Map mp{0u, (uint32_t)p.entries.size(), (uint32_t)(map_offs[g + 1] - map_offs[g])};
        uint64_t at = 0;
        for (uint64_t e = map_offs[g]; e < map_offs[g + 1]; ++e) {
            Entry en;
            memcpy(en.m, call.entry_pose + 12 * (size_t)e, sizeof en.m);
            en.slot = (uint32_t)slot_of[entry_frame[e]];
            en.pad[0] = en.pad[1] = en.pad[2] = 0u;
            if (opt.top_union) {
                en.pad[0] = (uint32_t)at;
                en.pad[1] = (uint32_t)frame_n[entry_frame[e]];
                at += frame_n[entry_frame[e]];
            }
            p.entries.push_back(en);
        }
        p.maps.push_back(mp);
        p.map_id.push_back(g);
        const uint64_t cap = map_capacity(frame_n, map_offs, entry_frame, g);
        if (opt.top_union) p.map_union_cap.push_back(cap);
        p.map_cap.push_back(opt.top_union ? top_max_out(cap) : cap);
    }
    /* the problems: by map, the call's order among equal maps */
    std::vector<uint64_t> keys((size_t)std::max(n_matches, 0));
    for (int m = 0; m < n_matches; ++m) keys[(size_t)m] = (uint64_t)(uint32_t)used[mt[m].match_idx] << 32 | (uint32_t)m;
    std::sort(keys.begin(), keys.end());
    for (uint64_t k : keys) {
        const uint32_t m = (uint32_t)k;
        p.probs.push_back(Problem{(uint32_t)slot_of[mt[m].query_idx], (uint32_t)(k >> 32), m, 0u});
    }
    /* the groups */
    p.map_key0.assign(p.maps.size(), 0);
    if (opt.top_union) p.map_u0.assign(p.maps.size(), 0);
    if (opt.grid_cap) p.map_cell0.assign(p.maps.size(), 0);
    size_t pr = 0;
    for (uint32_t u = 0; u < (uint32_t)p.maps.size();) {
        Group g;
        g.map0 = u;
        g.prob0 = (uint32_t)pr;
        while (u < (uint32_t)p.maps.size()) {
            const int D = opt.grid_cap;
            const uint64_t b = opt.top_union      ? map_top_union_bytes(p.map_union_cap[u], D)
                               : !opt.point_normal ? map_bytes(p.map_cap[u], opt.union_voxel, D)
                               : opt.union_voxel ? map_coarse_union_bytes(p.map_cap[u], D)
                                                 : map_coarse_bytes(p.map_cap[u], D);
            if (g.n_maps > 0 && g.bytes + b > cap_bytes) break;
            p.maps[u].pt0 = g.pts;
            if (opt.union_voxel) {
                const uint64_t slots = bevsubvox::key_slots(p.map_cap[u]);
                p.map_key0[u] = g.keys;
                g.keys += slots;
                g.max_slots = std::max(g.max_slots, slots);
            }
            if (opt.top_union) {
                p.map_u0[u] = g.union_pts;
                g.union_pts += p.map_union_cap[u];
                g.max_union = std::max(g.max_union, p.map_union_cap[u]);
            }
            if (D) {
                const uint64_t cells = grid_cells(p.map_cap[u], D);
                p.map_cell0[u] = g.cells;
                g.cells += cells + 1;
                g.max_cells = std::max(g.max_cells, cells);
            }
            g.pts += p.map_cap[u];
            g.max_cap = std::max(g.max_cap, p.map_cap[u]);
            g.bytes += b;
            ++g.n_maps;
            ++u;
        }
        while (pr < p.probs.size() && p.probs[pr].map < u) ++pr;
        g.n_probs = (uint32_t)pr - g.prob0;
        p.max_group_pts = std::max(p.max_group_pts, g.pts);
        p.max_group_maps = std::max(p.max_group_maps, g.n_maps);
        p.max_group_keys = std::max(p.max_group_keys, g.keys);
        p.max_group_union = std::max(p.max_group_union, g.union_pts);
        p.max_group_cells = std::max(p.max_group_cells, g.cells);
        p.groups.push_back(g);
    }
    return p;
}

} /* namespace bevsubreg */

#endif /* BEV_SUBMAP_REG_PLAN_H */
