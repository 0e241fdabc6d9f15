/*
 * bev_submap_plan.h — the host plan of a submap call (bev_submap_bev_device_resident, bev_submap_bev_batch):
 * which (frame, pose) entry goes into which grid of which launch group; and the packed-frame table of a call without maps
 * (frame_table), whose rows a group's rows are.  Plain C++, no HIP: the C ABI files build and upload the plan (TablesUp,
 * bev_packed_host.h), tests/submapcheck builds it, runs it on the host and checks its invariants.
 *
 * A call is cut into launch groups of at most `cap` consecutive maps; a map is a grid of its group.  Per group:
 *   rows     the distinct frames that have entries in the group's maps, ascending by frame index, as a packed-frame table
 *            (offset, count, workgroups of kBlockPoints points before the row; a closing row carries the group's workgroups);
 *   ent0     per row the first of its entries in the group's entry list (a closing value ends the last row's);
 *   entries  64 bytes each: the row-major 3 x 4 matrix and the grid (the map's index in the group) the moved points go into.
 * A frame that feeds maps of several groups has a row in each of them, with that group's entries only; a frame without
 * entries in a group has no row there and costs no workgroup.
 */
#ifndef BEV_SUBMAP_PLAN_H
#define BEV_SUBMAP_PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bevsub {

constexpr uint32_t kBlockPoints = 1024; /* points per workgroup of k_submap_splat (kProjBlock, bev_internal.h) */

struct Frame { /* ProjFrame's layout (bev_internal.h): packed_place reads the rows */
    uint64_t off;
    uint32_t n, blk0;
};
struct alignas(64) Entry { /* one aligned 64-byte line per entry: the splat reads it at a wave-uniform address */
    float m[12];
    uint32_t grid;
    uint32_t pad[3];
};
static_assert(sizeof(Frame) == 16 && sizeof(Entry) == 64, "the device reads these layouts");

/* The packed-frame table of nf frames, frame f = records [offs[f], offs[f + 1]) (offsets checked by the caller), in
 * rows[0 .. nf]: per frame its offset, its count and the workgroups before it, row nf closing the table with the workgroups of
 * a launch over all frames (*blocks) at offs[nf]; *n_max: the longest frame.  false: more workgroups than a launch can have
 * (2^31 - 1), the rows then unfinished. */
inline bool frame_table(Frame *rows, int nf, const uint64_t *offs, uint32_t *n_max, uint32_t *blocks)
{
    uint64_t b = 0;
    uint32_t m = 0;
    for (int f = 0; f < nf; ++f) {
        const uint32_t n = (uint32_t)(offs[f + 1] - offs[f]);
        rows[f] = Frame{offs[f], n, (uint32_t)b};
        b += ((uint64_t)n + kBlockPoints - 1u) / kBlockPoints; /* (in 64 bits: a count near 2^32 must not wrap to no workgroup) */
        m = std::max(m, n);
        if (b > 0x7fffffffull) return false;
    }
    rows[nf] = Frame{offs[nf], 0u, (uint32_t)b};
    *n_max = m;
    *blocks = (uint32_t)b;
    return true;
}

struct Group {
    int map0 = 0, n_maps = 0; /* maps [map0, map0 + n_maps) of the call: grids 0 .. n_maps - 1 */
    size_t row0 = 0;          /* its n_rows + 1 rows: [row0, row0 + n_rows] of Plan::rows, ::ent0 and ::frame */
    int n_rows = 0;
    size_t ent_at = 0, n_entries = 0; /* its entries: [ent_at, ent_at + n_entries) of Plan::entries; ent0 counts from ent_at */
    uint32_t blocks = 0;              /* workgroups of the splat over all its rows */
};
struct Plan {
    std::vector<Group> groups;
    std::vector<Frame> rows;
    std::vector<uint32_t> ent0;
    std::vector<int32_t> frame; /* the call's frame index of a row (-1 in a closing row) */
    std::vector<Entry> entries;
};

/* Appends the groups of maps [g0, g1) to the plan: frame f = records [offs[f], offs[f + 1]); map g owns entries
 * [map_offs[g], map_offs[g + 1]); entry e names frame entry_frame[e] (checked by the caller) and the matrix at
 * entry_pose + 12 * e.  false: a group would have more workgroups than a launch can (2^31). */
inline bool plan_maps(Plan &p, const uint64_t *offs, const uint64_t *map_offs, int g0, int g1, const int32_t *entry_frame,
                      const float *entry_pose, size_t cap)
{
    std::vector<uint64_t> keys; /* frame << 32 | entry - the group's first: sorted, a frame's entries lie together */
    std::vector<uint32_t> grid;
    const int step = (int)std::min<size_t>(std::max<size_t>(cap, 1), 0x7fffffffu);
    for (int m0 = g0; m0 < g1; m0 += std::min(step, g1 - m0)) {
        Group g;
        g.map0 = m0;
        g.n_maps = std::min(step, g1 - m0);
        g.row0 = p.rows.size();
        g.ent_at = p.entries.size();
        const uint64_t e_first = map_offs[m0];
        g.n_entries = (size_t)(map_offs[m0 + g.n_maps] - e_first);
        keys.resize(g.n_entries);
        grid.resize(g.n_entries);
        for (int m = m0; m < m0 + g.n_maps; ++m)
            for (uint64_t e = map_offs[m]; e < map_offs[m + 1]; ++e) {
                keys[(size_t)(e - e_first)] = (uint64_t)(uint32_t)entry_frame[e] << 32 | (e - e_first);
                grid[(size_t)(e - e_first)] = (uint32_t)(m - m0);
            }
        std::sort(keys.begin(), keys.end());
        uint64_t blocks = 0;
        p.entries.resize(g.ent_at + g.n_entries);
        for (size_t i = 0; i < g.n_entries; ++i) {
            const uint32_t f = (uint32_t)(keys[i] >> 32), rel = (uint32_t)keys[i];
            if (i == 0 || f != (uint32_t)(keys[i - 1] >> 32)) { /* a new row */
                const uint32_t n = (uint32_t)(offs[f + 1] - offs[f]);
                p.rows.push_back(Frame{offs[f], n, (uint32_t)blocks});
                p.ent0.push_back((uint32_t)i);
                p.frame.push_back((int32_t)f);
                blocks += (n + kBlockPoints - 1u) / kBlockPoints;
                if (blocks > 0x7fffffffull) return false;
            }
            Entry &en = p.entries[g.ent_at + i];
            memcpy(en.m, entry_pose + 12 * (size_t)(e_first + rel), sizeof en.m);
            en.grid = grid[rel];
            en.pad[0] = en.pad[1] = en.pad[2] = 0u;
        }
        g.n_rows = (int)(p.rows.size() - g.row0);
        g.blocks = (uint32_t)blocks;
        p.rows.push_back(Frame{0u, 0u, g.blocks}); /* the closing row */
        p.ent0.push_back((uint32_t)g.n_entries);
        p.frame.push_back(-1);
        p.groups.push_back(g);
    }
    return true;
}

/* Where a group's tables lie in the one block that goes up: rows, then ent0, then — from the next multiple of 64 — the
 * entries; the next group follows at `end` (a multiple of 64 when `at` is one). */
struct GroupBytes {
    size_t rows, ent0, entries, end;
};
inline GroupBytes group_bytes(const Group &g, size_t at)
{
    GroupBytes b;
    b.rows = at;
    b.ent0 = b.rows + ((size_t)g.n_rows + 1) * sizeof(Frame);
    b.entries = (b.ent0 + ((size_t)g.n_rows + 1) * sizeof(uint32_t) + 63) / 64 * 64;
    b.end = b.entries + g.n_entries * sizeof(Entry);
    return b;
}
/* The bytes of the block; dst != nullptr (64-byte aligned): written there, the gaps zeroed. */
inline size_t pack(const Plan &p, char *dst)
{
    size_t at = 0;
    for (const Group &g : p.groups) {
        const GroupBytes b = group_bytes(g, at);
        if (dst) {
            memset(dst + b.rows, 0, b.entries - b.rows);
            memcpy(dst + b.rows, p.rows.data() + g.row0, ((size_t)g.n_rows + 1) * sizeof(Frame));
            memcpy(dst + b.ent0, p.ent0.data() + g.row0, ((size_t)g.n_rows + 1) * sizeof(uint32_t));
            if (g.n_entries) memcpy(dst + b.entries, p.entries.data() + g.ent_at, g.n_entries * sizeof(Entry));
        }
        at = b.end;
    }
    return at;
}

} /* namespace bevsub */

#endif /* BEV_SUBMAP_PLAN_H */
