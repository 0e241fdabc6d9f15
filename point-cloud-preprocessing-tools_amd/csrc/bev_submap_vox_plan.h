/*
 * bev_submap_vox_plan.h — the sort of a map's union voxel grid (bev_submap_vox.h): the tile size, the padding of
 * a map's key array, the list of launches that sorts the keys of every map of a launch group, and the index rules of one
 * compare-exchange.  Plain C++, no HIP (the two index rules are also compiled for the device, where the kernels use them):
 * bev_capi_submap_reg.hip walks the schedule and launches it, tests/submapvoxcheck executes it sequentially on the host.
 *
 * The sort is the ascending bitonic network over np2 keys, np2 the smallest power of two >= a map's point count (known on the
 * device only), the keys behind the points padded with ~0:
 *   for k = 2, 4 .. np2:  for j = k / 2, k / 4 .. 1:  every pair (i, i | j) with i & j == 0 is put in ascending order when
 *   i & k == 0 and in descending order otherwise.
 * A workgroup holds kTile keys in LDS.  The stages (k, j) with k <= kTile touch one tile each: ONE launch sorts every tile
 * (kStageTile).  For k > kTile the stages with j >= kTile pair keys of different tiles: one launch each over global memory
 * (kStageGlobal); the stages j = kTile / 2 .. 1 of that k touch one tile each again: one launch (kStageMerge).  The schedule is
 * that of the largest key array of the launch group; a workgroup whose stage has k above its own map's np2, or whose tile
 * starts at or above it, returns at once.  The keys are distinct (the low word is the point's index), so the sorted order is the
 * one ascending order and nothing depends on the launch geometry.
 */
#ifndef BEV_SUBMAP_VOX_PLAN_H
#define BEV_SUBMAP_VOX_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define BEVSUBVOX_HD __host__ __device__
#else
#define BEVSUBVOX_HD
#endif

namespace bevsubvox {

constexpr uint32_t kTile = 4096;  /* keys a workgroup sorts in LDS: 32 KiB, five workgroups of 256 threads per CU */
constexpr uint64_t kPadKey = ~0ull;

inline uint64_t pow2_at_least(uint64_t n)
{
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

/* keys of the array of a map that can hold cap points: the smallest power of two >= cap (none for an empty map) */
inline uint64_t key_slots(uint64_t cap) { return cap ? pow2_at_least(cap) : 0; }
/* workgroups along x of every launch of the schedule of `slots` keys */
inline uint32_t tiles(uint64_t slots) { return (uint32_t)((slots + kTile - 1) / kTile); }

enum : uint32_t { kStageTile = 0, kStageGlobal = 1, kStageMerge = 2 };
struct Stage {
    uint32_t kind;
    uint32_t k, j; /* kStageTile: every (k, j) with k <= min(kTile, np2) (k, j here: 0); kStageGlobal: the stage (k, j);
                    * kStageMerge: the stages (k, kTile / 2) .. (k, 1) */
};

/* the launches that sort key arrays of up to `slots` keys (a power of two, or 0) */
inline std::vector<Stage> schedule(uint64_t slots)
{
    std::vector<Stage> s;
    if (slots < 2) return s;
    s.push_back(Stage{kStageTile, 0u, 0u});
    for (uint64_t k = 2 * (uint64_t)kTile; k <= slots; k <<= 1) {
        for (uint64_t j = k >> 1; j >= kTile; j >>= 1) s.push_back(Stage{kStageGlobal, (uint32_t)k, (uint32_t)j});
        s.push_back(Stage{kStageMerge, (uint32_t)k, kTile >> 1});
    }
    return s;
}

/* the lower index of pair p (0 .. np2 / 2 - 1) of a stage with distance j; its partner is that | j */
BEVSUBVOX_HD inline uint32_t pair_low(uint32_t p, uint32_t j) { return ((p & ~(j - 1u)) << 1) | (p & (j - 1u)); }
/* keys a at index i and b at i | j of step k: exchange them? */
BEVSUBVOX_HD inline bool exchange(uint64_t a, uint64_t b, uint32_t i, uint32_t k) { return (a > b) == ((i & k) == 0u); }

/* ---- the same launches on the host, workgroup by workgroup (tests/submapvoxcheck) ---------------------------------------- */
/* one tile in "LDS": the stages (k, j) for j = j_first .. 1; base: the tile's first index in the array */
inline void host_tile_steps(uint64_t *tile, uint32_t len, uint32_t base, uint32_t k, uint32_t j_first)
{
    for (uint32_t j = j_first; j > 0; j >>= 1)
        for (uint32_t p = 0; p < len / 2; ++p) {
            const uint32_t lo = pair_low(p, j), hi = lo | j;
            if (exchange(tile[lo], tile[hi], base + lo, k)) std::swap(tile[lo], tile[hi]);
        }
}

/* one launch of the schedule on a map's key array of np2 keys (np2: a power of two or 0; the array holds at least np2);
 * grid_tiles: workgroups along x (the launch group's, at least tiles(np2)) */
inline void host_run_stage(const Stage &st, uint64_t *keys, uint32_t np2, uint32_t grid_tiles)
{
    for (uint32_t b = 0; b < grid_tiles; ++b) {
        const uint64_t base = (uint64_t)b * kTile;
        if (base >= np2) continue; /* beyond the map's own power of two */
        const uint32_t len = std::min(kTile, np2);
        if (st.kind == kStageTile) {
            for (uint32_t k = 2; k <= len; k <<= 1) host_tile_steps(keys + base, len, (uint32_t)base, k, k >> 1);
        } else if (st.k > np2) {
            continue;
        } else if (st.kind == kStageMerge) {
            host_tile_steps(keys + base, len, (uint32_t)base, st.k, kTile >> 1);
        } else {
            for (uint32_t q = 0; q < kTile / 2; ++q) {
                const uint32_t lo = pair_low((uint32_t)(base / 2) + q, st.j), hi = lo | st.j;
                if (exchange(keys[lo], keys[hi], lo, st.k)) std::swap(keys[lo], keys[hi]);
            }
        }
    }
}

} /* namespace bevsubvox */

#endif /* BEV_SUBMAP_VOX_PLAN_H */
