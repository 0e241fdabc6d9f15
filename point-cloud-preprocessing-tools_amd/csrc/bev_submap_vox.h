/*
 * bev_submap_vox.h — a voxel grid over the UNION of a map's moved voxel clouds, between the concatenation of bev_submap_reg.h
 * and its ICP (bev_submap_voxel_registration_device_resident, bev_submap_voxel_registration_batch,
 * bev_submap_voxel_cloud_device_resident):
 *   target(g) = bev_voxel_grid_irct(concat(g), map_leaf), of which x, y, z exist here.
 * Per launch group of the plan (bev_submap_reg_plan.h with union_voxel), the sort as bev_submap_vox_plan.h schedules it:
 *   k_submap_vox_move    per map         : submap_move (bev_submap_reg.h): concat(g) into the moved array, its count
 *   k_submap_vox_keys    per map         : rf_voxel_bounds and rf_voxel_keys over the moved points (bev_reg_common.h): the
 *                                          union's bounds, div and overflow test, the keys voxel index << 32 | concatenation
 *                                          index, padded with ~0 to the map's own power of two
 *   k_submap_vox_tile    per (tile, map) : kTile keys in LDS: all stages with k <= kTile, or the stages j < kTile of one k
 *   k_submap_vox_global  per (tile, map) : one stage (k, j >= kTile) in global memory, kTile / 2 pairs per workgroup
 *   k_submap_vox_finish  per map         : rf_voxel_starts, then rf_voxel_centroids (key order is concatenation order) into
 *                                          the thinned array; the overflow branch copies the moved array; then
 *                                          reg_grid_build over the thinned points
 *   k_submap_out         per (part, map) : the cloud calls, this one's and §6q's: a map's points or PointNormal rows and its
 *                                          count into the caller's arrays
 * then k_submap_icp (bev_submap_reg.h) as it is, its SubmapRegWork pointing at the thinned arrays.
 * A map's point count is known on the device only: the sort's grids are the plan's (the group's largest key array), and a
 * workgroup whose tile starts at or above its map's own power of two, or whose stage has k above it, returns at once.  No float
 * sum depends on an atomic or on which workgroup ran first: a centroid is one lane's loop.  Every workgroup has 256 threads.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_VOX_H
#define BEV_SUBMAP_VOX_H

#include "bev_submap_vox_plan.h"

namespace bevk {

constexpr uint32_t kVoxTile = bevsubvox::kTile;
static_assert(sizeof(SubvoxHdr) == 32, "the plan counts 32 bytes");
static_assert(kVoxTile % (2 * kRegThreads) == 0 && (kVoxTile & (kVoxTile - 1)) == 0, "whole pairs per thread, a power of two");

/* map map0 + blockIdx.x: concat(g) and its count (n_out too: with map_leaf == 0 the moved array is the target) */
__global__ __launch_bounds__(kFineThreads) void k_submap_vox_move(const bevsubreg::Map *maps, uint32_t map0,
                                                                  const bevsubreg::Entry *entries, FineWork w,
                                                                  uint32_t *ent_start, SubmapVoxWork v)
{
    __shared__ uint32_t wave_sum[kRegWaves];
    __shared__ uint32_t s_base;
    const bevsubreg::Map mp = maps[map0 + blockIdx.x];
    const uint32_t n = submap_move(mp, entries, w, ent_start, v.moved + mp.pt0, wave_sum, s_base);
    if (threadIdx.x == 0) {
        SubvoxHdr h{};
        h.n = h.n_out = n;
        v.vh[blockIdx.x] = h;
    }
}

/* map map0 + blockIdx.x: k_fine_voxel's first steps on the moved points (np2 == 0: nothing to sort).  k_submap_pn_keys
 * (bev_submap_pn_vox.h) has these steps over rows and writes SubvoxHdr::div besides; one body for both cost this kernel 16
 * instructions and measured 1.9 - 3.5 % slower, so each keeps its own */
__global__ __launch_bounds__(kFineThreads) void k_submap_vox_keys(const bevsubreg::Map *maps, uint32_t map0, SubmapVoxWork v,
                                                                  float map_leaf)
{
    __shared__ float red[7 * kRegWaves];
    __shared__ int s_par[8]; /* overflow, nfin, minb xyz, div xyz */
    const int g = (int)blockIdx.x, t = (int)threadIdx.x;
    const uint32_t n = v.vh[g].n;
    const SubregPts fetch{v.moved + maps[map0 + g].pt0};
    const float inv = 1.0f / map_leaf;
    rf_voxel_bounds(n, fetch, inv, red, s_par);
    const uint32_t nf = (uint32_t)s_par[1];
    const bool sort = nf != 0 && !s_par[0];
    const uint32_t np2 = sort ? rf_pow2(n) : 0u;
    if (t == 0) {
        v.vh[g].np2 = np2;
        v.vh[g].nf = nf;
        v.vh[g].overflow = nf != 0 && s_par[0];
    }
    if (sort) rf_voxel_keys(n, np2, fetch, inv, s_par, v.keys + v.key0[map0 + g]);
}

/* the stages (k, j_first) .. (k, 1) on len keys in LDS; base: the tile's first index in the map's array */
__device__ __forceinline__ void subvox_tile_steps(uint64_t *s, uint32_t len, uint32_t base, uint32_t k, uint32_t j_first)
{
    for (uint32_t j = j_first; j > 0; j >>= 1) {
        for (uint32_t p = threadIdx.x; p < len / 2; p += kRegThreads) {
            const uint32_t lo = bevsubvox::pair_low(p, j), hi = lo | j;
            const uint64_t a = s[lo], b = s[hi];
            if (bevsubvox::exchange(a, b, base + lo, k)) {
                s[lo] = b;
                s[hi] = a;
            }
        }
        __syncthreads();
    }
}

/* tile blockIdx.x of map map0 + blockIdx.y.  k_merge == 0: every stage with k <= min(kVoxTile, np2); else the stages
 * j = kVoxTile / 2 .. 1 of step k_merge (> kVoxTile) */
__global__ __launch_bounds__(kFineThreads) void k_submap_vox_tile(uint32_t map0, SubmapVoxWork v, uint32_t k_merge)
{
    __shared__ uint64_t s[kVoxTile];
    const uint32_t g = blockIdx.y, np2 = v.vh[g].np2, base = blockIdx.x * kVoxTile;
    if (base >= np2 || k_merge > np2) return; /* (workgroup-uniform) */
    const uint32_t len = min(kVoxTile, np2);
    uint64_t *keys = v.keys + v.key0[map0 + g] + base;
    for (uint32_t i = threadIdx.x; i < len; i += kRegThreads) s[i] = keys[i];
    __syncthreads();
    if (k_merge == 0) {
        for (uint32_t k = 2; k <= len; k <<= 1) subvox_tile_steps(s, len, base, k, k >> 1);
    } else {
        subvox_tile_steps(s, len, base, k_merge, kVoxTile >> 1);
    }
    for (uint32_t i = threadIdx.x; i < len; i += kRegThreads) keys[i] = s[i];
}

/* the stage (k, j), j >= kVoxTile: pairs blockIdx.x * kVoxTile / 2 .. of map map0 + blockIdx.y (np2 >= k >= 2 * kVoxTile) */
__global__ __launch_bounds__(kFineThreads) void k_submap_vox_global(uint32_t map0, SubmapVoxWork v, uint32_t k, uint32_t j)
{
    const uint32_t g = blockIdx.y, np2 = v.vh[g].np2, p0 = blockIdx.x * (kVoxTile / 2);
    if (k > np2 || p0 >= np2 / 2) return;
    uint64_t *keys = v.keys + v.key0[map0 + g];
#pragma unroll
    for (uint32_t q = 0; q < kVoxTile / 2 / kRegThreads; ++q) {
        const uint32_t lo = bevsubvox::pair_low(p0 + q * kRegThreads + threadIdx.x, j), hi = lo | j;
        const uint64_t a = keys[lo], b = keys[hi];
        if (bevsubvox::exchange(a, b, lo, k)) {
            keys[lo] = b;
            keys[hi] = a;
        }
    }
}

/* map map0 + blockIdx.x: the thinned points t.pts + pt0, their count in vh[g].n_out, and (t.hdr != nullptr) their search
 * grid, whose dimension follows the thinned count */
__global__ __launch_bounds__(kFineThreads) void k_submap_vox_finish(const bevsubreg::Map *maps, uint32_t map0, SubmapVoxWork v,
                                                                    SubmapRegWork t)
{
    __shared__ uint32_t wave_cnt[kRegWaves];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const uint64_t pt0 = maps[map0 + g].pt0;
    const SubvoxHdr h = v.vh[g];
    const float4 *moved = v.moved + pt0;
    float4 *thin = t.pts + pt0;
    uint32_t n_out = 0;
    if (h.nf == 0) {
        /* no finite point: an empty target */
    } else if (h.overflow) { /* PCL: "leaf size is too small": the output is the input, non-finite points in their places */
        for (uint32_t i = tid; i < h.n; i += kRegThreads) thin[i] = moved[i];
        n_out = h.n;
    } else {
        const uint64_t *buf = v.keys + v.key0[map0 + g];
        uint32_t *vstart = v.vstart + pt0 + g; /* (cap + 1 words per map) */
        n_out = rf_voxel_starts(buf, h.nf, wave_cnt, vstart, [](uint32_t, uint32_t) {});
        __syncthreads();
        rf_voxel_centroids(buf, vstart, n_out, [moved](uint32_t i) { return moved[i]; }, thin);
    }
    if (tid == 0) v.vh[g].n_out = n_out;
    __syncthreads();
    if (t.hdr)
        reg_grid_build<kFineCells>(n_out, SubregPts{thin}, t.hdr + g, t.cell_off + (size_t)g * (kFineCells + 1), t.sorted + pt0);
}

/* the cloud calls (K_SUBMAP_VOX_OUT, K_SUBMAP_PN_OUT): map map0 + blockIdx.y's n_out rows of row_f4 float4 (a point: 1, a
 * PointNormal row: 3) from src + pt0 rows to out + (map0 + blockIdx.y) * stride rows, its count */
__global__ __launch_bounds__(kRegThreads) void k_submap_out(const bevsubreg::Map *maps, uint32_t map0, const SubvoxHdr *vh,
                                                            const float4 *src, float4 *out, uint64_t stride, uint32_t *counts,
                                                            uint32_t row_f4)
{
    const uint32_t g = blockIdx.y, n = vh[g].n_out;
    const float4 *from = src + maps[map0 + g].pt0 * row_f4;
    float4 *to = out + (uint64_t)(map0 + g) * stride * row_f4;
    const uint64_t n_f4 = (uint64_t)row_f4 * n, step = (uint64_t)gridDim.x * kRegThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kRegThreads + threadIdx.x; i < n_f4; i += step) to[i] = from[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[map0 + g] = n;
}

void launch_submap_vox_move(const void *maps, uint32_t map0, int n_maps, const void *entries, const FineWork &w,
                            uint32_t *ent_start, const SubmapVoxWork &v, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_vox_move, dim3(n_maps), dim3(kFineThreads), 0, st, static_cast<const bevsubreg::Map *>(maps),
                           map0, static_cast<const bevsubreg::Entry *>(entries), w, ent_start, v);
}

void launch_submap_vox_keys(const void *maps, uint32_t map0, int n_maps, const SubmapVoxWork &v, float map_leaf, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_vox_keys, dim3(n_maps), dim3(kFineThreads), 0, st, static_cast<const bevsubreg::Map *>(maps),
                           map0, v, map_leaf);
}

void launch_submap_vox_stage(uint32_t kind, uint32_t k, uint32_t j, uint32_t map0, int n_maps, uint32_t tiles,
                             const SubmapVoxWork &v, hipStream_t st)
{
    if (n_maps <= 0 || tiles == 0) return;
    const dim3 grid(tiles, (uint32_t)n_maps);
    if (kind == bevsubvox::kStageGlobal)
        hipLaunchKernelGGL(k_submap_vox_global, grid, dim3(kFineThreads), 0, st, map0, v, k, j);
    else
        hipLaunchKernelGGL(k_submap_vox_tile, grid, dim3(kFineThreads), 0, st, map0, v, kind == bevsubvox::kStageTile ? 0u : k);
}

void launch_submap_vox_finish(const void *maps, uint32_t map0, int n_maps, const SubmapVoxWork &v, const SubmapRegWork &t,
                              hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_vox_finish, dim3(n_maps), dim3(kFineThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), map0, v, t);
}

void launch_submap_out(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const SubvoxHdr *vh, const void *src,
                       void *out, uint64_t stride, uint32_t *counts, uint32_t row_f4, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_out, dim3(std::max(parts, 1u), (uint32_t)n_maps), dim3(kRegThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), map0, vh, static_cast<const float4 *>(src),
                           static_cast<float4 *>(out), stride, counts, row_f4);
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_VOX_H */
