/*
 * bev_submap_grid.h — a map's search grid sized to the map: the build of reg_grid_build (bev_reg_common.h) by SEVERAL
 * workgroups per map, its cell counts in global memory, so that the grid is not held to the 128 x 128 or 64 x 64 cells whose
 * counts fit one workgroup's LDS (bev_set_submap_search_grid).  The rule is reg_grid_build's with a settable cap:
 * dim = bevsubreg::grid_dim(n, cap) (bev_submap_reg_plan.h), bounds, s, inv_s, nx, ny, mag and n as there.  The target's points
 * and their count come from the stages that exist: k_submap_vox_move or k_submap_vox_finish (fine), k_submap_pn_move or the
 * thinned rows of §6q / §6r (coarse); the count is the map's SubvoxHdr::n_out.  Per launch group of a plan with grid_cap > 0, the
 * map along y and the parts along x as in §6l's sort:
 *   k_subgrid_bounds   per (part, map) : min and max of x and y over the part's finite points (order-free but for the sign of a
 *                                        zero bound, which changes no cell)
 *   k_subgrid_header   per map         : the parts' bounds reduced, the IcpGridHdr by the rule (n: 0 until the scan)
 *   k_subgrid_points   per (part, map) : counting: every finite point adds 1 to its cell's counter (the caller zeroed the
 *                                        counters on the same stream)
 *   k_subgrid_sums     per (tile, map) : the sum of the counts of kTile cells
 *   k_subgrid_scan     per (tile, map) : the sums of the tiles before it, then an exclusive scan of its tile: the offsets, and
 *                                        the counters turned into the cells' cursors; the last tile: offsets[nx * ny], hdr.n
 *   k_subgrid_points   per (part, map) : scattering: every finite point takes a position from its cell's cursor and goes to
 *                                        the searchable points as (x, y, z, index bits)
 * then the ICP loops against such a grid: bev_wide_icp.h.  The pair calls run the same six launches over their target slots
 * (bev_pair_grid.h; §6t): one launcher, launch_subgrid, takes the points as float4, as 32-byte records or as PointNormal rows.
 * The phases meet only through the order of launches on the call's stream: no workgroup waits for another.  The order of the
 * points inside a cell depends on the atomics; icp_nn's result does not (lowest index on equal distance).  No float or double sum
 * depends on an atomic: the integer counts and cursors do.  A map's n is known on the device only: the launch grids are the
 * plan's, and a workgroup beyond its map's points or cells returns at once.  Every workgroup has 256 threads.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_GRID_H
#define BEV_SUBMAP_GRID_H

#include "bev_pair_grid.h" /* PairgridRecs */
#include "bev_submap_reg_plan.h"

namespace bevk {

constexpr uint32_t kGridTile = bevsubreg::kGridScanTile, kGridPer = kGridTile / kRegThreads;
static_assert(kGridTile % kRegThreads == 0 && kSubgridParts == bevsubreg::kGridParts && kSubgridScanParts == bevsubreg::kGridScanParts,
              "the plan counts the partial results");

/* the position of point i of the map whose points begin at pt0: float4 points (fine), 48-byte PointNormal rows (coarse) */
struct SubgridPts {
    const float4 *pts;
    __device__ float3 operator()(uint64_t pt0, uint32_t i) const
    {
        const float4 p = pts[pt0 + i];
        return make_float3(p.x, p.y, p.z);
    }
};
struct SubgridRows {
    const float *rows;
    __device__ float3 operator()(uint64_t pt0, uint32_t i) const
    {
        const float4 p = *reinterpret_cast<const float4 *>(rows + (pt0 + i) * 12);
        return make_float3(p.x, p.y, p.z);
    }
};

__device__ __forceinline__ uint32_t subgrid_cell(const IcpGridHdr &h, float x, float y)
{
    return (uint32_t)(icp_cell(y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(x, h.minx, h.inv_s, h.nx));
}

/* part blockIdx.x of map map0 + blockIdx.y: its points' bounds into w.part_bounds (a part without a finite point: +inf, -inf) */
template <class Fetch>
__global__ __launch_bounds__(kRegThreads) void k_subgrid_bounds(const bevsubreg::Map *maps, uint32_t map0, const SubvoxHdr *vh,
                                                                Fetch fetch, SubmapGridWork w)
{
    __shared__ float red[4][kRegWaves];
    const uint32_t g = blockIdx.y, n = vh[g].n_out;
    const uint64_t pt0 = maps[map0 + g].pt0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (uint32_t i = blockIdx.x * kRegThreads + tid; i < n; i += gridDim.x * kRegThreads) {
        const float3 p = fetch(pt0, i);
        if (!finite3(p.x, p.y, p.z)) continue;
        mnx = fminf(mnx, p.x);
        mny = fminf(mny, p.y);
        mxx = fmaxf(mxx, p.x);
        mxy = fmaxf(mxy, p.y);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        mnx = fminf(mnx, __shfl_xor(mnx, off));
        mny = fminf(mny, __shfl_xor(mny, off));
        mxx = fmaxf(mxx, __shfl_xor(mxx, off));
        mxy = fmaxf(mxy, __shfl_xor(mxy, off));
    }
    if (lane == 0) {
        red[0][wave] = mnx;
        red[1][wave] = mny;
        red[2][wave] = mxx;
        red[3][wave] = mxy;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kRegWaves; ++k) {
            mnx = fminf(mnx, red[0][k]);
            mny = fminf(mny, red[1][k]);
            mxx = fmaxf(mxx, red[2][k]);
            mxy = fmaxf(mxy, red[3][k]);
        }
        w.part_bounds[(size_t)g * kSubgridParts + blockIdx.x] = make_float4(mnx, mny, mxx, mxy);
    }
}

/* map map0 + blockIdx.x (one wave): the parts' bounds reduced, the header by reg_grid_build's rule under the cap */
__global__ __launch_bounds__(64) void k_subgrid_header(const SubvoxHdr *vh, uint32_t parts, int cap, SubmapGridWork w)
{
    const uint32_t g = blockIdx.x, n = vh[g].n_out;
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (uint32_t k = threadIdx.x; k < parts; k += 64) {
        const float4 b = w.part_bounds[(size_t)g * kSubgridParts + k];
        mnx = fminf(mnx, b.x);
        mny = fminf(mny, b.y);
        mxx = fmaxf(mxx, b.z);
        mxy = fmaxf(mxy, b.w);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        mnx = fminf(mnx, __shfl_xor(mnx, off));
        mny = fminf(mny, __shfl_xor(mny, off));
        mxx = fmaxf(mxx, __shfl_xor(mxx, off));
        mxy = fmaxf(mxy, __shfl_xor(mxy, off));
    }
    if (threadIdx.x != 0) return;
    IcpGridHdr h{};
    h.nx = h.ny = 1;
    h.s = 1.0f;
    h.inv_s = 0.0f;
    if (mnx <= mxx) { /* some searchable point */
        h.minx = mnx;
        h.miny = mny;
        h.mag = fmaxf(fmaxf(fabsf(mnx), fabsf(mxx)), fmaxf(fabsf(mny), fabsf(mxy)));
        const float ex = mxx - mnx, ey = mxy - mny;
        const int dim = bevsubreg::grid_dim(n, cap);
        const float s = fmaxf(ex, ey) / (float)dim;
        if (s > 0.0f && isfinite(s) && isfinite(1.0f / s)) {
            h.s = s;
            h.inv_s = 1.0f / s;
            h.nx = min(dim, (int)(ex * h.inv_s) + 1);
            h.ny = min(dim, (int)(ey * h.inv_s) + 1);
        }
    }
    w.hdr[g] = h; /* (n: k_subgrid_scan's last tile) */
}

/* part blockIdx.x of map map0 + blockIdx.y.  scatter false: its finite points counted into their cells' counters; true: each
 * takes a position from its cell's cursor and goes to the searchable points */
template <class Fetch>
__global__ __launch_bounds__(kRegThreads) void k_subgrid_points(const bevsubreg::Map *maps, uint32_t map0, const SubvoxHdr *vh,
                                                                Fetch fetch, SubmapGridWork w, bool scatter)
{
    const uint32_t g = blockIdx.y, n = vh[g].n_out;
    if (blockIdx.x * kRegThreads >= n) return;
    const uint64_t pt0 = maps[map0 + g].pt0;
    const IcpGridHdr h = w.hdr[g];
    uint32_t *cnt = w.cnt + w.cell0[map0 + g];
    float4 *sorted = w.sorted + pt0;
    for (uint32_t i = blockIdx.x * kRegThreads + threadIdx.x; i < n; i += gridDim.x * kRegThreads) {
        const float3 p = fetch(pt0, i);
        if (!finite3(p.x, p.y, p.z)) continue;
        const uint32_t c = subgrid_cell(h, p.x, p.y);
        if (!scatter) {
            atomicAdd(&cnt[c], 1u);
        } else {
            const uint32_t pos = atomicAdd(&cnt[c], 1u);
            sorted[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
        }
    }
}

/* the sum of a thread's kGridPer cells of tile `tile`, cells at and above nc counting 0; v: the counts themselves */
__device__ __forceinline__ uint32_t subgrid_load(const uint32_t *cnt, uint32_t tile, uint32_t nc, uint32_t (&v)[kGridPer])
{
    const uint32_t c0 = tile * kGridTile + threadIdx.x * kGridPer;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kGridPer; ++k) {
        v[k] = c0 + k < nc ? cnt[c0 + k] : 0u;
        sum += v[k];
    }
    return sum;
}

/* tile blockIdx.x of map map0 + blockIdx.y: the sum of its cells' counts into w.part_sum */
__global__ __launch_bounds__(kRegThreads) void k_subgrid_sums(uint32_t map0, SubmapGridWork w)
{
    __shared__ uint32_t wave_sum[kRegWaves];
    const uint32_t g = blockIdx.y;
    const IcpGridHdr h = w.hdr[g];
    const uint32_t nc = (uint32_t)(h.nx * h.ny);
    if (blockIdx.x * kGridTile >= nc) return; /* (workgroup-uniform) */
    uint32_t v[kGridPer];
    uint32_t sum = subgrid_load(w.cnt + w.cell0[map0 + g], blockIdx.x, nc, v);
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < kRegWaves; ++k) s += wave_sum[k];
        w.part_sum[(size_t)g * kSubgridScanParts + blockIdx.x] = s;
    }
}

/* tile blockIdx.x of map map0 + blockIdx.y: the offsets of its cells, their counters set to the offsets (the cursors) */
__global__ __launch_bounds__(kRegThreads) void k_subgrid_scan(uint32_t map0, SubmapGridWork w)
{
    __shared__ uint32_t wave_sum[kRegWaves], wave_before[kRegWaves];
    const uint32_t g = blockIdx.y;
    const IcpGridHdr h = w.hdr[g];
    const uint32_t nc = (uint32_t)(h.nx * h.ny);
    if (blockIdx.x * kGridTile >= nc) return; /* (workgroup-uniform) */
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *cnt = w.cnt + w.cell0[map0 + g], *off = w.off + w.cell0[map0 + g];
    /* the cells before the tile: at most kSubgridScanParts sums, one per thread */
    uint32_t before = (uint32_t)tid < blockIdx.x ? w.part_sum[(size_t)g * kSubgridScanParts + tid] : 0u;
    for (int o = 32; o >= 1; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 0) wave_before[wave] = before;
    uint32_t v[kGridPer];
    const uint32_t sum = subgrid_load(cnt, blockIdx.x, nc, v);
    uint32_t incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (int k = 0; k < kRegWaves; ++k) run += wave_before[k] + (k < wave ? wave_sum[k] : 0u);
    const uint32_t c0 = blockIdx.x * kGridTile + tid * kGridPer;
#pragma unroll
    for (uint32_t k = 0; k < kGridPer; ++k) {
        if (c0 + k < nc) {
            off[c0 + k] = run;
            cnt[c0 + k] = run;
        }
        run += v[k];
    }
    if (c0 < nc && c0 + kGridPer >= nc) { /* the thread of the last cell */
        off[nc] = run;
        w.hdr[g].n = run;
    }
}

/* ---- launchers ---- */
template <class Fetch>
static void subgrid_launches(const bevsubreg::Map *maps, uint32_t map0, int n_maps, uint32_t parts, uint32_t tiles, int cap,
                             const SubvoxHdr *vh, Fetch fetch, const SubmapGridWork &w, int step, hipStream_t st)
{
    const dim3 pgrid(parts, (uint32_t)n_maps), tgrid(tiles, (uint32_t)n_maps), block(kRegThreads);
    switch (step) {
    case 0: hipLaunchKernelGGL(k_subgrid_bounds<Fetch>, pgrid, block, 0, st, maps, map0, vh, fetch, w); break;
    case 1: hipLaunchKernelGGL(k_subgrid_header, dim3((uint32_t)n_maps), dim3(64), 0, st, vh, parts, cap, w); break;
    case 2: hipLaunchKernelGGL(k_subgrid_points<Fetch>, pgrid, block, 0, st, maps, map0, vh, fetch, w, false); break;
    case 3: hipLaunchKernelGGL(k_subgrid_sums, tgrid, block, 0, st, map0, w); break;
    case 4: hipLaunchKernelGGL(k_subgrid_scan, tgrid, block, 0, st, map0, w); break;
    default: hipLaunchKernelGGL(k_subgrid_points<Fetch>, pgrid, block, 0, st, maps, map0, vh, fetch, w, true); break;
    }
}

void launch_subgrid(int step, const void *maps, uint32_t map0, int n_maps, uint32_t parts, uint32_t tiles, int cap,
                    const SubvoxHdr *vh, const SubgridSource &src, const SubmapGridWork &w, hipStream_t st)
{
    if (n_maps <= 0) return;
    parts = std::min(std::max(parts, 1u), kSubgridParts);
    tiles = std::min(std::max(tiles, 1u), kSubgridScanParts);
    const bevsubreg::Map *mp = static_cast<const bevsubreg::Map *>(maps);
    if (src.pts) subgrid_launches(mp, map0, n_maps, parts, tiles, cap, vh, SubgridPts{src.pts}, w, step, st);
    else if (src.recs) subgrid_launches(mp, map0, n_maps, parts, tiles, cap, vh, PairgridRecs{src.recs}, w, step, st);
    else subgrid_launches(mp, map0, n_maps, parts, tiles, cap, vh, SubgridRows{src.rows}, w, step, st);
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_GRID_H */
