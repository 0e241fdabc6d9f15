/*
 * bev_posed.h — the 24-layer occupancy BEV and the uint8 max-height BEV for a batch of frames, each under its own poses
 * (bev_posed_bev_device_resident, bev_posed_bev_batch): what bev_multi_bev / bev_single_bev give for
 * bev_transform_cloud(frame, pose), without the moved cloud ever being written.  Two kernels per launch group:
 *   k_posed_splat   per point and pose: posed_code (bev_exact.h) into two planes of M * M words per grid in a device workspace
 *                   (max heights, 24-bit layer masks), global atomics;
 *   k_posed_expand  per (grid, x-band): the band's rows of both planes into LDS, then store_planes (bev_raster.h), the
 *                   stores of the main raster.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_POSED_H
#define BEV_POSED_H

#include "bev_misc.h"
#include "bev_raster.h"

namespace bevk {
using namespace bevx;

/* One code (or kSkip) into one grid; every lane of the wave calls it.  A grid's two planes in the workspace: [0, M * M) max
 * heights, [M * M, 2 * M * M) layer masks, zeroed before the splat.  Consecutive points of a row-major sweep share cells, so
 * a lane leaves BOTH atomics out when the next lane of the wave has the same cell, the same layer and a height that is no
 * lower (float_bev_put's combine, bev_manip.h): chains of covered lanes end at a lane that is not covered and carries both.
 * Against one atomic pair per point this took 13-17 % off the kernel's time (profiles/posed_bev_combine_ab.txt). */
__device__ __forceinline__ void posed_put(uint32_t *__restrict__ planes, uint32_t cells, int M, uint32_t code)
{
    /* covered: the next lane's code differs in the height bits at most, and its height is no lower (kSkip has bit 31 set, a
     * code never: a skipped neighbour covers nothing) */
    constexpr uint32_t kHeightBits = 255u << 18;
    const uint32_t up = (uint32_t)__shfl_down((int)code, 1);
    if ((threadIdx.x & 63u) != 63u && ((up ^ code) & ~kHeightBits) == 0u && (up & kHeightBits) >= (code & kHeightBits)) code = kSkip;
    if (code == kSkip) return;
    const uint32_t idx = (uint32_t)(code_x(code) * M + code_y(code));
    const uint32_t h = (uint32_t)code_h(code), l = code_layer(code);
    if (h != 0u) atomicMax(&planes[idx], h);                        /* BatchMultiBevGen.cpp:353-355 (the planes start at 0) */
    if (l != kNoLayer) atomicOr(&planes[cells + idx], 1u << l);     /* :289-291 */
}

/* A map over packed frames (packed_place, load_packed_records; bev_dev.h): tab is a piece of the call's table, of which this
 * launch covers the nf frames from tab[0] on, so its first workgroup is the call's workgroup tab[0].blk0.  Of the first half of
 * a record only x, y, z are used (the compiler fetches those 12 bytes: four global_load_dwordx3); a point past the frame's end
 * has label 0: no code.  Then, per pose k of the frame (a uniform loop; the matrices are read at uniform addresses),
 * posed_code into the planes of grid f * max(1, n_poses) + k.  n_poses == 0: the raw coordinates.  No LDS. */
__global__ __launch_bounds__(256) void k_posed_splat(const bev_point_t *__restrict__ clouds, const ProjFrame *__restrict__ tab,
                                                     int nf, const Affine34 *__restrict__ poses, int n_poses,
                                                     RasterParams rp, uint32_t *__restrict__ planes)
{
    const PackedPlace pl = packed_place(tab, nf, blockIdx.x + tab[0].blk0);
    float4 a[kProjPerThread];
    int label[kProjPerThread];
    load_packed_records(clouds + pl.off, pl.n, pl.k0, true, 0, a, label);
    const int M = rp.mat_size;
    const uint32_t cells = (uint32_t)(M * M);
    const int per_frame = n_poses > 0 ? n_poses : 1;
    uint32_t *__restrict__ grid = planes + (size_t)pl.f * (size_t)per_frame * 2u * cells;
    if (n_poses == 0) {
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) posed_put(grid, cells, M, posed_code(a[j].x, a[j].y, a[j].z, label[j], nullptr, rp));
        return;
    }
    const Affine34 *__restrict__ pose = poses + (size_t)pl.f * (size_t)n_poses;
    for (int p = 0; p < n_poses; ++p, grid += 2u * cells) {
        const Affine34 m = pose[p];
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) posed_put(grid, cells, M, posed_code(a[j].x, a[j].y, a[j].z, label[j], m.m, rp));
    }
}

/* One workgroup per (grid, x-band of the images; RasterParams' bands): the band's rows of both planes from the workspace
 * into LDS with 16-byte loads — the layout of raster_body, masks then heights, raster_lds_bytes at most — and out through
 * store_planes with the grid's index as its frame index.  multi / single: nullptr = not wanted. */
__global__ __launch_bounds__(kRasterThreads) void k_posed_expand(const uint32_t *__restrict__ planes, uint8_t *__restrict__ multi,
                                                                 uint8_t *__restrict__ single, RasterParams rp)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_posed[];
    const int M = rp.mat_size, L = rp.n_layers, tid = threadIdx.x;
    const int g = (int)blockIdx.x / rp.bands, band = (int)blockIdx.x - g * rp.bands;
    const int x0 = raster_band_x0(band, rp), band_rows = raster_band_rows(band, rp);
    const int cells = band_rows * M; /* (M is a multiple of 16: whole uint4s, 16-byte aligned on both sides) */
    const size_t plane = (size_t)M * M;
    const uint4 *__restrict__ hsrc = reinterpret_cast<const uint4 *>(planes + (size_t)g * 2 * plane + (size_t)x0 * M);
    const uint4 *__restrict__ msrc = reinterpret_cast<const uint4 *>(planes + (size_t)g * 2 * plane + plane + (size_t)x0 * M);
    uint32_t *mask = lds_posed, *hmax = lds_posed + cells;
    for (int i = tid; i < cells / 4; i += kRasterThreads) {
        const uint4 mv = msrc[i], hv = hsrc[i];
        reinterpret_cast<uint4 *>(mask)[i] = mv;
        reinterpret_cast<uint4 *>(hmax)[i] = hv;
    }
    lds_barrier();
    store_planes(mask, hmax, multi, single, g, x0, band_rows, M, L, tid, kRasterThreads);
}

} /* namespace bevk */

#endif /* BEV_POSED_H */
