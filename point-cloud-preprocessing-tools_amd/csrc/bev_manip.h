/*
 * bev_manip.h — the float max-height BEV of the older tools for a batch of frames, under per-frame poses
 * (bev_float_bev_device_resident, bev_float_bev_batch): k_float_bev's raster (bev_misc.h) behind k_transform's
 * arithmetic, one launch for all frames and poses.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_MANIP_H
#define BEV_MANIP_H

#include "bev_misc.h"

namespace bevk {
using namespace bevx;

/* One point that has its cell (or -1) into one grid; every lane of the wave calls it.  Consecutive points of a row-major
 * sweep share cells, so a lane leaves its atomic out when the next lane of the wave has the same cell and a height that is no
 * lower: chains of covered lanes run upwards and end at a lane that is not covered, which carries their maximum.  Against
 * one atomic per point this took 11-13 % off the kernel's time. */
__device__ __forceinline__ void float_bev_put(uint32_t *__restrict__ grid, int cell, float h)
{
    const int up_cell = __shfl_down(cell, 1);
    const float up_h = __shfl_down(h, 1);
    if ((threadIdx.x & 63u) != 63u && up_cell == cell && up_h >= h) cell = -1;
    if (cell >= 0) atomicMax(&grid[cell], __float_as_uint(h));
}

/* A map over packed frames (packed_place, load_packed_records; bev_dev.h): the label is loaded only where it is tested.
 * Then, per pose k of the frame (a uniform loop; the matrices are read at uniform addresses), k_transform's association
 * (transform_xyz, bev_exact.h) and k_float_bev's raster into grid f * max(1, n_poses) + k.  n_poses == 0: the raw coordinates
 * (NOT an identity pose: 0 * inf is NaN, -0.0 + 0.0 is +0.0). */
__global__ __launch_bounds__(256) void k_float_bev_batch(const bev_point_t *__restrict__ clouds,
                                                         const ProjFrame *__restrict__ tab, int nf,
                                                         const Affine34 *__restrict__ poses, int n_poses, float interval, int M,
                                                         int skip_label0, uint32_t *__restrict__ grids)
{
    const PackedPlace pl = packed_place(tab, nf, blockIdx.x);
    const uint32_t n = pl.n, k0 = pl.k0;
    float4 a[kProjPerThread];
    int label[kProjPerThread];
    load_packed_records(clouds + pl.off, n, k0, skip_label0 != 0, 1, a, label);
    const size_t cells = (size_t)M * (size_t)M;
    uint32_t *__restrict__ grid = grids + (size_t)pl.f * (size_t)(n_poses > 0 ? n_poses : 1) * cells;
    if (n_poses == 0) {
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) {
            float h;
            int cell = float_bev_cell(a[j].x, a[j].y, a[j].z, label[j], interval, M, skip_label0, h);
            if (k0 + (uint32_t)j * 256u >= n) cell = -1;
            float_bev_put(grid, cell, h);
        }
        return;
    }
    const Affine34 *__restrict__ pose = poses + (size_t)pl.f * (size_t)n_poses;
    for (int p = 0; p < n_poses; ++p, grid += cells) {
        const Affine34 m = pose[p];
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) {
            float tx, ty, tz, h;
            transform_xyz(m.m, a[j].x, a[j].y, a[j].z, tx, ty, tz);
            int cell = float_bev_cell(tx, ty, tz, label[j], interval, M, skip_label0, h);
            if (k0 + (uint32_t)j * 256u >= n) cell = -1;
            float_bev_put(grid, cell, h);
        }
    }
}

} /* namespace bevk */

#endif /* BEV_MANIP_H */
