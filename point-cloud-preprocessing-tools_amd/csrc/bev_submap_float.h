/*
 * bev_submap_float.h — the float max-height BEV of submaps: windows of frames, each moved by its own pose, rastered into ONE
 * grid per map (bev_submap_float_bev_device_resident, bev_submap_float_bev_batch).  The host plan
 * (bev_submap_plan.h) says which (frame, pose) entry goes into which grid; the call is ONE launch group, a map's index its grid:
 *   k_submap_float_splat  per point and entry of its frame: transform_xyz (bev_exact.h), float_bev_cell (bev_misc.h) and
 *                         float_bev_put (bev_manip.h) into the entry's grid of the OUTPUT, global atomics.
 * The bit pattern of a non-negative float orders as its uint32, and float_bev_cell passes neither h <= 0 nor NaN: the output
 * grids, zeroed by the host, are the atomics' target; no workspace planes, no expand pass.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_FLOAT_H
#define BEV_SUBMAP_FLOAT_H

#include "bev_manip.h"
#include "bev_submap.h"

namespace bevk {
using namespace bevx;

/* A map over packed frames, k_submap_splat's shape: tab is a piece of the launch group's rows, of which this launch covers the
 * nf rows from tab[0] on (ent0: the same piece of the rows' entry starts), so its first workgroup is the group's workgroup
 * tab[0].blk0.  A workgroup is kProjBlock points of one row's frame; the label is loaded only where it is tested.  Then, per
 * entry of the row (a uniform loop; the 64-byte entries are read at uniform addresses), k_float_bev_batch's step into the
 * entry's grid; a point past the frame's end has no cell.  Every lane reaches every float_bev_put (it shuffles): no early
 * return.  No LDS. */
__global__ __launch_bounds__(256) void k_submap_float_splat(const bev_point_t *__restrict__ clouds,
                                                            const ProjFrame *__restrict__ tab,
                                                            const uint32_t *__restrict__ ent0, int nf,
                                                            const bevsub::Entry *__restrict__ entries, float interval, int M,
                                                            int skip_label0, uint32_t *__restrict__ out)
{
    const PackedPlace pl = packed_place(tab, nf, blockIdx.x + tab[0].blk0);
    const uint32_t n = pl.n, k0 = pl.k0;
    float4 a[kProjPerThread];
    int label[kProjPerThread];
    load_packed_records(clouds + pl.off, n, k0, skip_label0 != 0, 1, a, label);
    const size_t cells = (size_t)M * (size_t)M;
    const uint32_t e1 = ent0[pl.f + 1];
    for (uint32_t e = ent0[pl.f]; e < e1; ++e) {
        const bevsub::Entry en = entries[e];
        uint32_t *__restrict__ grid = out + (size_t)en.grid * cells;
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) {
            float tx, ty, tz, h;
            transform_xyz(en.m, a[j].x, a[j].y, a[j].z, tx, ty, tz);
            int cell = float_bev_cell(tx, ty, tz, label[j], interval, M, skip_label0, h);
            if (k0 + (uint32_t)j * 256u >= n) cell = -1;
            float_bev_put(grid, cell, h);
        }
    }
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_FLOAT_H */
