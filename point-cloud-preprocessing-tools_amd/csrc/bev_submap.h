/*
 * bev_submap.h — the 24-layer occupancy BEV and the uint8 max-height BEV of submaps: windows of frames, each moved by its
 * own pose, rastered into ONE grid per map (bev_submap_bev_device_resident, bev_submap_bev_batch).  The host
 * plan (bev_submap_plan.h) says which (frame, pose) entry goes into which grid of a launch group; per group
 *   k_submap_splat  per point and entry of its frame: posed_code (bev_exact.h) into the entry's grid through posed_put
 *                   (bev_posed.h), global atomics;
 *   k_posed_expand  (bev_posed.h, unchanged) turns the planes into the images, the map's index in the group as its grid.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_H
#define BEV_SUBMAP_H

#include "bev_posed.h"
#include "bev_submap_plan.h"

namespace bevk {
using namespace bevx;

static_assert(sizeof(bevsub::Frame) == sizeof(ProjFrame) && offsetof(bevsub::Frame, off) == offsetof(ProjFrame, off) &&
                  offsetof(bevsub::Frame, n) == offsetof(ProjFrame, n) && offsetof(bevsub::Frame, blk0) == offsetof(ProjFrame, blk0),
              "the plan's rows are read as ProjFrame");
static_assert(bevsub::kBlockPoints == (uint32_t)kProjBlock, "the plan counts the workgroups of this kernel");

/* A map over packed frames, k_posed_splat's shape: tab is a piece of a launch group's rows, of which this launch covers the nf
 * rows from tab[0] on (ent0: the same piece of the rows' entry starts), so its first workgroup is the group's workgroup
 * tab[0].blk0.  A workgroup is kProjBlock points of one row's frame; a point past the frame's end has label 0: no code.  Then,
 * per entry of the row (a uniform loop; the 64-byte entries are read at uniform addresses), posed_code under the entry's
 * matrix into the planes of the entry's grid.  No LDS. */
__global__ __launch_bounds__(256) void k_submap_splat(const bev_point_t *__restrict__ clouds, const ProjFrame *__restrict__ tab,
                                                      const uint32_t *__restrict__ ent0, int nf,
                                                      const bevsub::Entry *__restrict__ entries, RasterParams rp,
                                                      uint32_t *__restrict__ planes)
{
    const PackedPlace pl = packed_place(tab, nf, blockIdx.x + tab[0].blk0);
    float4 a[kProjPerThread];
    int label[kProjPerThread];
    load_packed_records(clouds + pl.off, pl.n, pl.k0, true, 0, a, label);
    const int M = rp.mat_size;
    const uint32_t cells = (uint32_t)(M * M);
    const uint32_t e1 = ent0[pl.f + 1];
    for (uint32_t e = ent0[pl.f]; e < e1; ++e) {
        const bevsub::Entry en = entries[e];
        uint32_t *__restrict__ grid = planes + (size_t)en.grid * 2u * cells;
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) posed_put(grid, cells, M, posed_code(a[j].x, a[j].y, a[j].z, label[j], en.m, rp));
    }
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_H */
