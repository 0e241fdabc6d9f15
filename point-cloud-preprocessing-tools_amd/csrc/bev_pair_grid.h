/*
 * bev_pair_grid.h — what the pair calls' search grids sized to the cloud (bev_set_pair_search_grid) add to the
 * build of bev_submap_grid.h, which they run over the TARGET SLOTS of a pair call.
 *
 * The build is k_subgrid_* as they are (bounds, header, count, sums, scan, scatter), fed from tables the host makes
 * (bev_pair_grid_plan.h): a target slot is a "map" whose points begin at pt0 = slot * Pn (fine: the slot's voxel cloud) or
 * frame * stride (coarse: the frame's PointNormal rows; the searchable points go to the same pt0, so under a cap the coarse
 * stage keeps them by FRAME), whose first counter lies at cell0 inside its build group, and whose
 * point count, which only the device knows, k_pairgrid_desc copies into a SubvoxHdr: vox_n[slot], or min(counts[frame], stride).
 * The coarse stage's rows go through SubgridRows, the very instantiations of §6s; the fine stage's records are 32 bytes, not
 * float4, so k_subgrid_bounds and k_subgrid_points are instantiated once more over PairgridRecs.  The launch grids come from
 * the host's capacities; a workgroup beyond its target's points or cells returns at once.
 *
 *   k_pairgrid_desc  per target    : the point count
 * The two ICP loops against such a grid, k_fine_icp_wide and k_icp_wide: bev_wide_icp.h.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only, ahead of bev_submap_grid.h, whose launcher
 * picks PairgridRecs for a source of records.
 */
#ifndef BEV_PAIR_GRID_H
#define BEV_PAIR_GRID_H

#include "bev_pair_grid_plan.h"

namespace bevk {

static_assert(bevpair::kBuildGroup == (uint32_t)kFineVoxelGroup && bevpair::kHdrBytes == sizeof(SubvoxHdr) &&
                  bevpair::kMapBytes == sizeof(bevsubreg::Map),
              "the plan counts these");

/* the position of record i of the slot whose records begin at pt0 */
struct PairgridRecs {
    const bev_point_t *pts;
    __device__ float3 operator()(uint64_t pt0, uint32_t i) const
    {
        const float4 p = *reinterpret_cast<const float4 *>(pts + pt0 + i);
        return make_float3(p.x, p.y, p.z);
    }
};

/* target t = blockIdx.x * 256 + threadIdx.x of n: its point count.  vox_n: the fine stage's counts by slot (the targets are the
 * first slots); else counts[frame] under the stride, the frame being the table's ent0 word */
__global__ __launch_bounds__(kRegThreads) void k_pairgrid_desc(const bevsubreg::Map *maps, uint32_t n, const uint32_t *vox_n,
                                                               const uint32_t *counts, uint64_t stride, SubvoxHdr *vh)
{
    const uint32_t t = blockIdx.x * kRegThreads + threadIdx.x;
    if (t >= n) return;
    SubvoxHdr h{};
    h.n_out = vox_n ? vox_n[t] : min(counts[maps[t].ent0], (uint32_t)stride);
    h.n = h.n_out;
    vh[t] = h;
}

/* ---- launchers ---- */
void launch_pairgrid_desc(const void *maps, int n, const uint32_t *vox_n, const uint32_t *counts, size_t stride, SubvoxHdr *vh,
                          hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_pairgrid_desc, dim3((n + kRegThreads - 1) / kRegThreads), dim3(kRegThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), (uint32_t)n, vox_n, counts, (uint64_t)stride, vh);
}

} /* namespace bevk */

#endif /* BEV_PAIR_GRID_H */
