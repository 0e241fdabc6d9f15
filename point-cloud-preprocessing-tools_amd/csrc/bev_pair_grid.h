/*
 * bev_pair_grid.h — the pair calls' search grids sized to the cloud (bev_set_pair_search_grid): the build of
 * bev_submap_grid.h run over the TARGET SLOTS of a pair call, and the two ICP loops against such a grid.
 *
 * The build is k_subgrid_* as they are (bounds, header, count, sums, scan, scatter), fed from tables the host makes
 * (bev_pair_grid_plan.h): a target slot is a "map" whose points begin at pt0 = slot * Pn (fine: the slot's voxel cloud) or
 * frame * stride (coarse: the frame's PointNormal rows; the searchable points go to the same pt0, so under a cap the coarse
 * stage keeps them by FRAME), whose first counter lies at cell0 inside its build group, and whose
 * point count, which only the device knows, k_pairgrid_desc copies into a SubvoxHdr: vox_n[slot], or min(counts[frame], stride).
 * The coarse stage's rows go through SubgridRows, the very instantiations of §6s; the fine stage's records are 32 bytes, not
 * float4, so k_subgrid_bounds and k_subgrid_points are instantiated once more over PairgridRecs.  The launch grids come from
 * the host's capacities; a workgroup beyond its target's points or cells returns at once.  No workgroup waits for another; no
 * float or double value depends on an atomic.
 *
 *   k_pairgrid_desc  per target    : the point count
 *   k_fine_icp_wide  per match     : k_fine_icp (bev_fine.h) with the target's offsets at slot * off_words of the wide table
 *   k_icp_wide       per problem   : k_icp's loop (bev_icp.h) with the offsets read from global memory: a call of
 *                                    submap_coarse_problem_wide (bev_submap_grid.h).  No body shared with k_icp (§6m: that costs
 *                                    k_icp two VGPRs); IcpShared::off stays unused
 * Both keep the scratch index modulo the problems of a launch, as k_fine_icp and k_icp do.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only, behind bev_submap_grid.h.
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

__global__ __launch_bounds__(kFineThreads) void k_fine_icp_wide(const FineProblem *probs, FineWork w, uint64_t off_words,
                                                                const bev_icp_result_t *coarse, const int32_t *best,
                                                                bev_icp_params_t prm, bev_icp_result_t *results)
{
    __shared__ FineShared sh;
    const FineProblem pb = probs[blockIdx.x];
    float G[16];
    fine_guess(pb, coarse, best, G);
    fine_icp_problem(sh, w.vox_n[pb.src_slot], w.vox + (size_t)pb.src_slot * w.Pn, FinePts{w.vox + (size_t)pb.tgt_slot * w.Pn},
                     w.hdr[pb.tgt_slot], w.cell_off + (size_t)pb.tgt_slot * off_words, w.sorted + (size_t)pb.tgt_slot * w.Pn,
                     w.cur + (size_t)(blockIdx.x % kFineProblemsPerLaunch) * w.Pn,
                     w.corr + (size_t)(blockIdx.x % kFineProblemsPerLaunch) * w.Pn, G, prm, results + pb.result);
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_wide(const float *pn, size_t stride, const uint32_t *counts,
                                                          const IcpProblem *probs, IcpWork w, uint64_t off_words,
                                                          bev_icp_params_t prm, bev_icp_result_t *results)
{
    __shared__ IcpShared sh;
    const IcpProblem pb = probs[blockIdx.x];
    submap_coarse_problem_wide(sh, min(counts[pb.src_frame], (uint32_t)stride), pn + (size_t)pb.src_frame * stride * 12,
                               pn + (size_t)pb.tgt_frame * stride * 12, w.sorted + (size_t)pb.tgt_frame * stride, w.hdr + pb.tgt_slot,
                               w.cell_off + (size_t)pb.tgt_slot * off_words,
                               w.cur + (size_t)(blockIdx.x % kIcpProblemsPerLaunch) * stride, pb.guess, prm, results + pb.result);
}

/* ---- launchers ---- */
void launch_pairgrid_desc(const void *maps, int n, const uint32_t *vox_n, const uint32_t *counts, size_t stride, SubvoxHdr *vh,
                          hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_pairgrid_desc, dim3((n + kRegThreads - 1) / kRegThreads), dim3(kRegThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), (uint32_t)n, vox_n, counts, (uint64_t)stride, vh);
}

void launch_pair_grid(int step, const void *maps, uint32_t t0, int n, uint32_t parts, uint32_t tiles, int cap, const SubvoxHdr *vh,
                      const bev_point_t *recs, const float *rows, const SubmapGridWork &w, hipStream_t st)
{
    if (n <= 0) return;
    parts = std::min(std::max(parts, 1u), kSubgridParts);
    tiles = std::min(std::max(tiles, 1u), kSubgridScanParts);
    const bevsubreg::Map *mp = static_cast<const bevsubreg::Map *>(maps);
    if (recs) subgrid_launches(mp, t0, n, parts, tiles, cap, vh, PairgridRecs{recs}, w, step, st);
    else subgrid_launches(mp, t0, n, parts, tiles, cap, vh, SubgridRows{rows}, w, step, st);
}

void launch_fine_icp_wide(const FineProblem *probs, int n, const FineWork &w, uint64_t off_words, const bev_icp_result_t *coarse,
                          const int32_t *best, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_fine_icp_wide, dim3(n), dim3(kFineThreads), 0, st, probs, w, off_words, coarse, best, prm, results);
}

void launch_icp_wide(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n, const IcpWork &w,
                     uint64_t off_words, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_icp_wide, dim3(n), dim3(kIcpThreads), 0, st, pn, stride, counts, probs, w, off_words, prm, results);
}

} /* namespace bevk */

#endif /* BEV_PAIR_GRID_H */
