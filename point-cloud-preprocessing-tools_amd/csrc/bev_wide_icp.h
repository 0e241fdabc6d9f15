/*
 * bev_wide_icp.h — the four ICP kernels against a search grid sized to the target (the build: bev_submap_grid.h), of the
 * scan-to-map calls (bev_set_submap_search_grid) and of the pair calls (bev_set_pair_search_grid; §6t).  Each is
 * the loop of its fixed-grid kernel with the target's cell offsets somewhere else: a map's at its cell base inside its launch
 * group (cell0, a plan table), a pair call's target slot's at slot * off_words of the wide table; the coarse ones read them from
 * global memory, since IcpShared::off holds 64 x 64 cells.
 *
 *   k_submap_icp_wide         per match   : k_submap_icp (bev_submap_reg.h)
 *   k_submap_coarse_icp_wide  per problem : k_submap_coarse_icp (bev_submap_coarse.h): submap_coarse_problem<false>, the one
 *                                           loop of both with the offsets read through the global pointer
 *   k_fine_icp_wide           per match   : k_fine_icp (bev_fine.h)
 *   k_icp_wide                per problem : k_icp's loop (bev_icp.h): submap_coarse_problem<false> too.  No body shared with
 *                                           k_icp (§6m: that costs k_icp two VGPRs); IcpShared::off stays unused
 * The pair kernels keep the scratch index modulo the problems of a launch, as k_fine_icp and k_icp do.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only, behind bev_submap_grid.h (one translation unit).
 */
#ifndef BEV_WIDE_ICP_H
#define BEV_WIDE_ICP_H

#include "bev_submap_reg_plan.h"

namespace bevk {

/* k_submap_icp (bev_submap_reg.h) with the map's cell offsets at its cell base */
__global__ __launch_bounds__(kFineThreads) void k_submap_icp_wide(const FineProblem *probs, const bevsubreg::Map *maps,
                                                                  uint32_t map0, FineWork w, SubmapRegWork t,
                                                                  const uint64_t *cell0, const bev_icp_result_t *coarse,
                                                                  const int32_t *best, bev_icp_params_t prm,
                                                                  bev_icp_result_t *results)
{
    __shared__ FineShared sh;
    const FineProblem pb = probs[blockIdx.x];
    const uint64_t pt0 = maps[pb.tgt_slot].pt0;
    const uint32_t g = pb.tgt_slot - map0;
    float G[16];
    fine_guess(pb, coarse, best, G);
    fine_icp_problem(sh, w.vox_n[pb.src_slot], w.vox + (size_t)pb.src_slot * w.Pn, SubregPts{t.pts + pt0}, t.hdr[g],
                     t.cell_off + cell0[pb.tgt_slot], t.sorted + pt0, w.cur + (size_t)blockIdx.x * w.Pn,
                     w.corr + (size_t)blockIdx.x * w.Pn, G, prm, results + pb.result);
}

/* k_submap_coarse_icp (bev_submap_coarse.h) with the map's cell offsets at its cell base, in global memory */
__global__ __launch_bounds__(kIcpThreads) void k_submap_coarse_icp_wide(const float *pn, size_t stride, const uint32_t *counts,
                                                                        const IcpProblem *probs, const bevsubreg::Map *maps,
                                                                        uint32_t map0, SubmapCoarseWork t, const uint64_t *cell0,
                                                                        bev_icp_params_t prm, bev_icp_result_t *results)
{
    __shared__ IcpShared sh;
    const IcpProblem pb = probs[blockIdx.x];
    const uint64_t pt0 = maps[pb.tgt_slot].pt0;
    const uint32_t g = pb.tgt_slot - map0;
    submap_coarse_problem<false>(sh, min(counts[pb.src_frame], (uint32_t)stride), pn + (size_t)pb.src_frame * stride * 12,
                                 t.rows + pt0 * 12, t.sorted + pt0, t.hdr + g, t.cell_off + cell0[pb.tgt_slot],
                                 t.cur + (size_t)blockIdx.x * stride, pb.guess, prm, results + pb.result);
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
    submap_coarse_problem<false>(sh, min(counts[pb.src_frame], (uint32_t)stride), pn + (size_t)pb.src_frame * stride * 12,
                                 pn + (size_t)pb.tgt_frame * stride * 12, w.sorted + (size_t)pb.tgt_frame * stride,
                                 w.hdr + pb.tgt_slot, w.cell_off + (size_t)pb.tgt_slot * off_words,
                                 w.cur + (size_t)(blockIdx.x % kIcpProblemsPerLaunch) * stride, pb.guess, prm, results + pb.result);
}

/* ---- launchers ---- */
void launch_submap_icp_wide(const FineProblem *probs, int n, const void *maps, uint32_t map0, const FineWork &w,
                            const SubmapRegWork &t, const uint64_t *cell0, const bev_icp_result_t *coarse, const int32_t *best,
                            const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_submap_icp_wide, dim3(n), dim3(kFineThreads), 0, st, probs, static_cast<const bevsubreg::Map *>(maps),
                           map0, w, t, cell0, coarse, best, prm, results);
}

void launch_submap_coarse_icp_wide(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                                   const void *maps, uint32_t map0, const SubmapCoarseWork &t, const uint64_t *cell0,
                                   const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_submap_coarse_icp_wide, dim3(n), dim3(kIcpThreads), 0, st, pn, stride, counts, probs,
                           static_cast<const bevsubreg::Map *>(maps), map0, t, cell0, prm, results);
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

#endif /* BEV_WIDE_ICP_H */
