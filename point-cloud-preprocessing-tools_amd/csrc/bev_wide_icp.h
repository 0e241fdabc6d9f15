/*
 * bev_wide_icp.h — the four ICP kernels against a search grid sized to the target (the build: bev_submap_grid.h), of the
 * scan-to-map calls (bev_set_submap_search_grid) and of the pair calls (bev_set_pair_search_grid; §6t).  Each is
 * the loop of its fixed-grid kernel with the target's cell offsets somewhere else: a map's at its cell base inside its launch
 * group (cell0, a plan table), a pair call's target slot's at slot * off_words of the wide table; the coarse ones read them from
 * global memory, since IcpShared::off holds 64 x 64 cells.
 *
 *   k_submap_icp_wide         per match   : k_submap_icp (bev_submap_reg.h)
 *   k_submap_coarse_icp_wide  per problem : k_submap_coarse_icp (bev_submap_coarse.h): a call of submap_coarse_problem_wide
 *   k_fine_icp_wide           per match   : k_fine_icp (bev_fine.h)
 *   k_icp_wide                per problem : k_icp's loop (bev_icp.h): a call of submap_coarse_problem_wide.  No body shared with
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

/* submap_coarse_problem (bev_submap_coarse.h), statement for statement, but that the cell offsets stay in global memory:
 * IcpShared::off holds 64 x 64 cells.  A COPY for the reason given there; sh.off is not used (icp_step takes an IcpShared). */
__device__ __forceinline__ void submap_coarse_problem_wide(IcpShared &sh, uint32_t n_src, const float *src, const float *tgt,
                                                           const float4 *tpts, const IcpGridHdr *hdr, const uint32_t *goff,
                                                           float4 *cur, const float *guess, const bev_icp_params_t &prm,
                                                           bev_icp_result_t *result)
{
    const int tid = threadIdx.x;
    if (tid == 0) sh.hdr = *hdr;
    __syncthreads();
    const IcpGridHdr h = sh.hdr;
    reg_start(sh.loop, guess, n_src, IcpRows{src}, cur);
    __syncthreads();
    const double D2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    double prev = 1.7976931348623157e308; /* DBL_MAX (thread 0's copy is the one used) */
    while (true) {
        reg_pass<0, 28>(sh.sums, n_src, [&](uint32_t i, float *, double *t) -> bool {
            const float4 s = cur[i];
            if (!finite3(s.x, s.y, s.z)) return false;
            float d;
            uint32_t j;
            if (!icp_nn(h, goff, tpts, s.x, s.y, s.z, D2, d, j) || !((double)d <= D2)) return false;
            const float4 tp = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12);
            const float4 tn = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12 + 4);
            const float nx = tn.x, ny = tn.y, nz = tn.z;
            if (finite3(nx, ny, nz)) {
                const float a = nz * s.y - ny * s.z, b = nx * s.z - nz * s.x, c = ny * s.x - nx * s.y;
                const float dd = ((((nx * tp.x + ny * tp.y) + nz * tp.z) - nx * s.x) - ny * s.y) - nz * s.z;
                const double r[6] = {a, b, c, nx, ny, nz};
                int k = 0;
#pragma unroll
                for (int u = 0; u < 6; ++u)
#pragma unroll
                    for (int v = u; v < 6; ++v) t[k++] = r[u] * r[v];
#pragma unroll
                for (int u = 0; u < 6; ++u) t[21 + u] = r[u] * (double)dd;
            }
            t[27] = (double)d;
            return true;
        });
        if (tid == 0) {
            if (sh.sums.cnt < 3) sh.loop.state = 5; /* NO_CORRESPONDENCES */
            else icp_step(sh, prm, prev);
        }
        __syncthreads();
        if (sh.loop.state != 0) break;
        reg_advance(sh.loop, n_src, cur);
    }
    reg_finish(sh.sums, sh.loop, n_src, IcpRows{src}, h, goff, tpts, result);
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
    submap_coarse_problem_wide(sh, min(counts[pb.src_frame], (uint32_t)stride), pn + (size_t)pb.src_frame * stride * 12,
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
    submap_coarse_problem_wide(sh, min(counts[pb.src_frame], (uint32_t)stride), pn + (size_t)pb.src_frame * stride * 12,
                               pn + (size_t)pb.tgt_frame * stride * 12, w.sorted + (size_t)pb.tgt_frame * stride, w.hdr + pb.tgt_slot,
                               w.cell_off + (size_t)pb.tgt_slot * off_words,
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
