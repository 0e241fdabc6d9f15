/*
 * bev_verify.h — verification of registered matches: two-way inlier counts under the returned transform
 * (bev_verify_clouds, bev_verify_registration_device_resident, bev_submap_verify_registration_device_resident).
 * Included by bev_kernels.hip after bev_reg_common.h, whose grid build (reg_grid_build) and exact 1-NN (icp_nn) it uses as
 * they are.  Per launch group of at most kVerifyProblemsPerLaunch matches:
 *
 *   k_verify_move   per match            : q' = icp_se3(T, q) of the query's voxel cloud as float4 into the group's scratch, the
 *                                          2-D search grid of the moved query (a NaN T: a grid of no point), then the match's
 *                                          result record: zeros, n_query and n_target from the two grid headers
 *   k_verify_count  (slices, matches, 2) : direction 0: the points q' against the target's grid; direction 1: the target's
 *                                          searchable points, as its sorted array holds them, against the moved query's grid.
 *                                          One icp_nn per point; per threshold a ballot per wave, added into LDS counters, and
 *                                          one global atomicAdd per non-zero counter into the record
 *
 * Every output is an integer count: no float sum, and integer adds commute, so nothing depends on an atomic's order, on the slice
 * or on the launch group.  The target's grid is whatever the caller built: k_fine_grid's per slot, k_submap_target's or
 * k_submap_vox_finish's per map.
 */
#pragma once

namespace bevk {

__global__ __launch_bounds__(kFineThreads) void k_verify_move(const VerifyProblem *probs, FineWork w, const bev_icp_result_t *results,
                                                              VerifyTarget t, VerifyWork v, bev_verify_result_t *out)
{
    const int tid = (int)threadIdx.x;
    const uint32_t m = blockIdx.x;
    const VerifyProblem pb = probs[m];
    float T[12];
    for (int k = 0; k < 12; ++k) T[k] = results[pb.result].T[k];
    const uint32_t n_src = w.vox_n[pb.src_slot];
    const bev_point_t *src = w.vox + (size_t)pb.src_slot * w.Pn;
    float4 *moved = v.moved + (size_t)m * v.Pn;
    for (uint32_t i = (uint32_t)tid; i < n_src; i += kRegThreads) {
        const float3 q = icp_se3(T, src[i].x, src[i].y, src[i].z);
        moved[i] = make_float4(q.x, q.y, q.z, 0.0f);
    }
    __syncthreads(); /* (the workgroup reads its own global writes behind a barrier: rf_bitonic) */
    reg_grid_build<kFineCells>(n_src, SubregPts{moved}, v.qhdr + m, v.qoff + (size_t)m * (kFineCells + 1), v.qsorted + (size_t)m * v.Pn);
    if (tid == 0) { /* (thread 0 wrote the header itself) */
        bev_verify_result_t r{};
        r.n_query = v.qhdr[m].n;
        r.n_target = t.hdr[pb.tgt_grid].n;
        out[pb.result] = r;
    }
}

__global__ __launch_bounds__(kFineThreads) void k_verify_count(const VerifyProblem *probs, FineWork w, VerifyTarget t, VerifyWork v,
                                                               bev_verify_params_t prm, uint32_t slice, bev_verify_result_t *out)
{
    __shared__ uint32_t cnt[BEV_VERIFY_MAX_THRESHOLDS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t m = blockIdx.y;
    const bool reverse = blockIdx.z != 0;
    const VerifyProblem pb = probs[m];
    const IcpGridHdr th = t.hdr[pb.tgt_grid], qh = v.qhdr[m];
    /* the points of this direction and the grid they are searched in */
    const float4 *pts = reverse ? t.sorted + pb.tgt_pt0 : v.moved + (size_t)m * v.Pn;
    const uint32_t n = reverse ? th.n : w.vox_n[pb.src_slot];
    const IcpGridHdr h = reverse ? qh : th;
    const uint32_t *off = reverse ? v.qoff + (size_t)m * (kFineCells + 1) : t.cell_off + (size_t)pb.tgt_grid * (kFineCells + 1);
    const float4 *gpts = reverse ? v.qsorted + (size_t)m * v.Pn : t.sorted + pb.tgt_pt0;
    const uint64_t i0 = (uint64_t)blockIdx.x * slice;
    if (i0 >= n || h.n == 0) return; /* (the whole workgroup) */
    const uint32_t i1 = (uint32_t)min(i0 + slice, (uint64_t)n);
    const int nt = prm.n_thresholds;
    double lim2[BEV_VERIFY_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < BEV_VERIFY_MAX_THRESHOLDS; ++k) lim2[k] = (double)prm.threshold[k] * (double)prm.threshold[k];
    const double last2 = (double)prm.threshold[nt - 1] * (double)prm.threshold[nt - 1];
    if (tid < BEV_VERIFY_MAX_THRESHOLDS) cnt[tid] = 0;
    __syncthreads();
    for (uint32_t b = (uint32_t)i0; b < i1; b += kRegThreads) { /* (a trip count the whole workgroup shares: the ballots) */
        const uint32_t i = b + (uint32_t)tid;
        bool found = false;
        float d = INFINITY;
        if (i < i1) {
            const float4 p = pts[i];
            uint32_t j;
            found = finite3(p.x, p.y, p.z) && icp_nn(h, off, gpts, p.x, p.y, p.z, last2, d, j);
        }
#pragma unroll
        for (int k = 0; k < BEV_VERIFY_MAX_THRESHOLDS; ++k) {
            const uint64_t bal = __ballot(found && k < nt && (double)d <= lim2[k]);
            if (lane == 0 && bal) atomicAdd(&cnt[k], (uint32_t)__popcll(bal));
        }
    }
    __syncthreads();
    if (tid < nt && cnt[tid]) {
        bev_verify_result_t *r = out + pb.result;
        atomicAdd(reverse ? &r->target_within[tid] : &r->query_within[tid], cnt[tid]);
    }
}

void launch_verify_move(const VerifyProblem *probs, int n, const FineWork &w, const bev_icp_result_t *results, const VerifyTarget &t,
                        const VerifyWork &v, bev_verify_result_t *out, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_verify_move, dim3(n), dim3(kFineThreads), 0, st, probs, w, results, t, v, out);
}

void launch_verify_count(const VerifyProblem *probs, int n, uint32_t slices, const FineWork &w, const VerifyTarget &t,
                         const VerifyWork &v, const bev_verify_params_t &prm, uint32_t slice, bev_verify_result_t *out, hipStream_t st)
{
    if (n > 0 && slices > 0)
        hipLaunchKernelGGL(k_verify_count, dim3(slices, n, 2), dim3(kFineThreads), 0, st, probs, w, t, v, prm, slice, out);
}

} /* namespace bevk */
