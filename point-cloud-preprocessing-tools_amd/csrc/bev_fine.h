/*
 * bev_fine.h — the fine stage of the registration tools (included by bev_kernels.hip after bev_reg_common.h, whose voxel
 * steps, grid build, search, ordered pass and loop it uses): pcl::VoxelGrid<PointXYZIRCT> on the full labelled clouds and
 * pcl::IterativeClosestPoint<PointXYZIRCT, PointXYZIRCT> (point-to-point, TransformationEstimationSVD) as performFineIcp
 * runs it (BatchTopPartRegistration.cpp:224-247, 480-497; BatchWholeRegistration.cpp:222-245, 372-389).  The contract
 * every line follows (and tests/fineicp/fine_icp_oracle.c restates) is DESIGN.md §6d.
 *
 *   k_fine_voxel  per frame        : bounds, voxel index, a bitonic sort of (voxel index, input index) keys in global
 *                                    scratch, voxel starts, then one lane per voxel: x, y, z, intensity summed in input
 *                                    order, the label vote of AccumulatorLabel
 *   k_fine_grid   per target frame : a uniform 2-D grid of at most kFineGridMax^2 cells over the voxel centroids, a
 *                                    counting sort of the searchable points by cell (the search is icp_nn)
 *   k_fine_icp    per match        : the whole loop in one workgroup — pass 1: correspondences, the six coordinate sums,
 *                                    the MSE; pass 2: the nine products of sigma; thread 0: Umeyama through a 3 x 3
 *                                    Jacobi SVD, the increment, convergence — then getFitnessScore
 *
 * No float or double sum depends on an atomic: every sum over source points runs over 64-point chunks as a fixed tree
 * (wave shuffles), the chunks in ascending order in one lane; the voxel sums run in one lane in input order.
 */
#pragma once

namespace bevk {

/* a record's position */
struct FinePts {
    const bev_point_t *pts;
    __device__ float3 operator()(uint32_t i) const { return make_float3(pts[i].x, pts[i].y, pts[i].z); }
};

/* ---- voxel grid on PointXYZIRCT ---------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kFineThreads) void k_fine_voxel(const bev_point_t *pts, const FineSlot *slots, int slot0,
                                                             FineWork w, float leaf)
{
    __shared__ float red[7 * kRegWaves];
    __shared__ uint32_t wave_cnt[kRegWaves];
    __shared__ int s_par[8]; /* overflow, nfin, minb xyz, div xyz */
    const int g = (int)blockIdx.x, s = slot0 + g, t = (int)threadIdx.x;
    const FineSlot sl = slots[s];
    const bev_point_t *src = pts + sl.off;
    const uint32_t m = sl.n;
    bev_point_t *out = w.vox + (size_t)s * w.Pn;
    uint32_t *vstart = w.vstart + (size_t)g * (w.Pn + 1);

    const FinePts fetch{src};
    const float inv = 1.0f / leaf;
    rf_voxel_bounds(m, fetch, inv, red, s_par);
    const uint32_t nf = (uint32_t)s_par[1];
    if (nf == 0) {
        if (t == 0) w.vox_n[s] = 0;
        return;
    }
    if (s_par[0]) { /* PCL: "leaf size is too small": the output is the input */
        for (uint32_t i = t; i < m; i += kFineThreads) out[i] = src[i];
        if (t == 0) w.vox_n[s] = m;
        return;
    }
    const uint32_t np2 = rf_pow2(m);
    uint64_t *buf = w.keys + (size_t)g * w.Kn;
    rf_voxel_keys(m, np2, fetch, inv, s_par, buf);
    rf_bitonic(buf, np2);
    const uint32_t nv = rf_voxel_starts(buf, nf, wave_cnt, vstart, [](uint32_t, uint32_t) {});
    if (t == 0) w.vox_n[s] = nv;
    __syncthreads();
    /* CentroidPoint<PointXYZIRCT>: AccumulatorXYZ, AccumulatorIntensity (float sums in input order / float(n)) and
     * AccumulatorLabel (std::map<uint32_t, size_t>: the most frequent label, on a tie the smallest as uint32 — the
     * order of uint16(label)); row, col, t have no accumulator and stay 0 */
    for (uint32_t v = t; v < nv; v += kFineThreads) {
        const uint32_t a = vstart[v], b = vstart[v + 1];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, si = 0.0f;
        for (uint32_t q = a; q < b; ++q) {
            const bev_point_t &p = src[(uint32_t)buf[q]];
            sx += p.x;
            sy += p.y;
            sz += p.z;
            si += p.intensity;
        }
        /* the vote: the distinct keys in ascending order, one pass each (a voxel holds few distinct labels) */
        int32_t last = -1, best_key = 0;
        uint32_t best_cnt = 0;
        while (true) {
            int32_t k_min = 0x10000;
            uint32_t cnt = 0;
            for (uint32_t q = a; q < b; ++q) {
                const int32_t k = (int32_t)(uint16_t)src[(uint32_t)buf[q]].label;
                if (k <= last) continue;
                if (k < k_min) {
                    k_min = k;
                    cnt = 1;
                } else if (k == k_min) {
                    ++cnt;
                }
            }
            if (k_min == 0x10000) break;
            if (cnt > best_cnt) {
                best_cnt = cnt;
                best_key = k_min;
            }
            last = k_min;
        }
        const float cf = (float)(b - a);
        bev_point_t o{};
        o.x = sx / cf;
        o.y = sy / cf;
        o.z = sz / cf;
        o.intensity = si / cf;
        o.label = (int16_t)(uint16_t)best_key;
        out[v] = o;
    }
}

/* ---- the target frames' grids ------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kFineThreads) void k_fine_grid(FineWork w)
{
    const int s = (int)blockIdx.x;
    reg_grid_build<kFineCells>(w.vox_n[s], FinePts{w.vox + (size_t)s * w.Pn}, w.hdr + s,
                               w.cell_off + (size_t)s * (kFineCells + 1), w.sorted + (size_t)s * w.Pn);
}

/* ---- Umeyama through Eigen's JacobiSVD<Matrix3f> ------------------------------------------------ */
/* apply_rotation_in_the_plane(x, y, (c, s)): x' = c x + s y, y' = -s x + c y; nothing when c == 1 and s == 0 */
__device__ __forceinline__ void fine_rot(float &x, float &y, float c, float s)
{
    const float a = x, b = y;
    x = c * a + s * b;
    y = -s * a + c * b;
}

/* det of a row-major 3 x 3: bruteforce_det3_helper(0,1,2) - (1,0,2) + (2,0,1) */
__device__ __forceinline__ float fine_det3(const float *M)
{
    const float h0 = M[0] * (M[4] * M[8] - M[5] * M[7]);
    const float h1 = M[1] * (M[3] * M[8] - M[5] * M[6]);
    const float h2 = M[2] * (M[3] * M[7] - M[4] * M[6]);
    return (h0 - h1) + h2;
}

/* sigma (row-major, finite) -> R (row-major): U S V^T with S = diag(1, 1, +-1).  (Inlined by force: left to the cost model,
 * unrelated edits of k_fine_icp move its register count across the 128 of four waves per SIMD.) */
__device__ __forceinline__ void fine_svd_rotation(const float *sigma, float *R)
{
    const float kMin = 1.17549435e-38f, kPrec = 2.0f * 1.1920929e-7f;
    float scale = 0.0f;
    for (int k = 0; k < 9; ++k) scale = fmaxf(scale, fabsf(sigma[k]));
    if (scale == 0.0f) scale = 1.0f;
    float W[9], U[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) W[k] = sigma[k] / scale;
    float maxd = fmaxf(fmaxf(fabsf(W[0]), fabsf(W[4])), fabsf(W[8]));
    for (int sweep = 0; sweep < kFineSvdSweeps; ++sweep) {
        bool finished = true;
        for (int p = 1; p < 3; ++p) {
            for (int q = 0; q < p; ++q) {
                const float thr = fmaxf(kMin, kPrec * maxd);
                if (!(fabsf(W[p * 3 + q]) > thr || fabsf(W[q * 3 + p]) > thr)) continue;
                finished = false;
                /* real_2x2_jacobi_svd */
                const float m00 = W[p * 3 + p], m01 = W[p * 3 + q], m10 = W[q * 3 + p], m11 = W[q * 3 + q];
                const float tt = m00 + m11, d = m10 - m01;
                float c1, s1;
                if (fabsf(d) < kMin) {
                    s1 = 0.0f;
                    c1 = 1.0f;
                } else {
                    const float u = tt / d, tmp = sqrtf(1.0f + u * u);
                    s1 = 1.0f / tmp;
                    c1 = u / tmp;
                }
                float n00 = m00, n01 = m01, n10 = m10, n11 = m11;
                if (!(c1 == 1.0f && s1 == 0.0f)) {
                    fine_rot(n00, n10, c1, s1);
                    fine_rot(n01, n11, c1, s1);
                }
                float cr, sr; /* makeJacobi(n00, n01, n11) */
                const float deno = 2.0f * fabsf(n01);
                if (deno < kMin) {
                    cr = 1.0f;
                    sr = 0.0f;
                } else {
                    const float tau = (n00 - n11) / deno, wv = sqrtf(tau * tau + 1.0f);
                    const float tj = tau > 0.0f ? 1.0f / (tau + wv) : 1.0f / (tau - wv);
                    const float sign_t = tj > 0.0f ? 1.0f : -1.0f;
                    const float nn = 1.0f / sqrtf(tj * tj + 1.0f);
                    sr = ((-sign_t * (n01 / fabsf(n01))) * fabsf(tj)) * nn;
                    cr = nn;
                }
                /* j_left = rot1 * j_right^T */
                const float cl = c1 * cr - s1 * (-sr), sl = c1 * (-sr) + s1 * cr;
                if (!(cl == 1.0f && sl == 0.0f)) {
                    for (int k = 0; k < 3; ++k) fine_rot(W[p * 3 + k], W[q * 3 + k], cl, sl); /* W.applyOnTheLeft */
                    for (int k = 0; k < 3; ++k) fine_rot(U[k * 3 + p], U[k * 3 + q], cl, sl); /* U.applyOnTheRight(jl^T) */
                }
                if (!(cr == 1.0f && -sr == 0.0f)) {
                    for (int k = 0; k < 3; ++k) fine_rot(W[k * 3 + p], W[k * 3 + q], cr, -sr); /* W.applyOnTheRight */
                    for (int k = 0; k < 3; ++k) fine_rot(V[k * 3 + p], V[k * 3 + q], cr, -sr);
                }
                maxd = fmaxf(maxd, fmaxf(fabsf(W[p * 3 + p]), fabsf(W[q * 3 + q])));
            }
        }
        if (finished) break;
    }
    float sv[3];
    for (int i = 0; i < 3; ++i) {
        const float a = W[i * 3 + i];
        sv[i] = fabsf(a);
        if (a < 0.0f)
            for (int k = 0; k < 3; ++k) U[k * 3 + i] = -U[k * 3 + i];
    }
    for (int i = 0; i < 3; ++i) sv[i] *= scale;
    for (int i = 0; i < 3; ++i) { /* descending; maxCoeff takes the first of equal values */
        int pos = i;
        for (int k = i + 1; k < 3; ++k)
            if (sv[k] > sv[pos]) pos = k;
        if (sv[pos] == 0.0f) break;
        if (pos != i) {
            const float tsv = sv[i];
            sv[i] = sv[pos];
            sv[pos] = tsv;
            for (int k = 0; k < 3; ++k) {
                float tu = U[k * 3 + i];
                U[k * 3 + i] = U[k * 3 + pos];
                U[k * 3 + pos] = tu;
                tu = V[k * 3 + i];
                V[k * 3 + i] = V[k * 3 + pos];
                V[k * 3 + pos] = tu;
            }
        }
    }
    const float sgn = fine_det3(U) * fine_det3(V) < 0.0f ? -1.0f : 1.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[i * 3 + j] = (U[i * 3] * V[j * 3] + U[i * 3 + 1] * V[j * 3 + 1]) + (U[i * 3 + 2] * sgn) * V[j * 3 + 2];
}

/* ---- the loop ----------------------------------------------------------------------------------------------------- */
struct FineShared {
    RegSums<9, 1> sums;
    RegLoop loop;
    float mean[6];
};

/* thread 0: sigma, the rotation, the translation, then the shared tail */
__device__ void fine_step(FineShared &sh, const bev_icp_params_t &prm, double mse_sum, double &prev)
{
    const float oon = 1.0f / (float)sh.sums.cnt;
    float sigma[9];
    bool finite = true;
    for (int k = 0; k < 9; ++k) {
        sigma[k] = oon * sh.sums.totf[k];
        finite = finite && isfinite(sigma[k]);
    }
    float *I = sh.loop.inc;
    if (finite) {
        float R[9];
        fine_svd_rotation(sigma, R);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) I[i * 4 + j] = R[i * 3 + j];
            I[i * 4 + 3] = sh.mean[3 + i] - ((R[i * 3] * sh.mean[0] + R[i * 3 + 1] * sh.mean[1]) + R[i * 3 + 2] * sh.mean[2]);
        }
    } else {
        for (int k = 0; k < 12; ++k) I[k] = __uint_as_float(0x7fc00000u);
    }
    I[12] = 0.0f;
    I[13] = 0.0f;
    I[14] = 0.0f;
    I[15] = 1.0f;
    reg_converge(sh.loop, prm, mse_sum, sh.sums.cnt, prev);
}

/* a problem's first guess: the better coarse result of its match (top-part tool), or the one it carries */
__device__ __forceinline__ void fine_guess(const FineProblem &pb, const bev_icp_result_t *coarse, const int32_t *best, float *G)
{
    if (pb.coarse_match != 0xffffffffu) {
        const uint32_t m = pb.coarse_match;
        const bev_icp_result_t &r = coarse[2 * (size_t)m + (best[m] ? 1 : 0)];
        for (int k = 0; k < 16; ++k) G[k] = r.T[k];
    } else {
        for (int k = 0; k < 16; ++k) G[k] = pb.guess[k];
    }
}

/* One problem by its workgroup: the voxel cloud src of n_src points onto a target that is read through tgt(j), the position of
 * target point j, and its search grid (h, toff, tpts); cur, corr: the problem's scratch.  k_fine_icp's target is a slot's voxel
 * cloud, k_submap_icp's (bev_submap_reg.h) a map's moved points. */
template <class Tgt>
__device__ __forceinline__ void fine_icp_problem(FineShared &sh, uint32_t n_src, const bev_point_t *src, Tgt tgt,
                                                 const IcpGridHdr &h, const uint32_t *toff, const float4 *tpts, float4 *cur,
                                                 uint32_t *corr, const float *G, const bev_icp_params_t &prm,
                                                 bev_icp_result_t *result)
{
    const int tid = threadIdx.x;
    reg_start(sh.loop, G, n_src, FinePts{src}, cur);
    __syncthreads();
    const double D2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    double prev = 1.7976931348623157e308; /* DBL_MAX (thread 0's copy is the one used) */
    while (true) {
        /* pass 1: correspondences, the source and target coordinate sums (float), the MSE (double) */
        reg_pass<6, 1>(sh.sums, n_src, [&](uint32_t i, float *t, double *td) -> bool {
            const float4 s = cur[i];
            uint32_t j = 0xffffffffu;
            float d;
            if (!finite3(s.x, s.y, s.z) || !icp_nn(h, toff, tpts, s.x, s.y, s.z, D2, d, j) || !((double)d <= D2)) {
                corr[i] = 0xffffffffu;
                return false;
            }
            corr[i] = j;
            const float3 tp = tgt(j);
            t[0] = s.x;
            t[1] = s.y;
            t[2] = s.z;
            t[3] = tp.x;
            t[4] = tp.y;
            t[5] = tp.z;
            td[0] = (double)d;
            return true;
        });
        if (tid == 0) {
            if (sh.sums.cnt < 3) {
                sh.loop.state = 5; /* NO_CORRESPONDENCES */
            } else {
                const float oon = 1.0f / (float)sh.sums.cnt;
                for (int k = 0; k < 6; ++k) sh.mean[k] = sh.sums.totf[k] * oon;
            }
        }
        __syncthreads();
        if (sh.loop.state != 0) break;
        const double mse_sum = sh.sums.totd[0];
        float M[6];
        for (int k = 0; k < 6; ++k) M[k] = sh.mean[k];
        /* pass 2: sigma's nine products dst_demean[a] * src_demean[b] (float); it counts the same correspondences */
        reg_pass<9, 0>(sh.sums, n_src, [&](uint32_t i, float *t, double *) -> bool {
            const uint32_t j = corr[i];
            if (j == 0xffffffffu) return false;
            const float4 s = cur[i];
            const float3 tp = tgt(j);
            const float sd[3] = {s.x - M[0], s.y - M[1], s.z - M[2]};
            const float dd[3] = {tp.x - M[3], tp.y - M[4], tp.z - M[5]};
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) t[a * 3 + b] = dd[a] * sd[b];
            return true;
        });
        if (tid == 0) fine_step(sh, prm, mse_sum, prev);
        __syncthreads();
        if (sh.loop.state != 0) break;
        reg_advance(sh.loop, n_src, cur);
    }
    reg_finish(sh.sums, sh.loop, n_src, FinePts{src}, h, toff, tpts, result);
}

__global__ __launch_bounds__(kFineThreads) void k_fine_icp(const FineProblem *probs, FineWork w,
                                                           const bev_icp_result_t *coarse, const int32_t *best,
                                                           bev_icp_params_t prm, bev_icp_result_t *results)
{
    __shared__ FineShared sh;
    const FineProblem pb = probs[blockIdx.x];
    float G[16];
    fine_guess(pb, coarse, best, G);
    fine_icp_problem(sh, w.vox_n[pb.src_slot], w.vox + (size_t)pb.src_slot * w.Pn, FinePts{w.vox + (size_t)pb.tgt_slot * w.Pn},
                     w.hdr[pb.tgt_slot], w.cell_off + (size_t)pb.tgt_slot * (kFineCells + 1),
                     w.sorted + (size_t)pb.tgt_slot * w.Pn, w.cur + (size_t)(blockIdx.x % kFineProblemsPerLaunch) * w.Pn,
                     w.corr + (size_t)(blockIdx.x % kFineProblemsPerLaunch) * w.Pn, G, prm, results + pb.result);
}

void launch_fine_voxel(const bev_point_t *pts, const FineSlot *slots, int slot0, int n, const FineWork &w, float leaf,
                       hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_fine_voxel, dim3(n), dim3(kFineThreads), 0, st, pts, slots, slot0, w, leaf);
}

void launch_fine_grid(int n_slots, const FineWork &w, hipStream_t st)
{
    if (n_slots > 0) hipLaunchKernelGGL(k_fine_grid, dim3(n_slots), dim3(kFineThreads), 0, st, w);
}

void launch_fine_icp(const FineProblem *probs, int n, const FineWork &w, const bev_icp_result_t *coarse,
                     const int32_t *best, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_fine_icp, dim3(n), dim3(kFineThreads), 0, st, probs, w, coarse, best, prm, results);
}

} /* namespace bevk */
