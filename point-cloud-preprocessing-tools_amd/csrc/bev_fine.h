/*
 * bev_fine.h — the fine stage of the registration tools (included by bev_kernels.hip, after bev_regfront.h and
 * bev_icp.h): pcl::VoxelGrid<PointXYZIRCT> on the full labelled clouds and pcl::IterativeClosestPoint<PointXYZIRCT,
 * PointXYZIRCT> (point-to-point, TransformationEstimationSVD) as performFineIcp runs it (BatchTopPartRegistration.cpp:
 * 224-247, 480-497; BatchWholeRegistration.cpp:222-245, 372-389).  The contract every line follows (and
 * tests/fineicp/fine_icp_oracle.c restates) is DESIGN.md §6d.
 *
 *   k_fine_voxel  per frame        : bounds, voxel index, a bitonic sort of (voxel index, input index) keys in global
 *                                    scratch, voxel starts, then one lane per voxel: x, y, z, intensity summed in input
 *                                    order, the label vote of AccumulatorLabel
 *   k_fine_grid   per target frame : a uniform 2-D grid of at most kFineGridMax^2 cells over the voxel centroids, a
 *                                    counting sort of the searchable points by cell (the search of bev_icp.h, icp_nn)
 *   k_fine_icp    per match        : the whole loop in one workgroup — pass 1: correspondences, the six coordinate sums,
 *                                    the MSE; pass 2: the nine products of sigma; thread 0: Umeyama through a 3 x 3
 *                                    Jacobi SVD, the increment, convergence — then getFitnessScore
 *
 * No float or double sum depends on an atomic: every sum over source points runs over 64-point chunks as a fixed tree
 * (wave shuffles), the chunks in ascending order in one lane; the voxel sums run in one lane in input order.
 */
#pragma once

namespace bevk {

/* ---- voxel grid on PointXYZIRCT ---------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kFineThreads) void k_fine_voxel(const bev_point_t *pts, const FineSlot *slots, int slot0,
                                                             FineWork w, float leaf)
{
    __shared__ float red[7][kFineThreads / 64];
    __shared__ uint32_t wave_cnt[kFineThreads / 64];
    __shared__ int s_par[8]; /* overflow, nfin, minb xyz, div xyz */
    const int g = (int)blockIdx.x, s = slot0 + g, t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    const FineSlot sl = slots[s];
    const bev_point_t *src = pts + sl.off;
    const uint32_t m = sl.n;
    bev_point_t *out = w.vox + (size_t)s * w.Pn;
    uint32_t *vstart = w.vstart + (size_t)g * (w.Pn + 1);

    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nfin = 0;
    for (uint32_t i = t; i < m; i += kFineThreads) {
        const bev_point_t &q = src[i];
        if (!rf_finite3(q.x, q.y, q.z)) continue;
        ++nfin;
        mn[0] = fminf(mn[0], q.x), mn[1] = fminf(mn[1], q.y), mn[2] = fminf(mn[2], q.z);
        mx[0] = fmaxf(mx[0], q.x), mx[1] = fmaxf(mx[1], q.y), mx[2] = fmaxf(mx[2], q.z);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        for (int d = 0; d < 3; ++d) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], off));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off));
        }
        nfin += __shfl_xor(nfin, off);
    }
    if (lane == 0) {
        for (int d = 0; d < 3; ++d) {
            red[d][wv] = mn[d];
            red[3 + d][wv] = mx[d];
        }
        red[6][wv] = __uint_as_float(nfin);
    }
    __syncthreads();
    const float inv = 1.0f / leaf;
    if (t == 0) {
        uint32_t nf = 0;
        for (int k = 0; k < kFineThreads / 64; ++k) {
            for (int d = 0; d < 3; ++d) {
                mn[d] = fminf(mn[d], red[d][k]);
                mx[d] = fmaxf(mx[d], red[3 + d][k]);
            }
            nf += __float_as_uint(red[6][k]);
        }
        int overflow = 0;
        double prod = 1.0;
        for (int d = 0; d < 3; ++d) {
            const float e = (mx[d] - mn[d]) * inv;
            if (!(e < 9.0e18f)) overflow = 1;
            else prod *= (double)((int64_t)e + 1);
        }
        overflow = overflow || prod > 2147483647.0;
        s_par[0] = overflow;
        s_par[1] = (int)nf;
        for (int d = 0; d < 3 && nf && !overflow; ++d) {
            s_par[2 + d] = (int)floorf(mn[d] * inv);
            s_par[5 + d] = (int)floorf(mx[d] * inv) - s_par[2 + d] + 1;
        }
    }
    __syncthreads();
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
    const int minb0 = s_par[2], minb1 = s_par[3], minb2 = s_par[4];
    const uint32_t div0 = (uint32_t)s_par[5], div1 = (uint32_t)s_par[6];
    const uint32_t mul2 = div0 * div1;
    const uint32_t np2 = rf_pow2(m);
    uint64_t *buf = w.keys + (size_t)g * w.Kn;
    for (uint32_t i = t; i < np2; i += kFineThreads) {
        uint64_t key = ~0ull;
        if (i < m) {
            const bev_point_t &q = src[i];
            if (rf_finite3(q.x, q.y, q.z)) {
                const uint32_t i0 = (uint32_t)(int)(floorf(q.x * inv) - (float)minb0);
                const uint32_t i1 = (uint32_t)(int)(floorf(q.y * inv) - (float)minb1);
                const uint32_t i2 = (uint32_t)(int)(floorf(q.z * inv) - (float)minb2);
                key = ((uint64_t)(i0 + i1 * div0 + i2 * mul2) << 32) | i; /* voxel index modulo 2^32, then input index */
            }
        }
        buf[i] = key;
    }
    __syncthreads();
    rf_bitonic(buf, np2);
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < nf; c0 += kFineThreads) {
        const uint32_t i = c0 + t;
        const bool start = i < nf && (i == 0 || (buf[i] >> 32) != (buf[i - 1] >> 32));
        const uint64_t bal = __ballot(start);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = base;
        for (int q = 0; q < wv; ++q) before += wave_cnt[q];
        before += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (start) vstart[before] = i;
        for (int q = 0; q < kFineThreads / 64; ++q) base += wave_cnt[q];
        __syncthreads();
    }
    const uint32_t nv = base;
    if (t == 0) {
        vstart[nv] = nf;
        w.vox_n[s] = nv;
    }
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
    __shared__ uint32_t cnt[kFineCells];
    __shared__ float red[4][kFineThreads / 64];
    __shared__ uint32_t part[kFineThreads];
    __shared__ IcpGridHdr hdr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = (int)blockIdx.x;
    const uint32_t n = w.vox_n[s];
    const bev_point_t *pts = w.vox + (size_t)s * w.Pn;
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (uint32_t i = tid; i < n; i += kFineThreads) {
        const bev_point_t &p = pts[i];
        if (!icp_finite3(p.x, p.y, p.z)) continue;
        mnx = fminf(mnx, p.x);
        mny = fminf(mny, p.y);
        mxx = fmaxf(mxx, p.x);
        mxy = fmaxf(mxy, p.y);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        mnx = fminf(mnx, __shfl_xor(mnx, off));
        mny = fminf(mny, __shfl_xor(mny, off));
        mxx = fmaxf(mxx, __shfl_xor(mxx, off));
        mxy = fmaxf(mxy, __shfl_xor(mxy, off));
    }
    if (lane == 0) {
        red[0][wave] = mnx;
        red[1][wave] = mny;
        red[2][wave] = mxx;
        red[3][wave] = mxy;
    }
    for (int c = tid; c < kFineCells; c += kFineThreads) cnt[c] = 0;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kFineThreads / 64; ++k) {
            mnx = fminf(mnx, red[0][k]);
            mny = fminf(mny, red[1][k]);
            mxx = fmaxf(mxx, red[2][k]);
            mxy = fmaxf(mxy, red[3][k]);
        }
        IcpGridHdr h{};
        h.nx = h.ny = 1;
        h.s = 1.0f;
        h.inv_s = 0.0f;
        if (mnx <= mxx) {
            h.minx = mnx;
            h.miny = mny;
            h.mag = fmaxf(fmaxf(fabsf(mnx), fabsf(mxx)), fmaxf(fabsf(mny), fabsf(mxy)));
            const float ex = mxx - mnx, ey = mxy - mny;
            const int dim = min(kFineGridMax, max(1, (int)ceilf(sqrtf((float)n))));
            const float sc = fmaxf(ex, ey) / (float)dim;
            if (sc > 0.0f && isfinite(sc) && isfinite(1.0f / sc)) {
                h.s = sc;
                h.inv_s = 1.0f / sc;
                h.nx = min(dim, (int)(ex * h.inv_s) + 1);
                h.ny = min(dim, (int)(ey * h.inv_s) + 1);
            }
        }
        hdr = h;
    }
    __syncthreads();
    const IcpGridHdr h = hdr;
    for (uint32_t i = tid; i < n; i += kFineThreads) {
        const bev_point_t &p = pts[i];
        if (!icp_finite3(p.x, p.y, p.z)) continue;
        atomicAdd(&cnt[icp_cell(p.y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(p.x, h.minx, h.inv_s, h.nx)], 1u);
    }
    __syncthreads();
    constexpr int kPer = kFineCells / kFineThreads;
    const int nc = h.nx * h.ny;
    uint32_t sum = 0;
    for (int k = 0; k < kPer; ++k) sum += tid * kPer + k < nc ? cnt[tid * kPer + k] : 0u;
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kFineThreads; ++k) {
            const uint32_t v = part[k];
            part[k] = run;
            run += v;
        }
        hdr.n = run;
    }
    __syncthreads();
    uint32_t *off = w.cell_off + (size_t)s * (kFineCells + 1);
    uint32_t run = part[tid];
    for (int k = 0; k < kPer; ++k) {
        const int c = tid * kPer + k;
        if (c >= nc) break;
        const uint32_t v = cnt[c];
        off[c] = run;
        cnt[c] = run; /* the cell's cursor */
        run += v;
    }
    if (tid == 0) {
        off[nc] = hdr.n;
        w.hdr[s] = hdr;
    }
    __syncthreads();
    float4 *sorted = w.sorted + (size_t)s * w.Pn;
    for (uint32_t i = tid; i < n; i += kFineThreads) {
        const bev_point_t &p = pts[i];
        if (!icp_finite3(p.x, p.y, p.z)) continue;
        const uint32_t pos =
            atomicAdd(&cnt[icp_cell(p.y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(p.x, h.minx, h.inv_s, h.nx)], 1u);
        sorted[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
    }
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

/* sigma (row-major, finite) -> R (row-major): U S V^T with S = diag(1, 1, +-1) */
__device__ void fine_svd_rotation(const float *sigma, float *R)
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
    float slotf[kIcpChunkSlots][9];
    double slotd[kIcpChunkSlots];
    uint32_t slot_cnt[kIcpChunkSlots];
    float totf[9];
    double totd;
    uint32_t cnt;
    int state, iters;
    float fin[16], inc[16], mean[6];
};

/* one pass over the source: term(i, tf, td) fills NF floats and one double and returns whether point i counts; totals
 * in sh.totf / sh.totd / sh.cnt.  Chunk c of 64 points is reduced by wave c % 4, so point i is thread i % 256's. */
template <int NF, class Term>
__device__ void fine_pass(FineShared &sh, uint32_t n_src, Term term)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nchunks = (n_src + 63) / 64;
    float accf = 0.0f;
    double accd = 0.0;
    uint32_t count = 0;
    for (uint32_t base = 0; base < nchunks; base += kIcpChunkSlots) {
        const uint32_t lim = min(nchunks - base, (uint32_t)kIcpChunkSlots);
        for (uint32_t c = wave; c < lim; c += kFineThreads / 64) {
            const uint32_t i = (base + c) * 64 + lane;
            float tf[NF > 0 ? NF : 1];
            double td = 0.0;
#pragma unroll
            for (int v = 0; v < NF; ++v) tf[v] = 0.0f;
            const bool hit = i < n_src && term(i, tf, td);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                for (int v = 0; v < NF; ++v) tf[v] = tf[v] + __shfl_down(tf[v], off);
                td = td + __shfl_down(td, off);
            }
            const uint32_t hits = (uint32_t)__popcll(__ballot(hit));
            if (lane == 0) {
#pragma unroll
                for (int v = 0; v < NF; ++v) sh.slotf[c][v] = tf[v];
                sh.slotd[c] = td;
                sh.slot_cnt[c] = hits;
            }
        }
        __syncthreads();
        if (tid < NF) {
            for (uint32_t c = 0; c < lim; ++c) accf = (base + c == 0) ? sh.slotf[c][tid] : accf + sh.slotf[c][tid];
        } else if (tid == 32) {
            for (uint32_t c = 0; c < lim; ++c) accd = (base + c == 0) ? sh.slotd[c] : accd + sh.slotd[c];
        } else if (tid == 63) {
            for (uint32_t c = 0; c < lim; ++c) count += sh.slot_cnt[c];
        }
        __syncthreads();
    }
    if (tid < NF) sh.totf[tid] = nchunks ? accf : 0.0f;
    else if (tid == 32) sh.totd = nchunks ? accd : 0.0;
    else if (tid == 63) sh.cnt = count;
    __syncthreads();
}

/* thread 0: sigma, the rotation, the translation, final = inc * final, the convergence test */
__device__ void fine_step(FineShared &sh, const bev_icp_params_t &prm, double &prev)
{
    const float oon = 1.0f / (float)sh.cnt;
    float sigma[9];
    bool finite = true;
    for (int k = 0; k < 9; ++k) {
        sigma[k] = oon * sh.totf[k];
        finite = finite && isfinite(sigma[k]);
    }
    float *I = sh.inc;
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
    float F[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            F[i * 4 + j] = ((I[i * 4] * sh.fin[j] + I[i * 4 + 1] * sh.fin[4 + j]) + I[i * 4 + 2] * sh.fin[8 + j]) +
                           I[i * 4 + 3] * sh.fin[12 + j];
    for (int k = 0; k < 16; ++k) sh.fin[k] = F[k];
    const int it = ++sh.iters;
    const double cos_angle = 0.5 * (double)(((I[0] + I[5]) + I[10]) - 1.0f);
    const double trans2 = (double)((I[3] * I[3] + I[7] * I[7]) + I[11] * I[11]);
    if (it >= prm.max_iterations) {
        sh.state = 1; /* ITERATIONS */
    } else if (cos_angle >= 1.0 - prm.transformation_epsilon && trans2 <= prm.transformation_epsilon) {
        sh.state = 2; /* TRANSFORM */
    } else {
        const double mse = sh.totd / (double)sh.cnt;
        if (fabs(mse - prev) < 1e-12) sh.state = 3;                                      /* ABS_MSE */
        else if (fabs(mse - prev) / prev < prm.euclidean_fitness_epsilon) sh.state = 4; /* REL_MSE */
        else prev = mse;
    }
}

__global__ __launch_bounds__(kFineThreads) void k_fine_icp(const FineProblem *probs, FineWork w,
                                                           const bev_icp_result_t *coarse, const int32_t *best,
                                                           bev_icp_params_t prm, bev_icp_result_t *results)
{
    __shared__ FineShared sh;
    const int tid = threadIdx.x;
    const FineProblem pb = probs[blockIdx.x];
    const uint32_t n_src = w.vox_n[pb.src_slot];
    const bev_point_t *src = w.vox + (size_t)pb.src_slot * w.Pn;
    const bev_point_t *tgt = w.vox + (size_t)pb.tgt_slot * w.Pn;
    const float4 *tpts = w.sorted + (size_t)pb.tgt_slot * w.Pn;
    const uint32_t *toff = w.cell_off + (size_t)pb.tgt_slot * (kFineCells + 1);
    const IcpGridHdr h = w.hdr[pb.tgt_slot];
    float4 *cur = w.cur + (size_t)(blockIdx.x % kFineProblemsPerLaunch) * w.Pn;
    uint32_t *corr = w.corr + (size_t)(blockIdx.x % kFineProblemsPerLaunch) * w.Pn;
    float G[16];
    if (pb.coarse_match != 0xffffffffu) { /* the better coarse result of the match (top-part tool) */
        const uint32_t m = pb.coarse_match;
        const bev_icp_result_t &r = coarse[2 * (size_t)m + (best[m] ? 1 : 0)];
        for (int k = 0; k < 16; ++k) G[k] = r.T[k];
    } else {
        for (int k = 0; k < 16; ++k) G[k] = pb.guess[k];
    }
    if (tid == 0) {
        sh.state = 0;
        sh.iters = 0;
    }
    if (tid < 16) sh.fin[tid] = G[tid];
    bool identity = true;
    for (int k = 0; k < 16; ++k) identity &= G[k] == ((k % 5 == 0) ? 1.0f : 0.0f);
    for (uint32_t i = tid; i < n_src; i += kFineThreads) {
        const bev_point_t &p = src[i];
        const float3 q = identity ? make_float3(p.x, p.y, p.z) : icp_se3(G, p.x, p.y, p.z);
        cur[i] = make_float4(q.x, q.y, q.z, 0.0f);
    }
    __syncthreads();
    const double D2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    double prev = 1.7976931348623157e308; /* DBL_MAX (thread 0's copy is the one used) */
    while (true) {
        /* pass 1: correspondences, the source and target coordinate sums (float), the MSE (double) */
        fine_pass<6>(sh, n_src, [&](uint32_t i, float *t, double &td) -> bool {
            const float4 s = cur[i];
            uint32_t j = 0xffffffffu;
            float d;
            if (!icp_finite3(s.x, s.y, s.z) || !icp_nn(h, toff, tpts, s.x, s.y, s.z, D2, d, j) || !((double)d <= D2)) {
                corr[i] = 0xffffffffu;
                return false;
            }
            corr[i] = j;
            const bev_point_t &tp = tgt[j];
            t[0] = s.x;
            t[1] = s.y;
            t[2] = s.z;
            t[3] = tp.x;
            t[4] = tp.y;
            t[5] = tp.z;
            td = (double)d;
            return true;
        });
        if (tid == 0) {
            if (sh.cnt < 3) {
                sh.state = 5; /* NO_CORRESPONDENCES */
            } else {
                const float oon = 1.0f / (float)sh.cnt;
                for (int k = 0; k < 6; ++k) sh.mean[k] = sh.totf[k] * oon;
            }
        }
        __syncthreads();
        if (sh.state != 0) break;
        const double mse_sum = sh.totd;
        float M[6];
        for (int k = 0; k < 6; ++k) M[k] = sh.mean[k];
        /* pass 2: sigma's nine products dst_demean[a] * src_demean[b] (float) */
        fine_pass<9>(sh, n_src, [&](uint32_t i, float *t, double &) -> bool {
            const uint32_t j = corr[i];
            if (j == 0xffffffffu) return false;
            const float4 s = cur[i];
            const bev_point_t &tp = tgt[j];
            const float sd[3] = {s.x - M[0], s.y - M[1], s.z - M[2]};
            const float dd[3] = {tp.x - M[3], tp.y - M[4], tp.z - M[5]};
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) t[a * 3 + b] = dd[a] * sd[b];
            return true;
        });
        if (tid == 0) {
            sh.totd = mse_sum; /* (pass 2 counted the same correspondences) */
            fine_step(sh, prm, prev);
        }
        __syncthreads();
        if (sh.state != 0) break;
        float I[12];
        for (int k = 0; k < 12; ++k) I[k] = sh.inc[k];
        for (uint32_t i = tid; i < n_src; i += kFineThreads) {
            const float4 p = cur[i];
            const float3 q = icp_se3(I, p.x, p.y, p.z);
            cur[i] = make_float4(q.x, q.y, q.z, 0.0f);
        }
    }
    float F[16];
    for (int k = 0; k < 16; ++k) F[k] = sh.fin[k];
    fine_pass<0>(sh, n_src, [&](uint32_t i, float *, double &td) -> bool {
        const bev_point_t &p = src[i];
        const float3 q = icp_se3(F, p.x, p.y, p.z);
        if (!icp_finite3(q.x, q.y, q.z)) return false;
        float d;
        uint32_t j;
        if (!icp_nn(h, toff, tpts, q.x, q.y, q.z, INFINITY, d, j) || !isfinite(d)) return false;
        td = (double)d;
        return true;
    });
    if (tid == 0) {
        bev_icp_result_t r{};
        for (int k = 0; k < 16; ++k) r.T[k] = isnan(F[k]) ? __uint_as_float(0x7fc00000u) : F[k];
        r.fitness = sh.cnt ? sh.totd / (double)sh.cnt : 1.7976931348623157e308;
        if (isnan(r.fitness)) r.fitness = bevx::f64_qnan();
        r.iterations = sh.iters;
        r.state = sh.state;
        r.converged = sh.state >= 1 && sh.state <= 4;
        results[pb.result] = r;
    }
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
