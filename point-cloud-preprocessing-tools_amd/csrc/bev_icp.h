/*
 * bev_icp.h — coarse point-to-plane ICP (included by bev_kernels.hip): pcl::IterativeClosestPointWithNormals<PointNormal,
 * PointNormal> as performCoarseIcp runs it (BatchTopPartRegistration.cpp:192-221), on the registration front end's
 * PointNormal clouds.  The contract every line follows (and tests/icp/icp_oracle.c restates) is DESIGN.md §6c.
 *
 *   k_icp_grid   per target frame : bounds of the searchable points (finite x, y, z), a uniform 2-D grid of at most
 *                                   kIcpGridMax^2 square cells, a counting sort of the points by cell (x, y, z, index)
 *   k_icp        per problem      : the whole ICP loop of one (match, guess) in one workgroup — correspondences, the
 *                                   27 LLS sums and the MSE in the pinned order, the 6 x 6 solve, the increment,
 *                                   convergence — then getFitnessScore
 *   k_icp_best   per match        : guess 0 iff fitness0 < fitness1
 *
 * Exact 1-NN: ring search on the grid, lowest index on equal distance.  The grid is only an accelerator: the order of the
 * points inside a cell (an atomic) changes nothing, and a ring is skipped only when a lower bound on the xy distance of
 * every point in it, taken with a wide margin for rounding, exceeds the best distance (or D^2).  No float or double sum
 * depends on an atomic: every sum runs over 64-point chunks as a fixed tree (wave shuffles), the chunks in ascending
 * order in one lane.  Point i of the source is transformed, read and written by thread i % 256 only.
 */
#pragma once

#include "bev_libm_f64.h"

namespace bevk {

__device__ __forceinline__ bool icp_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

/* cell coordinate: monotone in v, so cell boundaries are ordered (the ring bound relies on that alone) */
__device__ __forceinline__ int icp_cell(float v, float mn, float inv, int n)
{
    float t = (v - mn) * inv;
    t = fminf(fmaxf(t, 0.0f), (float)(n - 1)); /* (fmaxf drops the NaN of inf * 0) */
    return (int)t;
}

/* Transformer::se3 over rows 0..2 of a row-major 4 x 4 */
__device__ __forceinline__ float3 icp_se3(const float *T, float x, float y, float z)
{
    return make_float3(T[0] * x + (T[1] * y + (T[2] * z + T[3])), T[4] * x + (T[5] * y + (T[6] * z + T[7])),
                       T[8] * x + (T[9] * y + (T[10] * z + T[11])));
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_grid(const float *pn, size_t stride, const uint32_t *counts,
                                                          const uint32_t *slot_frame, IcpWork w)
{
    __shared__ uint32_t cnt[kIcpCells];
    __shared__ float red[4][4];
    __shared__ uint32_t part[kIcpThreads];
    __shared__ IcpGridHdr hdr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t frame = slot_frame[blockIdx.x];
    const uint32_t n = min(counts[frame], (uint32_t)stride);
    const float *pts = pn + (size_t)frame * stride * 12;
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (uint32_t i = tid; i < n; i += kIcpThreads) {
        const float4 p = *reinterpret_cast<const float4 *>(pts + (size_t)i * 12);
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
        red[wave][0] = mnx;
        red[wave][1] = mny;
        red[wave][2] = mxx;
        red[wave][3] = mxy;
    }
    for (int c = tid; c < kIcpCells; c += kIcpThreads) cnt[c] = 0;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) {
            mnx = fminf(mnx, red[k][0]);
            mny = fminf(mny, red[k][1]);
            mxx = fmaxf(mxx, red[k][2]);
            mxy = fmaxf(mxy, red[k][3]);
        }
        IcpGridHdr h{};
        h.nx = h.ny = 1;
        h.s = 1.0f;
        h.inv_s = 0.0f;
        if (mnx <= mxx) { /* some searchable point */
            h.minx = mnx;
            h.miny = mny;
            h.mag = fmaxf(fmaxf(fabsf(mnx), fabsf(mxx)), fmaxf(fabsf(mny), fabsf(mxy)));
            const float ex = mxx - mnx, ey = mxy - mny;
            const int dim = min(kIcpGridMax, max(1, (int)ceilf(sqrtf((float)n))));
            const float s = fmaxf(ex, ey) / (float)dim;
            if (s > 0.0f && isfinite(s) && isfinite(1.0f / s)) {
                h.s = s;
                h.inv_s = 1.0f / s;
                h.nx = min(dim, (int)(ex * h.inv_s) + 1);
                h.ny = min(dim, (int)(ey * h.inv_s) + 1);
            }
        }
        hdr = h;
    }
    __syncthreads();
    const IcpGridHdr h = hdr;
    for (uint32_t i = tid; i < n; i += kIcpThreads) {
        const float4 p = *reinterpret_cast<const float4 *>(pts + (size_t)i * 12);
        if (!icp_finite3(p.x, p.y, p.z)) continue;
        atomicAdd(&cnt[icp_cell(p.y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(p.x, h.minx, h.inv_s, h.nx)], 1u);
    }
    __syncthreads();
    /* exclusive scan of the nx * ny counts: 16 cells per thread, then the 256 partial sums in one lane */
    constexpr int kPer = kIcpCells / kIcpThreads;
    const int nc = h.nx * h.ny;
    uint32_t sum = 0;
    for (int k = 0; k < kPer; ++k) sum += tid * kPer + k < nc ? cnt[tid * kPer + k] : 0u;
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kIcpThreads; ++k) {
            const uint32_t v = part[k];
            part[k] = run;
            run += v;
        }
        hdr.n = run;
    }
    __syncthreads();
    uint32_t *off = w.cell_off + (size_t)blockIdx.x * (kIcpCells + 1);
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
        w.hdr[blockIdx.x] = hdr;
    }
    __syncthreads();
    float4 *sorted = w.sorted + (size_t)blockIdx.x * stride;
    for (uint32_t i = tid; i < n; i += kIcpThreads) {
        const float4 p = *reinterpret_cast<const float4 *>(pts + (size_t)i * 12);
        if (!icp_finite3(p.x, p.y, p.z)) continue;
        const uint32_t pos =
            atomicAdd(&cnt[icp_cell(p.y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(p.x, h.minx, h.inv_s, h.nx)], 1u);
        sorted[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
    }
}

/* the nearest searchable point of q: lowest index on equal float distance ((dx^2 + dy^2) + dz^2).  lim2: no interest in
 * points whose distance exceeds it (the search may then stop early).  false: the grid has no searchable point */
__device__ bool icp_nn(const IcpGridHdr &h, const uint32_t *off, const float4 *pts, float qx, float qy, float qz,
                       double lim2, float &best, uint32_t &bi)
{
    best = INFINITY;
    bi = 0xffffffffu;
    if (h.n == 0) return false;
    const int qcx = icp_cell(qx, h.minx, h.inv_s, h.nx), qcy = icp_cell(qy, h.miny, h.inv_s, h.ny);
    const int maxr = max(max(qcx, h.nx - 1 - qcx), max(qcy, h.ny - 1 - qcy));
    const double s = h.s, margin = 1e-4 * s + 1e-6 * (double)h.mag;
    for (int r = 0; r <= maxr; ++r) {
        if (r >= 2) {
            /* a point r rings out is more than the width of r - 1 cells away in x or y */
            const double lb = (double)(r - 1) * s - ((double)r * s * 1e-5 + margin);
            if (lb > 0.0) {
                const double lb2 = lb * lb * (1.0 - 1e-5);
                if ((bi != 0xffffffffu && lb2 > (double)best) || lb2 > lim2) break;
            }
        }
        const int y0 = max(qcy - r, 0), y1 = min(qcy + r, h.ny - 1);
        for (int cy = y0; cy <= y1; ++cy) {
            const bool full = cy == qcy - r || cy == qcy + r;
            const int xa = max(qcx - r, 0), xb = min(qcx + r, h.nx - 1);
            const int step = full ? 1 : 2 * r;
            for (int cx = full ? xa : qcx - r; cx <= (full ? xb : qcx + r); cx += step) {
                if (cx < 0 || cx >= h.nx) continue;
                const int c = cy * h.nx + cx;
                for (uint32_t k = off[c], e = off[c + 1]; k < e; ++k) {
                    const float4 p = pts[k];
                    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    const uint32_t j = __float_as_uint(p.w);
                    if (d < best || (d == best && j < bi)) {
                        best = d;
                        bi = j;
                    }
                }
            }
        }
    }
    return bi != 0xffffffffu;
}

struct IcpShared {
    double slot[kIcpChunkSlots][28];
    uint32_t slot_cnt[kIcpChunkSlots];
    double tot[28];
    uint32_t cnt;
    int state, iters;
    float fin[16], inc[16];
    IcpGridHdr hdr;
    uint32_t off[kIcpCells + 1];
};

/* one pass over the source: term(i, t) fills NV doubles and returns whether point i counts; totals in sh.tot / sh.cnt */
template <int NV, class Term>
__device__ void icp_pass(IcpShared &sh, uint32_t n_src, Term term)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nchunks = (n_src + 63) / 64;
    double acc = 0.0;
    uint32_t count = 0;
    for (uint32_t base = 0; base < nchunks; base += kIcpChunkSlots) {
        const uint32_t lim = min(nchunks - base, (uint32_t)kIcpChunkSlots);
        for (uint32_t c = wave; c < lim; c += kIcpThreads / 64) {
            const uint32_t i = (base + c) * 64 + lane;
            double t[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) t[v] = 0.0;
            const bool hit = i < n_src && term(i, t);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                for (int v = 0; v < NV; ++v) t[v] = t[v] + __shfl_down(t[v], off);
            }
            const uint32_t hits = (uint32_t)__popcll(__ballot(hit));
            if (lane == 0) {
#pragma unroll
                for (int v = 0; v < NV; ++v) sh.slot[c][v] = t[v];
                sh.slot_cnt[c] = hits;
            }
        }
        __syncthreads();
        if (tid < NV) {
            for (uint32_t c = 0; c < lim; ++c) acc = (base + c == 0) ? sh.slot[c][tid] : acc + sh.slot[c][tid];
        } else if (tid == 63) {
            for (uint32_t c = 0; c < lim; ++c) count += sh.slot_cnt[c];
        }
        __syncthreads();
    }
    if (tid < NV) sh.tot[tid] = acc;
    else if (tid == 63) sh.cnt = count;
    __syncthreads();
}

/* thread 0: the 6 x 6 solve, the increment, final = inc * final, the convergence test */
__device__ void icp_step(IcpShared &sh, const bev_icp_params_t &prm, double &prev)
{
    double M[6][6], v[6], x[6];
    bool ok[6];
    {
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) M[a][b] = M[b][a] = sh.tot[k++];
        for (int a = 0; a < 6; ++a) v[a] = sh.tot[21 + a];
    }
    for (int k = 0; k < 6; ++k) {
        ok[k] = M[k][k] > 0.0;
        if (!ok[k]) continue;
        for (int i = k + 1; i < 6; ++i) {
            const double f = M[i][k] / M[k][k];
            for (int j = k + 1; j < 6; ++j) M[i][j] -= f * M[k][j];
            v[i] -= f * v[k];
        }
    }
    for (int k = 5; k >= 0; --k) {
        if (!ok[k]) {
            x[k] = 0.0;
            continue;
        }
        double s = v[k];
        for (int j = k + 1; j < 6; ++j) s -= M[k][j] * x[j];
        x[k] = s / M[k][k];
    }
    /* constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz) */
    const double sa = bevx::fd_sin(x[0]), ca = bevx::fd_cos(x[0]), sb = bevx::fd_sin(x[1]), cb = bevx::fd_cos(x[1]);
    const double sg = bevx::fd_sin(x[2]), cg = bevx::fd_cos(x[2]);
    float *I = sh.inc;
    I[0] = (float)(cg * cb);
    I[1] = (float)(-sg * ca + cg * sb * sa);
    I[2] = (float)(sg * sa + cg * sb * ca);
    I[3] = (float)x[3];
    I[4] = (float)(sg * cb);
    I[5] = (float)(cg * ca + sg * sb * sa);
    I[6] = (float)(-cg * sa + sg * sb * ca);
    I[7] = (float)x[4];
    I[8] = (float)(-sb);
    I[9] = (float)(cb * sa);
    I[10] = (float)(cb * ca);
    I[11] = (float)x[5];
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
    /* DefaultConvergenceCriteria::hasConverged; Eigen sums the float entries in float */
    const double cos_angle = 0.5 * (double)(((I[0] + I[5]) + I[10]) - 1.0f);
    const double trans2 = (double)((I[3] * I[3] + I[7] * I[7]) + I[11] * I[11]);
    if (it >= prm.max_iterations) {
        sh.state = 1; /* ITERATIONS */
    } else if (cos_angle >= 1.0 - prm.transformation_epsilon && trans2 <= prm.transformation_epsilon) {
        sh.state = 2; /* TRANSFORM */
    } else {
        const double mse = sh.tot[27] / (double)sh.cnt;
        if (fabs(mse - prev) < 1e-12) sh.state = 3;                                        /* ABS_MSE */
        else if (fabs(mse - prev) / prev < prm.euclidean_fitness_epsilon) sh.state = 4;   /* REL_MSE */
        else prev = mse;
    }
}

__global__ __launch_bounds__(kIcpThreads) void k_icp(const float *pn, size_t stride, const uint32_t *counts,
                                                     const IcpProblem *probs, IcpWork w, bev_icp_params_t prm,
                                                     bev_icp_result_t *results)
{
    __shared__ IcpShared sh;
    const int tid = threadIdx.x;
    const IcpProblem pb = probs[blockIdx.x];
    const uint32_t n_src = min(counts[pb.src_frame], (uint32_t)stride);
    const float *src = pn + (size_t)pb.src_frame * stride * 12;
    const float *tgt = pn + (size_t)pb.tgt_frame * stride * 12;
    const float4 *tpts = w.sorted + (size_t)pb.tgt_slot * stride;
    float4 *cur = w.cur + (size_t)(blockIdx.x % kIcpProblemsPerLaunch) * stride;
    if (tid == 0) {
        sh.hdr = w.hdr[pb.tgt_slot];
        sh.state = 0;
        sh.iters = 0;
    }
    if (tid < 16) sh.fin[tid] = pb.guess[tid];
    __syncthreads();
    const IcpGridHdr h = sh.hdr;
    const uint32_t *goff = w.cell_off + (size_t)pb.tgt_slot * (kIcpCells + 1);
    for (int c = tid; c <= h.nx * h.ny; c += kIcpThreads) sh.off[c] = goff[c];
    bool identity = true;
    for (int k = 0; k < 16; ++k) identity &= pb.guess[k] == ((k % 5 == 0) ? 1.0f : 0.0f);
    for (uint32_t i = tid; i < n_src; i += kIcpThreads) {
        const float4 p = *reinterpret_cast<const float4 *>(src + (size_t)i * 12);
        const float3 q = identity ? make_float3(p.x, p.y, p.z) : icp_se3(pb.guess, p.x, p.y, p.z);
        cur[i] = make_float4(q.x, q.y, q.z, 0.0f);
    }
    __syncthreads();
    const double D2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    double prev = 1.7976931348623157e308; /* DBL_MAX (thread 0's copy is the one used) */
    while (true) {
        icp_pass<28>(sh, n_src, [&](uint32_t i, double *t) -> bool {
            const float4 s = cur[i];
            if (!icp_finite3(s.x, s.y, s.z)) return false;
            float d;
            uint32_t j;
            if (!icp_nn(h, sh.off, tpts, s.x, s.y, s.z, D2, d, j) || !((double)d <= D2)) return false;
            const float4 tp = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12);
            const float4 tn = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12 + 4);
            const float nx = tn.x, ny = tn.y, nz = tn.z;
            if (icp_finite3(nx, ny, nz)) {
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
            if (sh.cnt < 3) sh.state = 5; /* NO_CORRESPONDENCES */
            else icp_step(sh, prm, prev);
        }
        __syncthreads();
        if (sh.state != 0) break;
        float I[12];
        for (int k = 0; k < 12; ++k) I[k] = sh.inc[k];
        for (uint32_t i = tid; i < n_src; i += kIcpThreads) {
            const float4 p = cur[i];
            const float3 q = icp_se3(I, p.x, p.y, p.z);
            cur[i] = make_float4(q.x, q.y, q.z, 0.0f);
        }
        /* (the next pass begins with LDS writes that no thread still reads: sh.inc is rewritten after its barrier) */
    }
    float F[16];
    for (int k = 0; k < 16; ++k) F[k] = sh.fin[k];
    icp_pass<1>(sh, n_src, [&](uint32_t i, double *t) -> bool {
        const float4 p = *reinterpret_cast<const float4 *>(src + (size_t)i * 12);
        const float3 q = icp_se3(F, p.x, p.y, p.z);
        if (!icp_finite3(q.x, q.y, q.z)) return false;
        float d;
        uint32_t j;
        if (!icp_nn(h, sh.off, tpts, q.x, q.y, q.z, INFINITY, d, j) || !isfinite(d)) return false;
        t[0] = (double)d;
        return true;
    });
    if (tid == 0) {
        bev_icp_result_t r{};
        for (int k = 0; k < 16; ++k) r.T[k] = isnan(F[k]) ? __uint_as_float(0x7fc00000u) : F[k];
        r.fitness = sh.cnt ? sh.tot[0] / (double)sh.cnt : 1.7976931348623157e308;
        if (isnan(r.fitness)) r.fitness = bevx::f64_qnan();
        r.iterations = sh.iters;
        r.state = sh.state;
        r.converged = sh.state >= 1 && sh.state <= 4;
        results[pb.result] = r;
    }
}

__global__ void k_icp_best(const bev_icp_result_t *res, int n_matches, int32_t *best)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < n_matches) best[m] = res[2 * m].fitness < res[2 * m + 1].fitness ? 0 : 1;
}

void launch_icp_grid(const float *pn, size_t stride, const uint32_t *counts, const uint32_t *slot_frame, int n_slots,
                     const IcpWork &w, hipStream_t st)
{
    if (n_slots > 0) hipLaunchKernelGGL(k_icp_grid, dim3(n_slots), dim3(kIcpThreads), 0, st, pn, stride, counts, slot_frame, w);
}

void launch_icp(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                const IcpWork &w, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_icp, dim3(n), dim3(kIcpThreads), 0, st, pn, stride, counts, probs, w, prm, results);
}

void launch_icp_best(const bev_icp_result_t *res, int n_matches, int32_t *best, hipStream_t st)
{
    if (n_matches > 0) hipLaunchKernelGGL(k_icp_best, dim3((n_matches + 255) / 256), dim3(256), 0, st, res, n_matches, best);
}

} /* namespace bevk */
