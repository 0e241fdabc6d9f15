/*
 * bev_reg_common.h — what the registration stages share (included by bev_kernels.hip before bev_regfront.h, bev_icp.h and
 * bev_fine.h):
 *
 *   helpers        finite3, rf_canon, icp_cell, icp_se3, rf_pow2, rf_bitonic; SubregPts / IcpRows: a point's position in a
 *                  float4 array, in PointNormal rows
 *   voxel grid     rf_voxel_bounds / rf_voxel_keys / rf_voxel_starts: the three steps of pcl::VoxelGrid that k_rf_voxel
 *                  (PointXYZ), k_fine_voxel (PointXYZIRCT) and the union grids of the scan-to-map calls have in common, and
 *                  rf_voxel_centroids, the x y z centroids of all but k_fine_voxel; sort buffer and outputs are theirs
 *   search grid    reg_grid_build<kCells>: bounds, header, counts, scan and counting sort of a target cloud (k_icp_grid,
 *                  k_fine_grid and the scan-to-map targets), and icp_nn, the exact 1-NN on it
 *   ordered pass   RegSums<NF, ND> / reg_pass: the pinned summation order of every sum over a source cloud
 *   loop           RegLoop / reg_start / reg_advance / reg_converge / reg_finish: what k_icp and k_fine_icp do around
 *                  their own estimators
 *
 * Every workgroup of these kernels has 256 threads (kRfThreads = kIcpThreads = kFineThreads).
 */
#pragma once

#include "bev_libm_f64.h"

namespace bevk {

constexpr int kRegThreads = 256, kRegWaves = kRegThreads / 64;
static_assert(kRfThreads == kRegThreads && kIcpThreads == kRegThreads && kFineThreads == kRegThreads, "one workgroup shape");

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

/* where a cloud's positions lie, one functor per layout (bev_fine.h has the 32-byte records' FinePts): float4 points ... */
struct SubregPts {
    const float4 *pts;
    __device__ float3 operator()(uint32_t i) const
    {
        const float4 p = pts[i];
        return make_float3(p.x, p.y, p.z);
    }
};
/* ... and PointNormal rows of 12 floats */
struct IcpRows {
    const float *rows;
    __device__ float3 operator()(uint32_t i) const
    {
        const float4 p = *reinterpret_cast<const float4 *>(rows + (size_t)i * 12);
        return make_float3(p.x, p.y, p.z);
    }
};

/* every NaN as the one quiet NaN the checkers write */
__device__ __forceinline__ float rf_canon(float f) { return isnan(f) ? __uint_as_float(0x7fc00000u) : f; }

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

__device__ __forceinline__ uint32_t rf_pow2(uint32_t n)
{
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

/* ascending bitonic sort of np2 (a power of two) keys by the whole workgroup; buf is LDS or global memory (a workgroup's
 * global writes are visible to its other waves after the barrier: they share the CU's vector cache) */
__device__ void rf_bitonic(uint64_t *buf, uint32_t np2)
{
    for (uint32_t k = 2; k <= np2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < np2; i += blockDim.x) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t a = buf[i], b = buf[l];
                    if ((a > b) == ((i & k) == 0)) {
                        buf[i] = b;
                        buf[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

/* ---- voxel grid: pcl::VoxelGrid::applyFilter up to the voxel starts ------------------------------------------------------ */
/* getMinMax3D over the finite points of fetch(0 .. m - 1) and the overflow test -> s_par[8]: overflow, finite points,
 * minb xyz, div xyz (the last six only where there is a finite point and no overflow).  min / max / integer adds are
 * order-free but for the sign of a zero bound, which no consumer sees: floorf(mn * inv) cast to int, (mx - mn) * inv.
 * red: 7 * kRegWaves floats of LDS, free again on return; the workgroup is in step on return. */
template <class Fetch>
__device__ void rf_voxel_bounds(uint32_t m, Fetch fetch, float inv, float *red, int *s_par)
{
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nfin = 0;
    for (uint32_t i = t; i < m; i += kRegThreads) {
        const float3 q = fetch(i);
        if (!finite3(q.x, q.y, q.z)) continue;
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
            red[d * kRegWaves + wv] = mn[d];
            red[(3 + d) * kRegWaves + wv] = mx[d];
        }
        red[6 * kRegWaves + wv] = __uint_as_float(nfin);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t nf = 0;
        for (int k = 0; k < kRegWaves; ++k) {
            for (int d = 0; d < 3; ++d) {
                mn[d] = fminf(mn[d], red[d * kRegWaves + k]);
                mx[d] = fmaxf(mx[d], red[(3 + d) * kRegWaves + k]);
            }
            nf += __float_as_uint(red[6 * kRegWaves + k]);
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
}

/* buf[0 .. np2): (voxel index modulo 2^32) << 32 | input index of the finite points, ~0 for the others and the padding */
template <class Fetch>
__device__ void rf_voxel_keys(uint32_t m, uint32_t np2, Fetch fetch, float inv, const int *s_par, uint64_t *buf)
{
    const int minb0 = s_par[2], minb1 = s_par[3], minb2 = s_par[4];
    const uint32_t div0 = (uint32_t)s_par[5], div1 = (uint32_t)s_par[6];
    const uint32_t mul2 = div0 * div1;
    for (uint32_t i = threadIdx.x; i < np2; i += kRegThreads) {
        uint64_t key = ~0ull;
        if (i < m) {
            const float3 q = fetch(i);
            if (finite3(q.x, q.y, q.z)) {
                const uint32_t i0 = (uint32_t)(int)(floorf(q.x * inv) - (float)minb0);
                const uint32_t i1 = (uint32_t)(int)(floorf(q.y * inv) - (float)minb1);
                const uint32_t i2 = (uint32_t)(int)(floorf(q.z * inv) - (float)minb2);
                key = ((uint64_t)(i0 + i1 * div0 + i2 * mul2) << 32) | i;
            }
        }
        buf[i] = key;
    }
    __syncthreads();
}

/* voxel starts: an exclusive scan of "first key of its voxel" over the nf sorted keys, 256 at a time.  vstart[v] = the
 * first key of voxel v, vstart[nv] = nf; on_start(v, i) for every start; returns nv.  wave_cnt: kRegWaves words of LDS. */
template <class OnStart>
__device__ uint32_t rf_voxel_starts(const uint64_t *buf, uint32_t nf, uint32_t *wave_cnt, uint32_t *vstart, OnStart on_start)
{
    const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < nf; c0 += kRegThreads) {
        const uint32_t i = c0 + t;
        const bool start = i < nf && (i == 0 || (buf[i] >> 32) != (buf[i - 1] >> 32));
        const uint64_t bal = __ballot(start);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = base;
        for (int q = 0; q < wv; ++q) before += wave_cnt[q];
        before += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (start) {
            vstart[before] = i;
            on_start(before, i);
        }
        for (int q = 0; q < kRegWaves; ++q) base += wave_cnt[q];
        __syncthreads();
    }
    if (t == 0) vstart[base] = nf;
    return base;
}

/* the nv centroids (AccumulatorXYZ; k_fine_voxel's loop also sums intensity and votes labels): one lane per voxel, x, y, z
 * of point(input index) summed in key order, that is ascending input index, divided by float(count) */
template <class Point>
__device__ __forceinline__ void rf_voxel_centroids(const uint64_t *buf, const uint32_t *vstart, uint32_t nv, Point point,
                                                   float4 *out)
{
    for (uint32_t v = threadIdx.x; v < nv; v += kRegThreads) {
        const uint32_t a = vstart[v], b = vstart[v + 1];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        for (uint32_t q = a; q < b; ++q) {
            const float4 s = point((uint32_t)buf[q]);
            sx += s.x;
            sy += s.y;
            sz += s.z;
        }
        const float cf = (float)(b - a);
        out[v] = make_float4(sx / cf, sy / cf, sz / cf, 0.0f);
    }
}

constexpr int reg_isqrt(int n)
{
    int r = 0;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

/* ---- the 2-D search grid of a target cloud ------------------------------------------------------------------------------- */
/* over the searchable points (finite x, y, z) of fetch(0 .. n - 1): bounds, a uniform grid of at most dim x dim square
 * cells, dim = min(sqrt(kCells), ceil(sqrt(n))), and a counting sort of the points by cell (x, y, z, index bits).  Inlined
 * by force: several kernels share an instantiation, and each keeps the code it had as the only caller */
template <int kCells, class Fetch>
__device__ __forceinline__ void reg_grid_build(uint32_t n, Fetch fetch, IcpGridHdr *hdr_out, uint32_t *off_out, float4 *sorted_out)
{
    constexpr int kGridMax = reg_isqrt(kCells); /* kIcpGridMax, kFineGridMax */
    static_assert(kGridMax * kGridMax == kCells && kCells % kRegThreads == 0, "a square grid, whole cells per thread");
    __shared__ uint32_t cnt[kCells];
    __shared__ float red[4][kRegWaves];
    __shared__ uint32_t part[kRegThreads];
    __shared__ IcpGridHdr hdr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (uint32_t i = tid; i < n; i += kRegThreads) {
        const float3 p = fetch(i);
        if (!finite3(p.x, p.y, p.z)) continue;
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
    for (int c = tid; c < kCells; c += kRegThreads) cnt[c] = 0;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kRegWaves; ++k) {
            mnx = fminf(mnx, red[0][k]);
            mny = fminf(mny, red[1][k]);
            mxx = fmaxf(mxx, red[2][k]);
            mxy = fmaxf(mxy, red[3][k]);
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
            const int dim = min(kGridMax, max(1, (int)ceilf(sqrtf((float)n))));
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
    for (uint32_t i = tid; i < n; i += kRegThreads) {
        const float3 p = fetch(i);
        if (!finite3(p.x, p.y, p.z)) continue;
        atomicAdd(&cnt[icp_cell(p.y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(p.x, h.minx, h.inv_s, h.nx)], 1u);
    }
    __syncthreads();
    /* exclusive scan of the nx * ny counts: kPer cells per thread, then the 256 partial sums in one lane */
    constexpr int kPer = kCells / kRegThreads;
    const int nc = h.nx * h.ny;
    uint32_t sum = 0;
    for (int k = 0; k < kPer; ++k) sum += tid * kPer + k < nc ? cnt[tid * kPer + k] : 0u;
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < kRegThreads; ++k) {
            const uint32_t v = part[k];
            part[k] = run;
            run += v;
        }
        hdr.n = run;
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (int k = 0; k < kPer; ++k) {
        const int c = tid * kPer + k;
        if (c >= nc) break;
        const uint32_t v = cnt[c];
        off_out[c] = run;
        cnt[c] = run; /* the cell's cursor */
        run += v;
    }
    if (tid == 0) {
        off_out[nc] = hdr.n;
        *hdr_out = hdr;
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kRegThreads) {
        const float3 p = fetch(i);
        if (!finite3(p.x, p.y, p.z)) continue;
        const uint32_t pos =
            atomicAdd(&cnt[icp_cell(p.y, h.miny, h.inv_s, h.ny) * h.nx + icp_cell(p.x, h.minx, h.inv_s, h.nx)], 1u);
        sorted_out[pos] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
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

/* ---- the ordered pass over a source cloud -------------------------------------------------------------------------------- */
/* chunk sums and totals of up to NF floats and ND doubles (an empty array keeps one element) */
template <int NF, int ND>
struct RegSums {
    static constexpr int kF = NF, kD = ND;
    float slotf[kIcpChunkSlots][NF > 0 ? NF : 1];
    double slotd[kIcpChunkSlots][ND > 0 ? ND : 1];
    uint32_t slot_cnt[kIcpChunkSlots];
    float totf[NF > 0 ? NF : 1];
    double totd[ND > 0 ? ND : 1];
    uint32_t cnt;
};

/* one pass over the source: term(i, tf, td) fills NF floats and ND doubles (zero on entry) and returns whether point i
 * counts; totals in sh.totf / sh.totd / sh.cnt.  The order of every sum is pinned: chunk c of 64
 * points is a shuffle tree 32 -> 1 in wave c % 4 (so point i is thread i % 256's), the chunk sums are added in ascending
 * order in one lane per value, the first one assigned (0.0 + -0.0 would lose the sign); an empty source gives zeros. */
template <int NF, int ND, class Sums, class Term>
__device__ void reg_pass(Sums &sh, uint32_t n_src, Term term)
{
    constexpr int kD0 = NF > 0 ? 32 : 0; /* floats: lanes 0 .., doubles: the lanes after them, count: lane 63 */
    static_assert(NF <= Sums::kF && ND <= Sums::kD && NF <= 32 && kD0 + ND <= 63, "one lane per value");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nchunks = (n_src + 63) / 64;
    float accf = 0.0f;
    double accd = 0.0;
    uint32_t count = 0;
    for (uint32_t base = 0; base < nchunks; base += kIcpChunkSlots) {
        const uint32_t lim = min(nchunks - base, (uint32_t)kIcpChunkSlots);
        for (uint32_t c = wave; c < lim; c += kRegWaves) {
            const uint32_t i = (base + c) * 64 + lane;
            float tf[NF > 0 ? NF : 1];
            double td[ND > 0 ? ND : 1];
#pragma unroll
            for (int v = 0; v < NF; ++v) tf[v] = 0.0f;
#pragma unroll
            for (int v = 0; v < ND; ++v) td[v] = 0.0;
            const bool hit = i < n_src && term(i, tf, td);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
                for (int v = 0; v < NF; ++v) tf[v] = tf[v] + __shfl_down(tf[v], off);
#pragma unroll
                for (int v = 0; v < ND; ++v) td[v] = td[v] + __shfl_down(td[v], off);
            }
            const uint32_t hits = (uint32_t)__popcll(__ballot(hit));
            if (lane == 0) {
#pragma unroll
                for (int v = 0; v < NF; ++v) sh.slotf[c][v] = tf[v];
#pragma unroll
                for (int v = 0; v < ND; ++v) sh.slotd[c][v] = td[v];
                sh.slot_cnt[c] = hits;
            }
        }
        __syncthreads();
        if (tid < NF) {
            for (uint32_t c = 0; c < lim; ++c) accf = (base + c == 0) ? sh.slotf[c][tid] : accf + sh.slotf[c][tid];
        } else if (tid >= kD0 && tid < kD0 + ND) {
            for (uint32_t c = 0; c < lim; ++c) accd = (base + c == 0) ? sh.slotd[c][tid - kD0] : accd + sh.slotd[c][tid - kD0];
        } else if (tid == 63) {
            for (uint32_t c = 0; c < lim; ++c) count += sh.slot_cnt[c];
        }
        __syncthreads();
    }
    if (tid < NF) sh.totf[tid] = accf;
    else if (tid >= kD0 && tid < kD0 + ND) sh.totd[tid - kD0] = accd;
    else if (tid == 63) sh.cnt = count;
    __syncthreads();
}

/* ---- the loop around an estimator ---------------------------------------------------------------------------------------- */
struct RegLoop {
    int state, iters;         /* 0: running; 1 .. 4: converged (ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE); 5: NO_CORRESPONDENCES */
    float fin[16], inc[16];   /* the transform so far; the last increment (row-major) */
};

/* state, final = G, cur = G * source (the source itself where G is the identity); the caller's barrier follows */
template <class Fetch>
__device__ void reg_start(RegLoop &lp, const float *G, uint32_t n_src, Fetch fetch, float4 *cur)
{
    const int tid = threadIdx.x;
    if (tid == 0) {
        lp.state = 0;
        lp.iters = 0;
    }
    if (tid < 16) lp.fin[tid] = G[tid];
    bool identity = true;
    for (int k = 0; k < 16; ++k) identity &= G[k] == ((k % 5 == 0) ? 1.0f : 0.0f);
    for (uint32_t i = tid; i < n_src; i += kRegThreads) {
        const float3 p = fetch(i);
        const float3 q = identity ? p : icp_se3(G, p.x, p.y, p.z);
        cur[i] = make_float4(q.x, q.y, q.z, 0.0f);
    }
}

/* cur = inc * cur (point i by thread i % 256, as the passes read it; lp.inc is rewritten only after the next barrier) */
__device__ void reg_advance(const RegLoop &lp, uint32_t n_src, float4 *cur)
{
    float I[12];
    for (int k = 0; k < 12; ++k) I[k] = lp.inc[k];
    for (uint32_t i = threadIdx.x; i < n_src; i += kRegThreads) {
        const float4 p = cur[i];
        const float3 q = icp_se3(I, p.x, p.y, p.z);
        cur[i] = make_float4(q.x, q.y, q.z, 0.0f);
    }
}

/* thread 0, lp.inc set: final = inc * final, ++iters, DefaultConvergenceCriteria::hasConverged */
__device__ void reg_converge(RegLoop &lp, const bev_icp_params_t &prm, double mse_sum, uint32_t cnt, double &prev)
{
    const float *I = lp.inc;
    float F[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            F[i * 4 + j] = ((I[i * 4] * lp.fin[j] + I[i * 4 + 1] * lp.fin[4 + j]) + I[i * 4 + 2] * lp.fin[8 + j]) +
                           I[i * 4 + 3] * lp.fin[12 + j];
    for (int k = 0; k < 16; ++k) lp.fin[k] = F[k];
    const int it = ++lp.iters;
    /* Eigen sums the float entries in float */
    const double cos_angle = 0.5 * (double)(((I[0] + I[5]) + I[10]) - 1.0f);
    const double trans2 = (double)((I[3] * I[3] + I[7] * I[7]) + I[11] * I[11]);
    if (it >= prm.max_iterations) {
        lp.state = 1; /* ITERATIONS */
    } else if (cos_angle >= 1.0 - prm.transformation_epsilon && trans2 <= prm.transformation_epsilon) {
        lp.state = 2; /* TRANSFORM */
    } else {
        const double mse = mse_sum / (double)cnt;
        if (fabs(mse - prev) < 1e-12) lp.state = 3;                                      /* ABS_MSE */
        else if (fabs(mse - prev) / prev < prm.euclidean_fitness_epsilon) lp.state = 4; /* REL_MSE */
        else prev = mse;
    }
}

/* getFitnessScore of final * source against the grid, then the result record: canonical quiet NaNs, DBL_MAX where no
 * point found a neighbour */
template <class Sums, class Fetch>
__device__ void reg_finish(Sums &sums, const RegLoop &lp, uint32_t n_src, Fetch fetch, const IcpGridHdr &h,
                           const uint32_t *off, const float4 *tpts, bev_icp_result_t *result)
{
    float F[16];
    for (int k = 0; k < 16; ++k) F[k] = lp.fin[k];
    reg_pass<0, 1>(sums, n_src, [&](uint32_t i, float *, double *td) -> bool {
        const float3 p = fetch(i);
        const float3 q = icp_se3(F, p.x, p.y, p.z);
        if (!finite3(q.x, q.y, q.z)) return false;
        float d;
        uint32_t j;
        if (!icp_nn(h, off, tpts, q.x, q.y, q.z, INFINITY, d, j) || !isfinite(d)) return false;
        td[0] = (double)d;
        return true;
    });
    if (threadIdx.x == 0) {
        bev_icp_result_t r{};
        for (int k = 0; k < 16; ++k) r.T[k] = isnan(F[k]) ? __uint_as_float(0x7fc00000u) : F[k];
        r.fitness = sums.cnt ? sums.totd[0] / (double)sums.cnt : 1.7976931348623157e308;
        if (isnan(r.fitness)) r.fitness = bevx::f64_qnan();
        r.iterations = lp.iters;
        r.state = lp.state;
        r.converged = lp.state >= 1 && lp.state <= 4;
        *result = r;
    }
}

} /* namespace bevk */
