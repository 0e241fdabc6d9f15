/*
 * bev_regfront.h — the registration front end (included by bev_kernels.hip): what the reference's three registration
 * tools do to every cloud before ICP (TopPartRegistration.cpp, BatchTopPartRegistration.cpp, BatchWholeRegistration.cpp):
 *
 *   k_rf_cells    per frame        : the 20 m cell of every point (extractTopAndFlatten, TopPartRegistration.cpp:94-110),
 *                                    per-cell counts, the cells' input and output offsets, one sort key per point
 *                                    (descending z, then ascending index) bucketed by cell
 *   k_rf_top      per (cell, frame): sorts the cell's keys, writes the first round(0.2f * n) points flattened
 *                                    (:113-133)
 *   k_rf_voxel    per frame        : pcl::VoxelGrid<PointXYZ>::applyFilter — bounds, voxel index, stable sort by voxel,
 *                                    one lane sums one voxel's points in input order (the steps are bev_reg_common.h's)
 *   k_rf_normals  per query        : Normal2dEstimation::compute in radius mode (src/Normal2dEstimation.cpp,
 *                                    src/PCA2D.cpp): the neighbours in ascending index order, closed-form 2 x 2 eigenvector
 *                                    (Normal2d, which k_submap_pn_normals runs too)
 * rf_top_rank, rf_top_cell and rf_z_desc_key are bev_submap_top.h's too, rf_lower_bound is bev_submap_pn_vox.h's.
 *
 * The contract every line follows (and tests/regfront/regfront_oracle.c restates) is DESIGN.md "Registration front end".
 * No float sum depends on an atomic: counts are atomics (integers), every float sum runs in one lane in a fixed order.
 * Sorting is a bitonic sort by one workgroup, in LDS up to kRfLdsKeys keys, else in a global scratch region
 * (a cell that holds most of a frame).
 */
#pragma once

namespace bevk {

/* 32-bit key whose ascending order is DESCENDING z; -0 and +0 are one value */
__device__ __forceinline__ uint32_t rf_z_desc_key(float z)
{
    if (z == 0.0f) z = 0.0f;
    uint32_t u = __float_as_uint(z);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

/* cell gx * 10 + gy of extractTopAndFlatten, or -1: label 0, a non-finite coordinate, outside the grid (round, not floor:
 * x in [-110, -90) is cell 0, x >= 90 is dropped) */
__device__ __forceinline__ int rf_top_cell(const bev_point_t &p)
{
    if (p.label == 0) return -1;
    if (!finite3(p.x, p.y, p.z)) return -1;
    const float gx = roundf((p.x + 100.0f) / 20.0f);
    const float gy = roundf((p.y + 100.0f) / 20.0f);
    if (!(gx >= 0.0f && gx < (float)kRfGrid && gy >= 0.0f && gy < (float)kRfGrid)) return -1;
    return (int)gx * kRfGrid + (int)gy;
}

/* points kept of a cell of n: the highest fifth, none of a cell with fewer than kRfMinCellPoints (:113-133) */
__device__ __forceinline__ uint32_t rf_top_rank(uint32_t n)
{
    return n >= (uint32_t)kRfMinCellPoints ? (uint32_t)roundf(0.2f * (float)n) : 0u;
}

__device__ __forceinline__ void rf_frame(const RfIn &in, int f, const bev_point_t **p, uint32_t *n)
{
    if (in.offs) {
        const uint64_t a = in.offs[f], b = in.offs[f + 1];
        *p = in.pts + a;
        *n = (uint32_t)(b - a);
    } else {
        *p = in.pts + (size_t)f * in.stride;
        *n = in.n_uniform;
    }
}

/* ---- top part: cells ---------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kRfThreads) void k_rf_cells(RfIn in, RfWork w)
{
    const int f = (int)blockIdx.x;
    __shared__ uint32_t cnt[kRfCells], fill[kRfCells];
    const bev_point_t *p;
    uint32_t n;
    rf_frame(in, f, &p, &n);
    for (int c = threadIdx.x; c < kRfCells; c += blockDim.x) cnt[c] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int c = rf_top_cell(p[i]);
        if (c >= 0) atomicAdd(&cnt[c], 1u);
    }
    __syncthreads();
    uint32_t *cell_cnt = w.cell_cnt + (size_t)f * kRfCells;
    uint32_t *cell_off = w.cell_off + (size_t)f * (kRfCells + 1);
    uint32_t *out_off = w.out_off + (size_t)f * (kRfCells + 1);
    if (threadIdx.x == 0) {
        uint32_t off = 0, o = 0;
        for (int c = 0; c < kRfCells; ++c) {
            cell_cnt[c] = cnt[c];
            cell_off[c] = off;
            out_off[c] = o;
            fill[c] = off;
            off += cnt[c];
            o += rf_top_rank(cnt[c]);
        }
        cell_off[kRfCells] = off;
        out_off[kRfCells] = o;
        w.meta[f].m = o;
    }
    __syncthreads();
    uint64_t *keys = w.keys + (size_t)f * w.P;
    /* (the order inside a bucket does not matter: k_rf_top sorts on keys that hold the input index) */
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const bev_point_t &q = p[i];
        const int c = rf_top_cell(q);
        if (c < 0) continue;
        const uint32_t pos = atomicAdd(&fill[c], 1u);
        keys[pos] = ((uint64_t)rf_z_desc_key(q.z) << 32) | i;
    }
}

/* ---- top part: one cell's highest points -------------------------------------------------------------------------- */
__global__ __launch_bounds__(kRfThreads) void k_rf_top(RfIn in, RfWork w)
{
    __shared__ uint64_t lds[kRfLdsKeys];
    const int c = (int)blockIdx.x, f = (int)blockIdx.y;
    const uint32_t n = w.cell_cnt[(size_t)f * kRfCells + c];
    /* (rf_top_rank's rule in this kernel's own two statements, so that its code stays what it was: DESIGN.md §6w) */
    if (n < (uint32_t)kRfMinCellPoints) return;
    const uint32_t k = (uint32_t)roundf(0.2f * (float)n);
    const uint32_t off = w.cell_off[(size_t)f * (kRfCells + 1) + c];
    const uint32_t out0 = w.out_off[(size_t)f * (kRfCells + 1) + c];
    const bev_point_t *p;
    uint32_t np;
    rf_frame(in, f, &p, &np);
    const uint32_t np2 = rf_pow2(n);
    /* global fallback: the cell's region of the frame's scratch, [2 off, 2 off + np2) (np2 <= 2 n) */
    uint64_t *buf = np2 <= (uint32_t)kRfLdsKeys ? lds : w.scr + (size_t)f * 2 * w.P + 2 * (size_t)off;
    const uint64_t *keys = w.keys + (size_t)f * w.P + off;
    for (uint32_t i = threadIdx.x; i < np2; i += blockDim.x) buf[i] = i < n ? keys[i] : ~0ull;
    __syncthreads();
    rf_bitonic(buf, np2);
    float4 *flat = w.flat + (size_t)f * w.Q + out0;
    for (uint32_t r = threadIdx.x; r < k; r += blockDim.x) {
        const bev_point_t &q = p[(uint32_t)buf[r]];
        flat[r] = make_float4(q.x, q.y, 0.0f, 0.0f);
    }
}

/* ---- voxel grid ----------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(kRfThreads) void k_rf_voxel(RfWork w, float leaf, uint32_t *counts)
{
    __shared__ uint64_t lds[kRfLdsKeys];
    __shared__ uint32_t wave_cnt[kRfThreads / 64];
    __shared__ int s_par[8]; /* overflow, nfin, minb xyz, div xyz */
    const int f = (int)blockIdx.x, t = (int)threadIdx.x;
    RfFrameMeta *meta = w.meta + f;
    const uint32_t m = meta->m;
    const float4 *src = w.flat + (size_t)f * w.Q;
    float4 *vpts = w.vpts + (size_t)f * w.Q;
    uint32_t *vidx = w.vidx + (size_t)f * w.Q;
    uint32_t *vstart = w.vstart + (size_t)f * (w.Q + 1);

    const auto fetch = [src](uint32_t i) { return make_float3(src[i].x, src[i].y, src[i].z); };
    const float inv = 1.0f / leaf;
    /* (the reduction borrows the sort buffer: it is done with it before the keys are written) */
    rf_voxel_bounds(m, fetch, inv, reinterpret_cast<float *>(lds), s_par);
    const uint32_t nf = (uint32_t)s_par[1];
    if (nf == 0) {
        if (t == 0) {
            meta->nv = 0;
            meta->windowed = 0;
            if (counts) counts[f] = 0;
        }
        return;
    }
    if (s_par[0]) { /* PCL: "leaf size is too small": the output is the input */
        for (uint32_t i = t; i < m; i += blockDim.x) vpts[i] = src[i];
        if (t == 0) {
            meta->nv = m;
            meta->windowed = 0;
            if (counts) counts[f] = m;
        }
        return;
    }
    const uint32_t div0 = (uint32_t)s_par[5], div1 = (uint32_t)s_par[6], div2 = (uint32_t)s_par[7];
    const uint32_t np2 = rf_pow2(m);
    uint64_t *buf = np2 <= (uint32_t)kRfLdsKeys ? lds : w.scr + (size_t)f * 2 * w.P;
    rf_voxel_keys(m, np2, fetch, inv, s_par, buf);
    rf_bitonic(buf, np2);
    const uint32_t nv = rf_voxel_starts(buf, nf, wave_cnt, vstart,
                                        [=](uint32_t v, uint32_t i) { vidx[v] = (uint32_t)(buf[i] >> 32); });
    if (t == 0) {
        meta->nv = nv;
        meta->div_x = div0;
        meta->div_y = div1;
        /* the neighbour window of k_rf_normals needs index = i + j * div_x exactly: one z layer, no wrap */
        meta->windowed = div2 == 1 && (uint64_t)div0 * div1 < (1ull << 32);
        if (counts) counts[f] = nv;
    }
    __syncthreads();
    rf_voxel_centroids(buf, vstart, nv, [src](uint32_t i) { return src[i]; }, vpts);
}

/* ---- 2-D normals ---------------------------------------------------------------------------------------------------- */
/* the first of the n ascending voxel indices a that is >= x */
__device__ __forceinline__ uint32_t rf_lower_bound(const uint32_t *a, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* Normal2dEstimation::compute in radius mode for one query q (src/Normal2dEstimation.cpp, src/PCA2D.cpp), in the steps its two
 * passes over the candidates need: first() per candidate j (position p) in ascending index; where cnt >= 3, mean() and then
 * second() per candidate again; then the record (f64 sqrt and division, the flip towards the viewpoint).  k_rf_normals walks a
 * window in global memory, k_submap_pn_normals (bev_submap_pn_vox.h) chunks staged in LDS. */
struct Normal2d {
    float4 q;
    float r2;
    uint32_t cnt = 0, n0 = 0, n1 = 0;
    float sx = 0.0f, sy = 0.0f, mx = 0.0f, my = 0.0f, a = 0.0f, b = 0.0f, c = 0.0f;
    __device__ __forceinline__ bool near(const float4 p) const
    {
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        return (dx * dx + dy * dy) + dz * dz <= r2;
    }
    __device__ __forceinline__ void first(uint32_t j, const float4 p)
    {
        if (near(p)) {
            if (cnt == 0) n0 = j;
            if (cnt == 1) n1 = j;
            ++cnt;
            sx += p.x;
            sy += p.y;
        }
    }
    __device__ __forceinline__ void mean()
    {
        mx = sx / (float)cnt;
        my = sy / (float)cnt;
    }
    __device__ __forceinline__ void second(const float4 p)
    {
        if (near(p)) {
            const float ex = p.x - mx, ey = p.y - my;
            a += ex * ex;
            b += ex * ey;
            c += ey * ey;
        }
    }
    /* pts: the queries' cloud (the two neighbours of the |N| = 2 branch); o: a pcl::PointNormal record (12 floats) where
     * kPointNormal, else a pcl::Normal record (8 floats) */
    template <bool kPointNormal>
    __device__ __forceinline__ void write(const float4 *pts, float vpx, float vpy, float4 *o) const
    {
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = 0.0f;
        if (cnt == 1) {
            nx = ny = nz = curv = __uint_as_float(0x7fc00000u);
        } else if (cnt == 2) {
            const double vx = (double)(float)(pts[n0].x - pts[n1].x);
            const double vy = (double)(float)(pts[n0].y - pts[n1].y);
            const double norm = sqrt(vx * vx + vy * vy);
            nx = (float)(-vy / norm);
            ny = (float)(vx / norm);
        } else if (cnt >= 3) {
            double vx, vy;
            const double h = 0.5 * ((double)c - (double)a);
            const double s = sqrt(h * h + (double)b * (double)b);
            if (b == 0.0f) {
                vx = a <= c ? 1.0 : 0.0;
                vy = a <= c ? 0.0 : 1.0;
            } else if (h >= 0.0) {
                vx = h + s;
                vy = -(double)b;
            } else {
                vx = (double)b;
                vy = h - s;
            }
            const double len = sqrt(vx * vx + vy * vy);
            nx = (float)(vx / len);
            ny = (float)(vy / len);
            const float lx = -ny, ly = nx; /* the large eigenvector (-n.y, n.x): eigen_vec(0), eigen_vec(1) */
            curv = ly / (lx + ly);
        }
        if (cnt >= 2) { /* flipNormalTowardsViewpoint (Normal2dEstimation.cpp) */
            const float cs = (float)((double)(vpx - q.x) * (double)nx + (double)(vpy - q.y) * (double)ny);
            if (cs < 0.0f) {
                nx = -nx;
                ny = -ny;
                nz = -nz;
            }
        }
        if (kPointNormal) *o++ = make_float4(q.x, q.y, q.z, 0.0f);
        o[0] = make_float4(rf_canon(nx), rf_canon(ny), rf_canon(nz), 0.0f);
        o[1] = make_float4(rf_canon(curv), 0.0f, 0.0f, 0.0f);
    }
};

/* kPointNormal: pcl::PointNormal records (12 floats) at out + f * out_stride (the chain); else pcl::Normal records
 * (8 floats) at out + f * out_stride.  Neighbours are scanned in ascending index: over all points, or — where the points
 * are voxel centroids sorted by index i + j * div_x (meta.windowed) — over the rows j +- win, a contiguous index range. */
template <bool kPointNormal>
__global__ __launch_bounds__(kRfThreads) void k_rf_normals(RfWork w, float r2, uint32_t win, float vpx, float vpy,
                                                          float *out, size_t out_stride)
{
    const int f = (int)blockIdx.y;
    const RfFrameMeta meta = w.meta[f];
    const uint32_t nv = meta.nv;
    const float4 *pts = w.vpts + (size_t)f * w.Q;
    const uint32_t *vidx = w.vidx + (size_t)f * w.Q;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += gridDim.x * blockDim.x) {
        Normal2d nrm;
        nrm.q = pts[v];
        nrm.r2 = r2;
        uint32_t lo = 0, hi = nv;
        if (meta.windowed) {
            const uint32_t j = vidx[v] / meta.div_x;
            const uint32_t jl = j > win ? j - win : 0u;
            const uint64_t jh = std::min<uint64_t>((uint64_t)j + win, (uint64_t)meta.div_y - 1u);
            lo = rf_lower_bound(vidx, nv, (uint64_t)jl * meta.div_x);
            hi = rf_lower_bound(vidx, nv, (jh + 1u) * meta.div_x);
        }
        for (uint32_t j = lo; j < hi; ++j) nrm.first(j, pts[j]);
        if (nrm.cnt >= 3) {
            nrm.mean();
            for (uint32_t j = lo; j < hi; ++j) nrm.second(pts[j]);
        }
        constexpr size_t kRow = kPointNormal ? 12 : 8;
        nrm.write<kPointNormal>(pts, vpx, vpy, reinterpret_cast<float4 *>(out + ((size_t)f * out_stride + v) * kRow));
    }
}

/* ---- launchers ------------------------------------------------------------------------------------------------------- */
void launch_rf_top(const RfIn &in, const RfWork &w, int nf, hipStream_t st, int phase)
{
    if (nf == 0) return;
    if (phase == 0) hipLaunchKernelGGL(k_rf_cells, dim3((unsigned)nf), dim3(kRfThreads), 0, st, in, w);
    else hipLaunchKernelGGL(k_rf_top, dim3(kRfCells, (unsigned)nf), dim3(kRfThreads), 0, st, in, w);
}
void launch_rf_voxel(const RfWork &w, int nf, float leaf, uint32_t *counts, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_rf_voxel, dim3((unsigned)nf), dim3(kRfThreads), 0, st, w, leaf, counts);
}
void launch_rf_normals(const RfWork &w, int nf, uint32_t max_points, float radius, float leaf, const float vp[2],
                       bool point_normal, float *out, size_t out_stride, hipStream_t st)
{
    if (nf == 0 || max_points == 0) return;
    const float r2 = (float)((double)radius * (double)radius);
    /* rows of the neighbour window: the radius in voxels, +2 for a centroid that rounds just outside its voxel */
    const double rows = leaf > 0.0f ? std::ceil((double)radius / (double)leaf) + 2.0 : 4294967295.0;
    const uint32_t win = rows < 4294967295.0 ? (uint32_t)rows : 0xffffffffu;
    const dim3 gr((max_points + kRfThreads - 1) / kRfThreads, (unsigned)nf), bl(kRfThreads);
    if (point_normal) hipLaunchKernelGGL(k_rf_normals<true>, gr, bl, 0, st, w, r2, win, vp[0], vp[1], out, out_stride);
    else hipLaunchKernelGGL(k_rf_normals<false>, gr, bl, 0, st, w, r2, win, vp[0], vp[1], out, out_stride);
}

} /* namespace bevk */
