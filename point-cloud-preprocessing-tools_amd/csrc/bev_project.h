/*
 * bev_project.h — range-image projection of raw XYZI returns (see bev_libm.h), batched: every kernel takes its frames from a
 * device table (ProjFrame, bev_internal.h), so a frame costs no launch of its own.  bev_project_xyzi is the one-frame call.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_PROJECT_H
#define BEV_PROJECT_H

#include "bev_dev.h"
#include "bev_libm.h"

namespace bevk {
using namespace bevx;

/* MulRan / Oxford: a pure map over packed frames (packed_place, bev_dev.h).  A thread's kProjPerThread returns lie 256 apart,
 * so a wave's load is 1 KiB of consecutive records (MulRan: one 16-byte load per lane; Oxford's planes start at any multiple
 * of 4 bytes: four 4-byte loads).  A record leaves as two 16-byte halves. */
template <int kKind>
__global__ __launch_bounds__(256) void k_project_batch(const float *__restrict__ xyzi, const ProjFrame *__restrict__ tab,
                                                       int nf, bev_point_t *__restrict__ out)
{
    const PackedPlace pl = packed_place(tab, nf, blockIdx.x);
    const uint64_t off = pl.off;
    const uint32_t n = pl.n, k0 = pl.k0;
    const float *__restrict__ src = xyzi + 4 * off;
    float x[kProjPerThread], y[kProjPerThread], z[kProjPerThread], it[kProjPerThread];
#pragma unroll
    for (int j = 0; j < kProjPerThread; ++j) {
        const uint32_t k = k0 + (uint32_t)j * 256u;
        x[j] = y[j] = z[j] = it[j] = 0.0f;
        if (k >= n) continue;
        if (kKind == BEV_PROJECT_MULRAN_OS1_64) {
            const float4 v = reinterpret_cast<const float4 *>(src)[k];
            x[j] = v.x; y[j] = v.y; z[j] = v.z; it[j] = v.w;
        } else {
            x[j] = -src[k]; y[j] = src[(size_t)n + k]; z[j] = -src[2 * (size_t)n + k]; it[j] = src[3 * (size_t)n + k];
        }
    }
#pragma unroll
    for (int j = 0; j < kProjPerThread; ++j) {
        const uint32_t k = k0 + (uint32_t)j * 256u; /* the index within the frame: MulRan's row = k % 64 */
        if (k >= n) continue;
        uint16_t row, col;
        if (kKind == BEV_PROJECT_MULRAN_OS1_64) project_mulran(k, x[j], y[j], row, col);
        else project_oxford(x[j], y[j], z[j], row, col);
        Half lo_, hi_;
        lo_.w[0] = __float_as_uint(x[j]); lo_.w[1] = __float_as_uint(y[j]); lo_.w[2] = __float_as_uint(z[j]); lo_.w[3] = 0u;
        hi_.w[0] = __float_as_uint(it[j]); hi_.w[1] = (uint32_t)row | ((uint32_t)col << 16); hi_.w[2] = 0u;
        hi_.w[3] = (uint32_t)(uint16_t)(int16_t)-2; /* label = -2 */
        Half *dst = reinterpret_cast<Half *>(out + off + k);
        dst[0] = lo_;
        dst[1] = hi_;
    }
}

/* ---- KITTI projection (see bev_libm.h): crossings -> chain of accepted crossings -> rings -> structured cloud ----
 * blockIdx.y is the frame of the launch group: its returns through tab[blockIdx.y], its piece of the workspace through
 * KittiWork's strides.  The grid's x covers the group's longest frame; workgroups past a frame's end leave at once. */
__device__ __forceinline__ KittiWork kitti_frame_work(const KittiWork &w, uint32_t g)
{
    KittiWork r = w;
    r.hdr = w.hdr + g;
    r.col = w.col + (size_t)g * w.n_cap;
    r.cnt = w.cnt + (size_t)g * w.blocks_cap;
    r.pos = w.pos + (size_t)g * w.blocks_cap * kKittiListCap;
    r.winner = w.winner + (size_t)g * (kKittiRows * kKittiCols);
    return r;
}

/* per point: azimuth, column, crossing flag; per block of 256 points: the ascending list of crossing positions */
__global__ __launch_bounds__(kKittiBlock) void k_kitti_crossings(const float *__restrict__ xyzi_all,
                                                                 const ProjFrame *__restrict__ tab, KittiWork wg)
{
    __shared__ float az[kKittiBlock + 1];
    __shared__ uint32_t wave_base[kKittiBlock / 64 + 1];
    const uint32_t n = tab[blockIdx.y].n;
    if (blockIdx.x * (uint32_t)kKittiBlock >= n) return;
    const float *__restrict__ xyzi = xyzi_all + 4 * tab[blockIdx.y].off;
    const KittiWork w = kitti_frame_work(wg, blockIdx.y);
    const uint32_t tid = threadIdx.x, i = blockIdx.x * (uint32_t)kKittiBlock + tid;
    float a = 0.0f;
    if (i < n) {
        const float4 v = reinterpret_cast<const float4 *>(xyzi)[i];
        a = kitti_azimuth(v.x, v.y);
        w.col[i] = kitti_col(a);
        if (i == 0) w.hdr->ring0 = a > 0.0f ? 0 : -1; /* :195-203 */
    }
    az[tid + 1] = a;
    if (tid == 0 && i >= 1 && i < n) {
        const float4 v = reinterpret_cast<const float4 *>(xyzi)[i - 1];
        az[0] = kitti_azimuth(v.x, v.y);
    }
    __syncthreads();
    const bool flag = i >= 1 && i < n && kitti_crossing(az[tid], az[tid + 1]);
    const uint64_t m = __ballot(flag);
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    if (lane == 0) wave_base[wave + 1] = (uint32_t)__popcll(m);
    __syncthreads();
    if (tid == 0) {
        wave_base[0] = 0;
        for (int k = 0; k < kKittiBlock / 64; ++k) wave_base[k + 1] += wave_base[k];
        w.cnt[blockIdx.x] = wave_base[kKittiBlock / 64];
    }
    __syncthreads();
    if (flag) w.pos[(size_t)blockIdx.x * kKittiListCap + wave_base[wave] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

/* one wave per frame walks the chain of accepted crossings */
__global__ __launch_bounds__(64) void k_kitti_chain(const ProjFrame *__restrict__ tab, KittiWork wg, uint32_t ring_min)
{
    const uint32_t n = tab[blockIdx.x].n;
    const KittiWork w = kitti_frame_work(wg, blockIdx.x);
    const uint32_t *__restrict__ cnt = w.cnt, *__restrict__ pos = w.pos;
    KittiHeader *hdr = w.hdr;
    const uint32_t lane = threadIdx.x, nblocks = (n + kKittiBlock - 1u) / kKittiBlock;
    if (n == 0) { /* (no return wrote ring0) */
        if (lane == 0) hdr->n_links = 0;
        return;
    }
    int ring = hdr->ring0;
    uint32_t last = 1, links = 0; /* count == i - last; before any crossing count == i - 1 (:210-212) */
    while (ring < kKittiRows && links < (uint32_t)kKittiMaxLinks) {
        const uint64_t target = ring == -1 ? 1ull : (uint64_t)last + ring_min;
        if (target >= n) break;
        uint32_t found = 0; /* crossings are at positions >= 1 */
        const uint32_t b = (uint32_t)(target / kKittiBlock), c = cnt[b];
        for (uint32_t k0 = 0; k0 < c && !found; k0 += 64) {
            const uint32_t k = k0 + lane;
            const uint32_t p = k < c ? pos[(size_t)b * kKittiListCap + k] : 0u;
            const uint64_t hit = __ballot(k < c && p >= target);
            if (hit) found = __shfl(p, __ffsll((long long)hit) - 1);
        }
        for (uint32_t b0 = b + 1; b0 < nblocks && !found; b0 += 64) {
            const uint32_t bb = b0 + lane;
            const uint64_t hit = __ballot(bb < nblocks && cnt[bb] > 0u);
            if (hit) found = pos[(size_t)(b0 + (uint32_t)__ffsll((long long)hit) - 1u) * kKittiListCap];
        }
        if (!found) break;
        ring = ring == -1 ? 0 : ring + 1;
        last = found;
        if (lane == 0) hdr->link[links] = found;
        ++links;
    }
    if (lane == 0) hdr->n_links = links;
}

/* ring of every point, then last-writer-wins on its slot (:240) */
__global__ __launch_bounds__(256) void k_kitti_assign(const ProjFrame *__restrict__ tab, KittiWork wg)
{
    __shared__ uint32_t link[kKittiMaxLinks];
    const uint32_t n = tab[blockIdx.y].n;
    if (blockIdx.x * 256u >= n) return;
    const KittiWork w = kitti_frame_work(wg, blockIdx.y);
    const uint32_t n_links = w.hdr->n_links;
    if (threadIdx.x < n_links) link[threadIdx.x] = w.hdr->link[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < 1u || i >= n) return; /* the loop at :212 starts at 1 */
    const int ring = kitti_ring_of(i, w.hdr->ring0, link, n_links), c = w.col[i];
    if (ring >= 0 && ring < kKittiRows && c >= 0) atomicMax(&w.winner[(uint32_t)ring * kKittiCols + (uint32_t)c], i + 1u);
}

/* the structured clouds: winners with intensity = -1, label = -2 (:235-238), empty slots all-zero (:207); frame g of the
 * group at out + g * 64 * 2083 */
__global__ __launch_bounds__(256) void k_kitti_gather(const float *__restrict__ xyzi_all, const ProjFrame *__restrict__ tab,
                                                      KittiWork wg, bev_point_t *__restrict__ out)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= (uint32_t)(kKittiRows * kKittiCols)) return;
    const float *__restrict__ xyzi = xyzi_all + 4 * tab[blockIdx.y].off;
    Half lo{{0, 0, 0, 0}}, hi{{0, 0, 0, 0}};
    const uint32_t w = wg.winner[(size_t)blockIdx.y * (kKittiRows * kKittiCols) + s];
    if (w != 0u) {
        const float4 v = reinterpret_cast<const float4 *>(xyzi)[w - 1u];
        lo.w[0] = __float_as_uint(v.x); lo.w[1] = __float_as_uint(v.y); lo.w[2] = __float_as_uint(v.z);
        hi.w[0] = __float_as_uint(-1.0f);
        hi.w[1] = (s / (uint32_t)kKittiCols) | ((s % (uint32_t)kKittiCols) << 16);
        hi.w[3] = (uint32_t)(uint16_t)(int16_t)-2;
    }
    Half *dst = reinterpret_cast<Half *>(out + (size_t)blockIdx.y * (kKittiRows * kKittiCols) + s);
    dst[0] = lo;
    dst[1] = hi;
}

} /* namespace bevk */

#endif /* BEV_PROJECT_H */
