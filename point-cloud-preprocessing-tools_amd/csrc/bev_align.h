/*
 * bev_align.h — a translation guess for retrieved pairs on the device (bev_align_grid_device_resident,
 * bev_align_hits_device_resident): Cartesian height grids of the candidates, and per hit the exhaustive search
 * over whole-cell shifts of the query's grid under each yaw hypothesis.  The arithmetic is bev_align_exact.h's, shared with
 * the host and the tests' checker.
 *   k_align_grid    per point (and entry of its frame): the cell and the height code, combined in an LDS plane per workgroup,
 *                   then atomicMax of its non-zero cells into the grid's plane of the workspace (zeroed by the host);
 *   k_align_finish  per grid: the bytes and the sum of squares;
 *   k_align_hit     per (hit, flip, k): the query's grid under the hypothesis in LDS, every shift's score by packed 4 x uint8
 *                   dot products, the best shift and its four neighbours' scores;
 *   k_align_pick    per hit: the order over k, the sub-cell offsets, both results, the detail and best.
 * A maximum has no order, the scores are integers and both orders are strict total orders: no output depends on an atomic's
 * order or on the launch shape.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_ALIGN_H
#define BEV_ALIGN_H

#include "bev_align_exact.h"
#include "bev_dev.h"
#include "bev_place.h"
#include "bev_submap.h"

namespace bevk {
using namespace bevx;

/* lds_max_splat (bev_place.h) over a Cartesian plane of G * G words (dynamic LDS) */
template <bool kMaps>
__global__ __launch_bounds__(256) void k_align_grid(const bev_point_t *__restrict__ clouds, const ProjFrame *__restrict__ tab,
                                                    const uint32_t *__restrict__ ent0, int nf,
                                                    const bevsub::Entry *__restrict__ entries, AlignShape as,
                                                    uint32_t *__restrict__ planes)
{
    extern __shared__ uint32_t align_grid_plane[];
    lds_max_splat<kMaps>(clouds, tab, ent0, nf, entries, as.skip_label0, as.lidar_to_ground, as.G * as.G, align_grid_plane, planes,
                         [=](float x, float y, int label) { return align_cell(x, y, label, as.G, as.cell, as.skip_label0); });
}

/* the sum of a value over a workgroup of 256 threads, in thread 0 (scratch: 4 words of LDS, free on entry) */
__device__ __forceinline__ uint32_t align_block_sum(uint32_t v, uint32_t *scratch)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

/* One workgroup per grid: the bytes, and the sum of squares (integers: any order of the sum gives the same) */
__global__ __launch_bounds__(256) void k_align_finish(const uint32_t *__restrict__ planes, AlignShape as, uint8_t *__restrict__ grids,
                                                      uint32_t *__restrict__ energy)
{
    __shared__ uint32_t s_sum[4];
    const int cells = as.G * as.G;
    const size_t g = blockIdx.x;
    const uint32_t *__restrict__ plane = planes + g * (size_t)cells;
    uint32_t e = 0u;
    for (int i = (int)threadIdx.x; i < cells; i += 256) {
        const uint32_t v = plane[i];
        grids[g * (size_t)cells + (size_t)i] = (uint8_t)v;
        e += v * v;
    }
    e = align_block_sum(e, s_sum);
    if (threadIdx.x == 0) energy[g] = e;
}

/* Where k_align_hit's pieces lie in its dynamic LDS, in words.  The plane of G * G words comes first and alone; once it is
 * packed, the same words hold: the query's bytes (G rows of Wq words, zero behind column G), the candidate's bytes padded by S
 * on every side (G + 2S rows of Pw words: a row's last word is read by the misaligned shifts and holds zeros), the score of
 * every shift, and the reductions' scratch. */
struct AlignLds {
    int Wq, Pw, c0, sc0, red0, words;
};
__host__ __device__ inline AlignLds align_lds(int G, int S)
{
    AlignLds l;
    l.Wq = (G + 3) / 4;
    l.Pw = l.Wq + (2 * S + 3) / 4 + 1;
    l.c0 = G * l.Wq;
#ifdef BEV_EXP_ALIGN_COPIES /* the measured alternative: four byte-shifted copies of the padded candidate */
    l.sc0 = l.c0 + 4 * (G + 2 * S) * l.Pw;
#else
    l.sc0 = l.c0 + (G + 2 * S) * l.Pw;
#endif
    l.red0 = l.sc0 + (2 * S + 1) * (2 * S + 1);
    l.words = l.red0 + 16;
    if (l.words < G * G) l.words = G * G;
    return l;
}
constexpr int kAlignPackPerThread = (kAlignMaxGrid * ((kAlignMaxGrid + 3) / 4) + 255) / 256; /* 16 packed words */

/* a shift on its way through a reduction */
struct AlignBest {
    uint32_t s;
    int dx, dy;
};
constexpr int kAlignNoShift = 1 << 10; /* a shift that stands for nothing: score 0 at this distance loses to every real one */
__device__ __forceinline__ AlignBest align_wave_best(AlignBest a)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        AlignBest b;
        b.s = (uint32_t)__shfl_xor((int)a.s, d);
        b.dx = __shfl_xor(a.dx, d);
        b.dy = __shfl_xor(a.dy, d);
        if (align_shift_better(b.s, b.dx, b.dy, a.s, a.dx, a.dy)) a = b;
    }
    return a;
}

/* Workgroup b: hypothesis b % (2K + 1) - K of flip (b / (2K + 1)) % 2 of hit b / (2 (2K + 1)).
 * The query's records are walked once into the plane (atomicMax in LDS: no global plane, no memset, no global atomic on the
 * query's side).  A thread then takes a row offset dy and FOUR consecutive column offsets that share their candidate words:
 * per query word (the same address in every lane: a broadcast, and a zero word — most of a sparse grid — is skipped by all
 * lanes together) two candidate words, the three misaligned words by v_alignbyte_b32, four dot products. */
__global__ __launch_bounds__(256) void k_align_hit(const bev_point_t *__restrict__ clouds, const AlignHit *__restrict__ hits,
                                                   const uint8_t *__restrict__ grids, AlignShape as, AlignHyp *__restrict__ hyp)
{
    extern __shared__ uint32_t align_hit_lds[];
    uint32_t *lds = align_hit_lds;
    const int G = as.G, S = as.S, nk = 2 * as.K + 1, tid = (int)threadIdx.x;
    const AlignLds l = align_lds(G, S);
    const int b = (int)blockIdx.x, k = b % nk - as.K, flip = (b / nk) & 1;
    const AlignHit h = hits[b / (2 * nk)];
    float T[16];
    icp_tool_guess(align_theta(h.angle_guess, k, as.yaw_step), flip, T);

    for (int i = tid; i < G * G; i += 256) lds[i] = 0u;
    __syncthreads();
    const bev_point_t *__restrict__ src = clouds + h.off;
    for (uint32_t i = (uint32_t)tid; i < h.n; i += 256u) {
        const float4 p = *reinterpret_cast<const float4 *>(src + i);
        const int label = as.skip_label0 ? (int)reinterpret_cast<const int16_t *>(src + i)[14] : 1;
        float x, y, z;
        transform_xyz(T, p.x, p.y, p.z, x, y, z);
        const int cell = align_cell(x, y, label, G, as.cell, as.skip_label0);
        const int v = place_value(z, as.lidar_to_ground);
        if (cell >= 0 && v > 0) atomicMax(&lds[cell], (uint32_t)v);
    }
    __syncthreads();

    /* the plane to bytes, in place: every thread's words into registers, then a barrier, then the stores */
    uint32_t packed[kAlignPackPerThread];
    uint32_t eq = 0u;
#pragma unroll
    for (int j = 0; j < kAlignPackPerThread; ++j) {
        const int i = tid + j * 256;
        packed[j] = 0u;
        if (i < l.c0) {
            const int iy = i / l.Wq, w = i - iy * l.Wq;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t v = 4 * w + c < G ? lds[iy * G + 4 * w + c] : 0u;
                packed[j] |= v << (8 * c);
                eq += v * v;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kAlignPackPerThread; ++j) {
        const int i = tid + j * 256;
        if (i < l.c0) lds[i] = packed[j];
    }
    for (int i = l.c0 + tid; i < l.sc0; i += 256) lds[i] = 0u;
    __syncthreads();
    eq = align_block_sum(eq, lds + l.red0); /* (thread 0's is the grid's) */
    if (h.cand >= 0) {
        const uint8_t *__restrict__ g = grids + (size_t)h.cand * (size_t)(G * G);
        uint8_t *c8 = reinterpret_cast<uint8_t *>(lds + l.c0);
        for (int i = tid; i < G * G; i += 256) {
            const int iy = i / G, ix = i - iy * G;
            c8[(iy + S) * l.Pw * 4 + S + ix] = g[i];
        }
    }
    __syncthreads();
#ifdef BEV_EXP_ALIGN_COPIES
    const int cw = (G + 2 * S) * l.Pw;
    for (int i = tid; i < cw; i += 256) {
        const uint32_t lo = lds[l.c0 + i], hi = i + 1 < cw ? lds[l.c0 + i + 1] : 0u;
        lds[l.c0 + cw + i] = __builtin_amdgcn_alignbyte(hi, lo, 1u);
        lds[l.c0 + 2 * cw + i] = __builtin_amdgcn_alignbyte(hi, lo, 2u);
        lds[l.c0 + 3 * cw + i] = __builtin_amdgcn_alignbyte(hi, lo, 3u);
    }
    __syncthreads();
#endif

    const int side = 2 * S + 1, ngroups = (2 * S) / 4 + 1;
    const uint32_t *__restrict__ q = lds, *__restrict__ c = lds + l.c0;
    uint32_t *score = lds + l.sc0;
    for (int task = tid; task < side * ngroups; task += 256) {
        const int dyi = task / ngroups, grp = task - dyi * ngroups;
        uint32_t a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u;
        for (int iy = 0; iy < G; ++iy) {
            const uint32_t *__restrict__ crow = c + (iy + dyi) * l.Pw + grp, *__restrict__ qrow = q + iy * l.Wq;
            for (int w = 0; w < l.Wq; ++w) {
                const uint32_t qw = qrow[w];
                if (qw == 0u) continue;
#ifdef BEV_EXP_ALIGN_COPIES
                a0 = place_dot4(qw, crow[w], a0);
                a1 = place_dot4(qw, crow[cw + w], a1);
                a2 = place_dot4(qw, crow[2 * cw + w], a2);
                a3 = place_dot4(qw, crow[3 * cw + w], a3);
#else
                const uint32_t lo = crow[w], hi = crow[w + 1];
                a0 = place_dot4(qw, lo, a0);
                a1 = place_dot4(qw, __builtin_amdgcn_alignbyte(hi, lo, 1u), a1);
                a2 = place_dot4(qw, __builtin_amdgcn_alignbyte(hi, lo, 2u), a2);
                a3 = place_dot4(qw, __builtin_amdgcn_alignbyte(hi, lo, 3u), a3);
#endif
            }
        }
        const int o = 4 * grp;
        uint32_t *row = score + dyi * side;
        row[o] = a0;
        if (o + 1 < side) row[o + 1] = a1;
        if (o + 2 < side) row[o + 2] = a2;
        if (o + 3 < side) row[o + 3] = a3;
    }
    __syncthreads();

    AlignBest best{0u, kAlignNoShift, kAlignNoShift};
    for (int i = tid; i < side * side; i += 256) {
        const int dyi = i / side, dxi = i - dyi * side;
        const uint32_t s = score[i];
        if (align_shift_better(s, dxi - S, dyi - S, best.s, best.dx, best.dy)) best = AlignBest{s, dxi - S, dyi - S};
    }
    best = align_wave_best(best);
    uint32_t *red = lds + l.red0 + 4;
    if ((tid & 63) == 0) {
        red[3 * (tid >> 6)] = best.s;
        red[3 * (tid >> 6) + 1] = (uint32_t)best.dx;
        red[3 * (tid >> 6) + 2] = (uint32_t)best.dy;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            const AlignBest o{red[3 * w], (int)red[3 * w + 1], (int)red[3 * w + 2]};
            if (align_shift_better(o.s, o.dx, o.dy, best.s, best.dx, best.dy)) best = o;
        }
        const int dxi = best.dx + S, dyi = best.dy + S;
        AlignHyp r;
        r.score = best.s;
        r.dx = best.dx;
        r.dy = best.dy;
        r.eq = eq;
        r.sxm = dxi > 0 ? score[dyi * side + dxi - 1] : 0u;
        r.sxp = dxi + 1 < side ? score[dyi * side + dxi + 1] : 0u;
        r.sym = dyi > 0 ? score[(dyi - 1) * side + dxi] : 0u;
        r.syp = dyi + 1 < side ? score[(dyi + 1) * side + dxi] : 0u;
        hyp[b] = r;
    }
}

/* A thread per hit: per flip the best k, its offsets and its record; then best */
__global__ __launch_bounds__(64) void k_align_pick(const AlignHit *__restrict__ hits, int n, const AlignHyp *__restrict__ hyp,
                                                   const uint32_t *__restrict__ energy, AlignShape as,
                                                   bev_icp_result_t *__restrict__ results, int32_t *__restrict__ best,
                                                   bev_align_detail_t *__restrict__ detail)
{
    const int m = (int)(blockIdx.x * 64u + threadIdx.x), nk = 2 * as.K + 1;
    if (m >= n) return;
    const AlignHit h = hits[m];
    const uint32_t ec = h.cand >= 0 ? energy[h.cand] : 0u;
    uint32_t top[2];
    for (int flip = 0; flip < 2; ++flip) {
        const AlignHyp *__restrict__ row = hyp + ((size_t)m * 2 + (size_t)flip) * (size_t)nk;
        int kb = -as.K;
        for (int k = -as.K + 1; k <= as.K; ++k)
            if (align_k_better(row[k + as.K].score, k, row[kb + as.K].score, kb)) kb = k;
        const AlignHyp w = row[kb + as.K];
        const double ox = align_offset(w.dx, as.S, w.sxm, w.score, w.sxp), oy = align_offset(w.dy, as.S, w.sym, w.score, w.syp);
        bev_icp_result_t r;
        icp_tool_guess(align_theta(h.angle_guess, kb, as.yaw_step), flip, r.T);
        r.T[3] = align_translation(w.dx, ox, as.cell);
        r.T[7] = align_translation(w.dy, oy, as.cell);
        r.fitness = align_fitness(w.score, w.eq, ec);
        r.converged = w.score > 0u ? 1 : 0;
        r.iterations = 0;
        r.state = BEV_ICP_NOT_CONVERGED;
        r._pad = 0;
        results[(size_t)m * 2 + (size_t)flip] = r;
        if (detail) {
            bev_align_detail_t d;
            d.dx = w.dx;
            d.dy = w.dy;
            d.k = kb;
            d.flip = flip;
            d.score = w.score;
            d.eq = w.eq;
            d.ec = ec;
            d.off_x = (float)ox;
            d.off_y = (float)oy;
            detail[(size_t)m * 2 + (size_t)flip] = d;
        }
        top[flip] = w.score;
    }
    best[m] = align_best_flip(top[0], top[1]);
}

size_t align_hit_lds_bytes(const AlignShape &as) { return (size_t)align_lds(as.G, as.S).words * sizeof(uint32_t); }

void launch_align_grid(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                       const void *entries, const AlignShape &as, uint32_t *planes, hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    const size_t lds = (size_t)as.G * (size_t)as.G * sizeof(uint32_t);
    if (ent0)
        hipLaunchKernelGGL(k_align_grid<true>, dim3(blocks), dim3(256), lds, st, clouds, static_cast<const ProjFrame *>(rows), ent0,
                           nf, static_cast<const bevsub::Entry *>(entries), as, planes);
    else
        hipLaunchKernelGGL(k_align_grid<false>, dim3(blocks), dim3(256), lds, st, clouds, static_cast<const ProjFrame *>(rows), ent0,
                           nf, static_cast<const bevsub::Entry *>(entries), as, planes);
}
void launch_align_finish(const uint32_t *planes, int n_grids, const AlignShape &as, uint8_t *grids, uint32_t *energy, hipStream_t st)
{
    if (n_grids == 0) return;
    hipLaunchKernelGGL(k_align_finish, dim3((unsigned)n_grids), dim3(256), 0, st, planes, as, grids, energy);
}
void launch_align_hit(const bev_point_t *clouds, const AlignHit *hits, int n, const uint8_t *grids, const AlignShape &as,
                      AlignHyp *hyp, hipStream_t st)
{
    if (n == 0) return;
#ifdef BEV_EXP_ALIGN_COPIES /* (above 64 KiB of dynamic LDS) */
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_align_hit), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)align_hit_lds_bytes(as));
#endif
    hipLaunchKernelGGL(k_align_hit, dim3((unsigned)n * 2u * (unsigned)(2 * as.K + 1)), dim3(256), align_hit_lds_bytes(as), st, clouds,
                       hits, grids, as, hyp);
}
void launch_align_pick(const AlignHit *hits, int n, const AlignHyp *hyp, const uint32_t *energy, const AlignShape &as,
                       bev_icp_result_t *results, int32_t *best, bev_align_detail_t *detail, hipStream_t st)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_align_pick, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, hits, n, hyp, energy, as, results, best, detail);
}

} /* namespace bevk */

#endif /* BEV_ALIGN_H */
