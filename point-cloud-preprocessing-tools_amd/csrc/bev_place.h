/*
 * bev_place.h — place retrieval on the device (bev_place_descriptor_device_resident, bev_place_match_device_resident;
 * DESIGN.md §6z): polar max-height descriptors of frames or of submaps, and the search over all pairs and all rotations.
 * The arithmetic is bev_place_exact.h's, shared with the host and the tests' checker.
 *   k_place_splat   per point (and entry of its frame): the polar cell and the height code, combined in an LDS plane per
 *                   workgroup and descriptor, then atomicMax into the descriptor's plane of the workspace (zeroed by the host);
 *   k_place_finish  per descriptor: the bytes, the unit columns and the column mask (PlaceHandle, bev_internal.h);
 *   k_place_pairs   per query and tile of candidates: the best shift of every pair, 4 x uint8 dot products;
 *   k_place_topk    per query: the best top_k candidates in the order of place_better.
 * A maximum has no order, the scores are integers and place_better is a strict total order: no output depends on an atomic's
 * order or on the launch shape.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_PLACE_H
#define BEV_PLACE_H

#include "bev_dev.h"
#include "bev_place_exact.h"
#include "bev_submap.h"

namespace bevk {
using namespace bevx;

/* The max-height splat of a workgroup of 256 threads over a plane of `cells` words of LDS at s_cell (free on entry; what else
 * of LDS cell_of reads is written by the caller, before the call).  The workgroup is kProjBlock points of one row's frame
 * (k_submap_float_splat's shape).  kMaps: per entry of the row (a uniform loop), the moved points into the entry's plane; else
 * the raw coordinates into plane pl.f (NOT an identity pose).  cell_of(x, y, label): the point's cell, or -1.  The LDS plane
 * takes the workgroup's maxima, and only its non-zero cells go out: a cell's value is 0 ... 127, 0 is "empty". */
template <bool kMaps, class Cell>
__device__ __forceinline__ void lds_max_splat(const bev_point_t *__restrict__ clouds, const ProjFrame *__restrict__ tab,
                                              const uint32_t *__restrict__ ent0, int nf, const bevsub::Entry *__restrict__ entries,
                                              int skip_label0, float lidar_to_ground, int cells, uint32_t *s_cell,
                                              uint32_t *__restrict__ planes, Cell cell_of)
{
    const PackedPlace pl = packed_place(tab, nf, blockIdx.x + tab[0].blk0);
    const uint32_t n = pl.n, k0 = pl.k0;
    for (int i = (int)threadIdx.x; i < cells; i += 256) s_cell[i] = 0u;
    float4 a[kProjPerThread];
    int label[kProjPerThread];
    load_packed_records(clouds + pl.off, n, k0, skip_label0 != 0, 1, a, label);
    __syncthreads();
    const uint32_t e0 = kMaps ? ent0[pl.f] : 0u, e1 = kMaps ? ent0[pl.f + 1] : 1u;
    for (uint32_t e = e0; e < e1; ++e) {
        bevsub::Entry en;
        if (kMaps) en = entries[e];
#pragma unroll
        for (int j = 0; j < kProjPerThread; ++j) {
            float x = a[j].x, y = a[j].y, z = a[j].z;
            if (kMaps) transform_xyz(en.m, a[j].x, a[j].y, a[j].z, x, y, z);
            int cell = cell_of(x, y, label[j]);
            if (k0 + (uint32_t)j * 256u >= n) cell = -1;
            const int v = place_value(z, lidar_to_ground);
            if (cell >= 0 && v > 0) atomicMax(&s_cell[cell], (uint32_t)v);
        }
        __syncthreads();
        uint32_t *__restrict__ plane = planes + (size_t)(kMaps ? en.grid : (uint32_t)pl.f) * (size_t)cells;
        for (int i = (int)threadIdx.x; i < cells; i += 256) {
            const uint32_t v = s_cell[i];
            if (v) {
                atomicMax(&plane[i], v);
                s_cell[i] = 0u; /* (the thread that zeroes a cell is the one that read it) */
            }
        }
        __syncthreads();
    }
}

/* lds_max_splat over the polar cells of a descriptor; the ring edges lie in LDS beside the plane */
template <bool kMaps>
__global__ __launch_bounds__(256) void k_place_splat(const bev_point_t *__restrict__ clouds, const ProjFrame *__restrict__ tab,
                                                     const uint32_t *__restrict__ ent0, int nf,
                                                     const bevsub::Entry *__restrict__ entries,
                                                     const float *__restrict__ edge2, PlaceShape ps, uint32_t *__restrict__ planes)
{
    __shared__ float s_edge[kPlaceMaxRings + 1];
    __shared__ uint32_t s_cell[kPlaceMaxRings * kPlaceMaxSectors];
    if ((int)threadIdx.x <= ps.n_rings) s_edge[threadIdx.x] = edge2[threadIdx.x];
    lds_max_splat<kMaps>(clouds, tab, ent0, nf, entries, ps.skip_label0, ps.lidar_to_ground, ps.n_rings * ps.n_sectors, s_cell, planes,
                         [=](float x, float y, int label) { return place_cell(s_edge, ps.n_rings, ps.n_sectors, x, y, label, ps.skip_label0); });
}

/* One wave per descriptor, lane s its sector s: the column's bytes, its squared length, its unit values padded to
 * kPlaceMaxRings rings (and the columns past n_sectors to zero), the mask of non-empty columns. */
__global__ __launch_bounds__(64) void k_place_finish(const uint32_t *__restrict__ planes, PlaceShape ps, uint8_t *__restrict__ desc,
                                                     PlaceHandle *__restrict__ units)
{
    const int s = (int)threadIdx.x, cells = ps.n_rings * ps.n_sectors;
    const size_t g = blockIdx.x;
    const uint32_t *__restrict__ plane = planes + g * (size_t)cells;
    int v[kPlaceMaxRings];
    int n2 = 0;
#pragma unroll
    for (int r = 0; r < kPlaceMaxRings; ++r) {
        v[r] = (r < ps.n_rings && s < ps.n_sectors) ? (int)plane[r * ps.n_sectors + s] : 0;
        n2 += v[r] * v[r];
    }
    if (desc && s < ps.n_sectors) {
#pragma unroll
        for (int r = 0; r < kPlaceMaxRings; ++r)
            if (r < ps.n_rings) desc[g * (size_t)cells + (size_t)(r * ps.n_sectors + s)] = (uint8_t)v[r];
    }
    if (!units) return;
    const uint64_t mask = __ballot(n2 > 0);
    PlaceHandle *__restrict__ h = units + g;
#pragma unroll
    for (int w = 0; w < kPlaceWords; ++w) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (n2 > 0) word |= (uint32_t)place_unit(v[4 * w + b], n2) << (8 * b);
        h->unit[s][w] = word;
    }
    if (s == 0) h->mask = mask;
    if (s < (int)(sizeof h->pad / sizeof h->pad[0])) h->pad[s] = 0u;
}

/* a * b summed over the four bytes of each, + c: the values are 0 ... 127, so signed and unsigned forms are both exact */
__device__ __forceinline__ uint32_t place_dot4(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int k = 0; k < 4; ++k) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
    return c;
#endif
}

/* a score on its way through a reduction: (S, cnt, shift) of a pair, idx what breaks a tie (the shift, or the candidate) */
struct PlaceScore {
    int32_t s, cnt, shift, idx;
};
__device__ __forceinline__ bool place_score_better(const PlaceScore &a, const PlaceScore &b)
{
    return place_better(a.s, a.cnt, a.idx, b.s, b.cnt, b.idx);
}
/* the best score of a wave, in every lane (place_better is a strict total order over distinct idx: a butterfly will do) */
__device__ __forceinline__ PlaceScore place_wave_best(PlaceScore a)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        PlaceScore b;
        b.s = __shfl_xor(a.s, d);
        b.cnt = __shfl_xor(a.cnt, d);
        b.shift = __shfl_xor(a.shift, d);
        b.idx = __shfl_xor(a.idx, d);
        if (place_score_better(b, a)) a = b;
    }
    return a;
}
constexpr int32_t kPlaceNoIdx = 0x7fffffff; /* a score that stands for nothing: cnt 0 and this idx lose to every other */

/* Workgroup (x, y): query q0 + y against the candidates of tile x, kPlaceTile of them, a wave a candidate at a time.  The
 * query's unit columns lie in LDS as the handle has them ([column][word]: every lane reads the same word, a broadcast); a
 * wave's candidate lies word-major ([word][column]: lane n reads column (j + n) % C, consecutive lanes consecutive banks).
 * Lane n sums shift n: C * kWords dot products of four rings; the wave then picks the pair's best shift.  kWords: the words of
 * a column that hold rings, ceil(n_rings / 4).  A tile wholly past the query's limit does nothing. */
template <int kWords>
__global__ __launch_bounds__(256) void k_place_pairs(const PlaceHandle *__restrict__ uq, int q0, const PlaceHandle *__restrict__ udb,
                                                     int n_db, const int32_t *__restrict__ limit, int n_sectors,
                                                     uint2 *__restrict__ pairs)
{
    __shared__ uint32_t s_q[kPlaceMaxSectors * kWords];
    __shared__ uint32_t s_c[4][kWords * kPlaceMaxSectors];
    const int q = q0 + (int)blockIdx.y, c0 = (int)blockIdx.x * kPlaceTile;
    const int lim = limit ? limit[q] : n_db;
    if (c0 >= lim) return;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const PlaceHandle *__restrict__ hq = uq + q;
    for (int i = (int)threadIdx.x; i < kPlaceMaxSectors * kWords; i += 256) s_q[i] = hq->unit[i / kWords][i % kWords];
    const uint64_t qmask = hq->mask;
    for (int round = 0; round < kPlaceTile / 4; ++round) {
        const int c = c0 + round * 4 + wave;
        const bool live = c < lim;
        __syncthreads(); /* (the query is there; the last round's reads are done) */
        if (live) {
#pragma unroll
            for (int w = 0; w < kWords; ++w) s_c[wave][w * kPlaceMaxSectors + lane] = udb[c].unit[lane][w];
        }
        __syncthreads();
        if (!live) continue;
        PlaceScore sc{0, 0, lane, kPlaceNoIdx};
        if (lane < n_sectors) {
            uint32_t acc = 0u;
            int idx = lane;
            for (int j = 0; j < n_sectors; ++j) {
#pragma unroll
                for (int w = 0; w < kWords; ++w) acc = place_dot4(s_q[j * kWords + w], s_c[wave][w * kPlaceMaxSectors + idx], acc);
                idx = idx + 1 == n_sectors ? 0 : idx + 1;
            }
            sc.s = (int32_t)acc;
            sc.cnt = __popcll(place_common(qmask, udb[c].mask, lane, n_sectors));
            sc.idx = lane;
        }
        sc = place_wave_best(sc);
        if (lane == 0) pairs[(size_t)blockIdx.y * (size_t)n_db + (size_t)c] = make_uint2((uint32_t)sc.s, (uint32_t)sc.cnt | (uint32_t)sc.shift << 16);
    }
}

/* One workgroup per query: top_k rounds, each the best of the candidates that the last round's winner beats (all of them in
 * the first), so a round needs no list of what is taken.  Rows past the candidates: match_idx -1, distance 2.0, shift 0. */
__global__ __launch_bounds__(256) void k_place_topk(const uint2 *__restrict__ pairs, int q0, int n_db, const int32_t *__restrict__ limit,
                                                    int n_sectors, int top_k, bev_place_hit_t *__restrict__ hits)
{
    __shared__ PlaceScore s_best[4];
    const int q = q0 + (int)blockIdx.x;
    const int lim = limit ? limit[q] : n_db;
    const uint2 *__restrict__ row = pairs + (size_t)blockIdx.x * (size_t)n_db;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    PlaceScore prev{0, 0, 0, kPlaceNoIdx};
    for (int k = 0; k < top_k; ++k) {
        PlaceScore best{0, 0, 0, kPlaceNoIdx};
        if (k == 0 || prev.idx != kPlaceNoIdx) {
            for (int c = (int)threadIdx.x; c < lim; c += 256) {
                const uint2 p = row[c];
                const PlaceScore sc{(int32_t)p.x, (int32_t)(p.y & 0xffffu), (int32_t)(p.y >> 16), c};
                if (k > 0 && !place_score_better(prev, sc)) continue;
                if (place_score_better(sc, best)) best = sc;
            }
        }
        best = place_wave_best(best);
        __syncthreads(); /* (the last round's s_best has been read) */
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        best = s_best[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (place_score_better(s_best[w], best)) best = s_best[w];
        prev = best;
        if (threadIdx.x == 0) {
            bev_place_hit_t h;
            const bool any = best.idx != kPlaceNoIdx;
            h.query_idx = q;
            h.match_idx = any ? best.idx : -1;
            h.angle_guess = any ? place_angle(best.shift, n_sectors) : 0.0f;
            h.shift = any ? best.shift : 0;
            h.distance = any ? place_distance(best.s, best.cnt) : kPlaceNoDistance;
            hits[(size_t)q * (size_t)top_k + (size_t)k] = h;
        }
    }
}

} /* namespace bevk */

#endif /* BEV_PLACE_H */
