/*
 * bev_submap_top.h — the top part over the UNION of a map's moved full clouds, in front of the union voxel grid and 2-D normals
 * of bev_submap_pn_vox.h (bev_submap_top_part_cloud_device_resident, bev_submap_top_part_coarse_registration_device_resident;
 * DESIGN.md §6r):
 *   top(g) = bev_top_part_flatten(union(g)),  union(g) = the concatenation of bev_transform_cloud(frame(e), pose(e)).
 * The union's records are never written.  A kept record is one 64-bit key
 *   cell (7 bits) << 57 | rf_z_desc_key(moved z) (32) << 25 | union index (25)
 * at its union index (~0 where the record is skipped), and a cell's round(0.2f * n) highest records are the keys at or below
 * the cell's k-th smallest key, which a radix select finds without sorting the cell.  The keys are unique (the index bits), so
 * that threshold is exact, and ties in z go to the lower union index, that is the earlier entry.  Per launch group of the plan
 * (bev_submap_reg_plan.h with top_union):
 *   k_submap_top_keys     per (part, map) : the entries in map order: transform_xyz (bev_exact.h), rf_top_cell and rf_z_desc_key
 *                                           (bev_regfront.h) of the moved record, the key; the cells' counts in LDS, then global
 *   k_submap_top_cells    per map         : a cell's rank round(0.2f * n) where n >= 20, the selection's size and the sort's header
 *   k_submap_top_hist     per (part, map) : one digit of kTopDigitBits bits, most significant first: the histogram per (cell,
 *                                           digit) of the keys that still share their cell's prefix, in LDS, then global
 *   k_submap_top_scan     per map         : per cell: the bucket that holds the rank; the prefix grows by its digit, or the cell is
 *                                           finished: the bucket's cumulative count is the rank (always so at the last digit)
 *   k_submap_top_compact  per (part, map) : the keys at or below their cell's threshold into the selection, in any order (a slot
 *                                           cursor, one global add per workgroup), padded with ~0 to its power of two
 *   k_submap_vox_tile, k_submap_vox_global (bev_submap_vox.h) as they are: cell, then z descending, then index
 *   k_submap_top_rows     per (part, map) : the sorted keys' records moved again: the rows x y 0 0 | 0 0 0 0 | 0 0 0 0, which are
 *                                           bev_submap_pn_vox.h's moved rows
 *   k_submap_pn_keys .. k_submap_pn_grid (bev_submap_pn_vox.h) as they are, with
 *   k_submap_top_overflow per map         : behind k_submap_pn_finish: a map in the voxel grid's overflow branch keeps top(g) as its
 *                                           positions and is marked for k_submap_pn_normals' full scan
 * then k_submap_coarse_icp and k_icp_best as they are.  No float value depends on an atomic or on which workgroup ran first:
 * atomics count records and hand out slots, and the sort removes the slots' order.  Every workgroup has 256 threads.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_TOP_H
#define BEV_SUBMAP_TOP_H

#include "bev_submap_reg_plan.h"

namespace bevk {

static_assert(sizeof(SubtopCells) == bevsubreg::kTopCellBytes, "the plan counts these bytes per map");
static_assert(kTopHistWords * 4 == bevsubreg::kTopHistBytes, "the plan counts these bytes per map");
static_assert(kRfCells <= 127, "a cell and the pad key's 127 in 7 bits");

constexpr uint64_t kTopKeyMask = (1ull << kTopKeyBits) - 1u;
constexpr uint32_t kTopIndexMask = (1u << kTopIndexBits) - 1u;

/* ctr[idx] += 1 for every lane with idx >= 0, called by whole waves.  One cell often holds most of a map and its keys share
 * their leading digits, so most lanes of a wave name one counter: the lanes that agree with the first waiting lane are counted
 * by a ballot and added once, twice over; what is left adds for itself. */
__device__ __forceinline__ void subtop_count(uint32_t *ctr, int idx)
{
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const unsigned long long waiting = __ballot(idx >= 0);
        if (!waiting) return;
        const int leader = __ffsll((long long)waiting) - 1;
        const int lead = __shfl(idx, leader);
        const unsigned long long same = __ballot(idx == lead);
        if (lane == leader) atomicAdd(&ctr[lead], (uint32_t)__popcll(same));
        if (idx == lead) idx = -1;
    }
    if (idx >= 0) atomicAdd(&ctr[idx], 1u);
}

/* records of a map's union: where its last entry ends (the plan's pad words: an entry's first union index, its records) */
__device__ __forceinline__ uint32_t subtop_union_n(const bevsubreg::Map &mp, const bevsubreg::Entry *entries)
{
    if (mp.n_ent == 0) return 0u;
    const bevsubreg::Entry &last = entries[mp.ent0 + mp.n_ent - 1u];
    return last.pad[0] + last.pad[1];
}

/* part blockIdx.x of map map0 + blockIdx.y: the keys of the map's union at t.ukeys + u0, the cells' counts */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_keys(const bevsubreg::Map *maps, uint32_t map0,
                                                                 const bevsubreg::Entry *entries, const FineSlot *slots,
                                                                 const bev_point_t *clouds, SubmapTopWork t)
{
    __shared__ uint32_t cnt[kRfCells];
    const uint32_t g = blockIdx.y, tid = threadIdx.x;
    const bevsubreg::Map mp = maps[map0 + g];
    uint64_t *keys = t.ukeys + t.u0[map0 + g];
    for (uint32_t c = tid; c < (uint32_t)kRfCells; c += kRegThreads) cnt[c] = 0;
    __syncthreads();
    for (uint32_t e = 0; e < mp.n_ent; ++e) {
        const bevsubreg::Entry &en = entries[mp.ent0 + e];
        const uint32_t start = en.pad[0], n = en.pad[1]; /* (the plan's: first union index, records) */
        const bev_point_t *in = clouds + slots[en.slot].off;
        float m[12];
        for (int k = 0; k < 12; ++k) m[k] = en.m[k];
        for (uint32_t base = blockIdx.x * kRegThreads; base < n; base += gridDim.x * kRegThreads) { /* (whole waves) */
            const uint32_t i = base + tid;
            int cell = -1;
            if (i < n) {
                bev_point_t q = in[i];
                float tx, ty, tz;
                transform_xyz(m, q.x, q.y, q.z, tx, ty, tz);
                q.x = tx, q.y = ty, q.z = tz;
                cell = rf_top_cell(q);
                keys[start + i] = cell < 0 ? ~0ull
                                           : (uint64_t)cell << kTopKeyBits | (uint64_t)rf_z_desc_key(tz) << kTopIndexBits |
                                                 (uint64_t)(start + i);
            }
            subtop_count(cnt, cell);
        }
    }
    __syncthreads();
    for (uint32_t c = tid; c < (uint32_t)kRfCells; c += kRegThreads)
        if (cnt[c]) atomicAdd(&t.cells[g].cnt[c], cnt[c]);
}

/* map map0 + blockIdx.x: the ranks (rf_top_rank, as k_rf_cells has them), the selection's size; the sort's header */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_cells(SubmapTopWork t, SubvoxHdr *vh)
{
    __shared__ uint32_t s_k[kRfCells];
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    SubtopCells &cs = t.cells[g];
    uint32_t k = 0;
    if (tid < (uint32_t)kRfCells) {
        k = rf_top_rank(cs.cnt[tid]);
        cs.k[tid] = cs.rank[tid] = s_k[tid] = k;
        cs.prefix[tid] = 0;
        cs.thr[tid] = 0;
    }
    const uint32_t open = (uint32_t)__syncthreads_count(k != 0);
    if (tid == 0) {
        uint32_t m = 0;
        for (int c = 0; c < kRfCells; ++c) m += s_k[c];
        cs.n_sel = m;
        cs.open = open;
        SubvoxHdr h{};
        h.n = h.n_out = m; /* (with pn_leaf == 0 the rows of top(g) are the cloud call's target) */
        h.np2 = m ? rf_pow2(m) : 0u;
        vh[g] = h;
    }
}

/* part blockIdx.x of map map0 + blockIdx.y, the digit at `shift`: cs.hist[cell][digit] += the keys of an open cell whose bits
 * above the digit are the cell's prefix */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_hist(const bevsubreg::Map *maps, uint32_t map0,
                                                                 const bevsubreg::Entry *entries, SubmapTopWork t, uint32_t shift)
{
    __shared__ uint32_t hist[kTopHistWords];
    __shared__ uint64_t s_prefix[kRfCells];
    __shared__ uint32_t s_rank[kRfCells];
    const uint32_t g = blockIdx.y, tid = threadIdx.x;
    const SubtopCells &cs = t.cells[g];
    if (cs.open == 0) return; /* (workgroup-uniform: every cell has its threshold) */
    const uint32_t n = subtop_union_n(maps[map0 + g], entries);
    if (blockIdx.x * kRegThreads >= n) return;
    const uint64_t *keys = t.ukeys + t.u0[map0 + g];
    for (uint32_t i = tid; i < kTopHistWords; i += kRegThreads) hist[i] = 0;
    if (tid < (uint32_t)kRfCells) s_prefix[tid] = cs.prefix[tid], s_rank[tid] = cs.rank[tid];
    __syncthreads();
    for (uint32_t base = blockIdx.x * kRegThreads; base < n; base += gridDim.x * kRegThreads) { /* (whole waves) */
        const uint32_t i = base + tid;
        int idx = -1;
        if (i < n) {
            const uint64_t key = keys[i];
            const uint32_t cell = (uint32_t)(key >> kTopKeyBits);
            const uint64_t k57 = key & kTopKeyMask;
            if (cell < (uint32_t)kRfCells && s_rank[cell] != 0 && (k57 >> (shift + kTopDigitBits)) == s_prefix[cell])
                idx = (int)(cell * kTopDigits + ((uint32_t)(k57 >> shift) & (kTopDigits - 1u)));
        }
        subtop_count(hist, idx);
    }
    __syncthreads();
    uint32_t *out = t.hist + (size_t)g * kTopHistWords;
    for (uint32_t i = tid; i < kTopHistWords; i += kRegThreads)
        if (hist[i]) atomicAdd(&out[i], hist[i]);
}

/* map map0 + blockIdx.x behind the digit at `shift`: an open cell's bucket; the histogram is zero again on return */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_scan(SubmapTopWork t, uint32_t shift)
{
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    SubtopCells &cs = t.cells[g];
    if (cs.open == 0) return; /* (workgroup-uniform; the histogram was not touched) */
    uint32_t *hist = t.hist + (size_t)g * kTopHistWords;
    uint32_t rank = tid < (uint32_t)kRfCells ? cs.rank[tid] : 0u;
    if (rank != 0) {
        const uint64_t prefix = cs.prefix[tid];
        uint32_t cum = 0, d = 0;
        for (; d < kTopDigits; ++d) {
            const uint32_t h = hist[tid * kTopDigits + d];
            if (cum + h >= rank) break;
            cum += h;
        }
        /* (d == kTopDigits: fewer keys than the rank, which the counts exclude; then the cell takes what shares its prefix) */
        const uint64_t upto = prefix << kTopDigitBits | (uint64_t)min(d, kTopDigits - 1u);
        const uint32_t in_bucket = d < kTopDigits ? hist[tid * kTopDigits + d] : 0u;
        if (d == kTopDigits || cum + in_bucket == rank || shift == 0) {
            cs.thr[tid] = (((upto + 1u) << shift) - 1u) & kTopKeyMask; /* every key of the cell up to the bucket's last */
            rank = 0;
        } else {
            cs.prefix[tid] = upto;
            rank -= cum;
        }
        cs.rank[tid] = rank;
    }
    const uint32_t open = (uint32_t)__syncthreads_count(rank != 0); /* (the barrier: the buckets are read) */
    for (uint32_t i = tid; i < kTopHistWords; i += kRegThreads) hist[i] = 0;
    if (tid == 0) cs.open = open;
}

/* part blockIdx.x of map map0 + blockIdx.y: the selected keys, cell included, into the map's sort keys; the padding.  The
 * workgroup reads its keys twice: it counts its selected keys, takes that many slots of the map's cursor in ONE global add
 * (a wave's add per 64 keys on one address was the whole kernel's time: DESIGN.md §6r), then hands them out from LDS */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_compact(const bevsubreg::Map *maps, uint32_t map0,
                                                                    const bevsubreg::Entry *entries, SubmapTopWork t,
                                                                    SubmapVoxWork v)
{
    __shared__ uint64_t s_thr[kRfCells];
    __shared__ uint32_t s_k[kRfCells];
    __shared__ uint32_t s_total, s_base, s_cur;
    const uint32_t g = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    SubtopCells &cs = t.cells[g];
    const uint32_t n = subtop_union_n(maps[map0 + g], entries), m = cs.n_sel, np2 = v.vh[g].np2;
    uint64_t *sel = v.keys + v.key0[map0 + g];
    const uint64_t *keys = t.ukeys + t.u0[map0 + g];
    if (tid < (uint32_t)kRfCells) s_thr[tid] = cs.thr[tid], s_k[tid] = cs.k[tid];
    if (tid == 0) s_total = 0, s_cur = 0;
    __syncthreads();
    const auto taken = [&](uint64_t key) {
        const uint32_t cell = (uint32_t)(key >> kTopKeyBits);
        return cell < (uint32_t)kRfCells && s_k[cell] != 0 && (key & kTopKeyMask) <= s_thr[cell];
    };
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * kRegThreads + tid; i < n; i += gridDim.x * kRegThreads) mine += taken(keys[i]) ? 1u : 0u;
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0 && mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (tid == 0) s_base = s_total ? atomicAdd(&cs.cursor, s_total) : 0u;
    __syncthreads();
    const uint32_t base0 = s_base;
    for (uint32_t base = blockIdx.x * kRegThreads; base < n && s_total; base += gridDim.x * kRegThreads) { /* (whole waves) */
        const uint32_t i = base + tid;
        const uint64_t key = i < n ? keys[i] : ~0ull;
        const bool take = i < n && taken(key);
        const unsigned long long mask = __ballot(take);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        uint32_t first = 0;
        if ((int)lane == leader) first = atomicAdd(&s_cur, (uint32_t)__popcll(mask));
        first = __shfl(first, leader);
        const uint32_t pos = base0 + first + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (take && pos < m) sel[pos] = key; /* (pos < m: the thresholds select exactly m keys) */
    }
    for (uint32_t i = m + blockIdx.x * kRegThreads + tid; i < np2; i += gridDim.x * kRegThreads) sel[i] = ~0ull;
}

/* part blockIdx.x of map map0 + blockIdx.y: row r of top(g) from sorted key r: its record, moved as k_submap_top_keys moved it */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_rows(const bevsubreg::Map *maps, uint32_t map0,
                                                                 const bevsubreg::Entry *entries, const FineSlot *slots,
                                                                 const bev_point_t *clouds, SubmapTopWork t, SubmapPnVoxWork p)
{
    const uint32_t g = blockIdx.y;
    const bevsubreg::Map mp = maps[map0 + g];
    const uint32_t m = t.cells[g].n_sel, n = subtop_union_n(mp, entries);
    const uint64_t *sel = p.v.keys + p.v.key0[map0 + g];
    float4 *rows = reinterpret_cast<float4 *>(p.moved + mp.pt0 * 12);
    const bevsubreg::Entry *ent = entries + mp.ent0;
    for (uint32_t r = blockIdx.x * kRegThreads + threadIdx.x; r < m; r += gridDim.x * kRegThreads) {
        const uint32_t u = (uint32_t)sel[r] & kTopIndexMask;
        float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (u < n && mp.n_ent != 0) {
            uint32_t lo = 0, hi = mp.n_ent; /* the last entry that starts at or before u: the one that holds it */
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ent[mid].pad[0] <= u) lo = mid;
                else hi = mid;
            }
            const bevsubreg::Entry &en = ent[lo];
            const uint32_t i = u - en.pad[0];
            if (i < en.pad[1]) {
                const bev_point_t &q = clouds[slots[en.slot].off + i];
                float tx, ty, tz;
                transform_xyz(en.m, q.x, q.y, q.z, tx, ty, tz);
                row = make_float4(tx, ty, 0.0f, 0.0f);
            }
        }
        rows[(size_t)r * 3] = row;
        rows[(size_t)r * 3 + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rows[(size_t)r * 3 + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

/* map map0 + blockIdx.x behind k_submap_pn_finish: "leaf size is too small" keeps top(g), and its normals are still computed:
 * the positions are the rows', the divisions say that an index is not known, so k_submap_pn_normals scans every point */
__global__ __launch_bounds__(kIcpThreads) void k_submap_top_overflow(const bevsubreg::Map *maps, uint32_t map0, SubmapPnVoxWork p)
{
    const uint32_t g = blockIdx.x;
    const SubvoxHdr h = p.v.vh[g];
    if (!h.overflow) return;
    const uint64_t pt0 = maps[map0 + g].pt0;
    const float4 *moved = reinterpret_cast<const float4 *>(p.moved + pt0 * 12);
    for (uint32_t i = threadIdx.x; i < h.n; i += kRegThreads) {
        p.vpos[pt0 + i] = moved[(size_t)i * 3];
        p.vidx[pt0 + i] = 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        SubvoxHdr &o = p.v.vh[g];
        o.overflow = 0;
        o.n_out = h.n;
        o.div[0] = o.div[1] = 65536u; /* (a layer of 2^32 voxels: not windowed) */
        o.div[2] = 1u;
    }
}

void launch_submap_top_keys(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries, const void *slots,
                            const bev_point_t *clouds, const SubmapTopWork &t, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_top_keys, dim3(std::max(parts, 1u), (uint32_t)n_maps), dim3(kIcpThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), map0, static_cast<const bevsubreg::Entry *>(entries),
                           static_cast<const FineSlot *>(slots), clouds, t);
}

void launch_submap_top_cells(int n_maps, const SubmapTopWork &t, SubvoxHdr *vh, hipStream_t st)
{
    if (n_maps > 0) hipLaunchKernelGGL(k_submap_top_cells, dim3(n_maps), dim3(kIcpThreads), 0, st, t, vh);
}

void launch_submap_top_digit(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries,
                             const SubmapTopWork &t, uint32_t shift, bool scan, hipStream_t st)
{
    if (n_maps <= 0) return;
    if (scan) hipLaunchKernelGGL(k_submap_top_scan, dim3(n_maps), dim3(kIcpThreads), 0, st, t, shift);
    else
        hipLaunchKernelGGL(k_submap_top_hist, dim3(std::max(parts, 1u), (uint32_t)n_maps), dim3(kIcpThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), map0, static_cast<const bevsubreg::Entry *>(entries), t, shift);
}

void launch_submap_top_compact(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries,
                               const SubmapTopWork &t, const SubmapVoxWork &v, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_top_compact, dim3(std::max(parts, 1u), (uint32_t)n_maps), dim3(kIcpThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), map0, static_cast<const bevsubreg::Entry *>(entries), t, v);
}

void launch_submap_top_rows(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries, const void *slots,
                            const bev_point_t *clouds, const SubmapTopWork &t, const SubmapPnVoxWork &p, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_top_rows, dim3(std::max(parts, 1u), (uint32_t)n_maps), dim3(kIcpThreads), 0, st,
                           static_cast<const bevsubreg::Map *>(maps), map0, static_cast<const bevsubreg::Entry *>(entries),
                           static_cast<const FineSlot *>(slots), clouds, t, p);
}

void launch_submap_top_overflow(const void *maps, uint32_t map0, int n_maps, const SubmapPnVoxWork &p, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_top_overflow, dim3(n_maps), dim3(kIcpThreads), 0, st, static_cast<const bevsubreg::Map *>(maps),
                           map0, p);
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_TOP_H */
