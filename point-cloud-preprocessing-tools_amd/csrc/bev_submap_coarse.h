/*
 * bev_submap_coarse.h — scan-to-map coarse ICP: a query frame's PointNormal cloud registered point-to-plane against a MAP, the
 * concatenation of the PointNormal clouds of the map's (frame, pose) entries, each moved by its entry's matrix
 * (bev_submap_coarse_registration_device_resident).  The host plan is §6k's (bev_submap_reg_plan.h) with every
 * frame counted at the call's stride and a PointNormal map's bytes; an entry's slot word holds the FRAME it moves.  Per launch
 * group of the plan:
 *   k_submap_pn_target   per map            : submap_pn_concat (shared with k_submap_pn_move, bev_submap_pn_vox.h): the entries'
 *                                             row counts min(counts[frame], stride) scanned into their first target index
 *                                             (submap_scan, bev_submap_reg.h), every entry's rows moved by pn_move into the
 *                                             map's row array; then reg_grid_build<kIcpCells> over the moved positions
 *                                             (bounds of the MOVED points)
 *   k_submap_coarse_icp  per (match, guess) : submap_coarse_problem (shared with bev_wide_icp.h; k_icp's loop, of which k_icp
 *                                             keeps a copy, see below), the target read from the map's arrays
 * then k_icp_best as it is.  A target point's index is its position in the concatenation: entries in map order, rows ascending
 * inside an entry; the search's "lowest index on ties" is over that index.  Rows that a matrix makes non-finite keep their
 * index and are not searchable; a moved normal with a non-finite component adds nothing to the sums, but its correspondence
 * counts (§6c).  No float or double sum depends on an atomic (the sums are reg_pass's).
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_COARSE_H
#define BEV_SUBMAP_COARSE_H

#include "bev_submap_reg_plan.h"

namespace bevk {
using namespace bevx;

static_assert(bevsubreg::kCoarseGridCells == (uint32_t)kIcpCells, "the plan sizes a PointNormal map's cell offsets");
static_assert(bevsubreg::kCoarseRowBytes == 48 + 16, "a moved row and its searchable copy");

/* one PointNormal record (three float4: x y z pad | nx ny nz pad | curvature pads) under the row-major 3 x 4 m: the position
 * by transform_xyz (bev_transform_cloud's association), the normal by the same association without the translation, neither
 * renormalised nor flipped; the curvature copied, the pads 0, every NaN canonical.  Plain float, no FMA. */
__device__ __forceinline__ void pn_move(const float m[12], const float4 p, const float4 nr, const float4 cv, float4 &op,
                                        float4 &on, float4 &oc)
{
    float tx, ty, tz;
    transform_xyz(m, p.x, p.y, p.z, tx, ty, tz);
    op = make_float4(rf_canon(tx), rf_canon(ty), rf_canon(tz), 0.0f);
    on = make_float4(rf_canon(m[0] * nr.x + (m[1] * nr.y + m[2] * nr.z)), rf_canon(m[4] * nr.x + (m[5] * nr.y + m[6] * nr.z)),
                     rf_canon(m[8] * nr.x + (m[9] * nr.y + m[10] * nr.z)), 0.0f);
    oc = make_float4(rf_canon(cv.x), 0.0f, 0.0f, 0.0f);
}

/* Steps 1 and 2 of a PointNormal map's target, by the whole workgroup (submap_move's counterpart, bev_submap_reg.h): the
 * entries' row counts min(counts[frame], stride) scanned into ent_start, every entry's rows moved into rows.  Returns the map's
 * row count; no barrier behind the rows: a caller whose other waves read them back sets one (k_submap_pn_target;
 * k_submap_pn_move, bev_submap_pn_vox.h, leaves them to the next launch). */
__device__ __forceinline__ uint32_t submap_pn_concat(const bevsubreg::Map &mp, const bevsubreg::Entry *entries, const float *pn,
                                                     size_t stride, const uint32_t *counts, uint32_t *ent_start, float *rows,
                                                     uint32_t *wave_sum, uint32_t &s_base)
{
    /* 1: the entries' first target indices (a map's total is at most n_ent * stride <= BEV_SUBMAP_COARSE_MAX_TARGET: the
     * host checked that) */
    const uint32_t n = submap_scan(
        mp, [&](uint32_t e) { return min(counts[entries[mp.ent0 + e].slot], (uint32_t)stride); }, ent_start, wave_sum, s_base);
    /* 2: every entry's rows under its matrix (a workgroup-uniform loop over the entries) */
    for (uint32_t e = 0; e < mp.n_ent; ++e) {
        const bevsubreg::Entry &en = entries[mp.ent0 + e];
        const uint32_t frame = en.slot, nr = min(counts[frame], (uint32_t)stride), at = ent_start[mp.ent0 + e];
        float m[12];
        for (int k = 0; k < 12; ++k) m[k] = en.m[k];
        const float4 *in = reinterpret_cast<const float4 *>(pn + (size_t)frame * stride * 12);
        float4 *out = reinterpret_cast<float4 *>(rows + (size_t)at * 12);
        for (uint32_t i = threadIdx.x; i < nr; i += kRegThreads) {
            float4 op, on, oc;
            pn_move(m, in[(size_t)i * 3], in[(size_t)i * 3 + 1], in[(size_t)i * 3 + 2], op, on, oc);
            out[(size_t)i * 3] = op;
            out[(size_t)i * 3 + 1] = on;
            out[(size_t)i * 3 + 2] = oc;
        }
    }
    return n;
}

/* Map map0 + blockIdx.x of the plan: the scan, the moved rows, the search grid of the moved positions.  The workgroup's own
 * global writes (ent_start, the rows) are read back by its other waves behind a barrier, as in submap_move. */
__global__ __launch_bounds__(kIcpThreads) void k_submap_pn_target(const bevsubreg::Map *maps, uint32_t map0,
                                                                  const bevsubreg::Entry *entries, const float *pn,
                                                                  size_t stride, const uint32_t *counts, uint32_t *ent_start,
                                                                  SubmapCoarseWork t)
{
    __shared__ uint32_t wave_sum[kRegWaves];
    __shared__ uint32_t s_base;
    const bevsubreg::Map mp = maps[map0 + blockIdx.x];
    float *rows = t.rows + mp.pt0 * 12;
    const uint32_t n = submap_pn_concat(mp, entries, pn, stride, counts, ent_start, rows, wave_sum, s_base);
    __syncthreads();
    /* 3: the search grid of the moved positions */
    reg_grid_build<kIcpCells>(n, IcpRows{rows}, t.hdr + blockIdx.x, t.cell_off + (size_t)blockIdx.x * (kIcpCells + 1),
                              t.sorted + mp.pt0);
}

/* One problem by the whole workgroup: k_icp's loop (bev_icp.h) against a target that is read only through tgt (its
 * PointNormal rows, by target index), tpts (its searchable points by cell), the grid's header *hdr and the cell offsets goff:
 * copied into IcpShared::off where kLdsOff (a grid of at most 64 x 64 cells: k_submap_coarse_icp), else left in global memory
 * and sh.off unused (the grids sized to the target: k_submap_coarse_icp_wide, k_icp_wide; bev_wide_icp.h).  cur: n_src float4
 * of scratch.  k_icp's own loop is a COPY of this one, statement for statement, not a call: with the body shared, k_icp went
 * from 194 to 196 VGPRs (scripts/isa_stats.sh), and bev_fine.h tells how easily such bodies move, so k_icp
 * stays untouched.  The parts (icp_step, icp_nn, reg_pass, reg_start, reg_advance, reg_finish) are shared; a change to one of
 * the two bodies belongs in the other. */
template <bool kLdsOff>
__device__ __forceinline__ void submap_coarse_problem(IcpShared &sh, uint32_t n_src, const float *src, const float *tgt,
                                                      const float4 *tpts, const IcpGridHdr *hdr, const uint32_t *goff,
                                                      float4 *cur, const float *guess, const bev_icp_params_t &prm,
                                                      bev_icp_result_t *result)
{
    const int tid = threadIdx.x;
    if (tid == 0) sh.hdr = *hdr;
    __syncthreads();
    const IcpGridHdr h = sh.hdr;
    if (kLdsOff)
        for (int c = tid; c <= h.nx * h.ny; c += kIcpThreads) sh.off[c] = goff[c];
    const uint32_t *off = kLdsOff ? sh.off : goff;
    reg_start(sh.loop, guess, n_src, IcpRows{src}, cur);
    __syncthreads();
    const double D2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    double prev = 1.7976931348623157e308; /* DBL_MAX (thread 0's copy is the one used) */
    while (true) {
        reg_pass<0, 28>(sh.sums, n_src, [&](uint32_t i, float *, double *t) -> bool {
            const float4 s = cur[i];
            if (!finite3(s.x, s.y, s.z)) return false;
            float d;
            uint32_t j;
            if (!icp_nn(h, off, tpts, s.x, s.y, s.z, D2, d, j) || !((double)d <= D2)) return false;
            const float4 tp = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12);
            const float4 tn = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12 + 4);
            const float nx = tn.x, ny = tn.y, nz = tn.z;
            if (finite3(nx, ny, nz)) {
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
            if (sh.sums.cnt < 3) sh.loop.state = 5; /* NO_CORRESPONDENCES */
            else icp_step(sh, prm, prev);
        }
        __syncthreads();
        if (sh.loop.state != 0) break;
        reg_advance(sh.loop, n_src, cur);
    }
    reg_finish(sh.sums, sh.loop, n_src, IcpRows{src}, h, off, tpts, result);
}

/* probs: the launch's problems (tgt_slot: the map's index in the plan; tgt_frame is not read); §6c's loop against the map's
 * arrays */
__global__ __launch_bounds__(kIcpThreads) void k_submap_coarse_icp(const float *pn, size_t stride, const uint32_t *counts,
                                                                   const IcpProblem *probs, const bevsubreg::Map *maps,
                                                                   uint32_t map0, SubmapCoarseWork t, bev_icp_params_t prm,
                                                                   bev_icp_result_t *results)
{
    __shared__ IcpShared sh;
    const IcpProblem pb = probs[blockIdx.x];
    const uint64_t pt0 = maps[pb.tgt_slot].pt0;
    const uint32_t g = pb.tgt_slot - map0;
    submap_coarse_problem<true>(sh, min(counts[pb.src_frame], (uint32_t)stride), pn + (size_t)pb.src_frame * stride * 12,
                                t.rows + pt0 * 12, t.sorted + pt0, t.hdr + g, t.cell_off + (size_t)g * (kIcpCells + 1),
                                t.cur + (size_t)blockIdx.x * stride, pb.guess, prm, results + pb.result);
}

void launch_submap_pn_target(const void *maps, uint32_t map0, int n_maps, const void *entries, const float *pn, size_t stride,
                             const uint32_t *counts, uint32_t *ent_start, const SubmapCoarseWork &t, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_pn_target, dim3(n_maps), dim3(kIcpThreads), 0, st, static_cast<const bevsubreg::Map *>(maps),
                           map0, static_cast<const bevsubreg::Entry *>(entries), pn, stride, counts, ent_start, t);
}

void launch_submap_coarse_icp(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                              const void *maps, uint32_t map0, const SubmapCoarseWork &t, const bev_icp_params_t &prm,
                              bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_submap_coarse_icp, dim3(n), dim3(kIcpThreads), 0, st, pn, stride, counts, probs,
                           static_cast<const bevsubreg::Map *>(maps), map0, t, prm, results);
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_COARSE_H */
