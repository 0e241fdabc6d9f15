/*
 * bev_submap_reg.h — scan-to-map fine ICP: a query frame's voxel cloud registered against a MAP, the concatenation of the
 * voxel clouds of the map's (frame, pose) entries, each moved by its entry's matrix (bev_submap_registration_device_resident,
 * bev_submap_registration_batch).  The host plan (bev_submap_reg_plan.h) says which voxel cloud under which
 * matrix goes into which map, in the map's own entry order; the voxel clouds are k_fine_voxel's (bev_fine.h), one per
 * distinct frame.  Per launch group of the plan:
 *   k_submap_target  per map   : the entries' voxel counts scanned into their first target index, every entry's voxel points
 *                                moved by transform_xyz (bev_exact.h: bev_transform_cloud's association, no FMA) into the
 *                                map's point array, then reg_grid_build over that array (bounds of the MOVED points)
 *   k_submap_icp     per match : fine_icp_problem (bev_fine.h), the target read from the map's arrays
 * A target point's index is its position in the concatenation: entries in map order, voxels ascending inside an entry; the
 * search's "lowest index on ties" is over that index.  Points that a matrix makes non-finite keep their index and are not
 * searchable.  No float or double sum depends on an atomic (the sums are reg_pass's).
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_REG_H
#define BEV_SUBMAP_REG_H

#include "bev_submap_reg_plan.h"

namespace bevk {
using namespace bevx;

static_assert(bevsubreg::kGridCells == (uint32_t)kFineCells, "the plan sizes a map's cell offsets");
static_assert(sizeof(bevsubreg::Slot) == sizeof(FineSlot), "k_fine_voxel reads the plan's slots");

/* An exclusive scan of the row counts count_of(e) of a map's entries e = 0 .. n_ent - 1, by the whole workgroup, 256 entries at
 * a time: ent_start (one word per entry of the call) gets every entry's first target index.  Returns the map's total; the
 * workgroup is in step on return.  (k_submap_target, k_submap_vox_move: voxel counts; k_submap_pn_target, bev_submap_coarse.h:
 * PointNormal rows.) */
template <class CountOf>
__device__ __forceinline__ uint32_t submap_scan(const bevsubreg::Map &mp, CountOf count_of, uint32_t *ent_start,
                                                uint32_t *wave_sum, uint32_t &s_base)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (uint32_t e0 = 0; e0 < mp.n_ent; e0 += kRegThreads) {
        const uint32_t e = e0 + (uint32_t)tid;
        const uint32_t v = e < mp.n_ent ? count_of(e) : 0u;
        uint32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_sum[wv] = incl;
        __syncthreads();
        uint32_t before = s_base;
        for (int q = 0; q < wv; ++q) before += wave_sum[q];
        if (e < mp.n_ent) ent_start[mp.ent0 + e] = before + incl - v;
        __syncthreads();
        if (tid == kRegThreads - 1) s_base = before + incl;
        __syncthreads();
    }
    return s_base;
}

/* Steps 1 and 2 of a map's target, by the whole workgroup: the entries' voxel counts scanned into ent_start (one word per
 * entry of the call: the entry's first target index), every entry's voxel points moved into pts.  Returns the map's point
 * count; the workgroup is in step on return.  The workgroup's own global writes (ent_start, the moved points) are read back by
 * its other waves behind a barrier: they share the CU's vector cache (rf_bitonic). */
__device__ __forceinline__ uint32_t submap_move(const bevsubreg::Map &mp, const bevsubreg::Entry *entries, const FineWork &w,
                                                uint32_t *ent_start, float4 *pts, uint32_t *wave_sum, uint32_t &s_base)
{
    const int tid = (int)threadIdx.x;
    /* 1: an exclusive scan of the entries' voxel counts (a map's total is at most BEV_SUBMAP_REG_MAX_TARGET: the host checked
     * the record counts, which bound the voxel counts) */
    const uint32_t n = submap_scan(
        mp, [&](uint32_t e) { return w.vox_n[entries[mp.ent0 + e].slot]; }, ent_start, wave_sum, s_base);
    /* 2: every entry's voxel points under its matrix (a workgroup-uniform loop over the entries) */
    for (uint32_t e = 0; e < mp.n_ent; ++e) {
        const bevsubreg::Entry &en = entries[mp.ent0 + e];
        const uint32_t slot = en.slot, nv = w.vox_n[slot], at = ent_start[mp.ent0 + e];
        float m[12];
        for (int k = 0; k < 12; ++k) m[k] = en.m[k];
        const bev_point_t *vox = w.vox + (size_t)slot * w.Pn;
        for (uint32_t i = (uint32_t)tid; i < nv; i += kRegThreads) {
            float tx, ty, tz;
            transform_xyz(m, vox[i].x, vox[i].y, vox[i].z, tx, ty, tz);
            pts[at + i] = make_float4(tx, ty, tz, 0.0f);
        }
    }
    __syncthreads();
    return n;
}

/* Map map0 + blockIdx.x of the plan: submap_move, then the search grid of the moved points. */
__global__ __launch_bounds__(kFineThreads) void k_submap_target(const bevsubreg::Map *maps, uint32_t map0,
                                                                const bevsubreg::Entry *entries, FineWork w,
                                                                uint32_t *ent_start, SubmapRegWork t)
{
    __shared__ uint32_t wave_sum[kRegWaves];
    __shared__ uint32_t s_base;
    const bevsubreg::Map mp = maps[map0 + blockIdx.x];
    float4 *pts = t.pts + mp.pt0;
    const uint32_t n = submap_move(mp, entries, w, ent_start, pts, wave_sum, s_base);
    /* 3: the search grid of the moved points */
    reg_grid_build<kFineCells>(n, SubregPts{pts}, t.hdr + blockIdx.x, t.cell_off + (size_t)blockIdx.x * (kFineCells + 1),
                               t.sorted + mp.pt0);
}

/* probs: the launch's problems (tgt_slot: the map's index in the plan); §6d's loop against the map's arrays */
__global__ __launch_bounds__(kFineThreads) void k_submap_icp(const FineProblem *probs, const bevsubreg::Map *maps,
                                                             uint32_t map0, FineWork w, SubmapRegWork t,
                                                             const bev_icp_result_t *coarse, const int32_t *best,
                                                             bev_icp_params_t prm, bev_icp_result_t *results)
{
    __shared__ FineShared sh;
    const FineProblem pb = probs[blockIdx.x];
    const uint64_t pt0 = maps[pb.tgt_slot].pt0;
    const uint32_t g = pb.tgt_slot - map0;
    float G[16];
    fine_guess(pb, coarse, best, G);
    fine_icp_problem(sh, w.vox_n[pb.src_slot], w.vox + (size_t)pb.src_slot * w.Pn, SubregPts{t.pts + pt0}, t.hdr[g],
                     t.cell_off + (size_t)g * (kFineCells + 1), t.sorted + pt0, w.cur + (size_t)blockIdx.x * w.Pn,
                     w.corr + (size_t)blockIdx.x * w.Pn, G, prm, results + pb.result);
}

void launch_submap_target(const void *maps, uint32_t map0, int n_maps, const void *entries, const FineWork &w,
                          uint32_t *ent_start, const SubmapRegWork &t, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_target, dim3(n_maps), dim3(kFineThreads), 0, st, static_cast<const bevsubreg::Map *>(maps),
                           map0, static_cast<const bevsubreg::Entry *>(entries), w, ent_start, t);
}

void launch_submap_icp(const FineProblem *probs, int n, const void *maps, uint32_t map0, const FineWork &w,
                       const SubmapRegWork &t, const bev_icp_result_t *coarse, const int32_t *best, const bev_icp_params_t &prm,
                       bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_submap_icp, dim3(n), dim3(kFineThreads), 0, st, probs, static_cast<const bevsubreg::Map *>(maps),
                           map0, w, t, coarse, best, prm, results);
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_REG_H */
