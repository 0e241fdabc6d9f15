/*
 * bev_kernels.hip — hand-written HIP kernels (gfx950, wave64) for the
 * batch_multi_bev_gen hot path.  No MFMA: the path is scatter / stencil /
 * ordered reduction / raster, bounded by HBM.
 *
 * Pipeline for one sub-batch of frames (all launches on one stream):
 *
 *   (winner table: generation-tagged, cleared only when the tag wraps)
 *   order_scan      per input point : winner[slot] = max(index+1)          (getOrderedCloud, last writer wins)
 *   gather_ground   per slot        : ordered cloud, phase-A ground flag,
 *                                     BEV code, candidate list               (getOrderedCloud + markGroundPoints phase A)
 *   cell_sums       per frame       : stable counting sort of candidates by
 *                                     2 m cell, then IN-ORDER float sums     (markGroundPoints phase B + divide)
 *   ground_resolve  per frame row   : 4-neighbour height test, label fix-up (markGroundPoints phase C)
 *   bev_raster      per frame band  : LDS atomics, then coalesced 16 B stores
 *                                     of the 24 occupancy planes + max-height
 *                                     plane                                  (computeAndSave{Multi,Single}Bev rasters)
 *
 * Order-dependent results of the reference are reproduced by construction:
 *   - last-writer-wins scatter  -> atomicMax on (input index + 1);
 *   - row-major float32 accumulation per cell -> candidates are emitted in
 *     slot order, sorted STABLY by cell, and each cell is summed by one lane
 *     sequentially (a tree or atomic float reduction would change low bits).
 */
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "bev_internal.h"
#include "bev_libm.h"

#include "bev_dev.h"
#include "bev_front.h"
#include "bev_walk.h"
#include "bev_cell_sums.h"
#include "bev_resolve.h"
#include "bev_raster.h"
#include "bev_misc.h"
#include "bev_project.h"
#include "bev_manip.h"
#include "bev_posed.h"
#include "bev_submap.h"
#include "bev_submap_float.h"
#include "bev_reg_common.h"
#include "bev_regfront.h"
#include "bev_icp.h"
#include "bev_fine.h"
#include "bev_submap_reg.h"
#include "bev_submap_vox.h"
#include "bev_submap_coarse.h"
#include "bev_submap_pn_vox.h"
#include "bev_submap_top.h"
#include "bev_pair_grid.h"
#include "bev_submap_grid.h"
#include "bev_wide_icp.h"
#include "bev_place.h"
#include "bev_verify.h"
#include "bev_align.h"

using namespace bevx;

namespace bevk {

static const char *const kNames[K_COUNT] = {
    "k_order_scan", "k_walk", "k_cell_sums", "k_ground_resolve", "k_bev_raster",
    "k_gather_only", "k_ground_mat", "k_cloud_codes", "k_angle_debug", "k_float_bev", "k_project", "k_transform",
    "k_probe", "k_walk_general", "k_walk_structured", "k_walk_colmajor", "k_walk_colmajor_gen", "k_verdict", "k_stage",
    "k_rf_cells", "k_rf_top", "k_rf_voxel", "k_rf_normals", "k_icp_grid", "k_icp", "k_icp_best",
    "k_fine_voxel", "k_fine_grid", "k_fine_icp", "k_kitti_crossings", "k_kitti_chain", "k_kitti_assign", "k_kitti_gather",
    "k_float_bev_batch", "k_posed_splat", "k_posed_expand", "k_submap_splat", "k_submap_float_splat",
    "k_submap_target", "k_submap_icp",
    "k_submap_vox_move", "k_submap_vox_keys", "k_submap_vox_tile", "k_submap_vox_global", "k_submap_vox_finish", "k_submap_vox_out",
    "k_submap_pn_target", "k_submap_coarse_icp",
    "k_submap_pn_move", "k_submap_pn_keys", "k_submap_pn_finish", "k_submap_pn_normals", "k_submap_pn_grid", "k_submap_pn_out",
    "k_submap_top_keys", "k_submap_top_cells", "k_submap_top_hist", "k_submap_top_scan", "k_submap_top_compact", "k_submap_top_rows",
    "k_submap_top_overflow",
    "k_subgrid_bounds", "k_subgrid_header", "k_subgrid_count", "k_subgrid_sums", "k_subgrid_scan", "k_subgrid_scatter",
    "k_submap_icp_wide", "k_submap_coarse_icp_wide",
    "k_pairgrid_desc", "k_fine_icp_wide", "k_icp_wide",
    "k_place_splat", "k_place_finish", "k_place_pairs", "k_place_topk",
    "k_verify_move", "k_verify_count",
    "k_align_grid", "k_align_finish", "k_align_hit", "k_align_pick",
};
const char *kernel_name(int id) { return (id >= 0 && id < K_COUNT) ? kNames[id] : "?"; }

/* ------------------------------------------------------------------------- */
/* k_stage: the stages of FOUR consecutive sub-batches as workgroups of one grid.
 *
 * Rounds 2-5 ran the front (probe, walk) and the back (cell sums, resolve, rasters) of neighbouring sub-batches on two
 * streams of different priority.  The time lines of round 5 (profiles/r05_timeline_hdl_pipelined.txt) showed what that buys
 * and what it cannot: the back stage's kernels were not the walk's shape (512 threads, 50 KB of LDS) and started only
 * where two walk workgroups of one CU retired together; every hand-over between the streams and every kernel boundary left
 * the chip to a launch's tail.  Here every stage has the walk's shape (bev_internal.h: kStageThreads, kSlotLdsBytes), a
 * launch holds
 *     the walk of sub-batch t  |  phase B of t - 1  |  phase C of t - 2  |  the rasters of t - 3
 * and a workgroup's number says which it is: group slot i (8 frames, one per XCD: blocks b and b + 8 share an L2) holds
 * the walk's strips of frame group i and the later stages' workgroups of frame group i - lead, so that a CU holds a mix of
 * long memory-bound and short latency-bound workgroups at any time, the launch starts with walks alone and ends with the
 * short workgroups of the later stages (a launch's tail is as long as its last workgroups live).  The stages of ONE
 * sub-batch meet only through the order of launches on the stream. */
template <int kSrc, bool kPow2, bool kGm>
__global__ __launch_bounds__(kStageThreads, 4) void k_stage(StageArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char stage_arena[];
    static_assert(kSrc != kSrcColMajor && kSrc != kSrcColMajorGen, "the firing-order walks are launched apart");
    static_assert(kStripThreads == kStageThreads && kSumThreads == kStageThreads && kResolveThreads == kStageThreads && kRasterThreads == kStageThreads, "one workgroup shape");
    const int bid = (int)blockIdx.x, x = bid & 7, j = bid >> 3;
    const int strips = a.g.strips;
    const int per_slot = strips + kSumQ + kResolveWgs + a.g.raster_bands;
    const int i = j / per_slot;
    int k = j - i * per_slot;
    if (k < strips) {
        const int f = i * 8 + x;
        if (f < a.walk.nf) walk_body<kSrc, kPow2, kGm>(stage_arena, a.walk.b, a.g, f, k, a.want_mode, bid);
        return;
    }
    const int f = (i - a.lead) * 8 + x;
    if (i < a.lead) return;
    k -= strips;
    if (k < kSumQ) {
        if (f < a.sums.nf) cell_sums_body(reinterpret_cast<uint32_t *>(stage_arena), a.sums.b, a.g, f, k, bid);
        return;
    }
    k -= kSumQ;
    if (k < kResolveWgs) {
        if (f < a.resolve.nf) resolve_body<kPow2>(stage_arena, a.resolve.b, a.g, f, k);
        return;
    }
    k -= kResolveWgs;
    if (f < a.raster.nf) raster_body(reinterpret_cast<uint32_t *>(stage_arena), a.raster.b, a.g, f, k, a.want_multi, a.want_single);
}

/* the two dispatchers of the walk's template parameters: fn(std::integral_constant<int, kSrc>) for a source ... */
template <class F>
static auto with_source(int source, F &&fn)
{
    switch (source) {
    case kSrcIdentity: return fn(std::integral_constant<int, kSrcIdentity>{});
    case kSrcInPlace: return fn(std::integral_constant<int, kSrcInPlace>{});
    case kSrcStructured: return fn(std::integral_constant<int, kSrcStructured>{});
    case kSrcColMajor: return fn(std::integral_constant<int, kSrcColMajor>{});
    case kSrcColMajorGen: return fn(std::integral_constant<int, kSrcColMajorGen>{});
    default: return fn(std::integral_constant<int, kSrcGather>{});
    }
}
/* ... and fn(kPow2, kGm) for the reciprocal / divide choice and the ground-mat output */
template <class F>
static void with_variant(bool pow2, bool gm, F &&fn)
{
    if (pow2 && !gm) fn(std::true_type{}, std::false_type{});
    else if (pow2) fn(std::true_type{}, std::true_type{});
    else if (!gm) fn(std::false_type{}, std::false_type{});
    else fn(std::false_type{}, std::true_type{});
}
static bool raster_is_pow2(const Geometry &g) { return g.rp.inv_interval != 0.0f && g.rp.inv_height_res != 0.0f; } /* every configuration of the reference */
/* the source k_stage is instantiated with.  (The firing-order walks are never fused — 50-53 KB of LDS would hold every stage
 * of the launch to three per CU; they are launched apart, see run_pipeline — and the stages behind them take the gather's.) */
constexpr int stage_source(int src) { return (src == kSrcColMajor || src == kSrcColMajorGen) ? (int)kSrcGather : src; }

size_t stage_lds_bytes(const Geometry &g, int source)
{
    const size_t w = with_source(source, [](auto s) { return sizeof(WalkLds<stage_source(decltype(s)::value)>); });
    const size_t others = std::max(std::max(SumDims::lds_bytes(g.segs), sizeof(ResolveLds)), raster_lds_bytes(g));
    return std::max(w, others);
}
void launch_stage(const StageArgs &a, int source, hipStream_t st)
{
    if (a.walk.nf == 0) source = kSrcInPlace; /* (any instantiation will do for a launch without a walk) */
    const Geometry &g = a.g;
    const bool gm = a.walk.nf > 0 && a.walk.b.gm != nullptr;
    const int back = std::max(a.sums.nf, std::max(a.resolve.nf, a.raster.nf));
    const int lead = back > 0 ? a.lead : 0;
    const int slots = std::max((a.walk.nf + 7) / 8, back > 0 ? (back + 7) / 8 + lead : 0);
    if (slots == 0) return;
    const int per_slot = g.strips + kSumQ + kResolveWgs + g.raster_bands;
    const dim3 gr((unsigned)(8 * slots * per_slot)), bl(kStageThreads);
    const size_t lds = stage_lds_bytes(g, source);
    StageArgs args = a;
    args.lead = lead;
    with_source(source, [&](auto s) {
        constexpr int kSrc = stage_source(decltype(s)::value);
        with_variant(raster_is_pow2(g), gm, [&](auto p, auto m) {
            hipLaunchKernelGGL((k_stage<kSrc, decltype(p)::value, decltype(m)::value>), gr, bl, lds, st, args);
        });
    });
}

/* ------------------------------------------------------------------------- */
/* launchers                                                                  */
hipError_t configure_kernels(const Geometry &g)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_cell_sums),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)SumDims::lds_bytes(kMaxSegs));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_bev_raster), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)raster_lds_bytes(g));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_posed_expand), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)raster_lds_bytes(g));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_bev_raster_dense),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)raster_lds_bytes(g));
}
void launch_order_scan(const Geometry &g, const BatchPtrs &b, int nf, uint32_t max_pts, bool thin, hipStream_t st)
{
    if (max_pts == 0 || nf == 0) return;
    const unsigned per_block = 256u * kScanPerThread;
    const unsigned blocks = (max_pts + per_block - 1u) / per_block;
    /* wide: one workgroup per 1024-point block (every load of a frame in flight at once: 20 % faster when frames do go
     * this way); thin: 8 per frame striding over the blocks, for the launch that is expected to find nothing to do */
    dim3 grid(thin && blocks > 8u ? 8u : blocks, (unsigned)nf);
    hipLaunchKernelGGL(k_order_scan, grid, dim3(256), 0, st, b.pts, b.frames, b.info, b.winner, g.N, g.H, g.S,
                       b.win_tag << b.win_shift);
}
void launch_gather_ground(const Geometry &g, const BatchPtrs &b, int nf, int source, uint32_t mode, hipStream_t st)
{
    if (nf == 0) return;
    const dim3 gr(xcd_grid(nf, g.strips)), bl(kStripThreads);
    with_source(source, [&](auto s) {
        constexpr int kSrc = decltype(s)::value;
        with_variant(raster_is_pow2(g), b.gm != nullptr, [&](auto p, auto m) {
            hipLaunchKernelGGL((k_walk<kSrc, decltype(p)::value, decltype(m)::value>), gr, bl, 0, st, b, g, nf, mode);
        });
    });
}
void launch_probe(const Geometry &g, const BatchPtrs &b, int nf, bool allow_stream, int layout_hint, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_probe, dim3(nf), dim3(kProbeThreads), 0, st, b, g, allow_stream ? 1 : 0, layout_hint);
}
void launch_verdict(const Geometry &g, const BatchPtrs &b, int nf, uint32_t *host_hint, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_verdict, dim3(1), dim3(1024), 0, st, b.info, nf, host_hint, b.cm_sync, g.N);
}
void launch_gather_only(const Geometry &g, const BatchPtrs &b, int nf, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_gather_only, dim3(xcd_grid(nf, g.tiles)), dim3(kGatherThreads), 0, st, b, g, nf);
}
void launch_cell_sums(const Geometry &g, const BatchPtrs &b, int nf, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_cell_sums, dim3(xcd_grid(nf, kSumQ)), dim3(kSumThreads), SumDims::lds_bytes(g.segs), st, b, g, nf);
}
void launch_ground_resolve(const Geometry &g, const BatchPtrs &b, int nf, hipStream_t st)
{
    if (nf == 0) return;
    const bool pow2 = g.rp.inv_interval != 0.0f && g.rp.inv_height_res != 0.0f;
    if (pow2) hipLaunchKernelGGL(k_ground_resolve<true>, dim3(nf * kResolveWgs), dim3(kResolveThreads), 0, st, b, g);
    else hipLaunchKernelGGL(k_ground_resolve<false>, dim3(nf * kResolveWgs), dim3(kResolveThreads), 0, st, b, g);
}
void launch_bev_raster(const Geometry &g, const BatchPtrs &b, bool want_multi, bool want_single, int nf, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_bev_raster, dim3(8 * ((nf + 7) / 8) * g.raster_bands), dim3(kRasterThreads), raster_lds_bytes(g), st, b,
                       g, nf, want_multi ? 1 : 0, want_single ? 1 : 0);
}
void launch_bev_raster_dense(const Geometry &g, const uint32_t *codes, uint32_t n_codes, uint8_t *multi, uint8_t *single,
                             hipStream_t st)
{
    hipLaunchKernelGGL(k_bev_raster_dense, dim3(g.raster_bands), dim3(kRasterThreads), raster_lds_bytes(g), st, codes,
                       n_codes, multi, single, g.rp);
}
void launch_ground_mat(const Geometry &g, const BatchPtrs &b, int8_t *out, int nf, hipStream_t st)
{
    if (nf == 0) return;
    hipLaunchKernelGGL(k_ground_mat, dim3(xcd_grid(nf, g.tiles)), dim3(kGatherThreads), 0, st, b, g, out, nf);
}
void launch_cloud_codes(const Geometry &g, const bev_point_t *cloud, uint32_t n, uint32_t *codes, hipStream_t st)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_cloud_codes, dim3((n + 255u) / 256u), dim3(256), 0, st, cloud, n, codes, g.rp);
}
void launch_float_bev(const bev_point_t *cloud, uint32_t n, float interval, int M, bool skip_label0, float *grid,
                      hipStream_t st)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_float_bev, dim3((n + 255u) / 256u), dim3(256), 0, st, cloud, n, interval, M,
                       skip_label0 ? 1 : 0, reinterpret_cast<uint32_t *>(grid));
}
void launch_transform(const bev_point_t *cloud, uint32_t n, const float m[12], bev_point_t *out, hipStream_t st)
{
    if (n == 0) return;
    Affine34 a;
    for (int k = 0; k < 12; ++k) a.m[k] = m[k];
    hipLaunchKernelGGL(k_transform, dim3((n + 255u) / 256u), dim3(256), 0, st, cloud, n, a, out);
}
void launch_project_batch(int kind, const float *xyzi, const ProjFrame *tab, int nf, uint32_t blocks, bev_point_t *out,
                          hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    if (kind == BEV_PROJECT_MULRAN_OS1_64)
        hipLaunchKernelGGL(k_project_batch<BEV_PROJECT_MULRAN_OS1_64>, dim3(blocks), dim3(256), 0, st, xyzi, tab, nf, out);
    else
        hipLaunchKernelGGL(k_project_batch<BEV_PROJECT_OXFORD_HDL_32E>, dim3(blocks), dim3(256), 0, st, xyzi, tab, nf, out);
}
void launch_float_bev_batch(const bev_point_t *clouds, const ProjFrame *tab, int nf, uint32_t blocks, const float *poses,
                            int n_poses, float interval, int M, bool skip_label0, float *grids, hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    static_assert(sizeof(Affine34) == 12 * sizeof(float), "a pose is 12 packed floats");
    hipLaunchKernelGGL(k_float_bev_batch, dim3(blocks), dim3(256), 0, st, clouds, tab, nf,
                       reinterpret_cast<const Affine34 *>(poses), n_poses, interval, M, skip_label0 ? 1 : 0,
                       reinterpret_cast<uint32_t *>(grids));
}
void launch_posed_splat(const bev_point_t *clouds, const ProjFrame *tab, int nf, uint32_t blocks, const float *poses, int n_poses,
                        const Geometry &g, uint32_t *planes, hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    hipLaunchKernelGGL(k_posed_splat, dim3(blocks), dim3(256), 0, st, clouds, tab, nf,
                       reinterpret_cast<const Affine34 *>(poses), n_poses, g.rp, planes);
}
void launch_posed_expand(const Geometry &g, const uint32_t *planes, int n_grids, uint8_t *multi, uint8_t *single, hipStream_t st)
{
    if (n_grids == 0) return;
    hipLaunchKernelGGL(k_posed_expand, dim3((unsigned)n_grids * (unsigned)g.raster_bands), dim3(kRasterThreads),
                       raster_lds_bytes(g), st, planes, multi, single, g.rp);
}
void launch_submap_splat(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                         const void *entries, const Geometry &g, uint32_t *planes, hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    hipLaunchKernelGGL(k_submap_splat, dim3(blocks), dim3(256), 0, st, clouds, static_cast<const ProjFrame *>(rows), ent0, nf,
                       static_cast<const bevsub::Entry *>(entries), g.rp, planes);
}
void launch_submap_float_splat(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                               const void *entries, float interval, int M, bool skip_label0, float *grids, hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    hipLaunchKernelGGL(k_submap_float_splat, dim3(blocks), dim3(256), 0, st, clouds, static_cast<const ProjFrame *>(rows), ent0,
                       nf, static_cast<const bevsub::Entry *>(entries), interval, M, skip_label0 ? 1 : 0,
                       reinterpret_cast<uint32_t *>(grids));
}
void launch_place_splat(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                        const void *entries, const float *edge2, const PlaceShape &ps, uint32_t *planes, hipStream_t st)
{
    if (blocks == 0 || nf == 0) return;
    if (ent0)
        hipLaunchKernelGGL(k_place_splat<true>, dim3(blocks), dim3(256), 0, st, clouds, static_cast<const ProjFrame *>(rows), ent0,
                           nf, static_cast<const bevsub::Entry *>(entries), edge2, ps, planes);
    else
        hipLaunchKernelGGL(k_place_splat<false>, dim3(blocks), dim3(256), 0, st, clouds, static_cast<const ProjFrame *>(rows), ent0,
                           nf, static_cast<const bevsub::Entry *>(entries), edge2, ps, planes);
}
void launch_place_finish(const uint32_t *planes, int n_desc, const PlaceShape &ps, uint8_t *desc, PlaceHandle *units, hipStream_t st)
{
    if (n_desc == 0) return;
    hipLaunchKernelGGL(k_place_finish, dim3((unsigned)n_desc), dim3(64), 0, st, planes, ps, desc, units);
}
/* fn(kWords) for the words of a column that hold rings */
template <class F>
static void with_place_words(int n_rings, F &&fn)
{
    switch ((n_rings + 3) / 4) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    default: return fn(std::integral_constant<int, 8>{});
    }
}
void launch_place_pairs(const PlaceHandle *uq, int q0, int nq, const PlaceHandle *udb, int n_db, const int32_t *limit,
                        const PlaceShape &ps, uint2 *pairs, hipStream_t st)
{
    if (nq == 0 || n_db == 0) return;
    const dim3 grid((unsigned)((n_db + kPlaceTile - 1) / kPlaceTile), (unsigned)nq);
    with_place_words(ps.n_rings, [&](auto w) {
        hipLaunchKernelGGL((k_place_pairs<decltype(w)::value>), grid, dim3(256), 0, st, uq, q0, udb, n_db, limit, ps.n_sectors, pairs);
    });
}
void launch_place_topk(const uint2 *pairs, int q0, int nq, int n_db, const int32_t *limit, const PlaceShape &ps, int top_k,
                       bev_place_hit_t *hits, hipStream_t st)
{
    if (nq == 0) return;
    hipLaunchKernelGGL(k_place_topk, dim3((unsigned)nq), dim3(256), 0, st, pairs, q0, n_db, limit, ps.n_sectors, top_k, hits);
}
void launch_project_kitti(int step, const float *xyzi, const ProjFrame *tab, int nf, uint32_t n_max, const KittiWork &w,
                          bev_point_t *out, hipStream_t st)
{
    if (nf == 0) return;
    const unsigned blocks = (n_max + kKittiBlock - 1u) / kKittiBlock;
    if (step == 0 && blocks) hipLaunchKernelGGL(k_kitti_crossings, dim3(blocks, (unsigned)nf), dim3(kKittiBlock), 0, st, xyzi, tab, w);
    if (step == 1) hipLaunchKernelGGL(k_kitti_chain, dim3((unsigned)nf), dim3(64), 0, st, tab, w, kitti_ring_min());
    if (step == 2 && blocks) hipLaunchKernelGGL(k_kitti_assign, dim3(blocks, (unsigned)nf), dim3(256), 0, st, tab, w);
    if (step == 3) hipLaunchKernelGGL(k_kitti_gather, dim3((kKittiRows * kKittiCols + 255) / 256, (unsigned)nf), dim3(256), 0, st, xyzi, tab, w, out);
}
void launch_angle_debug(const float *dx, const float *dy, const float *dz, uint8_t *out, size_t n, hipStream_t st)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_angle_debug, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx, dy, dz, out, n);
}
void launch_exact_eval(int id, const void *const in[4], const float *prm, uint32_t *out, uint32_t out_words, size_t n, hipStream_t st)
{
    if (n == 0) return;
    ExactEvalArgs a{};
    for (int k = 0; k < 4; ++k) a.in[k] = in[k];
    for (int k = 0; k < kEvParams; ++k) a.prm[k] = prm ? prm[k] : 0.0f;
    hipLaunchKernelGGL(k_exact_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, id, a, out, out_words, n);
}

} /* namespace bevk */
