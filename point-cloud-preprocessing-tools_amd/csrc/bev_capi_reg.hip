/*
 * bev_capi_reg.hip — the registration half of the extern "C" boundary declared in include/bev_mi355x.h: the front end
 * (top-part flatten, voxel grid, 2-D normals), coarse point-to-plane ICP (§6c), the fine stage (§6d) and
 * scan-to-map fine ICP (§6k), with the voxel grid over a map's union in front of it (§6l), and scan-to-map coarse ICP (§6m).
 * Host-side only; the kernels are in bev_kernels.hip (bev_reg_common.h, bev_regfront.h, bev_icp.h, bev_fine.h,
 * bev_submap_reg.h, bev_submap_vox.h, bev_submap_coarse.h).  With
 * the BEV pipeline of bev_capi.hip it shares the context (bev_ctx.h), its stream and the call prologue (begin_call).
 */
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "bev_ctx.h"
#include "bev_libm_f64.h"
#include "bev_submap_reg_plan.h"

using namespace bevk;
using namespace bevh;

/* ---- what the entry points keep between calls (RegState, bev_ctx.h; DevBuf and UploadTable themselves: bev_capi.hip) ---- */
void RegState::release()
{
    for (DevBuf *b : {&rf_buf, &icp_buf, &icp_one, &fine_buf, &fine_in, &sub_res}) b->release();
    for (UploadTable *t : {&rf_offs, &icp_tab, &fine_tab}) t->release();
    if (tail_ev) (void)hipEventDestroy(tail_ev);
    tail_ev = nullptr;
    tail_pending = false;
}

namespace {

constexpr size_t kRegTabMin = (size_t)1 << 16; /* smallest problem / slot table */

bool matches_in_range(const bev_match_t *h_matches, int n_matches, int n_frames)
{
    for (int m = 0; m < n_matches; ++m) {
        const bev_match_t &mt = h_matches[m];
        if (mt.query_idx < 0 || mt.query_idx >= n_frames || mt.match_idx < 0 || mt.match_idx >= n_frames) return false;
    }
    return true;
}

/* workspace of the registration front end (RfWork, bev_internal.h), allocated on first use; the BEV path's is untouched */
int ensure_rf(bev_ctx *c)
{
    RegState &r = c->reg;
    if (r.rf_buf.p) return BEV_OK;
    const size_t B = (size_t)c->max_batch, P = cloud_cap(c), Q = P;
    const size_t sz[] = {B * P * 8, B * 2 * P * 8, B * kRfCells * 4, B * (kRfCells + 1) * 4, B * (kRfCells + 1) * 4,
                         B * Q * 16, B * Q * 16, B * Q * 4, B * (Q + 1) * 4, B * sizeof(RfFrameMeta), P * 32};
    void **const dst[] = {(void **)&r.rf.keys, (void **)&r.rf.scr, (void **)&r.rf.cell_cnt, (void **)&r.rf.cell_off,
                          (void **)&r.rf.out_off, (void **)&r.rf.flat, (void **)&r.rf.vpts, (void **)&r.rf.vidx,
                          (void **)&r.rf.vstart, (void **)&r.rf.meta, (void **)&r.rf_nrm};
    const int rc = r.rf_buf.grow(c, carve(nullptr, sz, dst));
    if (rc != BEV_OK) return rc;
    carve(r.rf_buf.p, sz, dst);
    r.rf.P = P;
    r.rf.Q = Q;
    return BEV_OK;
}
/* how the front end's entry points begin, behind their argument checks */
int rf_begin(bev_ctx *c)
{
    const int rc = begin_call(c, false);
    return rc != BEV_OK ? rc : ensure_rf(c);
}

/* the chain on nf <= max_batch frames of the workspace: top part -> voxel grid -> normals (PointNormal at out) */
int rf_chain(bev_ctx *c, const RfIn &in, int nf, float leaf, float radius, const float vp[2], uint32_t n_max, float *out,
             size_t out_stride, uint32_t *counts)
{
    {
        ProfScope ps(c, K_RF_CELLS, nf);
        launch_rf_top(in, c->reg.rf, nf, c->stream, 0);
    }
    {
        ProfScope ps(c, K_RF_TOP, nf);
        launch_rf_top(in, c->reg.rf, nf, c->stream, 1);
    }
    {
        ProfScope ps(c, K_RF_VOXEL, nf);
        launch_rf_voxel(c->reg.rf, nf, leaf, counts, c->stream);
    }
    {
        ProfScope ps(c, K_RF_NORMALS, nf);
        launch_rf_normals(c->reg.rf, nf, bev_regfront_max_out(n_max), radius, leaf, vp, true, out, out_stride, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

extern "C" {

/* ---- registration front end ------------------------------------------------------------------------------------------ */
size_t bev_regfront_max_out(size_t n) { return n / 5 + 51; }

static bool rf_positive(float v) { return std::isfinite(v) && v > 0.0f; }

int bev_top_part_flatten(bev_ctx_t *c, const bev_point_t *cloud, uint32_t n, float *out, uint32_t *n_out)
{
    if (!c || !n_out || (n && (!cloud || !out))) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    *n_out = 0;
    int rc = rf_begin(c);
    if (rc != BEV_OK) return rc;
    if (n == 0) return BEV_OK;
    rc = ensure_staging(c);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemcpyAsync(c->st_in, cloud, (size_t)n * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    RfIn in{c->st_in, nullptr, n, n};
    {
        ProfScope ps(c, K_RF_CELLS, 1);
        launch_rf_top(in, c->reg.rf, 1, c->stream, 0);
    }
    {
        ProfScope ps(c, K_RF_TOP, 1);
        launch_rf_top(in, c->reg.rf, 1, c->stream, 1);
    }
    HIPCK(c, hipGetLastError());
    RfFrameMeta meta{};
    HIPCK(c, hipMemcpyAsync(&meta, c->reg.rf.meta, sizeof(meta), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (meta.m) HIPCK(c, hipMemcpy(out, c->reg.rf.flat, (size_t)meta.m * 16, hipMemcpyDeviceToHost));
    *n_out = meta.m;
    return BEV_OK;
}

int bev_voxel_grid_xyz(bev_ctx_t *c, const float *xyz, uint32_t n, float leaf, float *out, uint32_t *n_out)
{
    if (!c || !n_out || (n && (!xyz || !out)) || !rf_positive(leaf)) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    *n_out = 0;
    const int rc = rf_begin(c);
    if (rc != BEV_OK) return rc;
    if (n == 0) return BEV_OK;
    RfFrameMeta meta{};
    meta.m = n;
    HIPCK(c, hipMemcpyAsync(c->reg.rf.flat, xyz, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->reg.rf.meta, &meta, sizeof(meta), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, K_RF_VOXEL, 1);
        launch_rf_voxel(c->reg.rf, 1, leaf, nullptr, c->stream);
    }
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(&meta, c->reg.rf.meta, sizeof(meta), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (meta.nv) HIPCK(c, hipMemcpy(out, c->reg.rf.vpts, (size_t)meta.nv * 16, hipMemcpyDeviceToHost));
    *n_out = meta.nv;
    return BEV_OK;
}

int bev_normals_2d(bev_ctx_t *c, const float *xyz, uint32_t n, int k_search, float radius, const float *viewpoint,
                   float *out)
{
    if (!c || (n && (!xyz || !out))) return BEV_ERR_INVALID_ARG;
    if (k_search != 0) return BEV_ERR_UNSUPPORTED;
    if (!rf_positive(radius)) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    const int rc = rf_begin(c);
    if (rc != BEV_OK) return rc;
    if (n == 0) return BEV_OK;
    const float vp[2] = {viewpoint ? viewpoint[0] : 0.0f, viewpoint ? viewpoint[1] : 0.0f};
    RfFrameMeta meta{};
    meta.m = meta.nv = n;
    meta.windowed = 0; /* any order: every point is scanned */
    HIPCK(c, hipMemcpyAsync(c->reg.rf.vpts, xyz, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->reg.rf.meta, &meta, sizeof(meta), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, K_RF_NORMALS, 1);
        launch_rf_normals(c->reg.rf, 1, n, radius, 0.0f, vp, false, c->reg.rf_nrm, 0, c->stream);
    }
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(out, c->reg.rf_nrm, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

int bev_registration_front_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds,
                                           const uint64_t *h_offsets, float leaf, float radius, const float *viewpoint,
                                           void *d_out, size_t out_stride, uint32_t *d_counts)
{
    if (!c || n_frames < 0 || !rf_positive(leaf) || !rf_positive(radius)) return BEV_ERR_INVALID_ARG;
    if (n_frames > 0 && (!d_clouds || !d_out || !d_counts)) return BEV_ERR_INVALID_ARG;
    const size_t P = cloud_cap(c);
    uint32_t n_max = (uint32_t)c->geo.S;
    if (h_offsets) {
        n_max = 0;
        for (int f = 0; f < n_frames; ++f) {
            if (h_offsets[f + 1] < h_offsets[f] || h_offsets[f + 1] - h_offsets[f] > P) return BEV_ERR_TOO_LARGE;
            n_max = std::max(n_max, (uint32_t)(h_offsets[f + 1] - h_offsets[f]));
        }
    }
    if (n_frames > 0 && out_stride < bev_regfront_max_out(n_max)) return BEV_ERR_INVALID_ARG;
    int rc = rf_begin(c);
    if (rc != BEV_OK) return rc;
    if (n_frames == 0) return BEV_OK;
    rc = wait_default_stream(c); /* (the upload of packed clouds, typically) */
    if (rc != BEV_OK) return rc;
    const uint64_t *d_offs = nullptr;
    if (h_offsets) {
        const size_t bytes = ((size_t)n_frames + 1) * 8;
        void *h;
        rc = c->reg.rf_offs.begin(c, bytes, 1024 * 8, &h);
        if (rc != BEV_OK) return rc;
        std::memcpy(h, h_offsets, bytes);
        rc = c->reg.rf_offs.push(c, bytes);
        if (rc != BEV_OK) return rc;
        d_offs = static_cast<const uint64_t *>(c->reg.rf_offs.dev);
    }
    const float vp[2] = {viewpoint ? viewpoint[0] : 0.0f, viewpoint ? viewpoint[1] : 0.0f};
    for (int f0 = 0; f0 < n_frames; f0 += c->max_batch) {
        const int nf = std::min(c->max_batch, n_frames - f0);
        RfIn in{};
        if (h_offsets) {
            in.pts = d_clouds;
            in.offs = d_offs + f0;
        } else {
            in.pts = d_clouds + (size_t)f0 * c->geo.S;
            in.stride = (size_t)c->geo.S;
            in.n_uniform = (uint32_t)c->geo.S;
        }
        rc = rf_chain(c, in, nf, leaf, radius, vp, n_max, static_cast<float *>(d_out) + (size_t)f0 * out_stride * 12,
                      out_stride, d_counts + f0);
        if (rc != BEV_OK) return rc;
    }
    return record_tail(c);
}

/* ---- coarse point-to-plane ICP --------------------------------------------------------------------------------------- */
bev_icp_params_t bev_icp_coarse_defaults(void)
{
    bev_icp_params_t p{};
    p.max_correspondence_distance = 10.0; /* icp.setMaxCorrespondenceDistance(10.0f) */
    p.max_iterations = 10;                /* icp.setMaximumIterations(10) */
    p.transformation_epsilon = 0.0;
    p.euclidean_fitness_epsilon = -DBL_MAX;
    return p;
}

static bool icp_params_ok(const bev_icp_params_t &p)
{
    return p.max_iterations >= 1 && p.max_iterations <= 1000 && std::isfinite(p.max_correspondence_distance) &&
           p.max_correspondence_distance > 0.0;
}

namespace {

/* the grids of the target frames slot_frames, then every problem (launches of kIcpProblemsPerLaunch), then, when d_best is
 * set, the better guess of each of the n_best matches; all on the context's stream */
int icp_launch(bev_ctx *c, const float *d_pn, size_t stride, const uint32_t *d_counts,
               const std::vector<IcpProblem> &probs, const std::vector<uint32_t> &slot_frames,
               const bev_icp_params_t &prm, bev_icp_result_t *d_res, int n_best, int32_t *d_best)
{
    const size_t U = slot_frames.size(), P = probs.size(), L = std::min(P, (size_t)kIcpProblemsPerLaunch);
    IcpWork w{};
    const size_t sz[] = {U * sizeof(IcpGridHdr), U * 4 * (size_t)(kIcpCells + 1), U * 16 * stride, L * 16 * stride};
    void **const dst[] = {(void **)&w.hdr, (void **)&w.cell_off, (void **)&w.sorted, (void **)&w.cur};
    int rc = c->reg.icp_buf.grow(c, carve(nullptr, sz, dst));
    if (rc != BEV_OK) return rc;
    carve(c->reg.icp_buf.p, sz, dst);
    const size_t o_slots = align256(P * sizeof(IcpProblem)), tab = o_slots + U * 4;
    void *hv;
    rc = c->reg.icp_tab.begin(c, tab, kRegTabMin, &hv);
    if (rc != BEV_OK) return rc;
    char *h = static_cast<char *>(hv);
    std::memcpy(h, probs.data(), P * sizeof(IcpProblem));
    std::memcpy(h + o_slots, slot_frames.data(), U * 4);
    rc = c->reg.icp_tab.push(c, tab);
    if (rc != BEV_OK) return rc;
    const IcpProblem *d_probs = static_cast<const IcpProblem *>(c->reg.icp_tab.dev);
    const uint32_t *d_slots = reinterpret_cast<const uint32_t *>(static_cast<char *>(c->reg.icp_tab.dev) + o_slots);
    {
        ProfScope ps(c, K_ICP_GRID, (int)U);
        launch_icp_grid(d_pn, stride, d_counts, d_slots, (int)U, w, c->stream);
    }
    for (size_t p0 = 0; p0 < P; p0 += kIcpProblemsPerLaunch) {
        const int n = (int)std::min((size_t)kIcpProblemsPerLaunch, P - p0);
        ProfScope ps(c, K_ICP, n);
        launch_icp(d_pn, stride, d_counts, d_probs + p0, n, w, prm, d_res, c->stream);
    }
    if (d_best) {
        ProfScope ps(c, K_ICP_BEST, n_best);
        launch_icp_best(d_res, n_best, d_best, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

int bev_icp_point_to_plane(bev_ctx_t *c, const float *src, uint32_t n_src, const float *tgt, uint32_t n_tgt,
                           const float *guess16, const bev_icp_params_t *params, bev_icp_result_t *result)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_coarse_defaults();
    if (!c || !result || (n_src && !src) || (n_tgt && !tgt) || !icp_params_ok(prm)) return BEV_ERR_INVALID_ARG;
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    const size_t stride = std::max<size_t>(std::max(n_src, n_tgt), 1);
    const size_t need = 2 * stride * 48 + 256 + sizeof(bev_icp_result_t);
    rc = c->reg.icp_one.grow(c, need);
    if (rc != BEV_OK) return rc;
    char *d = static_cast<char *>(c->reg.icp_one.p);
    float *d_pn = reinterpret_cast<float *>(d);
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(d + 2 * stride * 48);
    bev_icp_result_t *d_res = reinterpret_cast<bev_icp_result_t *>(d + 2 * stride * 48 + 256);
    const uint32_t counts[2] = {n_src, n_tgt};
    if (n_src) HIPCK(c, hipMemcpyAsync(d_pn, src, (size_t)n_src * 48, hipMemcpyHostToDevice, c->stream));
    if (n_tgt) HIPCK(c, hipMemcpyAsync(d_pn + stride * 12, tgt, (size_t)n_tgt * 48, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(d_counts, counts, sizeof(counts), hipMemcpyHostToDevice, c->stream));
    std::vector<IcpProblem> probs(1);
    probs[0].src_frame = 0;
    probs[0].tgt_frame = 1;
    probs[0].tgt_slot = 0;
    probs[0].result = 0;
    for (int k = 0; k < 16; ++k) probs[0].guess[k] = guess16 ? guess16[k] : (k % 5 == 0 ? 1.0f : 0.0f);
    rc = icp_launch(c, d_pn, stride, d_counts, probs, std::vector<uint32_t>{1u}, prm, d_res, 0, nullptr);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemcpyAsync(result, d_res, sizeof(bev_icp_result_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

int bev_coarse_registration_device_resident(bev_ctx_t *c, int n_frames, const void *d_pn, size_t stride,
                                            const uint32_t *d_counts, int n_matches, const bev_match_t *h_matches,
                                            const bev_icp_params_t *params, bev_icp_result_t *d_results,
                                            int32_t *d_best)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_coarse_defaults();
    if (!c || n_frames < 0 || n_matches < 0 || !icp_params_ok(prm)) return BEV_ERR_INVALID_ARG;
    if (n_matches > 0) {
        if (!d_pn || !d_counts || !h_matches || !d_results || !d_best || stride == 0) return BEV_ERR_INVALID_ARG;
        if (!matches_in_range(h_matches, n_matches, n_frames)) return BEV_ERR_INVALID_ARG;
    }
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n_matches == 0) return BEV_OK;
    rc = wait_default_stream(c);
    if (rc != BEV_OK) return rc;
    std::vector<int32_t> slot_of((size_t)n_frames, -1);
    std::vector<uint32_t> slot_frames;
    std::vector<IcpProblem> probs((size_t)n_matches * 2);
    for (int m = 0; m < n_matches; ++m) {
        const bev_match_t &mt = h_matches[m];
        if (slot_of[mt.match_idx] < 0) {
            slot_of[mt.match_idx] = (int32_t)slot_frames.size();
            slot_frames.push_back((uint32_t)mt.match_idx);
        }
        for (int g = 0; g < 2; ++g) {
            IcpProblem &pb = probs[(size_t)m * 2 + g];
            pb.src_frame = (uint32_t)mt.query_idx;
            pb.tgt_frame = (uint32_t)mt.match_idx;
            pb.tgt_slot = (uint32_t)slot_of[mt.match_idx];
            pb.result = (uint32_t)(m * 2 + g);
            bevx::icp_tool_guess(mt.angle_guess, g, pb.guess);
        }
    }
    rc = icp_launch(c, static_cast<const float *>(d_pn), stride, d_counts, probs, slot_frames, prm, d_results, n_matches,
                    d_best);
    if (rc != BEV_OK) return rc;
    return record_tail(c);
}

/* ---- fine stage: VoxelGrid<PointXYZIRCT> and point-to-point ICP ------------------------------------------------------ */
bev_icp_params_t bev_icp_fine_defaults(void)
{
    bev_icp_params_t p{};
    p.max_correspondence_distance = 1.0; /* icp_full.setMaxCorrespondenceDistance(1.0f) (BatchTopPartRegistration.cpp:232) */
    p.transformation_epsilon = 1e-6;     /* setTransformationEpsilon(1e-6) */
    p.euclidean_fitness_epsilon = 0.01;  /* setEuclideanFitnessEpsilon(0.01) */
    p.max_iterations = 100;              /* setMaximumIterations(100) */
    return p;
}

bev_icp_params_t bev_icp_whole_defaults(void)
{
    bev_icp_params_t p{};
    p.max_correspondence_distance = 4.0; /* BatchWholeRegistration.cpp:232-235 */
    p.transformation_epsilon = 1e-6;
    p.euclidean_fitness_epsilon = 0.001;
    p.max_iterations = 200;
    return p;
}

namespace {

size_t pow2_at_least(size_t n)
{
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

/* the device workspace for U slots of at most Pn records and P problems (grown when a call needs more), the slot and
 * problem tables uploaded behind everything on the context's stream */
int fine_setup(bev_ctx *c, size_t U, size_t Pn, const std::vector<FineSlot> &slots, const std::vector<FineProblem> &probs,
               FineWork &w, const FineSlot **d_slots, const FineProblem **d_probs)
{
    const size_t P = probs.size(), G = std::min(U, (size_t)kFineVoxelGroup), L = std::min(P, (size_t)kFineProblemsPerLaunch);
    const size_t Kn = pow2_at_least(Pn);
    w = FineWork{};
    const size_t sz[] = {U * Pn * sizeof(bev_point_t), U * 4, G * Kn * 8, G * (Pn + 1) * 4, U * sizeof(IcpGridHdr),
                         U * 4 * (size_t)(kFineCells + 1), U * Pn * 16, L * Pn * 16, L * Pn * 4};
    void **const dst[] = {(void **)&w.vox, (void **)&w.vox_n, (void **)&w.keys, (void **)&w.vstart, (void **)&w.hdr,
                          (void **)&w.cell_off, (void **)&w.sorted, (void **)&w.cur, (void **)&w.corr};
    int rc = c->reg.fine_buf.grow(c, carve(nullptr, sz, dst));
    if (rc != BEV_OK) return rc;
    carve(c->reg.fine_buf.p, sz, dst);
    w.Pn = Pn;
    w.Kn = Kn;
    const size_t o_probs = align256(slots.size() * sizeof(FineSlot)), tab = o_probs + P * sizeof(FineProblem);
    void *hv;
    rc = c->reg.fine_tab.begin(c, tab, kRegTabMin, &hv);
    if (rc != BEV_OK) return rc;
    char *h = static_cast<char *>(hv);
    if (!slots.empty()) std::memcpy(h, slots.data(), slots.size() * sizeof(FineSlot));
    if (P) std::memcpy(h + o_probs, probs.data(), P * sizeof(FineProblem));
    rc = c->reg.fine_tab.push(c, tab);
    if (rc != BEV_OK) return rc;
    *d_slots = static_cast<const FineSlot *>(c->reg.fine_tab.dev);
    *d_probs = reinterpret_cast<const FineProblem *>(static_cast<char *>(c->reg.fine_tab.dev) + o_probs);
    return BEV_OK;
}

int fine_voxel(bev_ctx *c, const bev_point_t *d_pts, const FineSlot *d_slots, int U, const FineWork &w, float leaf)
{
    for (int s0 = 0; s0 < U; s0 += kFineVoxelGroup) {
        const int n = std::min(kFineVoxelGroup, U - s0);
        ProfScope ps(c, K_FINE_VOXEL, n);
        launch_fine_voxel(d_pts, d_slots, s0, n, w, leaf, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

int fine_icp(bev_ctx *c, int U, const FineProblem *d_probs, size_t P, const FineWork &w, const bev_icp_result_t *d_coarse,
             const int32_t *d_best, const bev_icp_params_t &prm, bev_icp_result_t *d_res)
{
    {
        ProfScope ps(c, K_FINE_GRID, U);
        launch_fine_grid(U, w, c->stream);
    }
    for (size_t p0 = 0; p0 < P; p0 += kFineProblemsPerLaunch) {
        const int n = (int)std::min((size_t)kFineProblemsPerLaunch, P - p0);
        ProfScope ps(c, K_FINE_ICP, n);
        launch_fine_icp(d_probs + p0, n, w, d_coarse, d_best, prm, d_res, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

/* host records -> c->reg.fine_in (grown on demand) */
int fine_upload(bev_ctx *c, const bev_point_t *const *clouds, const uint32_t *n, int k, size_t *offs)
{
    size_t total = 0;
    for (int i = 0; i < k; ++i) {
        offs[i] = total;
        total += n[i];
    }
    const size_t need = std::max<size_t>(total, 1) * sizeof(bev_point_t);
    const int rc = c->reg.fine_in.grow(c, need);
    if (rc != BEV_OK) return rc;
    for (int i = 0; i < k; ++i)
        if (n[i])
            HIPCK(c, hipMemcpyAsync(static_cast<bev_point_t *>(c->reg.fine_in.p) + offs[i], clouds[i], (size_t)n[i] * sizeof(bev_point_t),
                                    hipMemcpyHostToDevice, c->stream));
    return BEV_OK;
}

} // namespace

int bev_voxel_grid_irct(bev_ctx_t *c, const bev_point_t *cloud, uint32_t n, float leaf, bev_point_t *out, uint32_t *n_out)
{
    if (!c || !n_out || (n && (!cloud || !out)) || !(std::isfinite(leaf) && leaf > 0.0f)) return BEV_ERR_INVALID_ARG;
    *n_out = 0;
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n == 0) return BEV_OK;
    size_t off = 0;
    rc = fine_upload(c, &cloud, &n, 1, &off);
    if (rc != BEV_OK) return rc;
    FineWork w;
    const FineSlot *d_slots;
    const FineProblem *d_probs;
    rc = fine_setup(c, 1, n, std::vector<FineSlot>{FineSlot{0, n, 0}}, std::vector<FineProblem>{}, w, &d_slots, &d_probs);
    if (rc != BEV_OK) return rc;
    rc = fine_voxel(c, static_cast<const bev_point_t *>(c->reg.fine_in.p), d_slots, 1, w, leaf);
    if (rc != BEV_OK) return rc;
    uint32_t nv = 0;
    HIPCK(c, hipMemcpyAsync(&nv, w.vox_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (nv) HIPCK(c, hipMemcpy(out, w.vox, (size_t)nv * sizeof(bev_point_t), hipMemcpyDeviceToHost));
    *n_out = nv;
    return BEV_OK;
}

int bev_icp_point_to_point(bev_ctx_t *c, const bev_point_t *src, uint32_t n_src, const bev_point_t *tgt, uint32_t n_tgt,
                           const float *guess16, const bev_icp_params_t *params, bev_icp_result_t *result)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_fine_defaults();
    if (!c || !result || (n_src && !src) || (n_tgt && !tgt) || !icp_params_ok(prm)) return BEV_ERR_INVALID_ARG;
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    const size_t Pn = std::max<size_t>(std::max(n_src, n_tgt), 1);
    std::vector<FineProblem> probs(1);
    probs[0].src_slot = 0;
    probs[0].tgt_slot = 1;
    probs[0].result = 0;
    probs[0].coarse_match = 0xffffffffu;
    for (int k = 0; k < 16; ++k) probs[0].guess[k] = guess16 ? guess16[k] : (k % 5 == 0 ? 1.0f : 0.0f);
    FineWork w;
    const FineSlot *d_slots;
    const FineProblem *d_probs;
    rc = fine_setup(c, 2, Pn, std::vector<FineSlot>{}, probs, w, &d_slots, &d_probs);
    if (rc != BEV_OK) return rc;
    /* the clouds are the "voxel clouds" of slots 0 and 1; the result goes behind them in the sort scratch */
    const uint32_t counts[2] = {n_src, n_tgt};
    if (n_src) HIPCK(c, hipMemcpyAsync(w.vox, src, (size_t)n_src * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    if (n_tgt) HIPCK(c, hipMemcpyAsync(w.vox + Pn, tgt, (size_t)n_tgt * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(w.vox_n, counts, sizeof(counts), hipMemcpyHostToDevice, c->stream));
    bev_icp_result_t *d_res = reinterpret_cast<bev_icp_result_t *>(w.keys);
    rc = fine_icp(c, 2, d_probs, 1, w, nullptr, nullptr, prm, d_res);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemcpyAsync(result, d_res, sizeof(bev_icp_result_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

int bev_fine_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds,
                                          const uint64_t *h_offsets, float leaf, int n_matches,
                                          const bev_match_t *h_matches, const bev_icp_result_t *d_coarse,
                                          const int32_t *d_best, const bev_icp_params_t *params,
                                          bev_icp_result_t *d_results)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_fine_defaults();
    if (!c || n_frames < 0 || n_matches < 0 || !icp_params_ok(prm) || !(std::isfinite(leaf) && leaf > 0.0f) ||
        (d_coarse == nullptr) != (d_best == nullptr))
        return BEV_ERR_INVALID_ARG;
    if (n_matches > 0) {
        if (!d_clouds || !h_matches || !d_results) return BEV_ERR_INVALID_ARG;
        if (!matches_in_range(h_matches, n_matches, n_frames)) return BEV_ERR_INVALID_ARG;
        if (h_offsets)
            for (int f = 0; f < n_frames; ++f)
                if (h_offsets[f + 1] < h_offsets[f] || h_offsets[f + 1] - h_offsets[f] > 0xffffffffull) return BEV_ERR_INVALID_ARG;
    }
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n_matches == 0) return BEV_OK;
    rc = wait_default_stream(c);
    if (rc != BEV_OK) return rc;
    std::vector<int32_t> slot_of((size_t)n_frames, -1);
    std::vector<FineSlot> slots;
    size_t Pn = 1;
    auto slot = [&](int f) -> uint32_t {
        if (slot_of[f] < 0) {
            slot_of[f] = (int32_t)slots.size();
            FineSlot s{};
            if (h_offsets) {
                s.off = h_offsets[f];
                s.n = (uint32_t)(h_offsets[f + 1] - h_offsets[f]);
            } else {
                s.off = (uint64_t)f * c->geo.S;
                s.n = (uint32_t)c->geo.S;
            }
            Pn = std::max(Pn, (size_t)s.n);
            slots.push_back(s);
        }
        return (uint32_t)slot_of[f];
    };
    std::vector<FineProblem> probs((size_t)n_matches);
    for (int m = 0; m < n_matches; ++m) {
        const bev_match_t &mt = h_matches[m];
        FineProblem &pb = probs[(size_t)m];
        pb.src_slot = slot(mt.query_idx);
        pb.tgt_slot = slot(mt.match_idx);
        pb.result = (uint32_t)m;
        pb.coarse_match = d_coarse ? (uint32_t)m : 0xffffffffu;
        bevx::icp_tool_guess(mt.angle_guess, 0, pb.guess);
    }
    const int U = (int)slots.size();
    FineWork w;
    const FineSlot *d_slots;
    const FineProblem *d_probs;
    rc = fine_setup(c, (size_t)U, Pn, slots, probs, w, &d_slots, &d_probs);
    if (rc != BEV_OK) return rc;
    rc = fine_voxel(c, d_clouds, d_slots, U, w, leaf);
    if (rc != BEV_OK) return rc;
    rc = fine_icp(c, U, d_probs, probs.size(), w, d_coarse, d_best, prm, d_results);
    if (rc != BEV_OK) return rc;
    return record_tail(c);
}

/* ---- scan-to-map fine ICP: frames against submaps (bev_submap_reg_plan.h, bev_submap_reg.h) ------------- */
namespace {

constexpr uint64_t kSubmapRegCap = (uint64_t)8 << 30; /* bytes of a launch group's maps (BEV_SUBMAP_REG_GROUP): 8 GiB, of the order of
                                                        * the voxel clouds of a call on a thousand sweeps, and hundreds of maps of full sweeps
                                                        * in one launch (a map is one workgroup of k_submap_target, a match one of k_submap_icp) */

/* what both entries check behind their own arguments: BEV_OK, or what the entry returns.  frame_n: the frames' record counts */
static int submap_reg_check(int n_frames, const std::vector<uint64_t> &frame_n, int n_maps, const uint64_t *map_offs,
                     const int32_t *entry_frame, const float *entry_pose, int n_matches, const bev_match_t *h_matches)
{
    const int rc = check_submap_entries(n_frames, n_maps, map_offs, entry_frame, entry_pose);
    if (rc != BEV_OK) return rc;
    for (int m = 0; m < n_matches; ++m) {
        const bev_match_t &mt = h_matches[m];
        if (mt.query_idx < 0 || mt.query_idx >= n_frames || mt.match_idx < 0 || mt.match_idx >= n_maps) return BEV_ERR_INVALID_ARG;
    }
    for (int g = 0; g < n_maps; ++g)
        if (bevsubreg::map_capacity(frame_n.data(), map_offs, entry_frame, g) > BEV_SUBMAP_REG_MAX_TARGET) return BEV_ERR_TOO_LARGE;
    return BEV_OK;
}

/* the cloud call's outputs (bev_submap_voxel_cloud_device_resident) */
struct SubmapCloudOut {
    float4 *d_out;
    uint64_t stride;
    uint32_t *d_counts;
};

/* The call on the context's stream, behind the entries' checks and begin_call: frame f = frame_n[f] records at frame_off[f]
 * of d_clouds.  map_leaf > 0: the maps are thinned by a voxel grid over their union (bev_submap_vox.h);
 * map_leaf == 0 with matches: §6k's launches and workspace, unchanged.  cloud: no matches; every map's target goes out. */
static int submap_reg_frames(bev_ctx *c, int n_frames, const bev_point_t *d_clouds, const std::vector<uint64_t> &frame_off,
                      const std::vector<uint64_t> &frame_n, float leaf, float map_leaf, int n_maps, const uint64_t *map_offs,
                      const int32_t *entry_frame, const float *entry_pose, int n_matches, const bev_match_t *h_matches,
                      const bev_icp_result_t *d_coarse, const int32_t *d_best, const bev_icp_params_t &prm,
                      bev_icp_result_t *d_results, const SubmapCloudOut *cloud)
{
    const bool vox = map_leaf > 0.0f, staged = vox || cloud; /* staged: the moved points get an array of their own */
    std::vector<int32_t> query((size_t)n_matches), match_map((size_t)n_matches);
    for (int m = 0; m < n_matches; ++m) {
        query[(size_t)m] = h_matches[m].query_idx;
        match_map[(size_t)m] = h_matches[m].match_idx;
    }
    const uint64_t cap = c->submap_reg_group ? (uint64_t)c->submap_reg_group : kSubmapRegCap;
    const bevsubreg::Plan plan = bevsubreg::plan_call(n_frames, frame_off.data(), frame_n.data(), n_maps, map_offs, entry_frame,
                                                      entry_pose, n_matches, query.data(), match_map.data(), cap, vox,
                                                      cloud != nullptr);
    const size_t U = plan.slots.size(), P = plan.probs.size(), E = plan.entries.size(), Pn = plan.Pn, Kn = pow2_at_least(Pn);
    const size_t G = std::min(U, (size_t)kFineVoxelGroup), L = std::min(P, (size_t)kFineProblemsPerLaunch);
    const size_t T = std::max<size_t>((size_t)plan.max_group_pts, 1), M = std::max<size_t>(plan.max_group_maps, 1);
    const size_t NM = plan.maps.size();
    /* the workspace: the voxel clouds of the slots (no grids: no frame is a target), the scratch of a voxel launch and of an
     * ICP launch, the entries' first indices, the maps of one launch group; staged: the concatenations; vox: the union
     * grid's keys, voxel starts and headers (t.pts is then the thinned array) */
    FineWork w{};
    SubmapRegWork t{};
    SubmapVoxWork v{};
    uint32_t *ent_start = nullptr;
    const bool grid = !cloud, thin = !cloud || vox;
    const size_t sz[] = {U * Pn * sizeof(bev_point_t), U * 4, G * Kn * 8, G * (Pn + 1) * 4, L * Pn * 16, L * Pn * 4,
                         std::max<size_t>(E, 1) * 4, thin ? T * 16 : 0, grid ? T * 16 : 0, grid ? M * sizeof(IcpGridHdr) : 0,
                         grid ? M * 4 * (size_t)(kFineCells + 1) : 0, staged ? T * 16 : 0,
                         vox ? std::max<size_t>((size_t)plan.max_group_keys, 1) * 8 : 0, vox ? (T + M) * 4 : 0,
                         staged ? M * sizeof(SubvoxHdr) : 0};
    void **const dst[] = {(void **)&w.vox, (void **)&w.vox_n, (void **)&w.keys, (void **)&w.vstart, (void **)&w.cur,
                          (void **)&w.corr, (void **)&ent_start, (void **)&t.pts, (void **)&t.sorted, (void **)&t.hdr,
                          (void **)&t.cell_off, (void **)&v.moved, (void **)&v.keys, (void **)&v.vstart, (void **)&v.vh};
    int rc = c->reg.fine_buf.grow(c, carve(nullptr, sz, dst));
    if (rc != BEV_OK) return rc;
    carve(c->reg.fine_buf.p, sz, dst);
    if (!grid) t.sorted = nullptr, t.hdr = nullptr, t.cell_off = nullptr; /* (k_submap_vox_finish builds no grid) */
    w.Pn = Pn;
    w.Kn = Kn;
    /* the tables, one block: slots, maps, entries (64-byte aligned), problems; vox: the maps' first keys behind them */
    static_assert(sizeof(bevsubreg::Slot) == sizeof(FineSlot), "the plan's slots are k_fine_voxel's");
    const size_t o_maps = align256(U * sizeof(FineSlot)), o_ent = o_maps + align256(NM * sizeof(bevsubreg::Map)),
                 o_probs = o_ent + align256(E * sizeof(bevsubreg::Entry)),
                 o_key0 = vox ? o_probs + align256(P * sizeof(FineProblem)) : 0,
                 tab = vox ? o_key0 + NM * 8 : o_probs + P * sizeof(FineProblem);
    void *hv;
    rc = c->reg.fine_tab.begin(c, tab, kRegTabMin, &hv);
    if (rc != BEV_OK) return rc;
    char *h = static_cast<char *>(hv);
    if (U) std::memcpy(h, plan.slots.data(), U * sizeof(FineSlot));
    if (NM) std::memcpy(h + o_maps, plan.maps.data(), NM * sizeof(bevsubreg::Map));
    if (E) std::memcpy(h + o_ent, plan.entries.data(), E * sizeof(bevsubreg::Entry));
    if (vox && NM) std::memcpy(h + o_key0, plan.map_key0.data(), NM * 8);
    FineProblem *hp = reinterpret_cast<FineProblem *>(h + o_probs);
    for (size_t k = 0; k < P; ++k) {
        const bevsubreg::Problem &pp = plan.probs[k];
        FineProblem &pb = hp[k];
        pb.src_slot = pp.src_slot;
        pb.tgt_slot = pp.map;
        pb.result = pp.result;
        pb.coarse_match = d_coarse ? pp.result : 0xffffffffu;
        bevx::icp_tool_guess(h_matches[pp.result].angle_guess, 0, pb.guess);
    }
    rc = c->reg.fine_tab.push(c, tab);
    if (rc != BEV_OK) return rc;
    const char *dev = static_cast<const char *>(c->reg.fine_tab.dev);
    const FineSlot *d_slots = reinterpret_cast<const FineSlot *>(dev);
    const void *d_maps = dev + o_maps, *d_entries = dev + o_ent;
    const FineProblem *d_probs = reinterpret_cast<const FineProblem *>(dev + o_probs);
    v.key0 = vox ? reinterpret_cast<const uint64_t *>(dev + o_key0) : nullptr;
    rc = fine_voxel(c, d_clouds, d_slots, (int)U, w, leaf);
    if (rc != BEV_OK) return rc;
    /* the groups one behind the other on the stream: its order hands the maps' arrays from group to group */
    for (const bevsubreg::Group &g : plan.groups) {
        const int gm = (int)g.n_maps;
        if (!staged) {
            ProfScope ps(c, K_SUBMAP_TARGET, gm);
            launch_submap_target(d_maps, g.map0, gm, d_entries, w, ent_start, t, c->stream);
        } else {
            {
                ProfScope ps(c, K_SUBMAP_VOX_MOVE, gm);
                launch_submap_vox_move(d_maps, g.map0, gm, d_entries, w, ent_start, v, c->stream);
            }
            if (vox) {
                {
                    ProfScope ps(c, K_SUBMAP_VOX_KEYS, gm);
                    launch_submap_vox_keys(d_maps, g.map0, gm, v, map_leaf, c->stream);
                }
                const uint32_t tiles = bevsubvox::tiles(g.max_slots);
                for (const bevsubvox::Stage &sg : bevsubvox::schedule(g.max_slots)) {
                    ProfScope ps(c, sg.kind == bevsubvox::kStageGlobal ? K_SUBMAP_VOX_GLOBAL : K_SUBMAP_VOX_TILE, gm);
                    launch_submap_vox_stage(sg.kind, sg.k, sg.j, g.map0, gm, tiles, v, c->stream);
                }
                ProfScope ps(c, K_SUBMAP_VOX_FINISH, gm);
                launch_submap_vox_finish(d_maps, g.map0, gm, v, t, c->stream);
            }
            if (cloud) {
                uint64_t largest = 0;
                for (uint32_t u = g.map0; u < g.map0 + g.n_maps; ++u) largest = std::max(largest, plan.map_cap[u]);
                const uint32_t parts = (uint32_t)std::min<uint64_t>((largest + 4 * kFineThreads - 1) / (4 * kFineThreads), 256);
                ProfScope ps(c, K_SUBMAP_VOX_OUT, gm);
                launch_submap_vox_out(d_maps, g.map0, gm, parts, v.vh, vox ? t.pts : v.moved, cloud->d_out, cloud->stride,
                                      cloud->d_counts, c->stream);
            }
        }
        for (uint32_t p0 = 0; p0 < g.n_probs; p0 += kFineProblemsPerLaunch) {
            const int n = (int)std::min<uint32_t>(kFineProblemsPerLaunch, g.n_probs - p0);
            ProfScope ps(c, K_SUBMAP_ICP, n);
            launch_submap_icp(d_probs + g.prob0 + p0, n, d_maps, g.map0, w, t, d_coarse, d_best, prm, d_results, c->stream);
        }
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

int bev_submap_voxel_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds,
                                                  const uint64_t *h_offsets, float leaf, float map_leaf, int n_maps,
                                                  const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                                  const float *h_entry_pose, int n_matches, const bev_match_t *h_matches,
                                                  const bev_icp_result_t *d_coarse, const int32_t *d_best,
                                                  const bev_icp_params_t *params, bev_icp_result_t *d_results)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_fine_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm) || !(std::isfinite(leaf) && leaf > 0.0f) ||
        !(std::isfinite(map_leaf) && map_leaf >= 0.0f) || (d_coarse == nullptr) != (d_best == nullptr))
        return BEV_ERR_INVALID_ARG;
    std::vector<uint64_t> frame_off, frame_n;
    if (n_matches > 0) {
        if (!h_matches || !d_results) return BEV_ERR_INVALID_ARG;
        frame_off.resize((size_t)n_frames);
        frame_n.resize((size_t)n_frames);
        for (int f = 0; f < n_frames; ++f) {
            if (h_offsets && (h_offsets[f + 1] < h_offsets[f] || h_offsets[f + 1] - h_offsets[f] > 0xffffffffull)) return BEV_ERR_INVALID_ARG;
            frame_off[(size_t)f] = h_offsets ? h_offsets[f] : (uint64_t)f * c->geo.S;
            frame_n[(size_t)f] = h_offsets ? h_offsets[f + 1] - h_offsets[f] : (uint64_t)c->geo.S;
        }
        const int rc_ = submap_reg_check(n_frames, frame_n, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches);
        if (rc_ != BEV_OK) return rc_;
        if (!d_clouds) return BEV_ERR_INVALID_ARG;
    }
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n_matches == 0) return BEV_OK;
    rc = wait_default_stream(c);
    if (rc != BEV_OK) return rc;
    rc = submap_reg_frames(c, n_frames, d_clouds, frame_off, frame_n, leaf, map_leaf, n_maps, h_map_offsets, h_entry_frame,
                           h_entry_pose, n_matches, h_matches, d_coarse, d_best, prm, d_results, nullptr);
    if (rc != BEV_OK) return rc;
    return record_tail(c);
}

int bev_submap_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                            float leaf, int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                            const float *h_entry_pose, int n_matches, const bev_match_t *h_matches,
                                            const bev_icp_result_t *d_coarse, const int32_t *d_best,
                                            const bev_icp_params_t *params, bev_icp_result_t *d_results)
{
    return bev_submap_voxel_registration_device_resident(c, n_frames, d_clouds, h_offsets, leaf, 0.0f, n_maps, h_map_offsets,
                                                         h_entry_frame, h_entry_pose, n_matches, h_matches, d_coarse, d_best,
                                                         params, d_results);
}

int bev_submap_voxel_cloud_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                           float leaf, float map_leaf, int n_maps, const uint64_t *h_map_offsets,
                                           const int32_t *h_entry_frame, const float *h_entry_pose, uint64_t out_stride,
                                           float *d_out, uint32_t *d_counts)
{
    if (!c || n_frames < 0 || n_maps < 0 || !(std::isfinite(leaf) && leaf > 0.0f) || !(std::isfinite(map_leaf) && map_leaf >= 0.0f))
        return BEV_ERR_INVALID_ARG;
    std::vector<uint64_t> frame_off, frame_n;
    if (n_maps > 0) {
        if (!d_out || !d_counts) return BEV_ERR_INVALID_ARG;
        frame_off.resize((size_t)n_frames);
        frame_n.resize((size_t)n_frames);
        for (int f = 0; f < n_frames; ++f) {
            if (h_offsets && (h_offsets[f + 1] < h_offsets[f] || h_offsets[f + 1] - h_offsets[f] > 0xffffffffull)) return BEV_ERR_INVALID_ARG;
            frame_off[(size_t)f] = h_offsets ? h_offsets[f] : (uint64_t)f * c->geo.S;
            frame_n[(size_t)f] = h_offsets ? h_offsets[f + 1] - h_offsets[f] : (uint64_t)c->geo.S;
        }
        const int rc_ = submap_reg_check(n_frames, frame_n, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, 0, nullptr);
        if (rc_ != BEV_OK) return rc_;
        for (int g = 0; g < n_maps; ++g)
            if (bevsubreg::map_capacity(frame_n.data(), h_map_offsets, h_entry_frame, g) > out_stride) return BEV_ERR_INVALID_ARG;
        if (!d_clouds) return BEV_ERR_INVALID_ARG;
    }
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n_maps == 0) return BEV_OK;
    rc = wait_default_stream(c);
    if (rc != BEV_OK) return rc;
    const SubmapCloudOut out{reinterpret_cast<float4 *>(d_out), out_stride, d_counts};
    rc = submap_reg_frames(c, n_frames, d_clouds, frame_off, frame_n, leaf, map_leaf, n_maps, h_map_offsets, h_entry_frame,
                           h_entry_pose, 0, nullptr, nullptr, nullptr, bev_icp_fine_defaults(), nullptr, &out);
    if (rc != BEV_OK) return rc;
    return record_tail(c);
}

int bev_submap_voxel_registration_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                                        float leaf, float map_leaf, int n_maps, const uint64_t *h_map_offsets,
                                        const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                        const bev_match_t *h_matches, const bev_icp_params_t *params, bev_icp_result_t *results)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_fine_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm) || !(std::isfinite(leaf) && leaf > 0.0f) ||
        !(std::isfinite(map_leaf) && map_leaf >= 0.0f))
        return BEV_ERR_INVALID_ARG;
    if (n_frames > 0 && (!clouds || !n_pts)) return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (n_pts[f] && !clouds[f]) return BEV_ERR_INVALID_ARG;
    std::vector<uint64_t> frame_off((size_t)n_frames), frame_n((size_t)n_frames);
    if (n_matches > 0) {
        if (!h_matches || !results) return BEV_ERR_INVALID_ARG;
        for (int f = 0; f < n_frames; ++f) frame_n[(size_t)f] = n_pts[f];
        const int rc_ = submap_reg_check(n_frames, frame_n, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches);
        if (rc_ != BEV_OK) return rc_;
    }
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n_matches == 0) return BEV_OK;
    std::vector<size_t> offs((size_t)std::max(n_frames, 1));
    rc = fine_upload(c, clouds, n_pts, n_frames, offs.data());
    if (rc != BEV_OK) return rc;
    for (int f = 0; f < n_frames; ++f) frame_off[(size_t)f] = offs[(size_t)f];
    rc = c->reg.sub_res.grow(c, (size_t)n_matches * sizeof(bev_icp_result_t));
    if (rc != BEV_OK) return rc;
    bev_icp_result_t *d_res = static_cast<bev_icp_result_t *>(c->reg.sub_res.p);
    rc = submap_reg_frames(c, n_frames, static_cast<const bev_point_t *>(c->reg.fine_in.p), frame_off, frame_n, leaf, map_leaf,
                           n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches, nullptr, nullptr, prm, d_res,
                           nullptr);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemcpyAsync(results, d_res, (size_t)n_matches * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

int bev_submap_registration_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, float leaf,
                                  int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                  const float *h_entry_pose, int n_matches, const bev_match_t *h_matches,
                                  const bev_icp_params_t *params, bev_icp_result_t *results)
{
    return bev_submap_voxel_registration_batch(c, n_frames, clouds, n_pts, leaf, 0.0f, n_maps, h_map_offsets, h_entry_frame,
                                               h_entry_pose, n_matches, h_matches, params, results);
}

/* ---- scan-to-map coarse ICP: PointNormal frames against submaps (bev_submap_coarse.h) ------------------ */
int bev_submap_coarse_registration_device_resident(bev_ctx_t *c, int n_frames, const void *d_pn, size_t stride,
                                                   const uint32_t *d_counts, int n_maps, const uint64_t *h_map_offsets,
                                                   const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                   const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                   bev_icp_result_t *d_results, int32_t *d_best)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_coarse_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm)) return BEV_ERR_INVALID_ARG;
    if (n_matches > 0) {
        if (!d_pn || !d_counts || !h_matches || !d_results || !d_best || stride == 0) return BEV_ERR_INVALID_ARG;
        const int rc_ = check_submap_entries(n_frames, n_maps, h_map_offsets, h_entry_frame, h_entry_pose);
        if (rc_ != BEV_OK) return rc_;
        for (int m = 0; m < n_matches; ++m) {
            const bev_match_t &mt = h_matches[m];
            if (mt.query_idx < 0 || mt.query_idx >= n_frames || mt.match_idx < 0 || mt.match_idx >= n_maps) return BEV_ERR_INVALID_ARG;
        }
        /* a map's capacity is n_entries * stride rows: the true counts live on the device, and the host does not wait for them */
        for (int g = 0; g < n_maps; ++g) {
            const uint64_t ne = h_map_offsets[g + 1] - h_map_offsets[g];
            if (ne && (uint64_t)stride > BEV_SUBMAP_COARSE_MAX_TARGET / ne) return BEV_ERR_TOO_LARGE;
        }
    }
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    if (n_matches == 0) return BEV_OK;
    rc = wait_default_stream(c);
    if (rc != BEV_OK) return rc;
    /* §6k's plan with every frame counted at stride rows and a PointNormal map's bytes */
    std::vector<int32_t> query((size_t)n_matches), match_map((size_t)n_matches);
    for (int m = 0; m < n_matches; ++m) {
        query[(size_t)m] = h_matches[m].query_idx;
        match_map[(size_t)m] = h_matches[m].match_idx;
    }
    const std::vector<uint64_t> frame_off((size_t)n_frames, 0), frame_n((size_t)n_frames, (uint64_t)stride);
    const uint64_t cap = c->submap_reg_group ? (uint64_t)c->submap_reg_group : kSubmapRegCap;
    bevsubreg::Plan plan = bevsubreg::plan_call(n_frames, frame_off.data(), frame_n.data(), n_maps, h_map_offsets, h_entry_frame,
                                                h_entry_pose, n_matches, query.data(), match_map.data(), cap, false, false, true);
    for (bevsubreg::Entry &en : plan.entries) en.slot = (uint32_t)plan.slot_frame[en.slot]; /* the device reads the frame */
    const size_t P = 2 * plan.probs.size(), E = plan.entries.size(), NM = plan.maps.size();
    const size_t L = std::min(P, (size_t)kIcpProblemsPerLaunch);
    const size_t T = std::max<size_t>((size_t)plan.max_group_pts, 1), M = std::max<size_t>(plan.max_group_maps, 1);
    /* the workspace, in the coarse stage's buffer: the scratch of an ICP launch, the entries' first indices, the maps of one
     * launch group */
    SubmapCoarseWork t{};
    uint32_t *ent_start = nullptr;
    const size_t sz[] = {L * 16 * stride, std::max<size_t>(E, 1) * 4, T * 48, T * 16, M * sizeof(IcpGridHdr),
                         M * 4 * (size_t)(kIcpCells + 1)};
    void **const dst[] = {(void **)&t.cur, (void **)&ent_start, (void **)&t.rows, (void **)&t.sorted, (void **)&t.hdr,
                          (void **)&t.cell_off};
    rc = c->reg.icp_buf.grow(c, carve(nullptr, sz, dst));
    if (rc != BEV_OK) return rc;
    carve(c->reg.icp_buf.p, sz, dst);
    /* the tables, one block: maps, entries (64-byte aligned), problems: two per match, the guesses adjacent */
    const size_t o_ent = align256(NM * sizeof(bevsubreg::Map)), o_probs = o_ent + align256(E * sizeof(bevsubreg::Entry)),
                 tab = o_probs + P * sizeof(IcpProblem);
    void *hv;
    rc = c->reg.icp_tab.begin(c, tab, kRegTabMin, &hv);
    if (rc != BEV_OK) return rc;
    char *h = static_cast<char *>(hv);
    if (NM) std::memcpy(h, plan.maps.data(), NM * sizeof(bevsubreg::Map));
    if (E) std::memcpy(h + o_ent, plan.entries.data(), E * sizeof(bevsubreg::Entry));
    IcpProblem *hp = reinterpret_cast<IcpProblem *>(h + o_probs);
    for (size_t k = 0; k < plan.probs.size(); ++k) {
        const bevsubreg::Problem &pp = plan.probs[k];
        for (int g = 0; g < 2; ++g) {
            IcpProblem &pb = hp[2 * k + g];
            pb.src_frame = (uint32_t)h_matches[pp.result].query_idx;
            pb.tgt_frame = 0xffffffffu; /* (not read: the target is a map) */
            pb.tgt_slot = pp.map;
            pb.result = 2 * pp.result + (uint32_t)g;
            bevx::icp_tool_guess(h_matches[pp.result].angle_guess, g, pb.guess);
        }
    }
    rc = c->reg.icp_tab.push(c, tab);
    if (rc != BEV_OK) return rc;
    const char *dev = static_cast<const char *>(c->reg.icp_tab.dev);
    const void *d_maps = dev, *d_entries = dev + o_ent;
    const IcpProblem *d_probs = reinterpret_cast<const IcpProblem *>(dev + o_probs);
    const float *pn = static_cast<const float *>(d_pn);
    /* the groups one behind the other on the stream: its order hands the maps' arrays from group to group */
    for (const bevsubreg::Group &g : plan.groups) {
        {
            ProfScope ps(c, K_SUBMAP_PN_TARGET, (int)g.n_maps);
            launch_submap_pn_target(d_maps, g.map0, (int)g.n_maps, d_entries, pn, stride, d_counts, ent_start, t, c->stream);
        }
        for (uint32_t p0 = 0; p0 < 2 * g.n_probs; p0 += kIcpProblemsPerLaunch) {
            const int n = (int)std::min<uint32_t>(kIcpProblemsPerLaunch, 2 * g.n_probs - p0);
            ProfScope ps(c, K_SUBMAP_COARSE_ICP, n);
            launch_submap_coarse_icp(pn, stride, d_counts, d_probs + 2 * (size_t)g.prob0 + p0, n, d_maps, g.map0, t, prm, d_results,
                                     c->stream);
        }
    }
    {
        ProfScope ps(c, K_ICP_BEST, n_matches);
        launch_icp_best(d_results, n_matches, d_best, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return record_tail(c);
}

} /* extern "C" */
