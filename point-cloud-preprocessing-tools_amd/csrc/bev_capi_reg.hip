/*
 * bev_capi_reg.hip — the registration half of the extern "C" boundary declared in include/bev_mi355x.h: the front end
 * (top-part flatten, voxel grid, 2-D normals), coarse point-to-plane ICP (§6c) and the fine stage (§6d), frame
 * against frame.  Frames against submaps: bev_capi_submap_reg.hip, which shares bev_reg_host.h with this file (§6n).
 * Host-side only; the kernels are in bev_kernels.hip (bev_reg_common.h, bev_regfront.h, bev_icp.h, bev_fine.h).  With
 * the BEV pipeline of bev_capi.hip it shares the context (bev_ctx.h), its stream and the call prologue (begin_call).
 */
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "bev_reg_host.h"

#include "bev_libm_f64.h"
#include "bev_pair_grid_plan.h"

using namespace bevk;
using namespace bevh;

/* ---- what the entry points keep between calls (RegState, bev_ctx.h; DevBuf and UploadTable themselves: bev_capi.hip) ---- */
void RegState::release()
{
    for (DevBuf *b : {&rf_buf, &icp_buf, &icp_one, &fine_buf, &fine_in, &sub_res, &verify_buf, &verify_io}) b->release();
    for (UploadTable *t : {&rf_offs, &icp_tab, &fine_tab, &verify_tab}) t->release();
    if (tail_ev) (void)hipEventDestroy(tail_ev);
    tail_ev = nullptr;
    tail_pending = false;
}

namespace {

/* the guess of the single-pair calls: the caller's matrix, or the identity */
void guess_or_identity(const float *guess16, float *out)
{
    for (int k = 0; k < 16; ++k) out[k] = guess16 ? guess16[k] : (k % 5 == 0 ? 1.0f : 0.0f);
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
    BEVCK(r.rf_buf.grow(c, carve(nullptr, sz, dst)));
    carve(r.rf_buf.p, sz, dst);
    r.rf.P = P;
    r.rf.Q = Q;
    return BEV_OK;
}
/* how the front end's entry points begin, behind their argument checks */
int rf_begin(bev_ctx *c)
{
    BEVCK(begin_call(c, false));
    return ensure_rf(c);
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

/* ---- search grids sized to the cloud (bev_set_pair_search_grid; bev_pair_grid.h, bev_pair_grid_plan.h) ---- */

/* what a stage's cap D > 0 adds to its call: the layout, the host's tables of the targets and, behind pair_grid_work and
 * table_up, where the pieces lie on the device */
struct PairGrid {
    int cap = 0;
    size_t targets = 0;
    bevpair::Layout l;
    std::vector<bevsubreg::Map> maps; /* a target's first point, its slot (fine) or frame (coarse) */
    std::vector<uint64_t> cell0;      /* its first counter inside its build group */
    uint32_t *off = nullptr;          /* [targets][l.off_words] */
    SubmapGridWork gw{};              /* cnt, part_bounds, part_sum: one build group's */
    SubvoxHdr *vh = nullptr;          /* [targets] */
    void *d_maps = nullptr, *d_cell0 = nullptr;
};
/* the tables of `targets` targets of one capacity; target t's points begin at first[t] * capacity, first[t] its slot or frame */
template <class First>
void pair_grid_plan(PairGrid &g, int cap, size_t targets, size_t capacity, First first)
{
    g.cap = cap;
    g.targets = targets;
    g.l = bevpair::layout(targets, capacity, cap);
    if (!cap) return;
    for (size_t t = 0; t < targets; ++t) {
        g.maps.push_back(bevsubreg::Map{(uint64_t)first(t) * capacity, (uint32_t)first(t), 0u});
        g.cell0.push_back(bevpair::cell0(t, g.l));
    }
}
/* the grids of the call's targets, one build group behind the other on the context's stream: the point counts, then the build
 * (search_grid_build) per group.  hdr, sorted: the stage's own arrays; the points: src's records (fine) or rows (coarse) */
int pair_grid_build(bev_ctx *c, PairGrid &g, IcpGridHdr *hdr, float4 *sorted, const uint32_t *vox_n, const uint32_t *counts,
                    size_t stride, const SubgridSource &src)
{
    {
        ProfScope ps(c, K_PAIRGRID_DESC, (int)g.targets);
        launch_pairgrid_desc(g.d_maps, (int)g.targets, vox_n, counts, stride, g.vh, c->stream);
    }
    g.gw.sorted = sorted;
    g.gw.cell0 = static_cast<const uint64_t *>(g.d_cell0);
    for (const bevpair::Group &gr : bevpair::groups(g.targets, g.l)) {
        g.gw.hdr = hdr + gr.t0;
        g.gw.off = g.off + (size_t)gr.t0 * g.l.off_words;
        BEVCK(search_grid_build(c, g.d_maps, gr.t0, (int)gr.n, g.l.parts, g.l.tiles, g.cap, g.vh + gr.t0, src, g.gw,
                                (size_t)gr.n * g.l.off_words));
    }
    return BEV_OK;
}
/* what bev_debug_get_pair_grid reads of a call's matches, match m's first problem being probs[m * per_match]: the grid of
 * its target slot, whose offsets lie at slot * off_words */
template <class Problem>
void pair_grid_record(bev_ctx *c, int coarse, const IcpGridHdr *hdr, const uint32_t *cell_off, uint64_t off_words,
                      const std::vector<Problem> &probs, size_t per_match)
{
    GridRecord &r = c->pair_grid_rec[coarse];
    r = GridRecord{};
    r.uses = stage_buf(c, coarse).uses;
    r.hdr = hdr;
    r.cell_off = cell_off;
    for (size_t m = 0; m * per_match < probs.size(); ++m) {
        const uint64_t slot = probs[m * per_match].tgt_slot;
        r.items.push_back({slot, slot * off_words, off_words - 1});
    }
}

} // namespace

/* ---- the fine stage's steps that bev_capi_submap_reg.hip runs as well (bev_reg_host.h) ---- */
int bevh::fine_voxel(bev_ctx *c, const bev_point_t *d_pts, const FineSlot *d_slots, int U, const FineWork &w, float leaf)
{
    for (int s0 = 0; s0 < U; s0 += kFineVoxelGroup) {
        const int n = std::min(kFineVoxelGroup, U - s0);
        ProfScope ps(c, K_FINE_VOXEL, n);
        launch_fine_voxel(d_pts, d_slots, s0, n, w, leaf, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

/* ---- search grids sized to the target: the build's driver and the hooks' reader (bev_reg_host.h) ---- */
int bevh::search_grid_build(bev_ctx *c, const void *d_maps, uint32_t t0, int n, uint32_t parts, uint32_t tiles, int cap,
                            const SubvoxHdr *vh, const SubgridSource &src, const SubmapGridWork &w, size_t clear_words)
{
    HIPCK(c, hipMemsetAsync(w.cnt, 0, clear_words * 4, c->stream));
    for (int step = 0; step < 6; ++step) {
        ProfScope ps(c, K_SUBMAP_GRID_BOUNDS + step, n);
        launch_subgrid(step, d_maps, t0, n, parts, tiles, cap, vh, src, w, c->stream);
    }
    return BEV_OK;
}

int bevh::grid_record_read(bev_ctx *c, const GridRecord &r, int first, int n, uint32_t *out)
{
    BEVCK(begin_call(c, false));
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> off;
    for (int i = 0; i < n; ++i) {
        const GridRecord::Item &it = r.items[(size_t)(first + i)];
        IcpGridHdr h;
        HIPCK(c, hipMemcpy(&h, r.hdr + it.hdr, sizeof h, hipMemcpyDeviceToHost));
        if (h.nx < 1 || h.ny < 1 || (uint64_t)h.nx * (uint64_t)h.ny > it.cells) return BEV_ERR_INVALID_ARG; /* (not a grid) */
        off.resize((size_t)h.nx * (size_t)h.ny + 1);
        HIPCK(c, hipMemcpy(off.data(), r.cell_off + it.off0, off.size() * 4, hipMemcpyDeviceToHost));
        uint32_t largest = 0;
        for (size_t k = 0; k + 1 < off.size(); ++k) largest = std::max(largest, off[k + 1] - off[k]);
        out[4 * i] = (uint32_t)h.nx;
        out[4 * i + 1] = (uint32_t)h.ny;
        out[4 * i + 2] = h.n;
        out[4 * i + 3] = largest;
    }
    return BEV_OK;
}

/* host records -> c->reg.fine_in (grown on demand) */
int bevh::fine_upload(bev_ctx *c, const bev_point_t *const *clouds, const uint32_t *n, int k, size_t *offs)
{
    size_t total = 0;
    for (int i = 0; i < k; ++i) {
        offs[i] = total;
        total += n[i];
    }
    const size_t need = std::max<size_t>(total, 1) * sizeof(bev_point_t);
    BEVCK(c->reg.fine_in.grow(c, need));
    for (int i = 0; i < k; ++i)
        if (n[i])
            HIPCK(c, hipMemcpyAsync(static_cast<bev_point_t *>(c->reg.fine_in.p) + offs[i], clouds[i], (size_t)n[i] * sizeof(bev_point_t),
                                    hipMemcpyHostToDevice, c->stream));
    return BEV_OK;
}

extern "C" {

/* ---- registration front end ------------------------------------------------------------------------------------------ */
size_t bev_regfront_max_out(size_t n) { return n / 5 + 51; }

int bev_top_part_flatten(bev_ctx_t *c, const bev_point_t *cloud, uint32_t n, float *out, uint32_t *n_out)
{
    if (!c || !n_out || (n && (!cloud || !out))) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    *n_out = 0;
    BEVCK(rf_begin(c));
    if (n == 0) return BEV_OK;
    BEVCK(ensure_staging(c));
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
    if (!c || !n_out || (n && (!xyz || !out)) || !positive(leaf)) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    *n_out = 0;
    BEVCK(rf_begin(c));
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
    if (!positive(radius)) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    BEVCK(rf_begin(c));
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
    if (!c || n_frames < 0 || !positive(leaf) || !positive(radius)) return BEV_ERR_INVALID_ARG;
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
    BEVCK(rf_begin(c));
    if (n_frames == 0) return BEV_OK;
    BEVCK(wait_default_stream(c)); /* (the upload of packed clouds, typically) */
    const uint64_t *d_offs = nullptr;
    if (h_offsets) {
        const size_t bytes = ((size_t)n_frames + 1) * 8;
        void *h;
        BEVCK(c->reg.rf_offs.begin(c, bytes, 1024 * 8, &h));
        std::memcpy(h, h_offsets, bytes);
        BEVCK(c->reg.rf_offs.push(c, bytes));
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
        BEVCK(rf_chain(c, in, nf, leaf, radius, vp, n_max, static_cast<float *>(d_out) + (size_t)f0 * out_stride * 12, out_stride,
                       d_counts + f0));
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

namespace {

/* the grids of the target frames slot_frames, then every problem (launches of kIcpProblemsPerLaunch), then, when d_best is
 * set, the better guess of each of the n_best matches; all on the context's stream.  per_match: problems of a match (the hook's
 * record); cap: the stage's search grid cap, 0 the fixed grids; n_frames: the frames behind d_pn (read under a cap only) */
int icp_launch(bev_ctx *c, const float *d_pn, size_t stride, const uint32_t *d_counts, size_t n_frames,
               const std::vector<IcpProblem> &probs, size_t per_match, const std::vector<uint32_t> &slot_frames,
               const bev_icp_params_t &prm, bev_icp_result_t *d_res, int n_best, int32_t *d_best, int cap)
{
    const size_t U = slot_frames.size(), P = probs.size(), L = std::min(P, (size_t)kIcpProblemsPerLaunch);
    IcpWork w{};
    PairGrid g;
    pair_grid_plan(g, cap, U, stride, [&](size_t t) { return slot_frames[t]; });
    float4 *by_frame = nullptr; /* under a cap the searchable points lie by FRAME: the build writes them where it reads */
    const size_t sz[] = {U * sizeof(IcpGridHdr), cap ? 0 : U * 4 * (size_t)(kIcpCells + 1), cap ? 0 : U * 16 * stride, L * 16 * stride,
                         g.l.off_bytes, cap ? n_frames * 16 * stride : 0, g.l.cnt_bytes, g.l.bounds_bytes, g.l.sums_bytes,
                         g.l.hdr_bytes};
    void **const dst[] = {(void **)&w.hdr, (void **)&w.cell_off, (void **)&w.sorted, (void **)&w.cur, (void **)&g.off,
                          (void **)&by_frame, (void **)&g.gw.cnt, (void **)&g.gw.part_bounds, (void **)&g.gw.part_sum, (void **)&g.vh};
    BEVCK(c->reg.icp_buf.grow(c, carve(nullptr, sz, dst)));
    carve(c->reg.icp_buf.p, sz, dst);
    IcpProblem *d_probs;
    uint32_t *d_slots;
    const size_t tsz[] = {P * sizeof(IcpProblem), U * 4, g.l.map_bytes, g.l.cell0_bytes};
    const void *const tsrc[] = {probs.data(), slot_frames.data(), g.maps.data(), g.cell0.data()};
    void **const tdst[] = {(void **)&d_probs, (void **)&d_slots, &g.d_maps, &g.d_cell0};
    BEVCK(table_up(c, c->reg.icp_tab, tsz, tsrc, tdst));
    if (cap) {
        w.cell_off = g.off;
        w.sorted = by_frame;
        BEVCK(pair_grid_build(c, g, w.hdr, w.sorted, nullptr, d_counts, stride, SubgridSource{nullptr, nullptr, d_pn}));
    } else {
        ProfScope ps(c, K_ICP_GRID, (int)U);
        launch_icp_grid(d_pn, stride, d_counts, d_slots, (int)U, w, c->stream);
    }
    pair_grid_record(c, 1, w.hdr, w.cell_off, cap ? g.l.off_words : (uint64_t)kIcpCells + 1, probs, per_match);
    for (size_t p0 = 0; p0 < P; p0 += kIcpProblemsPerLaunch) {
        const int n = (int)std::min((size_t)kIcpProblemsPerLaunch, P - p0);
        ProfScope ps(c, cap ? K_ICP_WIDE : K_ICP, n);
        if (cap) launch_icp_wide(d_pn, stride, d_counts, d_probs + p0, n, w, g.l.off_words, prm, d_res, c->stream);
        else launch_icp(d_pn, stride, d_counts, d_probs + p0, n, w, prm, d_res, c->stream);
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
    BEVCK(begin_call(c, false));
    const size_t stride = std::max<size_t>(std::max(n_src, n_tgt), 1);
    const size_t need = 2 * stride * 48 + 256 + sizeof(bev_icp_result_t);
    BEVCK(c->reg.icp_one.grow(c, need));
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
    guess_or_identity(guess16, probs[0].guess);
    BEVCK(icp_launch(c, d_pn, stride, d_counts, 2, probs, 1, std::vector<uint32_t>{1u}, prm, d_res, 0, nullptr, c->pair_grid_cap[1]));
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
        if (!matches_in_range(h_matches, n_matches, n_frames, n_frames)) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
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
    BEVCK(icp_launch(c, static_cast<const float *>(d_pn), stride, d_counts, (size_t)n_frames, probs, 2, slot_frames, prm, d_results,
                     n_matches, d_best, c->pair_grid_cap[1]));
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

/* the device workspace for U slots of at most Pn records and P problems (grown when a call needs more), the slot and
 * problem tables uploaded behind everything on the context's stream.  cap: the stage's search grid cap (0: the fixed grids, the
 * layout of always); under a cap the first T slots are the call's targets, and g gets their grids' pieces and tables */
int fine_setup(bev_ctx *c, size_t U, size_t Pn, const std::vector<FineSlot> &slots, const std::vector<FineProblem> &probs,
               FineWork &w, const FineSlot **d_slots, const FineProblem **d_probs, int cap, size_t T, PairGrid &g)
{
    const size_t P = probs.size(), G = std::min(U, (size_t)kFineVoxelGroup), L = std::min(P, (size_t)kFineProblemsPerLaunch);
    const size_t Kn = pow2_at_least(Pn);
    w = FineWork{};
    pair_grid_plan(g, cap, T, Pn, [](size_t t) { return t; });
    const size_t sz[] = {U * Pn * sizeof(bev_point_t), U * 4, G * Kn * 8, G * (Pn + 1) * 4, U * sizeof(IcpGridHdr),
                         cap ? 0 : U * 4 * (size_t)(kFineCells + 1), U * Pn * 16, L * Pn * 16, L * Pn * 4,
                         g.l.off_bytes, g.l.cnt_bytes, g.l.bounds_bytes, g.l.sums_bytes, g.l.hdr_bytes};
    void **const dst[] = {(void **)&w.vox, (void **)&w.vox_n, (void **)&w.keys, (void **)&w.vstart, (void **)&w.hdr,
                          (void **)&w.cell_off, (void **)&w.sorted, (void **)&w.cur, (void **)&w.corr,
                          (void **)&g.off, (void **)&g.gw.cnt, (void **)&g.gw.part_bounds, (void **)&g.gw.part_sum, (void **)&g.vh};
    BEVCK(c->reg.fine_buf.grow(c, carve(nullptr, sz, dst)));
    carve(c->reg.fine_buf.p, sz, dst);
    if (cap) w.cell_off = g.off;
    w.Pn = Pn;
    w.Kn = Kn;
    const size_t tsz[] = {slots.size() * sizeof(FineSlot), P * sizeof(FineProblem), g.l.map_bytes, g.l.cell0_bytes};
    const void *const tsrc[] = {slots.data(), probs.data(), g.maps.data(), g.cell0.data()};
    void **const tdst[] = {(void **)d_slots, (void **)d_probs, &g.d_maps, &g.d_cell0};
    return table_up(c, c->reg.fine_tab, tsz, tsrc, tdst);
}

/* the grids, then the problems in launches of kFineProblemsPerLaunch.  g.cap == 0: a grid for every one of the U slots, as ever;
 * else the wide grids of the targets alone */
int fine_icp(bev_ctx *c, int U, const FineProblem *d_probs, size_t P, const FineWork &w, const bev_icp_result_t *d_coarse,
             const int32_t *d_best, const bev_icp_params_t &prm, bev_icp_result_t *d_res, PairGrid &g)
{
    if (g.cap) {
        BEVCK(pair_grid_build(c, g, w.hdr, w.sorted, w.vox_n, nullptr, w.Pn, SubgridSource{nullptr, w.vox, nullptr}));
    } else {
        ProfScope ps(c, K_FINE_GRID, U);
        launch_fine_grid(U, w, c->stream);
    }
    for (size_t p0 = 0; p0 < P; p0 += kFineProblemsPerLaunch) {
        const int n = (int)std::min((size_t)kFineProblemsPerLaunch, P - p0);
        ProfScope ps(c, g.cap ? K_FINE_ICP_WIDE : K_FINE_ICP, n);
        if (g.cap) launch_fine_icp_wide(d_probs + p0, n, w, g.l.off_words, d_coarse, d_best, prm, d_res, c->stream);
        else launch_fine_icp(d_probs + p0, n, w, d_coarse, d_best, prm, d_res, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

int bev_voxel_grid_irct(bev_ctx_t *c, const bev_point_t *cloud, uint32_t n, float leaf, bev_point_t *out, uint32_t *n_out)
{
    if (!c || !n_out || (n && (!cloud || !out)) || !positive(leaf)) return BEV_ERR_INVALID_ARG;
    *n_out = 0;
    BEVCK(begin_call(c, false));
    if (n == 0) return BEV_OK;
    size_t off = 0;
    BEVCK(fine_upload(c, &cloud, &n, 1, &off));
    FineWork w;
    const FineSlot *d_slots;
    const FineProblem *d_probs;
    PairGrid none;
    BEVCK(fine_setup(c, 1, n, std::vector<FineSlot>{FineSlot{0, n, 0}}, std::vector<FineProblem>{}, w, &d_slots, &d_probs, 0, 0, none));
    BEVCK(fine_voxel(c, static_cast<const bev_point_t *>(c->reg.fine_in.p), d_slots, 1, w, leaf));
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
    BEVCK(begin_call(c, false));
    const size_t Pn = std::max<size_t>(std::max(n_src, n_tgt), 1);
    const int cap = c->pair_grid_cap[0];
    const uint32_t ts = cap ? 0u : 1u, ss = 1u - ts; /* under a cap the targets are the first slots */
    std::vector<FineProblem> probs(1);
    probs[0].src_slot = ss;
    probs[0].tgt_slot = ts;
    probs[0].result = 0;
    probs[0].coarse_match = 0xffffffffu;
    guess_or_identity(guess16, probs[0].guess);
    FineWork w;
    const FineSlot *d_slots;
    const FineProblem *d_probs;
    PairGrid g;
    BEVCK(fine_setup(c, 2, Pn, std::vector<FineSlot>{}, probs, w, &d_slots, &d_probs, cap, 1, g));
    /* the clouds are the "voxel clouds" of the two slots; the result goes behind them in the sort scratch */
    uint32_t counts[2];
    counts[ss] = n_src;
    counts[ts] = n_tgt;
    if (n_src) HIPCK(c, hipMemcpyAsync(w.vox + ss * Pn, src, (size_t)n_src * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    if (n_tgt) HIPCK(c, hipMemcpyAsync(w.vox + ts * Pn, tgt, (size_t)n_tgt * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(w.vox_n, counts, sizeof(counts), hipMemcpyHostToDevice, c->stream));
    bev_icp_result_t *d_res = reinterpret_cast<bev_icp_result_t *>(w.keys);
    BEVCK(fine_icp(c, 2, d_probs, 1, w, nullptr, nullptr, prm, d_res, g));
    pair_grid_record(c, 0, w.hdr, w.cell_off, cap ? g.l.off_words : (uint64_t)kFineCells + 1, probs, 1);
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
    if (!c || n_frames < 0 || n_matches < 0 || !icp_params_ok(prm) || !positive(leaf) ||
        (d_coarse == nullptr) != (d_best == nullptr))
        return BEV_ERR_INVALID_ARG;
    bevsubreg::FrameTable frames;
    if (n_matches > 0) {
        if (!d_clouds || !h_matches || !d_results) return BEV_ERR_INVALID_ARG;
        if (!matches_in_range(h_matches, n_matches, n_frames, n_frames)) return BEV_ERR_INVALID_ARG;
        if (!frame_table(n_frames, h_offsets, (uint64_t)c->geo.S, frames)) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    std::vector<int32_t> slot_of((size_t)n_frames, -1);
    std::vector<FineSlot> slots;
    size_t Pn = 1;
    auto slot = [&](int f) -> uint32_t {
        if (slot_of[f] < 0) {
            slot_of[f] = (int32_t)slots.size();
            slots.push_back(FineSlot{frames.off[(size_t)f], (uint32_t)frames.n[(size_t)f], 0u});
            Pn = std::max(Pn, (size_t)slots.back().n);
        }
        return (uint32_t)slot_of[f];
    };
    /* under a cap the targets come first: their grids are built over the slots [0, T) and no others.  Which slot a frame gets
     * changes no result */
    const int cap = c->pair_grid_cap[0];
    for (int m = 0; cap && m < n_matches; ++m) slot(h_matches[m].match_idx);
    const size_t T = slots.size();
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
    PairGrid g;
    BEVCK(fine_setup(c, (size_t)U, Pn, slots, probs, w, &d_slots, &d_probs, cap, T, g));
    BEVCK(fine_voxel(c, d_clouds, d_slots, U, w, leaf));
    BEVCK(fine_icp(c, U, d_probs, probs.size(), w, d_coarse, d_best, prm, d_results, g));
    pair_grid_record(c, 0, w.hdr, w.cell_off, cap ? g.l.off_words : (uint64_t)kFineCells + 1, probs, 1);
    return record_tail(c);
}

/* ---- search grids sized to the cloud (bev_pair_grid.h) ---------------------------------------------------- */
int bev_set_pair_search_grid(bev_ctx_t *c, int fine_dim, int coarse_dim)
{
    static_assert(BEV_PAIR_SEARCH_GRID_MAX == bevpair::kGridCapMax, "one cap");
    if (!c || fine_dim < 0 || fine_dim > BEV_PAIR_SEARCH_GRID_MAX || coarse_dim < 0 || coarse_dim > BEV_PAIR_SEARCH_GRID_MAX)
        return BEV_ERR_INVALID_ARG;
    c->pair_grid_cap[0] = fine_dim;
    c->pair_grid_cap[1] = coarse_dim;
    return BEV_OK;
}

int bev_debug_get_pair_grid(bev_ctx_t *c, int coarse, int first_match, int n_matches, uint32_t *out)
{
    if (!c || (coarse != 0 && coarse != 1) || first_match < 0 || n_matches < 0 || !out) return BEV_ERR_INVALID_ARG;
    const GridRecord &r = c->pair_grid_rec[coarse];
    if (!r.hdr || (size_t)first_match + (size_t)n_matches > r.items.size()) return BEV_ERR_INVALID_ARG;
    if (r.uses != stage_buf(c, coarse).uses) return BEV_ERR_INVALID_ARG; /* a later call laid it out anew */
    return grid_record_read(c, r, first_match, n_matches, out);
}

} /* extern "C" */

/* ---- the fine stage's workspace without an ICP launch's scratch (bev_reg_host.h): what the verification calls work in ---- */
int bevh::fine_slots_setup(bev_ctx *c, size_t U, size_t Pn, const std::vector<FineSlot> &slots, FineWork &w, const FineSlot **d_slots)
{
    const FineProblem *d_probs;
    PairGrid none;
    return fine_setup(c, U, Pn, slots, std::vector<FineProblem>{}, w, d_slots, &d_probs, 0, 0, none);
}
