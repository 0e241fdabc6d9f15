/*
 * bev_capi_verify.hip — verification of registered matches of the extern "C" boundary declared in include/bev_mi355x.h
 * (DESIGN.md §6aa): under the transform a registration returned, the points of either cloud that have a neighbour in the other
 * within each of a few distances.  Host-side only; the kernels are bev_verify.h's.  The voxel clouds and the targets' grids are
 * the fine stage's and the scan-to-map calls', built by their own steps (bev_reg_host.h) in their own workspace; what this file
 * adds is a launch group's moved queries and their grids.  The sixth file over bev_ctx.h.
 */
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bev_reg_host.h"

using namespace bevk;
using namespace bevh;
using bevsubreg::Call, bevsubreg::Group, bevsubreg::Options, bevsubreg::Plan;

namespace {

/* n_thresholds in 1 ... 8; the first n_thresholds finite, > 0 and strictly ascending, the rest 0 */
bool verify_params_ok(const bev_verify_params_t &p)
{
    if (p.n_thresholds < 1 || p.n_thresholds > BEV_VERIFY_MAX_THRESHOLDS) return false;
    for (int k = 0; k < BEV_VERIFY_MAX_THRESHOLDS; ++k) {
        const float v = p.threshold[k];
        if (k >= p.n_thresholds) {
            if (!(v == 0.0f)) return false;
        } else if (!positive(v) || (k > 0 && !(v > p.threshold[k - 1]))) {
            return false;
        }
    }
    return true;
}

/* points of one k_verify_count workgroup: BEV_VERIFY_SLICE=<points> (tests: no result depends on it), else kVerifySlice */
uint32_t verify_slice()
{
    if (const char *e = getenv("BEV_VERIFY_SLICE")) return (uint32_t)std::max(1, std::min(1 << 20, atoi(e)));
    return kVerifySlice;
}

/* a call's scratch in verify_buf: the moved queries and their grids of a launch group of at most L matches of Pn points */
int verify_work(bev_ctx *c, size_t P, size_t Pn, VerifyWork &v)
{
    const size_t L = std::max<size_t>(std::min(P, (size_t)kVerifyProblemsPerLaunch), 1);
    v = VerifyWork{};
    const size_t sz[] = {L * Pn * 16, L * Pn * 16, L * 4 * (size_t)(kFineCells + 1), L * sizeof(IcpGridHdr)};
    void **const dst[] = {(void **)&v.moved, (void **)&v.qsorted, (void **)&v.qoff, (void **)&v.qhdr};
    BEVCK(c->reg.verify_buf.grow(c, carve(nullptr, sz, dst)));
    carve(c->reg.verify_buf.p, sz, dst);
    v.Pn = Pn;
    return BEV_OK;
}

/* the matches' table up the context's stream */
int verify_table(bev_ctx *c, const std::vector<VerifyProblem> &probs, const VerifyProblem **d_probs)
{
    const size_t tsz[] = {probs.size() * sizeof(VerifyProblem)};
    const void *const tsrc[] = {probs.data()};
    void **const tdst[] = {(void **)d_probs};
    return table_up(c, c->reg.verify_tab, tsz, tsrc, tdst);
}

/* n matches whose targets' grids stand at t, in launch groups of kVerifyProblemsPerLaunch: the moved queries, then both counts.
 * max_pts: the most points a query or a target of theirs can have */
void verify_launches(bev_ctx *c, const VerifyProblem *d_probs, size_t n, const FineWork &w, const VerifyTarget &t, const VerifyWork &v,
                     uint64_t max_pts, const bev_verify_params_t &prm, const bev_icp_result_t *d_results, bev_verify_result_t *d_verify)
{
    const uint32_t slice = verify_slice();
    const uint32_t slices = (uint32_t)((max_pts + slice - 1) / slice);
    for (size_t p0 = 0; p0 < n; p0 += kVerifyProblemsPerLaunch) {
        const int k = (int)std::min((size_t)kVerifyProblemsPerLaunch, n - p0);
        {
            ProfScope ps(c, K_VERIFY_MOVE, k);
            launch_verify_move(d_probs + p0, k, w, d_results, t, v, d_verify, c->stream);
        }
        ProfScope ps(c, K_VERIFY_COUNT, k);
        launch_verify_count(d_probs + p0, k, slices, w, t, v, prm, slice, d_verify, c->stream);
    }
}

/* the pair call on the context's stream, behind the entries' checks and begin_call: frame f = frames.n[f] records at
 * frames.off[f] of d_clouds */
int verify_pairs(bev_ctx *c, const bev_point_t *d_clouds, const bevsubreg::FrameTable &frames, int n_matches,
                 const bev_match_t *h_matches, const bev_icp_result_t *d_results, const bev_verify_params_t &prm,
                 bev_verify_result_t *d_verify)
{
    std::vector<int32_t> slot_of((size_t)frames.size(), -1);
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
    std::vector<VerifyProblem> probs((size_t)n_matches);
    for (int m = 0; m < n_matches; ++m) {
        VerifyProblem &pb = probs[(size_t)m];
        pb = VerifyProblem{};
        pb.src_slot = slot(h_matches[m].query_idx);
        pb.tgt_grid = slot(h_matches[m].match_idx);
        pb.result = (uint32_t)m;
    }
    for (VerifyProblem &pb : probs) pb.tgt_pt0 = (uint64_t)pb.tgt_grid * Pn;
    const int U = (int)slots.size();
    FineWork w;
    const FineSlot *d_slots = nullptr;
    BEVCK(fine_slots_setup(c, (size_t)U, Pn, slots, w, &d_slots));
    VerifyWork v;
    BEVCK(verify_work(c, probs.size(), Pn, v));
    const VerifyProblem *d_probs;
    BEVCK(verify_table(c, probs, &d_probs));
    BEVCK(fine_voxel(c, d_clouds, d_slots, U, w, prm.leaf));
    {
        ProfScope ps(c, K_FINE_GRID, U);
        launch_fine_grid(U, w, c->stream);
    }
    verify_launches(c, d_probs, probs.size(), w, VerifyTarget{w.hdr, w.cell_off, w.sorted}, v, Pn, prm, d_results, d_verify);
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

extern "C" {

bev_verify_params_t bev_verify_defaults(void)
{
    bev_verify_params_t p{};
    p.leaf = 0.2f;
    p.n_thresholds = 4;
    p.threshold[0] = 0.1f;
    p.threshold[1] = 0.2f;
    p.threshold[2] = 0.5f;
    p.threshold[3] = 1.0f;
    return p;
}

int bev_verify_clouds(bev_ctx_t *c, const bev_point_t *src, uint32_t n_src, const bev_point_t *tgt, uint32_t n_tgt,
                      const float *T16, const bev_verify_params_t *params, bev_verify_result_t *result)
{
    const bev_verify_params_t prm = params ? *params : bev_verify_defaults();
    if (!c || !result || !T16 || (n_src && !src) || (n_tgt && !tgt) || !verify_params_ok(prm)) return BEV_ERR_INVALID_ARG;
    BEVCK(begin_call(c, false));
    const size_t Pn = std::max<size_t>(std::max(n_src, n_tgt), 1);
    FineWork w;
    const FineSlot *d_slots = nullptr;
    BEVCK(fine_slots_setup(c, 2, Pn, std::vector<FineSlot>{}, w, &d_slots));
    VerifyWork v;
    BEVCK(verify_work(c, 1, Pn, v));
    std::vector<VerifyProblem> probs(1);
    probs[0] = VerifyProblem{};
    probs[0].src_slot = 0;
    probs[0].tgt_grid = 1;
    probs[0].tgt_pt0 = Pn;
    const VerifyProblem *d_probs;
    BEVCK(verify_table(c, probs, &d_probs));
    BEVCK(c->reg.verify_io.grow(c, sizeof(bev_icp_result_t) + sizeof(bev_verify_result_t)));
    bev_icp_result_t *d_res = static_cast<bev_icp_result_t *>(c->reg.verify_io.p);
    bev_verify_result_t *d_out = reinterpret_cast<bev_verify_result_t *>(d_res + 1);
    /* the clouds are the "voxel clouds" of the two slots, as bev_icp_point_to_point has them */
    const uint32_t counts[2] = {n_src, n_tgt};
    bev_icp_result_t r{};
    std::memcpy(r.T, T16, sizeof r.T);
    if (n_src) HIPCK(c, hipMemcpyAsync(w.vox, src, (size_t)n_src * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    if (n_tgt) HIPCK(c, hipMemcpyAsync(w.vox + Pn, tgt, (size_t)n_tgt * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(w.vox_n, counts, sizeof(counts), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(d_res, &r, sizeof r, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, K_FINE_GRID, 2);
        launch_fine_grid(2, w, c->stream);
    }
    verify_launches(c, d_probs, 1, w, VerifyTarget{w.hdr, w.cell_off, w.sorted}, v, Pn, prm, d_res, d_out);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipMemcpyAsync(result, d_out, sizeof(bev_verify_result_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

int bev_verify_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                            int n_matches, const bev_match_t *h_matches, const bev_icp_result_t *d_results,
                                            const bev_verify_params_t *params, bev_verify_result_t *d_verify)
{
    const bev_verify_params_t prm = params ? *params : bev_verify_defaults();
    if (!c || n_frames < 0 || n_matches < 0 || !verify_params_ok(prm) || !positive(prm.leaf)) return BEV_ERR_INVALID_ARG;
    bevsubreg::FrameTable frames;
    if (n_matches > 0) {
        if (!d_clouds || !h_matches || !d_results || !d_verify) return BEV_ERR_INVALID_ARG;
        if (!matches_in_range(h_matches, n_matches, n_frames, n_frames)) return BEV_ERR_INVALID_ARG;
        if (!frame_table(n_frames, h_offsets, (uint64_t)c->geo.S, frames)) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    BEVCK(verify_pairs(c, d_clouds, frames, n_matches, h_matches, d_results, prm, d_verify));
    return record_tail(c);
}

int bev_submap_verify_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds,
                                                   const uint64_t *h_offsets, int n_maps, const uint64_t *h_map_offsets,
                                                   const int32_t *h_entry_frame, const float *h_entry_pose, float map_leaf,
                                                   int n_matches, const bev_match_t *h_matches,
                                                   const bev_icp_result_t *d_results, const bev_verify_params_t *params,
                                                   bev_verify_result_t *d_verify)
{
    const bev_verify_params_t prm = params ? *params : bev_verify_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !verify_params_ok(prm) || !positive(prm.leaf) || !not_negative(map_leaf))
        return BEV_ERR_INVALID_ARG;
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches};
    if (n_matches > 0) {
        if (!h_matches || !d_results || !d_verify) return BEV_ERR_INVALID_ARG;
        if (!frame_table(n_frames, h_offsets, (uint64_t)c->geo.S, call.frames)) return BEV_ERR_INVALID_ARG;
        BEVCK(submap_reg_check(call));
        if (!d_clouds) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    /* the registration call's plan and targets under the default grids; a problem's target is its map's place in its group */
    Options opt;
    opt.union_voxel = map_leaf > 0.0f;
    const Plan plan = bevsubreg::plan_call(call, opt, group_cap(c));
    std::vector<VerifyProblem> probs(plan.probs.size());
    for (const Group &g : plan.groups)
        for (uint32_t i = g.prob0; i < g.prob0 + g.n_probs; ++i) {
            const bevsubreg::Problem &pp = plan.probs[i];
            VerifyProblem &pb = probs[i];
            pb = VerifyProblem{};
            pb.src_slot = pp.src_slot;
            pb.tgt_grid = pp.map - g.map0;
            pb.result = pp.result;
            pb.tgt_pt0 = plan.maps[pp.map].pt0;
        }
    SubmapFine s;
    c->submap_grid_rec[0] = GridRecord{}; /* the stage's workspace is laid out anew: bev_debug_get_submap_grid has nothing to read */
    BEVCK(submap_fine_begin(c, plan, opt, d_clouds, prm.leaf, s));
    VerifyWork v;
    BEVCK(verify_work(c, probs.size(), plan.Pn, v));
    const VerifyProblem *d_probs;
    BEVCK(verify_table(c, probs, &d_probs));
    for (const Group &g : plan.groups) { /* one behind the other: the stream's order hands the maps' arrays on */
        BEVCK(submap_fine_targets(c, g, opt, s, map_leaf));
        verify_launches(c, d_probs + g.prob0, g.n_probs, s.w, VerifyTarget{s.t.hdr, s.t.cell_off, s.t.sorted}, v,
                        std::max<uint64_t>(plan.Pn, g.max_cap), prm, d_results, d_verify);
    }
    HIPCK(c, hipGetLastError());
    return record_tail(c);
}

int bev_verify_registration_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                                  int n_matches, const bev_match_t *h_matches, const bev_icp_result_t *results,
                                  const bev_verify_params_t *params, bev_verify_result_t *verify)
{
    const bev_verify_params_t prm = params ? *params : bev_verify_defaults();
    if (!c || n_frames < 0 || n_matches < 0 || !verify_params_ok(prm) || !positive(prm.leaf)) return BEV_ERR_INVALID_ARG;
    if (!host_clouds_ok(n_frames, clouds, n_pts)) return BEV_ERR_INVALID_ARG;
    if (n_matches > 0) {
        if (!h_matches || !results || !verify) return BEV_ERR_INVALID_ARG;
        if (!matches_in_range(h_matches, n_matches, n_frames, n_frames)) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    std::vector<size_t> offs((size_t)std::max(n_frames, 1));
    BEVCK(fine_upload(c, clouds, n_pts, n_frames, offs.data()));
    bevsubreg::FrameTable frames;
    frames.off.assign(offs.begin(), offs.begin() + n_frames);
    frames.n.assign(n_pts, n_pts + n_frames);
    const size_t in_bytes = align256((size_t)n_matches * sizeof(bev_icp_result_t));
    BEVCK(c->reg.verify_io.grow(c, in_bytes + (size_t)n_matches * sizeof(bev_verify_result_t)));
    bev_icp_result_t *d_res = static_cast<bev_icp_result_t *>(c->reg.verify_io.p);
    bev_verify_result_t *d_out = reinterpret_cast<bev_verify_result_t *>(static_cast<char *>(c->reg.verify_io.p) + in_bytes);
    HIPCK(c, hipMemcpyAsync(d_res, results, (size_t)n_matches * sizeof(bev_icp_result_t), hipMemcpyHostToDevice, c->stream));
    BEVCK(verify_pairs(c, static_cast<const bev_point_t *>(c->reg.fine_in.p), frames, n_matches, h_matches, d_res, prm, d_out));
    HIPCK(c, hipMemcpyAsync(verify, d_out, (size_t)n_matches * sizeof(bev_verify_result_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

} /* extern "C" */
