/*
 * bev_capi_submap_reg.hip — the scan-to-map part of the extern "C" boundary declared in include/bev_mi355x.h: fine ICP of frames
 * against submaps, the voxel grid over a map's union in front of it (§6l), coarse ICP against them (§6m) and
 * against maps thinned over their union with recomputed normals (§6q), and against the top part over the union of a map's moved
 * full clouds, thinned the same way (§6r).
 * Host-side only: the kernels are in bev_kernels.hip, the plan of a call in bev_submap_reg_plan.h; bev_reg_host.h is shared with
 * bev_capi_reg.hip, the context (bev_ctx.h) with every file of the C ABI.  What is shared and what is not: DESIGN.md §6n, §6u.
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "bev_reg_host.h"

#include "bev_libm_f64.h"

using namespace bevk;
using namespace bevh;
using bevsubreg::Call, bevsubreg::Group, bevsubreg::Options, bevsubreg::Plan;

/* ---- what the verification calls run as well (bev_reg_host.h) ---- */
/* bytes of a launch group's maps (BEV_SUBMAP_REG_GROUP): 8 GiB, of the order of the voxel clouds of a call on a thousand sweeps,
 * and hundreds of maps of full sweeps in one launch (a map is one workgroup of k_submap_target, a match one of k_submap_icp) */
constexpr uint64_t kSubmapRegCap = (uint64_t)8 << 30;
uint64_t bevh::group_cap(const bev_ctx *c) { return c->submap_reg_group ? (uint64_t)c->submap_reg_group : kSubmapRegCap; }

/* what the fine entries check behind their own arguments: BEV_OK, or what the entry returns */
int bevh::submap_reg_check(const Call &call)
{
    const int n_frames = call.frames.size();
    BEVCK(check_submap_entries(n_frames, call.n_maps, call.map_offs, call.entry_frame, call.entry_pose));
    if (!matches_in_range(call.matches, call.n_matches, n_frames, call.n_maps)) return BEV_ERR_INVALID_ARG;
    for (int g = 0; g < call.n_maps; ++g)
        if (bevsubreg::map_capacity(call.frames.n.data(), call.map_offs, call.entry_frame, g) > BEV_SUBMAP_REG_MAX_TARGET)
            return BEV_ERR_TOO_LARGE;
    return BEV_OK;
}

namespace {

/* the plan's tables in one block of tab, the device's on return (PlanDev, bev_reg_host.h) */
int plan_up(bev_ctx *c, UploadTable &tab, const Plan &plan, const Options &opt, PlanDev &d, const void *probs = nullptr,
            size_t prob_bytes = 0)
{
    static_assert(sizeof(bevsubreg::Slot) == sizeof(FineSlot), "the plan's slots are k_fine_voxel's");
    const void *const src[] = {plan.slots.data(), plan.maps.data(), plan.entries.data(), probs, plan.map_key0.data(),
                               plan.map_u0.data(), plan.map_cell0.data()};
    const size_t sz[] = {opt.point_normal && !opt.top_union ? 0 : plan.slots.size() * sizeof(FineSlot),
                         plan.maps.size() * sizeof(bevsubreg::Map), plan.entries.size() * sizeof(bevsubreg::Entry), prob_bytes,
                         opt.union_voxel ? plan.maps.size() * 8 : 0, opt.top_union ? plan.maps.size() * 8 : 0,
                         opt.grid_cap ? plan.maps.size() * 8 : 0};
    void **const dst[] = {&d.slots, &d.maps, &d.entries, &d.probs, &d.key0, &d.u0, &d.cell0};
    BEVCK(table_up(c, tab, sz, src, dst));
    if (!sz[4]) d.key0 = nullptr;
    if (!sz[5]) d.u0 = nullptr;
    if (!sz[6]) d.cell0 = nullptr;
    return BEV_OK;
}

/* ---- search grids sized to the maps (bev_set_submap_search_grid; bev_submap_grid.h) ---- */

/* the pieces a wide grid adds to a stage's workspace, behind everything else (all 0 without one, so that the layout stands):
 * the counters, the parts' bounds, the tiles' sums */
struct GridPieces {
    size_t cnt, bounds, sums;
};
GridPieces grid_pieces(const Plan &plan, bool wide)
{
    const size_t C = std::max<size_t>((size_t)plan.max_group_cells, 1), M = std::max<size_t>(plan.max_group_maps, 1);
    return wide ? GridPieces{C * 4, M * kSubgridParts * sizeof(float4), M * kSubgridScanParts * 4} : GridPieces{0, 0, 0};
}

/* the search grids of a group's maps by several workgroups per map (search_grid_build, bev_reg_host.h): the maps' point counts
 * are vh's n_out, their points src's */
int submap_grid_build(bev_ctx *c, const Group &g, int cap, const void *d_maps, const SubvoxHdr *vh, const SubgridSource &src,
                      const SubmapGridWork &w)
{
    /* workgroups of 2048 points of the largest map, of 4096 cells of the largest grid */
    const uint32_t parts = (uint32_t)std::min<uint64_t>((g.max_cap + 8 * kIcpThreads - 1) / (8 * kIcpThreads), kSubgridParts);
    const uint32_t tiles = (uint32_t)((g.max_cells + bevsubreg::kGridScanTile - 1) / bevsubreg::kGridScanTile);
    return search_grid_build(c, d_maps, g.map0, (int)g.n_maps, parts, tiles, cap, vh, src, w, (size_t)g.cells);
}

/* what bev_debug_get_submap_grid reads of a stage's call: the grids of its last group, in the stage's workspace */
void submap_grid_record(bev_ctx *c, int coarse, const Plan &plan, int cap, const IcpGridHdr *hdr, const uint32_t *cell_off)
{
    const uint64_t fixed_cells = coarse ? kIcpCells : kFineCells;
    GridRecord &r = c->submap_grid_rec[coarse];
    r = GridRecord{};
    if (plan.groups.empty()) return;
    const Group &g = plan.groups.back();
    r.buf = stage_buf(c, coarse).p;
    r.hdr = hdr;
    r.cell_off = cell_off;
    for (uint32_t i = 0; i < g.n_maps; ++i)
        r.items.push_back({i, cap ? plan.map_cell0[g.map0 + i] : i * (fixed_cells + 1),
                           cap ? bevsubreg::grid_cells(plan.map_cap[g.map0 + i], cap) : fixed_cells});
}

/* the sort of a group's key arrays as bev_submap_vox_plan.h schedules it */
void submap_sort_keys(bev_ctx *c, const Group &g, const SubmapVoxWork &v)
{
    const uint32_t tiles = bevsubvox::tiles(g.max_slots);
    for (const bevsubvox::Stage &sg : bevsubvox::schedule(g.max_slots)) {
        ProfScope ps(c, sg.kind == bevsubvox::kStageGlobal ? K_SUBMAP_VOX_GLOBAL : K_SUBMAP_VOX_TILE, (int)g.n_maps);
        launch_submap_vox_stage(sg.kind, sg.k, sg.j, g.map0, (int)g.n_maps, tiles, v, c->stream);
    }
}

/* ---- the fine path: registration (§6k, §6l) and the cloud call (§6l) ---- */

/* A fine call's workspace in fine_buf, and its tables: the voxel clouds of the slots (no grids: no frame is a target), the scratch
 * of a voxel launch and of an ICP launch, the entries' first indices, the maps of one launch group.  Of the group's arrays, a call
 * with matches (icp: every one but the cloud call) has t.pts and the search grids t.sorted, t.hdr, t.cell_off; the union grid
 * (vox) has v.keys, v.vstart and thins into t.pts; who concatenates into an array of its own (vox, the cloud call): v.moved, v.vh
 * (SubmapFine: bev_reg_host.h) */
int submap_fine_work(bev_ctx *c, const Plan &plan, const Options &opt, SubmapFine &s)
{
    /* wide: the concatenation is k_submap_vox_move's (v.moved, v.vh) where the maps are not thinned, and t.pts points at it */
    const bool icp = !opt.all_maps, vox = opt.union_voxel, wide = opt.grid_cap > 0 && icp, staged = vox || !icp || wide;
    const GridPieces gp = grid_pieces(plan, wide);
    const size_t U = plan.slots.size(), P = plan.probs.size(), E = plan.entries.size(), Pn = plan.Pn, Kn = pow2_at_least(Pn);
    const size_t G = std::min(U, (size_t)kFineVoxelGroup), L = std::min(P, (size_t)kFineProblemsPerLaunch);
    const size_t T = std::max<size_t>((size_t)plan.max_group_pts, 1), M = std::max<size_t>(plan.max_group_maps, 1);
    const size_t sz[] = {U * Pn * sizeof(bev_point_t), U * 4, G * Kn * 8, G * (Pn + 1) * 4, L * Pn * 16, L * Pn * 4,
                         std::max<size_t>(E, 1) * 4, (icp && !wide) || vox ? T * 16 : 0, icp ? T * 16 : 0,
                         icp ? M * sizeof(IcpGridHdr) : 0, !icp ? 0 : wide ? gp.cnt : M * 4 * (size_t)(kFineCells + 1),
                         staged ? T * 16 : 0, vox ? std::max<size_t>((size_t)plan.max_group_keys, 1) * 8 : 0, vox ? (T + M) * 4 : 0,
                         staged ? M * sizeof(SubvoxHdr) : 0, gp.cnt, gp.bounds, gp.sums};
    void **const dst[] = {(void **)&s.w.vox, (void **)&s.w.vox_n, (void **)&s.w.keys, (void **)&s.w.vstart, (void **)&s.w.cur,
                          (void **)&s.w.corr, (void **)&s.ent_start, (void **)&s.t.pts, (void **)&s.t.sorted, (void **)&s.t.hdr,
                          (void **)&s.t.cell_off, (void **)&s.v.moved, (void **)&s.v.keys, (void **)&s.v.vstart, (void **)&s.v.vh,
                          (void **)&s.gw.cnt, (void **)&s.gw.part_bounds, (void **)&s.gw.part_sum};
    BEVCK(c->reg.fine_buf.grow(c, carve(nullptr, sz, dst)));
    carve(c->reg.fine_buf.p, sz, dst);
    if (!icp) s.t.sorted = nullptr, s.t.hdr = nullptr, s.t.cell_off = nullptr; /* k_submap_vox_finish builds no grid at nullptr */
    if (wide && !vox) s.t.pts = s.v.moved;
    s.gw.hdr = s.t.hdr;
    s.gw.off = s.t.cell_off;
    s.gw.sorted = s.t.sorted;
    s.w.Pn = Pn;
    s.w.Kn = Kn;
    return BEV_OK;
}

} // namespace

/* the workspace, the tables and the voxel clouds of the plan's slots: frame f = frames.n[f] records at frames.off[f] of d_clouds */
int bevh::submap_fine_begin(bev_ctx *c, const Plan &plan, const Options &opt, const bev_point_t *d_clouds, float leaf, SubmapFine &s,
                            const std::vector<FineProblem> &probs)
{
    BEVCK(submap_fine_work(c, plan, opt, s));
    BEVCK(plan_up(c, c->reg.fine_tab, plan, opt, s.d, probs.data(), probs.size() * sizeof(FineProblem)));
    s.v.key0 = static_cast<const uint64_t *>(s.d.key0);
    s.gw.cell0 = static_cast<const uint64_t *>(s.d.cell0);
    return fine_voxel(c, d_clouds, static_cast<const FineSlot *>(s.d.slots), (int)plan.slots.size(), s.w, leaf);
}

/* a group's targets in s.t.pts (the plain cloud call: in s.v.moved): the entries' voxel clouds moved and concatenated, with their
 * search grids where the call has matches; map_leaf > 0: thinned by the voxel grid over the union */
int bevh::submap_fine_targets(bev_ctx *c, const Group &g, const Options &opt, const SubmapFine &s, float map_leaf)
{
    const int gm = (int)g.n_maps;
    const PlanDev &d = s.d;
    const bool wide = opt.grid_cap > 0 && !opt.all_maps;
    const SubgridSource pts{s.t.pts, nullptr, nullptr};
    if (!opt.union_voxel && !opt.all_maps && !wide) {
        ProfScope ps(c, K_SUBMAP_TARGET, gm);
        launch_submap_target(d.maps, g.map0, gm, d.entries, s.w, s.ent_start, s.t, c->stream);
        return BEV_OK;
    }
    {
        ProfScope ps(c, K_SUBMAP_VOX_MOVE, gm);
        launch_submap_vox_move(d.maps, g.map0, gm, d.entries, s.w, s.ent_start, s.v, c->stream);
    }
    if (!opt.union_voxel) return wide ? submap_grid_build(c, g, opt.grid_cap, d.maps, s.v.vh, pts, s.gw) : BEV_OK;
    {
        ProfScope ps(c, K_SUBMAP_VOX_KEYS, gm);
        launch_submap_vox_keys(d.maps, g.map0, gm, s.v, map_leaf, c->stream);
    }
    submap_sort_keys(c, g, s.v);
    {
        SubmapRegWork t = s.t;
        if (wide) t.sorted = nullptr, t.hdr = nullptr, t.cell_off = nullptr; /* (no grid at nullptr) */
        ProfScope ps(c, K_SUBMAP_VOX_FINISH, gm);
        launch_submap_vox_finish(d.maps, g.map0, gm, s.v, t, c->stream);
    }
    return wide ? submap_grid_build(c, g, opt.grid_cap, d.maps, s.v.vh, pts, s.gw) : BEV_OK;
}

namespace {

/* the registration call on the context's stream, behind the entries' checks and begin_call.  map_leaf > 0: the maps are thinned
 * (DESIGN.md §6l); 0: §6k's launches and workspace */
int submap_reg_frames(bev_ctx *c, const bev_point_t *d_clouds, const Call &call, float leaf, float map_leaf,
                      const bev_icp_result_t *d_coarse, const int32_t *d_best, const bev_icp_params_t &prm,
                      bev_icp_result_t *d_results)
{
    Options opt;
    opt.union_voxel = map_leaf > 0.0f;
    opt.grid_cap = c->submap_grid_cap[0];
    const Plan plan = bevsubreg::plan_call(call, opt, group_cap(c));
    std::vector<FineProblem> probs(plan.probs.size());
    for (size_t i = 0; i < probs.size(); ++i) {
        const bevsubreg::Problem &pp = plan.probs[i];
        FineProblem &pb = probs[i];
        pb.src_slot = pp.src_slot;
        pb.tgt_slot = pp.map;
        pb.result = pp.result;
        pb.coarse_match = d_coarse ? pp.result : 0xffffffffu;
        bevx::icp_tool_guess(call.matches[pp.result].angle_guess, 0, pb.guess);
    }
    SubmapFine s;
    BEVCK(submap_fine_begin(c, plan, opt, d_clouds, leaf, s, probs));
    const FineProblem *d_probs = static_cast<const FineProblem *>(s.d.probs);
    for (const Group &g : plan.groups) { /* one behind the other: the stream's order hands the maps' arrays on */
        BEVCK(submap_fine_targets(c, g, opt, s, map_leaf));
        for (uint32_t p0 = 0; p0 < g.n_probs; p0 += kFineProblemsPerLaunch) {
            const int n = (int)std::min<uint32_t>(kFineProblemsPerLaunch, g.n_probs - p0);
            ProfScope ps(c, opt.grid_cap ? K_SUBMAP_ICP_WIDE : K_SUBMAP_ICP, n);
            if (opt.grid_cap)
                launch_submap_icp_wide(d_probs + g.prob0 + p0, n, s.d.maps, g.map0, s.w, s.t, s.gw.cell0, d_coarse, d_best, prm,
                                       d_results, c->stream);
            else
                launch_submap_icp(d_probs + g.prob0 + p0, n, s.d.maps, g.map0, s.w, s.t, d_coarse, d_best, prm, d_results, c->stream);
        }
    }
    submap_grid_record(c, 0, plan, opt.grid_cap, s.t.hdr, s.t.cell_off);
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

/* ---- the coarse path (§6m) and its thinned maps (§6q) ---- */

/* A coarse call's workspace in the coarse stage's buffer: the scratch of an ICP launch (icp: the registration calls), the
 * entries' first indices, the maps of one launch group: the target rows and their search grids (icp), and for maps thinned over
 * their union (vox) or written out (the cloud call) the moved rows, the sort's arrays, the voxel indices and positions */
struct SubmapCoarse {
    SubmapCoarseWork t{};
    SubmapPnVoxWork p{};
    uint32_t *ent_start = nullptr;
    PlanDev d{};
    int grid_cap = 0;    /* > 0: the wide grids, in place of k_submap_pn_target's and k_submap_pn_grid's */
    SubmapGridWork gw{}; /* ... (gw.off is t.cell_off, gw.hdr t.hdr, gw.sorted t.sorted) */
};
/* the target rows' searchable copies, headers and offsets are the wide grid's too */
void submap_coarse_grid_work(SubmapCoarse &s, const Options &opt, const PlanDev &d)
{
    s.grid_cap = opt.all_maps ? 0 : opt.grid_cap;
    s.gw.hdr = s.t.hdr;
    s.gw.off = s.t.cell_off;
    s.gw.sorted = s.t.sorted;
    s.gw.cell0 = static_cast<const uint64_t *>(d.cell0);
}
int submap_coarse_work(bev_ctx *c, const Plan &plan, const Options &opt, size_t stride, SubmapCoarse &s)
{
    /* wide: the concatenation is k_submap_pn_move's (p.moved, p.v.vh) where the maps are not thinned, and t.rows points at it */
    const bool icp = !opt.all_maps, vox = opt.union_voxel, wide = opt.grid_cap > 0 && icp, staged = vox || !icp || wide;
    const GridPieces gp = grid_pieces(plan, wide);
    const size_t L = icp ? std::min(2 * plan.probs.size(), (size_t)kIcpProblemsPerLaunch) : 0, E = plan.entries.size();
    const size_t T = std::max<size_t>((size_t)plan.max_group_pts, 1), M = std::max<size_t>(plan.max_group_maps, 1);
    s.t = SubmapCoarseWork{};
    s.p = SubmapPnVoxWork{};
    const size_t sz[] = {L * 16 * stride, std::max<size_t>(E, 1) * 4, (icp && !wide) || vox ? T * 48 : 0, icp ? T * 16 : 0,
                         icp ? M * sizeof(IcpGridHdr) : 0, !icp ? 0 : wide ? gp.cnt : M * 4 * (size_t)(kIcpCells + 1),
                         staged ? T * 48 : 0, vox ? std::max<size_t>((size_t)plan.max_group_keys, 1) * 8 : 0, vox ? (T + M) * 4 : 0,
                         vox ? T * 4 : 0, vox ? T * 16 : 0, staged ? M * sizeof(SubvoxHdr) : 0, gp.cnt, gp.bounds, gp.sums};
    void **const dst[] = {(void **)&s.t.cur, (void **)&s.ent_start, (void **)&s.t.rows, (void **)&s.t.sorted, (void **)&s.t.hdr,
                          (void **)&s.t.cell_off, (void **)&s.p.moved, (void **)&s.p.v.keys, (void **)&s.p.v.vstart,
                          (void **)&s.p.vidx, (void **)&s.p.vpos, (void **)&s.p.v.vh, (void **)&s.gw.cnt, (void **)&s.gw.part_bounds,
                          (void **)&s.gw.part_sum};
    BEVCK(c->reg.icp_buf.grow(c, carve(nullptr, sz, dst)));
    carve(c->reg.icp_buf.p, sz, dst);
    if (!icp) s.t.sorted = nullptr, s.t.hdr = nullptr, s.t.cell_off = nullptr, s.t.cur = nullptr;
    if (wide && !vox) s.t.rows = s.p.moved;
    return BEV_OK;
}

/* the coarse ICP of a group's problems (two per match), in launches of kIcpProblemsPerLaunch, against the grids the group has */
void submap_coarse_icp_launches(bev_ctx *c, const Group &g, const SubmapCoarse &s, const float *pn, size_t stride,
                                const uint32_t *d_counts, const IcpProblem *d_probs, const bev_icp_params_t &prm,
                                bev_icp_result_t *d_results)
{
    for (uint32_t p0 = 0; p0 < 2 * g.n_probs; p0 += kIcpProblemsPerLaunch) {
        const int n = (int)std::min<uint32_t>(kIcpProblemsPerLaunch, 2 * g.n_probs - p0);
        ProfScope ps(c, s.grid_cap ? K_SUBMAP_COARSE_ICP_WIDE : K_SUBMAP_COARSE_ICP, n);
        if (s.grid_cap)
            launch_submap_coarse_icp_wide(pn, stride, d_counts, d_probs + 2 * (size_t)g.prob0 + p0, n, s.d.maps, g.map0, s.t,
                                          s.gw.cell0, prm, d_results, c->stream);
        else
            launch_submap_coarse_icp(pn, stride, d_counts, d_probs + 2 * (size_t)g.prob0 + p0, n, s.d.maps, g.map0, s.t, prm,
                                     d_results, c->stream);
    }
}

/* what the coarse entries check behind their own arguments, with maps to build: BEV_OK, or what the entry returns */
int submap_coarse_check(int n_frames, const void *d_pn, size_t stride, const uint32_t *d_counts, int n_maps,
                        const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose)
{
    if (!d_pn || !d_counts || stride == 0) return BEV_ERR_INVALID_ARG;
    BEVCK(check_submap_entries(n_frames, n_maps, h_map_offsets, h_entry_frame, h_entry_pose));
    return BEV_OK;
}
/* a map's capacity is n_entries * stride rows: the true counts live on the device, and the host does not wait for them */
int submap_coarse_capacity(size_t stride, int n_maps, const uint64_t *h_map_offsets)
{
    for (int g = 0; g < n_maps; ++g) {
        const uint64_t ne = h_map_offsets[g + 1] - h_map_offsets[g];
        if (ne && (uint64_t)stride > BEV_SUBMAP_COARSE_MAX_TARGET / ne) return BEV_ERR_TOO_LARGE;
    }
    return BEV_OK;
}

/* §6k's plan with every frame counted at stride rows and a PointNormal map's bytes; the device reads an entry's FRAME */
Plan submap_coarse_plan(bev_ctx *c, Call &call, const Options &opt, int n_frames, size_t stride)
{
    call.frames.off.assign((size_t)n_frames, 0);
    call.frames.n.assign((size_t)n_frames, (uint64_t)stride);
    Plan plan = bevsubreg::plan_call(call, opt, group_cap(c));
    for (bevsubreg::Entry &en : plan.entries) en.slot = (uint32_t)plan.slot_frame[en.slot];
    return plan;
}

/* two problems per match, the guesses adjacent */
std::vector<IcpProblem> submap_coarse_problems(const Plan &plan, const bev_match_t *h_matches)
{
    std::vector<IcpProblem> probs;
    probs.reserve(2 * plan.probs.size());
    for (const bevsubreg::Problem &pp : plan.probs)
        for (int g = 0; g < 2; ++g) {
            IcpProblem pb{};
            pb.src_frame = (uint32_t)h_matches[pp.result].query_idx;
            pb.tgt_frame = 0xffffffffu; /* (not read: the target is a map) */
            pb.tgt_slot = pp.map;
            pb.result = 2 * pp.result + (uint32_t)g;
            bevx::icp_tool_guess(h_matches[pp.result].angle_guess, g, pb.guess);
            probs.push_back(pb);
        }
    return probs;
}

/* how the two coarse registration calls end: the hook's record, the better guess of every match, the tail */
int submap_coarse_end(bev_ctx *c, const Plan &plan, const SubmapCoarse &s, bev_icp_result_t *d_results, int n_matches,
                      int32_t *d_best)
{
    submap_grid_record(c, 1, plan, s.grid_cap, s.t.hdr, s.t.cell_off);
    {
        ProfScope ps(c, K_ICP_BEST, n_matches);
        launch_icp_best(d_results, n_matches, d_best, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return record_tail(c);
}

/* a group's targets out of s.p.moved (thinned: s.t.rows), as the two cloud calls write them */
void submap_pn_out(bev_ctx *c, const Group &g, const SubmapCoarse &s, bool vox, float *d_out, uint64_t out_stride,
                   uint32_t *d_counts_out)
{
    const uint32_t parts = (uint32_t)std::min<uint64_t>((3 * g.max_cap + 4 * kIcpThreads - 1) / (4 * kIcpThreads), 256);
    ProfScope ps(c, K_SUBMAP_PN_OUT, (int)g.n_maps);
    launch_submap_out(s.d.maps, g.map0, (int)g.n_maps, parts, s.p.v.vh, vox ? s.t.rows : s.p.moved, d_out, out_stride,
                      d_counts_out, 3, c->stream);
}

/* a group's entries' rows moved and concatenated into s.p.moved */
void submap_pn_move(bev_ctx *c, const Group &g, const SubmapCoarse &s, const float *pn, size_t stride, const uint32_t *d_counts)
{
    ProfScope ps(c, K_SUBMAP_PN_MOVE, (int)g.n_maps);
    launch_submap_pn_move(s.d.maps, g.map0, (int)g.n_maps, s.d.entries, pn, stride, d_counts, s.ent_start, s.p, c->stream);
}

/* the rows of a group's maps in s.p.moved thinned over their union into s.t.rows: keys, the sort, centroids,
 * (overflow: §6r's count of a top part cut short,) normals; the search grids, wide or fixed, where the call has matches */
int submap_pn_thin(bev_ctx *c, const Group &g, const SubmapCoarse &s, bool overflow, float pn_leaf, float radius, const float vp[2])
{
    const int gm = (int)g.n_maps;
    const PlanDev &d = s.d;
    {
        ProfScope ps(c, K_SUBMAP_PN_KEYS, gm);
        launch_submap_pn_keys(d.maps, g.map0, gm, s.p, pn_leaf, c->stream);
    }
    submap_sort_keys(c, g, s.p.v);
    {
        ProfScope ps(c, K_SUBMAP_PN_FINISH, gm);
        launch_submap_pn_finish(d.maps, g.map0, gm, s.p, s.t.rows, c->stream);
    }
    if (overflow) {
        ProfScope ps(c, K_SUBMAP_TOP_OVERFLOW, gm);
        launch_submap_top_overflow(d.maps, g.map0, gm, s.p, c->stream);
    }
    {
        ProfScope ps(c, K_SUBMAP_PN_NORMALS, gm);
        launch_submap_pn_normals(d.maps, g.map0, gm, (uint32_t)((g.max_cap + kIcpThreads - 1) / kIcpThreads), s.p, radius, pn_leaf, vp,
                                 s.t.rows, c->stream);
    }
    if (s.t.hdr && s.grid_cap)
        return submap_grid_build(c, g, s.grid_cap, d.maps, s.p.v.vh, SubgridSource{nullptr, nullptr, s.t.rows}, s.gw);
    if (s.t.hdr) {
        ProfScope ps(c, K_SUBMAP_PN_GRID, gm);
        launch_submap_pn_grid(d.maps, g.map0, gm, s.p.v.vh, s.t, c->stream);
    }
    return BEV_OK;
}

/* a group's targets thinned over their union (§6q) */
int submap_coarse_thin(bev_ctx *c, const Group &g, const SubmapCoarse &s, const float *pn, size_t stride, const uint32_t *d_counts,
                       float pn_leaf, float radius, const float vp[2])
{
    submap_pn_move(c, g, s, pn, stride, d_counts);
    return submap_pn_thin(c, g, s, false, pn_leaf, radius, vp);
}
/* ... as they are, under a wide grid: the concatenation is s.t.rows (submap_coarse_work) */
int submap_coarse_wide(bev_ctx *c, const Group &g, const SubmapCoarse &s, const float *pn, size_t stride, const uint32_t *d_counts)
{
    submap_pn_move(c, g, s, pn, stride, d_counts);
    return submap_grid_build(c, g, s.grid_cap, s.d.maps, s.p.v.vh, SubgridSource{nullptr, nullptr, s.t.rows}, s.gw);
}

/* ---- the top part over the union of a map's moved full clouds (§6r) ---- */

/* what the two entries check behind their own arguments, with maps to build: the frame table, the entries, the unions' sizes;
 * largest: the largest union of the call's maps */
int submap_top_check(bev_ctx *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets, Call &call, uint64_t *largest)
{
    if (!frame_table(n_frames, h_offsets, (uint64_t)c->geo.S, call.frames)) return BEV_ERR_INVALID_ARG;
    BEVCK(check_submap_entries(n_frames, call.n_maps, call.map_offs, call.entry_frame, call.entry_pose));
    *largest = 0;
    for (int g = 0; g < call.n_maps; ++g) {
        const uint64_t cap = bevsubreg::map_capacity(call.frames.n.data(), call.map_offs, call.entry_frame, g);
        if (cap > BEV_SUBMAP_TOP_MAX_UNION) return BEV_ERR_INVALID_ARG;
        *largest = std::max(*largest, cap);
    }
    return d_clouds ? BEV_OK : BEV_ERR_INVALID_ARG;
}

/* A call's workspace in the coarse stage's buffer: submap_coarse_work's pieces for thinned maps of top_max_out rows (icp: the
 * registration call's scratch and search grids), and the select's: a key per record of the group's unions, the cells' tables and
 * histograms (adjacent: one memset clears both) */
struct SubmapTop {
    SubmapCoarse s;
    SubmapTopWork t{};
    size_t cell_stride = 0; /* bytes from the cells' tables to the histograms */
};
int submap_top_work(bev_ctx *c, const Plan &plan, bool icp, int grid_cap, size_t stride, SubmapTop &w)
{
    SubmapCoarse &s = w.s;
    const size_t L = icp ? std::min(2 * plan.probs.size(), (size_t)kIcpProblemsPerLaunch) : 0;
    const size_t T = std::max<size_t>((size_t)plan.max_group_pts, 1), M = std::max<size_t>(plan.max_group_maps, 1);
    const size_t U = std::max<size_t>((size_t)plan.max_group_union, 1);
    const bool wide = grid_cap > 0 && icp;
    const GridPieces gp = grid_pieces(plan, wide);
    s.t = SubmapCoarseWork{};
    s.p = SubmapPnVoxWork{};
    const size_t sz[] = {L * 16 * stride, T * 48, icp ? T * 16 : 0, icp ? M * sizeof(IcpGridHdr) : 0,
                         !icp ? 0 : wide ? gp.cnt : M * 4 * (size_t)(kIcpCells + 1), T * 48,
                         std::max<size_t>((size_t)plan.max_group_keys, 1) * 8, (T + M) * 4, T * 4, T * 16, M * sizeof(SubvoxHdr), U * 8,
                         M * sizeof(SubtopCells), M * (size_t)kTopHistWords * 4, gp.cnt, gp.bounds, gp.sums};
    void **const dst[] = {(void **)&s.t.cur, (void **)&s.t.rows, (void **)&s.t.sorted, (void **)&s.t.hdr, (void **)&s.t.cell_off,
                          (void **)&s.p.moved, (void **)&s.p.v.keys, (void **)&s.p.v.vstart, (void **)&s.p.vidx, (void **)&s.p.vpos,
                          (void **)&s.p.v.vh, (void **)&w.t.ukeys, (void **)&w.t.cells, (void **)&w.t.hist, (void **)&s.gw.cnt,
                          (void **)&s.gw.part_bounds, (void **)&s.gw.part_sum};
    BEVCK(c->reg.icp_buf.grow(c, carve(nullptr, sz, dst)));
    carve(c->reg.icp_buf.p, sz, dst);
    if (!icp) s.t.sorted = nullptr, s.t.hdr = nullptr, s.t.cell_off = nullptr, s.t.cur = nullptr;
    w.cell_stride = align256(M * sizeof(SubtopCells));
    return BEV_OK;
}

/* a group's targets: the keys of the unions, the select, the sorted selection, the rows of top(g) in s.p.moved;
 * pn_leaf > 0: thinned with their normals into s.t.rows as §6q thins a concatenation, the search grids where the call has matches */
int submap_top_targets(bev_ctx *c, const Group &g, const SubmapTop &w, const bev_point_t *d_clouds, float pn_leaf,
                       float radius, const float vp[2])
{
    const int gm = (int)g.n_maps;
    const SubmapCoarse &s = w.s;
    const PlanDev &d = s.d;
    /* workgroups of 4096 records of the largest union, of 256 rows of the largest top part */
    const uint32_t parts = (uint32_t)std::min<uint64_t>((g.max_union + 16 * kIcpThreads - 1) / (16 * kIcpThreads), 512);
    const uint32_t row_parts = (uint32_t)std::min<uint64_t>((g.max_cap + kIcpThreads - 1) / kIcpThreads, 1024);
    HIPCK(c, hipMemsetAsync(w.t.cells, 0, w.cell_stride + (size_t)gm * kTopHistWords * 4, c->stream));
    {
        ProfScope ps(c, K_SUBMAP_TOP_KEYS, gm);
        launch_submap_top_keys(d.maps, g.map0, gm, parts, d.entries, d.slots, d_clouds, w.t, c->stream);
    }
    {
        ProfScope ps(c, K_SUBMAP_TOP_CELLS, gm);
        launch_submap_top_cells(gm, w.t, s.p.v.vh, c->stream);
    }
    for (int shift = (int)((kTopKeyBits - 1) / kTopDigitBits * kTopDigitBits); shift >= 0; shift -= (int)kTopDigitBits) {
        {
            ProfScope ps(c, K_SUBMAP_TOP_HIST, gm);
            launch_submap_top_digit(d.maps, g.map0, gm, parts, d.entries, w.t, (uint32_t)shift, false, c->stream);
        }
        ProfScope ps(c, K_SUBMAP_TOP_SCAN, gm);
        launch_submap_top_digit(d.maps, g.map0, gm, parts, d.entries, w.t, (uint32_t)shift, true, c->stream);
    }
    {
        ProfScope ps(c, K_SUBMAP_TOP_COMPACT, gm);
        launch_submap_top_compact(d.maps, g.map0, gm, parts, d.entries, w.t, s.p.v, c->stream);
    }
    submap_sort_keys(c, g, s.p.v);
    {
        ProfScope ps(c, K_SUBMAP_TOP_ROWS, gm);
        launch_submap_top_rows(d.maps, g.map0, gm, row_parts, d.entries, d.slots, d_clouds, w.t, s.p, c->stream);
    }
    return pn_leaf > 0.0f ? submap_pn_thin(c, g, s, true, pn_leaf, radius, vp) : BEV_OK;
}

} // namespace

extern "C" {

/* ---- scan-to-map fine ICP: frames against submaps (bev_submap_reg_plan.h, bev_submap_reg.h) ------- */
int bev_submap_voxel_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds,
                                                  const uint64_t *h_offsets, float leaf, float map_leaf, int n_maps,
                                                  const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                                  const float *h_entry_pose, int n_matches, const bev_match_t *h_matches,
                                                  const bev_icp_result_t *d_coarse, const int32_t *d_best,
                                                  const bev_icp_params_t *params, bev_icp_result_t *d_results)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_fine_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm) || !positive(leaf) || !not_negative(map_leaf) ||
        (d_coarse == nullptr) != (d_best == nullptr))
        return BEV_ERR_INVALID_ARG;
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches};
    if (n_matches > 0) {
        if (!h_matches || !d_results) return BEV_ERR_INVALID_ARG;
        if (!frame_table(n_frames, h_offsets, (uint64_t)c->geo.S, call.frames)) return BEV_ERR_INVALID_ARG;
        BEVCK(submap_reg_check(call));
        if (!d_clouds) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    BEVCK(submap_reg_frames(c, d_clouds, call, leaf, map_leaf, d_coarse, d_best, prm, d_results));
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
    if (!c || n_frames < 0 || n_maps < 0 || !positive(leaf) || !not_negative(map_leaf)) return BEV_ERR_INVALID_ARG;
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, 0, nullptr};
    if (n_maps > 0) {
        if (!d_out || !d_counts) return BEV_ERR_INVALID_ARG;
        if (!frame_table(n_frames, h_offsets, (uint64_t)c->geo.S, call.frames)) return BEV_ERR_INVALID_ARG;
        BEVCK(submap_reg_check(call));
        for (int g = 0; g < n_maps; ++g)
            if (bevsubreg::map_capacity(call.frames.n.data(), h_map_offsets, h_entry_frame, g) > out_stride)
                return BEV_ERR_INVALID_ARG;
        if (!d_clouds) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_maps == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    /* no matches and no ICP: every map's target, built as the registration call builds it, goes out */
    Options opt;
    opt.union_voxel = map_leaf > 0.0f;
    opt.all_maps = true;
    const Plan plan = bevsubreg::plan_call(call, opt, group_cap(c));
    SubmapFine s;
    BEVCK(submap_fine_begin(c, plan, opt, d_clouds, leaf, s));
    for (const Group &g : plan.groups) {
        BEVCK(submap_fine_targets(c, g, opt, s, map_leaf));
        const uint32_t parts = (uint32_t)std::min<uint64_t>((g.max_cap + 4 * kFineThreads - 1) / (4 * kFineThreads), 256);
        ProfScope ps(c, K_SUBMAP_VOX_OUT, (int)g.n_maps);
        launch_submap_out(s.d.maps, g.map0, (int)g.n_maps, parts, s.v.vh, opt.union_voxel ? s.t.pts : s.v.moved, d_out,
                          out_stride, d_counts, 1, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return record_tail(c);
}

int bev_submap_voxel_registration_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                                        float leaf, float map_leaf, int n_maps, const uint64_t *h_map_offsets,
                                        const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                        const bev_match_t *h_matches, const bev_icp_params_t *params, bev_icp_result_t *results)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_fine_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm) || !positive(leaf) || !not_negative(map_leaf))
        return BEV_ERR_INVALID_ARG;
    if (n_frames > 0 && (!clouds || !n_pts)) return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (n_pts[f] && !clouds[f]) return BEV_ERR_INVALID_ARG;
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches};
    if (n_matches > 0) {
        if (!h_matches || !results) return BEV_ERR_INVALID_ARG;
        call.frames.n.assign(n_pts, n_pts + n_frames);
        BEVCK(submap_reg_check(call));
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    std::vector<size_t> offs((size_t)std::max(n_frames, 1));
    BEVCK(fine_upload(c, clouds, n_pts, n_frames, offs.data()));
    call.frames.off.assign(offs.begin(), offs.begin() + n_frames);
    BEVCK(c->reg.sub_res.grow(c, (size_t)n_matches * sizeof(bev_icp_result_t)));
    bev_icp_result_t *d_res = static_cast<bev_icp_result_t *>(c->reg.sub_res.p);
    BEVCK(submap_reg_frames(c, static_cast<const bev_point_t *>(c->reg.fine_in.p), call, leaf, map_leaf, nullptr, nullptr, prm, d_res));
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

/* ---- scan-to-map coarse ICP: PointNormal frames against submaps (bev_submap_coarse.h), and against submaps
 * thinned over their union with their normals recomputed (bev_submap_pn_vox.h) ---------------------------- */
int bev_submap_coarse_voxel_registration_device_resident(bev_ctx_t *c, int n_frames, const void *d_pn, size_t stride,
                                                         const uint32_t *d_counts, float pn_leaf, float radius,
                                                         const float *viewpoint, int n_maps, const uint64_t *h_map_offsets,
                                                         const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                         const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                         bev_icp_result_t *d_results, int32_t *d_best)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_coarse_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm) || !not_negative(pn_leaf)) return BEV_ERR_INVALID_ARG;
    const bool vox = pn_leaf > 0.0f;
    if (vox && !positive(radius)) return BEV_ERR_INVALID_ARG;
    if (n_matches > 0) {
        if (!h_matches || !d_results || !d_best) return BEV_ERR_INVALID_ARG;
        BEVCK(submap_coarse_check(n_frames, d_pn, stride, d_counts, n_maps, h_map_offsets, h_entry_frame, h_entry_pose));
        if (!matches_in_range(h_matches, n_matches, n_frames, n_maps)) return BEV_ERR_INVALID_ARG;
        BEVCK(submap_coarse_capacity(stride, n_maps, h_map_offsets));
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches};
    Options opt;
    opt.point_normal = true;
    opt.union_voxel = vox;
    opt.grid_cap = c->submap_grid_cap[1];
    const Plan plan = submap_coarse_plan(c, call, opt, n_frames, stride);
    SubmapCoarse s;
    BEVCK(submap_coarse_work(c, plan, opt, stride, s));
    const std::vector<IcpProblem> probs = submap_coarse_problems(plan, h_matches);
    BEVCK(plan_up(c, c->reg.icp_tab, plan, opt, s.d, probs.data(), probs.size() * sizeof(IcpProblem)));
    s.p.v.key0 = static_cast<const uint64_t *>(s.d.key0);
    submap_coarse_grid_work(s, opt, s.d);
    const float vp[2] = {viewpoint && vox ? viewpoint[0] : 0.0f, viewpoint && vox ? viewpoint[1] : 0.0f};
    const float *pn = static_cast<const float *>(d_pn);
    const IcpProblem *d_probs = static_cast<const IcpProblem *>(s.d.probs);
    for (const Group &g : plan.groups) {
        if (vox) {
            BEVCK(submap_coarse_thin(c, g, s, pn, stride, d_counts, pn_leaf, radius, vp));
        } else if (s.grid_cap) {
            BEVCK(submap_coarse_wide(c, g, s, pn, stride, d_counts));
        } else {
            ProfScope ps(c, K_SUBMAP_PN_TARGET, (int)g.n_maps);
            launch_submap_pn_target(s.d.maps, g.map0, (int)g.n_maps, s.d.entries, pn, stride, d_counts, s.ent_start, s.t, c->stream);
        }
        submap_coarse_icp_launches(c, g, s, pn, stride, d_counts, d_probs, prm, d_results);
    }
    return submap_coarse_end(c, plan, s, d_results, n_matches, d_best);
}

int bev_submap_coarse_registration_device_resident(bev_ctx_t *c, int n_frames, const void *d_pn, size_t stride,
                                                   const uint32_t *d_counts, int n_maps, const uint64_t *h_map_offsets,
                                                   const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                   const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                   bev_icp_result_t *d_results, int32_t *d_best)
{
    return bev_submap_coarse_voxel_registration_device_resident(c, n_frames, d_pn, stride, d_counts, 0.0f, 0.0f, nullptr, n_maps,
                                                                h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches,
                                                                params, d_results, d_best);
}

int bev_submap_pn_cloud_device_resident(bev_ctx_t *c, int n_frames, const void *d_pn, size_t stride, const uint32_t *d_counts,
                                        float pn_leaf, float radius, const float *viewpoint, int n_maps,
                                        const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                                        uint64_t out_stride, float *d_out, uint32_t *d_counts_out)
{
    if (!c || n_frames < 0 || n_maps < 0 || !not_negative(pn_leaf)) return BEV_ERR_INVALID_ARG;
    const bool vox = pn_leaf > 0.0f;
    if (vox && !positive(radius)) return BEV_ERR_INVALID_ARG;
    if (n_maps > 0) {
        if (!d_out || !d_counts_out) return BEV_ERR_INVALID_ARG;
        BEVCK(submap_coarse_check(n_frames, d_pn, stride, d_counts, n_maps, h_map_offsets, h_entry_frame, h_entry_pose));
        BEVCK(submap_coarse_capacity(stride, n_maps, h_map_offsets));
        for (int g = 0; g < n_maps; ++g)
            if ((h_map_offsets[g + 1] - h_map_offsets[g]) * (uint64_t)stride > out_stride) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_maps == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    /* no matches and no ICP: every map's target, built as the registration call builds it, goes out */
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, 0, nullptr};
    Options opt;
    opt.point_normal = true;
    opt.union_voxel = vox;
    opt.all_maps = true;
    const Plan plan = submap_coarse_plan(c, call, opt, n_frames, stride);
    SubmapCoarse s;
    BEVCK(submap_coarse_work(c, plan, opt, stride, s));
    BEVCK(plan_up(c, c->reg.icp_tab, plan, opt, s.d));
    s.p.v.key0 = static_cast<const uint64_t *>(s.d.key0);
    const float vp[2] = {viewpoint && vox ? viewpoint[0] : 0.0f, viewpoint && vox ? viewpoint[1] : 0.0f};
    const float *pn = static_cast<const float *>(d_pn);
    for (const Group &g : plan.groups) {
        if (vox) BEVCK(submap_coarse_thin(c, g, s, pn, stride, d_counts, pn_leaf, radius, vp));
        else submap_pn_move(c, g, s, pn, stride, d_counts);
        submap_pn_out(c, g, s, vox, d_out, out_stride, d_counts_out);
    }
    HIPCK(c, hipGetLastError());
    return record_tail(c);
}

/* ---- the top part over the union of a map's moved full clouds, thinned, as the coarse stage's target (bev_submap_top.h;
 * DESIGN.md §6r) ---------------------------------------------------------------------------------------------------------- */
size_t bev_submap_top_part_max_out(size_t union_records) { return (size_t)bevsubreg::top_max_out(union_records); }

int bev_submap_top_part_cloud_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                              float pn_leaf, float radius, const float *viewpoint, int n_maps,
                                              const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                              const float *h_entry_pose, uint64_t out_stride, float *d_out, uint32_t *d_counts_out)
{
    if (!c || n_frames < 0 || n_maps < 0 || !not_negative(pn_leaf)) return BEV_ERR_INVALID_ARG;
    const bool vox = pn_leaf > 0.0f;
    if (vox && !positive(radius)) return BEV_ERR_INVALID_ARG;
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, 0, nullptr};
    if (n_maps > 0) {
        if (!d_out || !d_counts_out) return BEV_ERR_INVALID_ARG;
        uint64_t largest = 0;
        BEVCK(submap_top_check(c, n_frames, d_clouds, h_offsets, call, &largest));
        if (out_stride < bevsubreg::top_max_out(largest)) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_maps == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    Options opt;
    opt.point_normal = opt.union_voxel = opt.top_union = opt.all_maps = true;
    const Plan plan = bevsubreg::plan_call(call, opt, group_cap(c));
    SubmapTop w;
    BEVCK(submap_top_work(c, plan, false, 0, 0, w));
    BEVCK(plan_up(c, c->reg.icp_tab, plan, opt, w.s.d));
    w.s.p.v.key0 = static_cast<const uint64_t *>(w.s.d.key0);
    w.t.u0 = static_cast<const uint64_t *>(w.s.d.u0);
    const float vp[2] = {viewpoint && vox ? viewpoint[0] : 0.0f, viewpoint && vox ? viewpoint[1] : 0.0f};
    for (const Group &g : plan.groups) {
        BEVCK(submap_top_targets(c, g, w, d_clouds, pn_leaf, radius, vp));
        submap_pn_out(c, g, w.s, vox, d_out, out_stride, d_counts_out);
    }
    HIPCK(c, hipGetLastError());
    return record_tail(c);
}

int bev_submap_top_part_coarse_registration_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds,
                                                            const uint64_t *h_offsets, const void *d_pn, size_t stride,
                                                            const uint32_t *d_counts, float pn_leaf, float radius,
                                                            const float *viewpoint, int n_maps, const uint64_t *h_map_offsets,
                                                            const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                            const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                            bev_icp_result_t *d_results, int32_t *d_best)
{
    const bev_icp_params_t prm = params ? *params : bev_icp_coarse_defaults();
    if (!c || n_frames < 0 || n_maps < 0 || n_matches < 0 || !icp_params_ok(prm) || !positive(pn_leaf) || !positive(radius))
        return BEV_ERR_INVALID_ARG;
    Call call{{}, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, n_matches, h_matches};
    if (n_matches > 0) {
        if (!h_matches || !d_results || !d_best || !d_pn || !d_counts || stride == 0) return BEV_ERR_INVALID_ARG;
        uint64_t largest = 0;
        BEVCK(submap_top_check(c, n_frames, d_clouds, h_offsets, call, &largest));
        if (!matches_in_range(h_matches, n_matches, n_frames, n_maps)) return BEV_ERR_INVALID_ARG;
    }
    BEVCK(begin_call(c, false));
    if (n_matches == 0) return BEV_OK;
    BEVCK(wait_default_stream(c));
    Options opt;
    opt.point_normal = opt.union_voxel = opt.top_union = true;
    opt.grid_cap = c->submap_grid_cap[1];
    const Plan plan = bevsubreg::plan_call(call, opt, group_cap(c));
    SubmapTop w;
    BEVCK(submap_top_work(c, plan, true, opt.grid_cap, stride, w));
    const std::vector<IcpProblem> probs = submap_coarse_problems(plan, h_matches);
    BEVCK(plan_up(c, c->reg.icp_tab, plan, opt, w.s.d, probs.data(), probs.size() * sizeof(IcpProblem)));
    w.s.p.v.key0 = static_cast<const uint64_t *>(w.s.d.key0);
    w.t.u0 = static_cast<const uint64_t *>(w.s.d.u0);
    submap_coarse_grid_work(w.s, opt, w.s.d);
    const float vp[2] = {viewpoint ? viewpoint[0] : 0.0f, viewpoint ? viewpoint[1] : 0.0f};
    const float *pn = static_cast<const float *>(d_pn);
    const IcpProblem *d_probs = static_cast<const IcpProblem *>(w.s.d.probs);
    for (const Group &g : plan.groups) {
        BEVCK(submap_top_targets(c, g, w, d_clouds, pn_leaf, radius, vp));
        submap_coarse_icp_launches(c, g, w.s, pn, stride, d_counts, d_probs, prm, d_results);
    }
    return submap_coarse_end(c, plan, w.s, d_results, n_matches, d_best);
}

/* ---- search grids sized to the maps (bev_submap_grid.h) ---------------------------------------------------- */
int bev_set_submap_search_grid(bev_ctx_t *c, int fine_dim, int coarse_dim)
{
    static_assert(BEV_SUBMAP_SEARCH_GRID_MAX == bevsubreg::kGridCapMax, "one cap");
    if (!c || fine_dim < 0 || fine_dim > BEV_SUBMAP_SEARCH_GRID_MAX || coarse_dim < 0 || coarse_dim > BEV_SUBMAP_SEARCH_GRID_MAX)
        return BEV_ERR_INVALID_ARG;
    c->submap_grid_cap[0] = fine_dim;
    c->submap_grid_cap[1] = coarse_dim;
    return BEV_OK;
}

int bev_debug_get_submap_grid(bev_ctx_t *c, int coarse, int first_map, int n_maps, uint32_t *out)
{
    if (!c || (coarse != 0 && coarse != 1) || first_map < 0 || n_maps < 0 || !out) return BEV_ERR_INVALID_ARG;
    const GridRecord &r = c->submap_grid_rec[coarse];
    if (!r.hdr || (size_t)first_map + (size_t)n_maps > r.items.size()) return BEV_ERR_INVALID_ARG;
    if (r.buf != stage_buf(c, coarse).p) return BEV_ERR_INVALID_ARG; /* a later call has moved the workspace */
    return grid_record_read(c, r, first_map, n_maps, out);
}

} /* extern "C" */
