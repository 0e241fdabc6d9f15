/*
 * bev_reg_host.h — what the registration files of the C ABI share over bev_ctx.h: bev_capi_reg.hip (the front end and the
 * pair stages), bev_capi_submap_reg.hip (scan-to-map) and bev_capi_verify.hip (verification of their results,
 * which runs their voxel, grid and target steps as they are; §6aa).  Argument checks, the frame table of a packed or
 * d_ordered buffer, upload tables laid out by carve, the host driver of a search grid's build and the reader of the two grid
 * hooks (§6u), and the fine stage's two steps that scan-to-map runs as they are.
 * Declarations and short inline functions, no state (RegState: bev_ctx.h).  Private.
 */
#ifndef BEV_REG_HOST_H
#define BEV_REG_HOST_H

#include <cmath>
#include <cstring>
#include <vector>

#include "bev_ctx.h"
#include "bev_submap_reg_plan.h"

namespace bevh {

/* a step that returns a status: anything but BEV_OK is what the caller returns */
#define BEVCK(expr)                    \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ != BEV_OK) return rc_; \
    } while (0)

constexpr size_t kRegTabMin = (size_t)1 << 16; /* smallest problem / slot table */

/* ---- argument checks ---- */
inline bool positive(float v) { return std::isfinite(v) && v > 0.0f; }      /* a leaf, a radius */
inline bool not_negative(float v) { return std::isfinite(v) && v >= 0.0f; } /* map_leaf: 0 is "no second grid" */
inline bool icp_params_ok(const bev_icp_params_t &p)
{
    return p.max_iterations >= 1 && p.max_iterations <= 1000 && std::isfinite(p.max_correspondence_distance) &&
           p.max_correspondence_distance > 0.0;
}
/* every query_idx inside the n_queries frames, every match_idx inside the n_targets frames or maps */
inline bool matches_in_range(const bev_match_t *h_matches, int n_matches, int n_queries, int n_targets)
{
    for (int m = 0; m < n_matches; ++m) {
        const bev_match_t &mt = h_matches[m];
        if (mt.query_idx < 0 || mt.query_idx >= n_queries || mt.match_idx < 0 || mt.match_idx >= n_targets) return false;
    }
    return true;
}
/* the n_frames frames of a packed buffer (h_offsets) or of d_ordered (NULL: S records each); false for decreasing offsets or
 * a frame above 2^32 - 1 records */
inline bool frame_table(int n_frames, const uint64_t *h_offsets, uint64_t S, bevsubreg::FrameTable &ft)
{
    ft.off.resize((size_t)n_frames);
    ft.n.resize((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        if (h_offsets && (h_offsets[f + 1] < h_offsets[f] || h_offsets[f + 1] - h_offsets[f] > 0xffffffffull)) return false;
        ft.off[(size_t)f] = h_offsets ? h_offsets[f] : (uint64_t)f * S;
        ft.n[(size_t)f] = h_offsets ? h_offsets[f + 1] - h_offsets[f] : S;
    }
    return true;
}

inline size_t pow2_at_least(size_t n)
{
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

/* ---- an upload table in carve's pieces: piece i is sz[i] bytes from src[i]; the block goes up the context's stream, and dst
 * points at the device's copies ---- */
template <size_t N>
int table_up(bev_ctx *c, UploadTable &t, const size_t (&sz)[N], const void *const (&src)[N], void **const (&dst)[N])
{
    void *h;
    const size_t total = carve(nullptr, sz, dst);
    BEVCK(t.begin(c, total, kRegTabMin, &h));
    carve(h, sz, dst);
    for (size_t i = 0; i < N; ++i)
        if (sz[i]) std::memcpy(*dst[i], src[i], sz[i]);
    BEVCK(t.push(c, total));
    carve(t.dev, sz, dst);
    return BEV_OK;
}

/* ---- search grids sized to the target (bev_submap_grid.h; defined in bev_capi_reg.hip) ---- */
/* the workspace of a stage: 0 fine, 1 coarse, as the hooks count */
inline DevBuf &stage_buf(bev_ctx *c, int coarse) { return coarse ? c->reg.icp_buf : c->reg.fine_buf; }
/* the grids of the n targets from t0 on of the table d_maps, on the context's stream: clear_words counters at w.cnt zeroed, then
 * the build's six steps.  parts, tiles: the caller's launch grids over the largest target's points and cells */
int search_grid_build(bev_ctx *c, const void *d_maps, uint32_t t0, int n, uint32_t parts, uint32_t tiles, int cap, const SubvoxHdr *vh,
                      const SubgridSource &src, const SubmapGridWork &w, size_t clear_words);
/* what both hooks do behind their own argument and staleness checks: the stream waited for, {nx, ny, n, largest cell} of items
 * first .. first + n - 1 into out; BEV_ERR_INVALID_ARG for an item whose header is not a grid that fits its offsets */
int grid_record_read(bev_ctx *c, const GridRecord &r, int first, int n, uint32_t *out);

/* ---- of the fine stage (bev_capi_reg.hip) ---- */
/* the voxel clouds of U slots, in launches of kFineVoxelGroup, on the context's stream */
int fine_voxel(bev_ctx *c, const bev_point_t *d_pts, const FineSlot *d_slots, int U, const FineWork &w, float leaf);
/* host records -> c->reg.fine_in (grown on demand); offs[i]: where cloud i went */
int fine_upload(bev_ctx *c, const bev_point_t *const *clouds, const uint32_t *n, int k, size_t *offs);
/* the fine stage's workspace for U slots of at most Pn records and no problem, under the default grids (fine_setup without an
 * ICP launch's scratch); the slot table goes up the context's stream.  What the verification calls voxelise and search in */
int fine_slots_setup(bev_ctx *c, size_t U, size_t Pn, const std::vector<FineSlot> &slots, FineWork &w, const FineSlot **d_slots);

/* ---- of the scan-to-map fine path (bev_capi_submap_reg.hip) ---- */
/* bytes of a launch group's maps (BEV_SUBMAP_REG_GROUP) */
uint64_t group_cap(const bev_ctx *c);
/* what the fine entries check behind their own arguments: BEV_OK, or what the entry returns */
int submap_reg_check(const bevsubreg::Call &call);
/* the plan's tables in one block of tab, the device's on return: the slots (fine, top_union), the maps, the entries (64-byte
 * aligned), the caller's problems if it has any, the maps' first keys (union_voxel; else nullptr), their first union keys
 * (top_union; else nullptr), their first cells (grid_cap > 0; else nullptr) */
struct PlanDev {
    void *slots, *maps, *entries, *probs, *key0, *u0, *cell0;
};
/* a fine call's workspace in fine_buf and its tables (submap_fine_work, bev_capi_submap_reg.hip) */
struct SubmapFine {
    FineWork w{};
    SubmapRegWork t{};
    SubmapVoxWork v{};
    uint32_t *ent_start = nullptr;
    PlanDev d{};
    SubmapGridWork gw{}; /* grid_cap > 0: the wide grids (gw.off is t.cell_off, gw.hdr t.hdr, gw.sorted t.sorted) */
};
/* the workspace, the tables and the voxel clouds of the plan's slots: frame f = frames.n[f] records at frames.off[f] of d_clouds */
int submap_fine_begin(bev_ctx *c, const bevsubreg::Plan &plan, const bevsubreg::Options &opt, const bev_point_t *d_clouds, float leaf,
                      SubmapFine &s, const std::vector<FineProblem> &probs = {});
/* a group's targets in s.t.pts with their search grids where the call has matches; map_leaf > 0: thinned over the union */
int submap_fine_targets(bev_ctx *c, const bevsubreg::Group &g, const bevsubreg::Options &opt, const SubmapFine &s, float map_leaf);

} // namespace bevh
#endif
