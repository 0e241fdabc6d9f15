/*
 * bev_capi_packed.hip — the batched calls over packed frames (several clouds one after the other in one buffer, described by
 * n_frames + 1 offsets) of the boundary declared extern "C" in include/bev_mi355x.h: projection of raw sweeps, float BEV,
 * posed BEVs, submap BEVs, float submap BEVs (DESIGN.md §6e – §6j).  Host-side only.  They share one path (§6h): the frame table
 * (upload_packed_table over bevsub::frame_table), the bracket of the device-resident calls (resident_call, bev_ctx.h), the chunk
 * loop of the host-buffer calls (packed_host_chunks) and the planes of a launch group (plane_pair_bytes, expand_planes).  What
 * the calls over maps share with place retrieval and the translation guess is bev_packed_host.h's: the prologue of a
 * device-resident call (resident_maps_call), the tables on their way up (TablesUp) and the loops of the host-buffer calls.
 */
#include "bev_packed_host.h"
#include "bev_libm.h"

using namespace bevh; /* (and through it bevk) */

namespace {

/* The frame table of a call over packed frames (packed_place, bev_dev.h) and, behind it in the same block, the call's poses,
 * as the host filled them and where they are on the device. */
struct PackedTable {
    ProjFrame *host = nullptr;
    const ProjFrame *dev = nullptr;
    const float *d_poses = nullptr; /* 12 floats per frame and pose, behind the table */
    size_t bytes = 0;
    uint32_t blocks = 0; /* workgroups of kProjBlock points of a launch over all frames: host[nf].blk0 */
    uint32_t n_max = 0;  /* the longest frame */
};
/* Fills t's host block (UploadTable::begin): per frame f = [offs[f], offs[f + 1]) (offsets checked by the caller) its offset,
 * its count and the workgroups before it, entry nf closing the table; then the nf * n_poses matrices at h_poses.
 * BEV_ERR_TOO_LARGE for a grid that one launch cannot have (2^41 points in one call). */
int fill_packed_table(bev_ctx *c, UploadTable &t, size_t min_cap, int nf, const uint64_t *offs, int n_poses, const float *h_poses,
                      PackedTable *pt)
{
    const size_t tab_bytes = ((size_t)nf + 1) * sizeof(ProjFrame), pose_bytes = (size_t)nf * n_poses * 12 * sizeof(float);
    char *h = nullptr;
    const int rc = t.begin(c, tab_bytes + pose_bytes, min_cap, reinterpret_cast<void **>(&h));
    if (rc != BEV_OK) return rc;
    ProjFrame *tab = reinterpret_cast<ProjFrame *>(h);
    uint32_t b = 0, m = 0;
    if (!bevsub::frame_table(reinterpret_cast<bevsub::Frame *>(tab), nf, offs, &m, &b)) return BEV_ERR_TOO_LARGE;
    if (pose_bytes) memcpy(h + tab_bytes, h_poses, pose_bytes);
    const char *d = static_cast<const char *>(t.dev); /* (begin alone sets dev; push only copies into it) */
    *pt = PackedTable{tab, reinterpret_cast<const ProjFrame *>(d), reinterpret_cast<const float *>(d + tab_bytes),
                      tab_bytes + pose_bytes, b, m};
    return BEV_OK;
}
/* ... and sends it up the context's stream.  Each call has an UploadTable of its own: a shared one would make a call wait for
 * another call's upload event. */
int upload_packed_table(bev_ctx *c, UploadTable &t, size_t min_cap, int nf, const uint64_t *offs, int n_poses,
                        const float *h_poses, PackedTable *pt)
{
    const int rc = fill_packed_table(c, t, min_cap, nf, offs, n_poses, h_poses, pt);
    return rc != BEV_OK ? rc : t.push(c, pt->bytes);
}

bool poses_ok(int n_poses, const float *h_poses, int max_poses)
{
    return n_poses >= 0 && n_poses <= max_poses && (n_poses == 0 || h_poses);
}

/* The host route of a batched call over packed frames (after begin_call with the staging): packed_chunks' chunks
 * (bev_packed_host.h), body queueing the downloads of a chunk's results, and the one synchronisation that ends the call. */
template <class Body>
int packed_host_chunks(bev_ctx *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, Body body)
{
    return end_host_call(c, packed_chunks(c, n_frames, clouds, n_pts, body));
}

/* The float BEV of nf frames on the context's stream: frame f = records [offs[f], offs[f + 1]) of d_clouds (offsets checked by
 * the caller), its pose k the 12 floats at h_poses + (f * n_poses + k) * 12; nf * max(1, n_poses) grids of M * M floats at
 * d_out, zeroed here.  ONE launch; the frame table and the matrices go up in one block. */
int float_bev_frames(bev_ctx *c, int nf, const bev_point_t *d_clouds, const uint64_t *offs, float interval, size_t M,
                     bool skip_label0, int n_poses, const float *h_poses, float *d_out)
{
    if (nf == 0) return BEV_OK;
    PackedTable pt;
    const int rc = upload_packed_table(c, c->manip_tab, 64 * 1024, nf, offs, n_poses, h_poses, &pt);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemsetAsync(d_out, 0, (size_t)nf * std::max(1, n_poses) * M * M * sizeof(float), c->stream));
    {
        ProfScope ps(c, K_FLOAT_BEV_BATCH, nf);
        launch_float_bev_batch(d_clouds, pt.dev, nf, pt.blocks, pt.d_poses, n_poses, interval, (int)M, skip_label0, d_out,
                               c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

constexpr size_t kPosedWsCap = (size_t)256 << 20; /* (see posed_bev_frames) */
/* a grid's plane pair, the cap of a launch group in grids (maps take the planes of the posed call) */
size_t plane_pair_bytes(const bev_ctx *c)
{
    const size_t M = (size_t)c->geo.rp.mat_size;
    return 2 * M * M * sizeof(uint32_t);
}
size_t posed_cap_grids(const bev_ctx *c)
{
    return c->posed_group > 0 ? (size_t)c->posed_group : std::max<size_t>(1, kPosedWsCap / plane_pair_bytes(c));
}
/* a launch group's n_grids splatted grids expanded into images first ... of d_multi / d_single (nullptr: not wanted); frames: for the profile */
void expand_planes(bev_ctx *c, const uint32_t *planes, size_t n_grids, size_t first, uint8_t *d_multi, uint8_t *d_single, int frames)
{
    ProfScope ps(c, K_POSED_EXPAND, frames);
    launch_posed_expand(c->geo, planes, (int)n_grids, d_multi ? d_multi + first * c->multi_bytes : nullptr,
                        d_single ? d_single + first * c->single_bytes : nullptr, c->stream);
}

/* The 24-layer and uint8 BEVs of nf frames on the context's stream: frames and poses as for float_bev_frames;
 * nf * max(1, n_poses) images at d_multi and at d_single (nullptr: not wanted).  The table and the matrices go up once; the
 * frames go in launch groups of consecutive whole frames whose grids fit the workspace cap: the group's planes are zeroed,
 * k_posed_splat fills them, k_posed_expand turns them into the images, and stream order hands the workspace from group to
 * group.  256 MiB is the size of the memory-side cache and bounds the workspace; it is not a tuned figure: in one run per
 * setting, not alternated, one group per call was 3-5 % faster at 0 and 1 poses and 10 % at 8, and groups of 64 grids were a
 * third slower (profiles/posed_bev_groups.txt). */
int posed_bev_frames(bev_ctx *c, int nf, const bev_point_t *d_clouds, const uint64_t *offs, int n_poses, const float *h_poses,
                     uint8_t *d_multi, uint8_t *d_single)
{
    if (nf == 0) return BEV_OK;
    PackedTable pt;
    int rc = fill_packed_table(c, c->posed_tab, 64 * 1024, nf, offs, n_poses, h_poses, &pt);
    if (rc != BEV_OK) return rc;
    const size_t K = (size_t)std::max(1, n_poses);
    const int per_group = (int)std::min<size_t>((size_t)nf, std::max<size_t>(1, posed_cap_grids(c) / K)); /* (every frame has K grids) */
    rc = c->posed_ws.grow(c, (size_t)per_group * K * plane_pair_bytes(c)); /* (a grow waits for the stream: before the table goes up) */
    if (rc != BEV_OK) return rc;
    rc = c->posed_tab.push(c, pt.bytes);
    if (rc != BEV_OK) return rc;
    uint32_t *planes = static_cast<uint32_t *>(c->posed_ws.p);
    for (int f0 = 0; f0 < nf; f0 += per_group) {
        const int g = std::min(per_group, nf - f0);
        const size_t grids = (size_t)g * K;
        HIPCK(c, hipMemsetAsync(planes, 0, grids * plane_pair_bytes(c), c->stream));
        {
            ProfScope ps(c, K_POSED_SPLAT, g);
            launch_posed_splat(d_clouds, pt.dev + f0, g, pt.host[f0 + g].blk0 - pt.host[f0].blk0,
                               pt.d_poses + (size_t)f0 * n_poses * 12, n_poses, c->geo, planes, c->stream);
        }
        expand_planes(c, planes, grids, (size_t)f0 * K, d_multi, d_single, g);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

/* ---- submaps: windows of posed frames rastered into one grid per map (bev_submap_plan.h, bev_submap.h) ---- */
/* the planes of a plan's largest group in posed_ws */
int submap_planes(bev_ctx *c, const bevsub::Plan &plan, uint32_t **planes)
{
    int most = 0;
    for (const bevsub::Group &g : plan.groups) most = std::max(most, g.n_maps);
    const int rc = c->posed_ws.grow(c, (size_t)most * plane_pair_bytes(c));
    *planes = static_cast<uint32_t *>(c->posed_ws.p);
    return rc;
}
/* group gi of an uploaded plan on the context's stream: its rows [r0, r0 + nr) splatted from d_clouds (left out where they hold no point) */
void submap_splat(bev_ctx *c, const TablesUp &u, size_t gi, const bev_point_t *d_clouds, int r0, int nr, uint32_t *planes)
{
    const TablesUp::Slice s = u.slice(gi, r0, nr);
    if (s.blocks == 0) return;
    ProfScope ps(c, K_SUBMAP_SPLAT, nr);
    launch_submap_splat(d_clouds, s.rows, s.ent0, nr, s.blocks, s.entries, c->geo, planes, c->stream);
}

/* The images of n_maps maps over nf frames in device memory, on the context's stream (arguments checked by the caller) */
int submap_bev_frames(bev_ctx *c, const bev_point_t *d_clouds, const uint64_t *offs, int n_maps, const uint64_t *map_offs,
                      const int32_t *entry_frame, const float *entry_pose, uint8_t *d_multi, uint8_t *d_single)
{
    TablesUp u;
    if (!bevsub::plan_maps(u.plan, offs, map_offs, 0, n_maps, entry_frame, entry_pose, posed_cap_grids(c))) return BEV_ERR_TOO_LARGE;
    uint32_t *planes = nullptr;
    int rc = submap_planes(c, u.plan, &planes); /* (a grow waits for the stream: before the tables go up) */
    if (rc != BEV_OK) return rc;
    rc = u.up(c, c->submap_tab);
    if (rc != BEV_OK) return rc;
    for (size_t gi = 0; gi < u.plan.groups.size(); ++gi) {
        const bevsub::Group &g = u.plan.groups[gi];
        HIPCK(c, hipMemsetAsync(planes, 0, (size_t)g.n_maps * plane_pair_bytes(c), c->stream));
        submap_splat(c, u, gi, d_clouds, 0, g.n_rows, planes);
        expand_planes(c, planes, (size_t)g.n_maps, (size_t)g.map0, d_multi, d_single, g.n_maps);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

/* ---- the float max-height BEV of submaps (bev_submap_float.h): ONE launch group, the output its accumulator ---- */
struct FloatGrid {
    float interval;
    size_t M;
    bool skip_label0;
};
/* the rows [r0, r0 + nr) of an uploaded plan's one group splatted from d_clouds into grids (left out where they hold no point) */
void submap_float_splat(bev_ctx *c, const TablesUp &u, const bev_point_t *d_clouds, int r0, int nr, const FloatGrid &fg,
                        float *grids)
{
    const TablesUp::Slice s = u.slice(0, r0, nr);
    if (s.blocks == 0) return;
    ProfScope ps(c, K_SUBMAP_FLOAT_SPLAT, nr);
    launch_submap_float_splat(d_clouds, s.rows, s.ent0, nr, s.blocks, s.entries, fg.interval, (int)fg.M, fg.skip_label0, grids,
                              c->stream);
}
/* The grids of n_maps > 0 maps over frames in device memory, on the context's stream (arguments checked by the caller): map g's
 * grid at d_out + g * M * M, zeroed here */
int submap_float_frames(bev_ctx *c, const bev_point_t *d_clouds, const uint64_t *offs, const FloatGrid &fg, int n_maps,
                        const uint64_t *map_offs, const int32_t *entry_frame, const float *entry_pose, float *d_out)
{
    TablesUp u;
    if (!bevsub::plan_maps(u.plan, offs, map_offs, 0, n_maps, entry_frame, entry_pose, (size_t)n_maps)) return BEV_ERR_TOO_LARGE;
    const int rc = u.up(c, c->submap_tab);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemsetAsync(d_out, 0, (size_t)n_maps * fg.M * fg.M * sizeof(float), c->stream));
    submap_float_splat(c, u, d_clouds, 0, u.plan.groups[0].n_rows, fg, d_out);
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

/* What the submap entry points (and those of bev_capi_submap_reg.hip) check of the maps: BEV_OK, or what the entry point returns.
 * The entry arrays are read only when their length has passed. */
int bevh::check_submap_entries(int n_frames, int n_maps, const uint64_t *map_offs, const int32_t *entry_frame,
                               const float *entry_pose)
{
    if (n_maps < 0 || !map_offs) return BEV_ERR_INVALID_ARG;
    for (int g = 0; g < n_maps; ++g)
        if (map_offs[g + 1] < map_offs[g]) return BEV_ERR_INVALID_ARG;
    const uint64_t n_entries = map_offs[n_maps] - map_offs[0];
    if (n_entries > BEV_SUBMAP_MAX_ENTRIES) return BEV_ERR_TOO_LARGE;
    if (n_entries && (!entry_frame || !entry_pose)) return BEV_ERR_INVALID_ARG;
    for (uint64_t e = map_offs[0]; e < map_offs[n_maps]; ++e)
        if (entry_frame[e] < 0 || entry_frame[e] >= n_frames) return BEV_ERR_INVALID_ARG;
    return BEV_OK;
}

/* The projection of nf frames on the context's stream: frame f = returns [offs[f], offs[f + 1]) of d_xyzi (offsets checked by
 * the caller).  Kinds 0 / 1: ONE launch, records at the same offsets of d_out.  KITTI: launch groups of kitti_group frames
 * over one workspace (stream order hands it from group to group), frame f's structured cloud at d_out + f * 64 * 2083. */
int bevh::project_frames(bev_ctx *c, int kind, int nf, const float *d_xyzi, const uint64_t *offs, bev_point_t *d_out)
{
    if (nf == 0) return BEV_OK;
    PackedTable pt;
    int rc = upload_packed_table(c, c->proj_tab, 1024 * sizeof(ProjFrame), nf, offs, 0, nullptr, &pt);
    if (rc != BEV_OK) return rc;
    if (kind != BEV_PROJECT_KITTI_HDL_64E) {
        ProfScope ps(c, K_PROJECT, nf);
        launch_project_batch(kind, d_xyzi, pt.dev, nf, pt.blocks, d_out, c->stream);
    } else {
        c->layout_hint = BEV_LAYOUT_STRUCTURED; /* what this writes are structured clouds (bev_set_layout_hint) */
        const size_t S = (size_t)bevx::kKittiRows * bevx::kKittiCols, G = (size_t)std::min(c->kitti_group, nf);
        KittiWork w{};
        w.n_cap = pt.n_max;
        w.blocks_cap = (pt.n_max + bevx::kKittiBlock - 1u) / bevx::kKittiBlock;
        const size_t sz[] = {G * sizeof(KittiHeader), G * w.n_cap * 4, G * w.blocks_cap * 4,
                             G * w.blocks_cap * bevx::kKittiListCap * 4, G * S * 4};
        void **const dst[] = {(void **)&w.hdr, (void **)&w.col, (void **)&w.cnt, (void **)&w.pos, (void **)&w.winner};
        rc = c->kitti_ws.grow(c, carve(nullptr, sz, dst));
        if (rc != BEV_OK) return rc;
        carve(c->kitti_ws.p, sz, dst);
        for (int f0 = 0; f0 < nf; f0 += (int)G) {
            const int g = std::min((int)G, nf - f0);
            HIPCK(c, hipMemsetAsync(w.winner, 0, (size_t)g * S * sizeof(uint32_t), c->stream));
            for (int step = 0; step < 4; ++step) {
                ProfScope ps(c, K_KITTI_CROSSINGS + step, g);
                launch_project_kitti(step, d_xyzi, pt.dev + f0, g, pt.n_max, w, d_out + (size_t)f0 * S, c->stream);
            }
        }
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

/* ---- the entry points (C linkage: their declarations in include/bev_mi355x.h) ---- */
size_t bev_project_out_points(int kind, uint32_t n)
{
    switch (kind) {
    case BEV_PROJECT_MULRAN_OS1_64:
    case BEV_PROJECT_OXFORD_HDL_32E: return n;
    case BEV_PROJECT_KITTI_HDL_64E: return (size_t)bevx::kKittiRows * bevx::kKittiCols;
    default: return 0;
    }
}

int bev_project_xyzi(bev_ctx_t *c, int kind, const float *xyzi, uint32_t n, bev_point_t *out)
{
    const size_t n_out = bev_project_out_points(kind, n);
    if (!c || (n && !xyzi) || (n_out && !out)) return BEV_ERR_INVALID_ARG;
    if (!project_kind_ok(kind)) return BEV_ERR_INVALID_ARG;
    if ((size_t)n > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_out == 0) return BEV_OK;
    int rc = begin_call(c, true);
    if (rc != BEV_OK) return rc;
    /* raw floats are staged in the ordered-cloud staging buffer (16 B per point fit its 32 B per slot) */
    float *d_raw = reinterpret_cast<float *>(c->st_ordered);
    if ((size_t)n * 16 > (size_t)c->max_batch * c->geo.S * sizeof(bev_point_t)) return BEV_ERR_TOO_LARGE;
    if (n_out > c->st_in_elems) return BEV_ERR_TOO_LARGE;
    if (n) HIPCK(c, hipMemcpyAsync(d_raw, xyzi, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    const uint64_t offs[2] = {0, n}; /* one frame of the batched code (n = 0, KITTI: the all-zero structured cloud) */
    rc = project_frames(c, kind, 1, d_raw, offs, c->st_in);
    if (rc != BEV_OK) return rc;
    HIPCK(c, hipMemcpyAsync(out, c->st_in, n_out * sizeof(bev_point_t), hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return BEV_OK;
}

size_t bev_project_batch_out_points(int kind, int n_frames, const uint64_t *h_offsets)
{
    if (!project_kind_ok(kind) || n_frames < 0 || !h_offsets) return 0;
    for (int f = 0; f < n_frames; ++f)
        if (h_offsets[f + 1] < h_offsets[f]) return 0;
    if (kind == BEV_PROJECT_KITTI_HDL_64E) return (size_t)n_frames * bevx::kKittiRows * bevx::kKittiCols;
    return (size_t)h_offsets[n_frames]; /* records sit at their returns' offsets */
}

int bev_project_device_resident(bev_ctx_t *c, int kind, int n_frames, const float *d_xyzi, const uint64_t *h_offsets,
                                bev_point_t *d_out)
{
    if (!project_kind_ok(kind)) return BEV_ERR_INVALID_ARG;
    const int rc = check_packed_frames(c, n_frames, h_offsets);
    if (rc != BEV_OK) return rc;
    if (n_frames == 0) return BEV_OK;
    const bool any_in = h_offsets[n_frames] != h_offsets[0], any_out = any_in || kind == BEV_PROJECT_KITTI_HDL_64E;
    if ((any_in && !d_xyzi) || (any_out && !d_out)) return BEV_ERR_INVALID_ARG;
    return resident_call(c, [&] { return project_frames(c, kind, n_frames, d_xyzi, h_offsets, d_out); });
}

int bev_float_bev_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                  float interval, int skip_label0, int n_poses, const float *h_poses, float *d_out)
{
    if (!poses_ok(n_poses, h_poses, BEV_FLOAT_BEV_MAX_POSES)) return BEV_ERR_INVALID_ARG;
    const int rc = check_packed_frames(c, n_frames, h_offsets);
    if (rc == BEV_ERR_INVALID_ARG) return rc;
    const size_t M = bev_float_bev_size(interval);
    if (M == 0) return BEV_ERR_UNSUPPORTED;
    if (rc != BEV_OK) return rc; /* (a frame that is too large: behind the interval) */
    if (n_frames == 0) return BEV_OK;
    if (!d_out || (!d_clouds && h_offsets[n_frames] != h_offsets[0])) return BEV_ERR_INVALID_ARG;
    return resident_call(c, [&] {
        return float_bev_frames(c, n_frames, d_clouds, h_offsets, interval, M, skip_label0 != 0, n_poses, h_poses, d_out);
    });
}

int bev_float_bev_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, float interval,
                        int skip_label0, int n_poses, const float *h_poses, float *const *out)
{
    if (!c || n_frames < 0 || !host_clouds_ok(n_frames, clouds, n_pts) || (n_frames > 0 && !out) ||
        !poses_ok(n_poses, h_poses, BEV_FLOAT_BEV_MAX_POSES))
        return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (!out[f]) return BEV_ERR_INVALID_ARG;
    const size_t M = bev_float_bev_size(interval);
    if (M == 0) return BEV_ERR_UNSUPPORTED;
    for (int f = 0; f < n_frames; ++f)
        if ((size_t)n_pts[f] > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_frames == 0) return BEV_OK;
    int rc = begin_call(c, true);
    if (rc != BEV_OK) return rc;
    const size_t per_frame = (size_t)std::max(1, n_poses) * M * M;
    rc = c->manip_grids.grow(c, (size_t)std::min(n_frames, c->max_batch) * per_frame * sizeof(float));
    if (rc != BEV_OK) return rc;
    float *grids = static_cast<float *>(c->manip_grids.p);
    return packed_host_chunks(c, n_frames, clouds, n_pts, [&](int f0, int nb, const uint64_t *off) -> int {
        const int rc_ = float_bev_frames(c, nb, c->st_in, off, interval, M, skip_label0 != 0, n_poses,
                                         n_poses ? h_poses + (size_t)f0 * n_poses * 12 : nullptr, grids);
        if (rc_ != BEV_OK) return rc_;
        for (int f = 0; f < nb; ++f)
            HIPCK(c, hipMemcpyAsync(out[f0 + f], grids + (size_t)f * per_frame, per_frame * sizeof(float), hipMemcpyDeviceToHost,
                                    c->stream));
        return BEV_OK;
    });
}

int bev_posed_bev_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                  int n_poses, const float *h_poses, uint8_t *d_multi, uint8_t *d_single)
{
    if (!poses_ok(n_poses, h_poses, BEV_POSED_BEV_MAX_POSES)) return BEV_ERR_INVALID_ARG;
    const int rc = check_packed_frames(c, n_frames, h_offsets);
    if (rc != BEV_OK) return rc;
    if (n_frames == 0) return BEV_OK;
    if ((!d_multi && !d_single) || (!d_clouds && h_offsets[n_frames] != h_offsets[0])) return BEV_ERR_INVALID_ARG;
    return resident_call(c, [&] { return posed_bev_frames(c, n_frames, d_clouds, h_offsets, n_poses, h_poses, d_multi, d_single); });
}

int bev_posed_bev_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, int n_poses,
                        const float *h_poses, uint8_t *const *multi_out, uint8_t *const *single_out)
{
    if (!c || n_frames < 0 || !host_clouds_ok(n_frames, clouds, n_pts) || (n_frames > 0 && !multi_out && !single_out) ||
        !poses_ok(n_poses, h_poses, BEV_POSED_BEV_MAX_POSES))
        return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if ((multi_out && !multi_out[f]) || (single_out && !single_out[f])) return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if ((size_t)n_pts[f] > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_frames == 0) return BEV_OK;
    int rc = begin_call(c, true);
    if (rc != BEV_OK) return rc;
    const size_t K = (size_t)std::max(1, n_poses), multi_frame = multi_out ? K * c->multi_bytes : 0,
                 single_frame = single_out ? K * c->single_bytes : 0, nb_max = (size_t)std::min(n_frames, c->max_batch);
    rc = c->posed_imgs.grow(c, nb_max * (multi_frame + single_frame));
    if (rc != BEV_OK) return rc;
    uint8_t *d_multi = multi_out ? static_cast<uint8_t *>(c->posed_imgs.p) : nullptr;
    uint8_t *d_single = single_out ? static_cast<uint8_t *>(c->posed_imgs.p) + nb_max * multi_frame : nullptr;
    return packed_host_chunks(c, n_frames, clouds, n_pts, [&](int f0, int nb, const uint64_t *off) -> int {
        const int rc_ = posed_bev_frames(c, nb, c->st_in, off, n_poses, n_poses ? h_poses + (size_t)f0 * n_poses * 12 : nullptr,
                                         d_multi, d_single);
        if (rc_ != BEV_OK) return rc_;
        for (int f = 0; f < nb; ++f) {
            if (multi_out)
                HIPCK(c, hipMemcpyAsync(multi_out[f0 + f], d_multi + (size_t)f * multi_frame, multi_frame, hipMemcpyDeviceToHost,
                                        c->stream));
            if (single_out)
                HIPCK(c, hipMemcpyAsync(single_out[f0 + f], d_single + (size_t)f * single_frame, single_frame,
                                        hipMemcpyDeviceToHost, c->stream));
        }
        return BEV_OK;
    });
}

int bev_submap_bev_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets, int n_maps,
                                   const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                                   uint8_t *d_multi, uint8_t *d_single)
{
    const FramesAndMaps a{n_frames, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose};
    return resident_maps_call(c, a, false, BEV_OK, d_multi || d_single, [&] {
        return submap_bev_frames(c, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, d_multi, d_single);
    });
}

/* host_map_chunks' chunks and pieces (bev_packed_host.h): a chunk's pieces are splatted into its planes, which are then
 * expanded into the chunk's images. */
int bev_submap_bev_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, int n_maps,
                         const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                         uint8_t *const *multi_out, uint8_t *const *single_out)
{
    if (!c || n_frames < 0 || !host_clouds_ok(n_frames, clouds, n_pts)) return BEV_ERR_INVALID_ARG;
    int rc = check_submap_entries(n_frames, n_maps, h_map_offsets, h_entry_frame, h_entry_pose);
    if (rc != BEV_OK) return rc;
    if (n_maps > 0 && !multi_out && !single_out) return BEV_ERR_INVALID_ARG;
    for (int g = 0; g < n_maps; ++g)
        if ((multi_out && !multi_out[g]) || (single_out && !single_out[g])) return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if ((size_t)n_pts[f] > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_maps == 0) return BEV_OK;
    rc = begin_call(c, true);
    if (rc != BEV_OK) return rc;
    const int chunk = (int)std::min<size_t>((size_t)std::min(n_maps, c->max_batch), posed_cap_grids(c));
    const size_t multi_map = multi_out ? c->multi_bytes : 0, single_map = single_out ? c->single_bytes : 0;
    rc = c->posed_imgs.grow(c, (size_t)chunk * (multi_map + single_map));
    if (rc != BEV_OK) return rc;
    uint8_t *d_multi = multi_out ? static_cast<uint8_t *>(c->posed_imgs.p) : nullptr;
    uint8_t *d_single = single_out ? static_cast<uint8_t *>(c->posed_imgs.p) + (size_t)chunk * multi_map : nullptr;
    rc = c->posed_ws.grow(c, (size_t)chunk * plane_pair_bytes(c));
    if (rc != BEV_OK) return rc;
    uint32_t *planes = static_cast<uint32_t *>(c->posed_ws.p);
    const HostMaps a{n_frames, clouds, n_pts, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, &c->submap_tab};
    return end_host_call(c, host_map_chunks(
        c, a, chunk,
        [&](int, int nm) -> int {
            HIPCK(c, hipMemsetAsync(planes, 0, (size_t)nm * plane_pair_bytes(c), c->stream));
            return BEV_OK;
        },
        [&](const TablesUp &u, int r0, int nr) { submap_splat(c, u, 0, c->st_in, r0, nr, planes); },
        [&](int m0, int nm) -> int {
            expand_planes(c, planes, (size_t)nm, 0, d_multi, d_single, nm);
            HIPCK(c, hipGetLastError());
            for (int m = 0; m < nm; ++m) {
                if (multi_out)
                    HIPCK(c, hipMemcpyAsync(multi_out[m0 + m], d_multi + (size_t)m * multi_map, multi_map, hipMemcpyDeviceToHost,
                                            c->stream));
                if (single_out)
                    HIPCK(c, hipMemcpyAsync(single_out[m0 + m], d_single + (size_t)m * single_map, single_map,
                                            hipMemcpyDeviceToHost, c->stream));
            }
            return BEV_OK;
        }));
}

int bev_submap_float_bev_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                         float interval, int skip_label0, int n_maps, const uint64_t *h_map_offsets,
                                         const int32_t *h_entry_frame, const float *h_entry_pose, float *d_out)
{
    const FloatGrid fg{interval, bev_float_bev_size(interval), skip_label0 != 0};
    const FramesAndMaps a{n_frames, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose};
    /* (a frame that is too large: behind the arguments that are wrong and the interval) */
    return resident_maps_call(c, a, false, fg.M == 0 ? BEV_ERR_UNSUPPORTED : BEV_OK, d_out != nullptr, [&] {
        return submap_float_frames(c, d_clouds, h_offsets, fg, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, d_out);
    });
}

/* host_map_chunks' chunks and pieces; the chunk's grids in the float-grid buffer of bev_float_bev_batch. */
int bev_submap_float_bev_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, float interval,
                               int skip_label0, int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                               const float *h_entry_pose, float *const *out)
{
    if (!c || n_frames < 0 || !host_clouds_ok(n_frames, clouds, n_pts)) return BEV_ERR_INVALID_ARG;
    int rc = check_submap_entries(n_frames, n_maps, h_map_offsets, h_entry_frame, h_entry_pose);
    if (rc != BEV_OK) return rc;
    if (n_maps > 0 && !out) return BEV_ERR_INVALID_ARG;
    for (int g = 0; g < n_maps; ++g)
        if (!out[g]) return BEV_ERR_INVALID_ARG;
    const FloatGrid fg{interval, bev_float_bev_size(interval), skip_label0 != 0};
    if (fg.M == 0) return BEV_ERR_UNSUPPORTED;
    for (int f = 0; f < n_frames; ++f)
        if ((size_t)n_pts[f] > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_maps == 0) return BEV_OK;
    rc = begin_call(c, true);
    if (rc != BEV_OK) return rc;
    const int chunk = std::min(n_maps, c->max_batch);
    const size_t per_map = fg.M * fg.M;
    rc = c->manip_grids.grow(c, (size_t)chunk * per_map * sizeof(float));
    if (rc != BEV_OK) return rc;
    float *grids = static_cast<float *>(c->manip_grids.p);
    const HostMaps a{n_frames, clouds, n_pts, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, &c->submap_tab};
    return end_host_call(c, host_map_chunks(
        c, a, chunk,
        [&](int, int nm) -> int {
            HIPCK(c, hipMemsetAsync(grids, 0, (size_t)nm * per_map * sizeof(float), c->stream));
            return BEV_OK;
        },
        [&](const TablesUp &u, int r0, int nr) { submap_float_splat(c, u, c->st_in, r0, nr, fg, grids); },
        [&](int m0, int nm) -> int {
            HIPCK(c, hipGetLastError());
            for (int m = 0; m < nm; ++m)
                HIPCK(c, hipMemcpyAsync(out[m0 + m], grids + (size_t)m * per_map, per_map * sizeof(float), hipMemcpyDeviceToHost,
                                        c->stream));
            return BEV_OK;
        }));
}
