/*
 * bev_capi_align.hip — the translation guess of retrieved pairs of the boundary declared extern "C" in include/bev_mi355x.h
 * (DESIGN.md §6ab): Cartesian height grids of frames or of submaps over packed frames, and per hit of a match list the table of
 * initial transforms the fine registration calls take.  Host-side only; the kernels are bev_align.h's, the arithmetic
 * bev_align_exact.h's, the maps' plan bev_submap_plan.h's (§6i); the prologue of the grid call and the tables on their way up
 * are bev_packed_host.h's, shared with the submap calls and place retrieval.
 */
#include <cstdlib>

#include "bev_packed_host.h"
#include "bev_align_exact.h"

using namespace bevh; /* (and through it bevk) */
using namespace bevx;

namespace {

bool align_call(const bev_ctx *c, const bev_align_params_t *params, AlignShape *as)
{
    const bev_align_params_t p = params ? *params : bev_align_defaults();
    if (!align_params_ok(p.grid, p.cell, p.max_shift, p.yaw_steps, p.yaw_step, p.skip_label0)) return false;
    *as = AlignShape{p.grid, p.max_shift, p.yaw_steps, p.skip_label0, p.cell, p.yaw_step, c ? c->geo.rp.lidar_to_ground : 0.0f};
    return true;
}

/* The grids of nf frames (map_offs == nullptr), or of n_maps maps over them, in device memory, on the context's stream
 * (arguments checked by the caller; at least one grid).  The tables go up in ONE block of align_tab (TablesUp,
 * bev_packed_host.h): the frame table of a call without maps or the one launch group of a plan over maps (§6i). */
int align_grids(bev_ctx *c, const AlignShape &as, int nf, const bev_point_t *d_clouds, const uint64_t *offs, int n_maps,
                const uint64_t *map_offs, const int32_t *entry_frame, const float *entry_pose, uint8_t *d_grids, uint32_t *d_energy)
{
    TablesUp u;
    const int n_grids = map_offs ? n_maps : nf;
    if (map_offs ? !bevsub::plan_maps(u.plan, offs, map_offs, 0, n_maps, entry_frame, entry_pose, (size_t)n_maps) : !u.frames(nf, offs))
        return BEV_ERR_TOO_LARGE;
    const size_t plane_bytes = (size_t)n_grids * (size_t)as.G * (size_t)as.G * sizeof(uint32_t);
    int rc = c->align_planes.grow(c, plane_bytes); /* (a grow waits for the stream: before the tables go up) */
    if (rc != BEV_OK) return rc;
    uint32_t *planes = static_cast<uint32_t *>(c->align_planes.p);
    HIPCK(c, hipMemsetAsync(planes, 0, plane_bytes, c->stream));
    rc = u.up(c, c->align_tab);
    if (rc != BEV_OK) return rc;
    const int nr = u.plan.groups[0].n_rows;
    const TablesUp::Slice s = u.slice(0, 0, nr);
    if (s.blocks) {
        ProfScope ps(c, K_ALIGN_GRID, nr);
        launch_align_grid(d_clouds, s.rows, s.ent0, nr, s.blocks, s.entries, as, planes, c->stream);
    }
    {
        ProfScope ps(c, K_ALIGN_FINISH, n_grids);
        launch_align_finish(planes, n_grids, as, d_grids, d_energy, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

constexpr int kAlignGroup = 4096; /* hits of a launch group: 32 bytes per hypothesis, 14 hypotheses at most */

bool hits_ok(int n_frames, int n_db, int n_hits, const bev_match_t *h_hits)
{
    for (int m = 0; m < n_hits; ++m)
        if (h_hits[m].query_idx < 0 || h_hits[m].query_idx >= n_frames || h_hits[m].match_idx >= n_db) return false;
    return true;
}
/* The results of n_hits > 0 hits on the context's stream (arguments checked by the caller): the hits go up once, then groups of
 * them over one buffer of hypotheses, stream order handing it from group to group */
int align_hits(bev_ctx *c, const AlignShape &as, const bev_point_t *d_clouds, const uint64_t *offs, const uint8_t *d_grids,
               const uint32_t *d_energy, int n_hits, const bev_match_t *h_hits, bev_icp_result_t *d_results, int32_t *d_best,
               bev_align_detail_t *d_detail)
{
    int group = kAlignGroup;
    if (const char *e = getenv("BEV_ALIGN_GROUP")) group = std::max(1, atoi(e));
    group = std::min(group, n_hits);
    const size_t per_hit = (size_t)2 * (size_t)(2 * as.K + 1);
    int rc = c->align_hyp.grow(c, (size_t)group * per_hit * sizeof(AlignHyp));
    if (rc != BEV_OK) return rc;
    AlignHit *h = nullptr;
    rc = c->align_hits.begin(c, (size_t)n_hits * sizeof(AlignHit), 4096, reinterpret_cast<void **>(&h));
    if (rc != BEV_OK) return rc;
    for (int m = 0; m < n_hits; ++m) {
        const int q = h_hits[m].query_idx;
        h[m] = AlignHit{offs[q], (uint32_t)(offs[q + 1] - offs[q]), h_hits[m].match_idx < 0 ? -1 : h_hits[m].match_idx,
                        h_hits[m].angle_guess, 0u};
    }
    rc = c->align_hits.push(c, (size_t)n_hits * sizeof(AlignHit));
    if (rc != BEV_OK) return rc;
    const AlignHit *d_hits = static_cast<const AlignHit *>(c->align_hits.dev);
    AlignHyp *hyp = static_cast<AlignHyp *>(c->align_hyp.p);
    for (int m0 = 0; m0 < n_hits; m0 += group) {
        const int n = std::min(group, n_hits - m0);
        {
            ProfScope ps(c, K_ALIGN_HIT, n);
            launch_align_hit(d_clouds, d_hits + m0, n, d_grids, as, hyp, c->stream);
        }
        ProfScope ps(c, K_ALIGN_PICK, n);
        launch_align_pick(d_hits + m0, n, hyp, d_energy, as, d_results + (size_t)2 * m0, d_best + m0,
                          d_detail ? d_detail + (size_t)2 * m0 : nullptr, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

extern "C" {

bev_align_params_t bev_align_defaults(void) { return bev_align_params_t{128, 0.5f, 16, 1, 2.0f, 1}; }

size_t bev_align_grid_bytes(const bev_align_params_t *params)
{
    AlignShape as;
    return align_call(nullptr, params, &as) ? (size_t)as.G * (size_t)as.G : 0;
}

int bev_align_grid_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets, int n_maps,
                                   const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                                   const bev_align_params_t *params, uint8_t *d_grids, uint32_t *d_energy)
{
    AlignShape as;
    if (!c || !align_call(c, params, &as)) return BEV_ERR_INVALID_ARG;
    const FramesAndMaps a{n_frames, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose};
    return resident_maps_call(c, a, true, BEV_OK, d_grids && d_energy, [&] {
        return align_grids(c, as, n_frames, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, d_grids, d_energy);
    });
}

int bev_align_hits_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets, int n_db,
                                   const uint8_t *d_grids, const uint32_t *d_energy, int n_hits, const bev_match_t *h_hits,
                                   const bev_align_params_t *params, bev_icp_result_t *d_results, int32_t *d_best,
                                   bev_align_detail_t *d_detail)
{
    AlignShape as;
    if (!c || !align_call(c, params, &as)) return BEV_ERR_INVALID_ARG;
    const int rc = check_packed_frames(c, n_frames, h_offsets);
    if (rc == BEV_ERR_INVALID_ARG) return rc;
    if (n_db < 0 || n_hits < 0 || (n_hits > 0 && !h_hits) || !hits_ok(n_frames, n_db, n_hits, h_hits)) return BEV_ERR_INVALID_ARG;
    if (rc != BEV_OK) return rc;
    if (n_hits == 0) return BEV_OK;
    if (!d_results || !d_best) return BEV_ERR_INVALID_ARG;
    for (int m = 0; m < n_hits; ++m) {
        const int q = h_hits[m].query_idx;
        if (h_hits[m].match_idx >= 0 && (!d_grids || !d_energy)) return BEV_ERR_INVALID_ARG;
        if (!d_clouds && h_offsets[q + 1] != h_offsets[q]) return BEV_ERR_INVALID_ARG;
    }
    return resident_call(c, [&] {
        return align_hits(c, as, d_clouds, h_offsets, d_grids, d_energy, n_hits, h_hits, d_results, d_best, d_detail);
    });
}

/* Every frame goes up into one packed buffer of align_io, behind it the grids, their sums of squares and the records coming out;
 * then the two device-resident bodies and one copy back per output. */
int bev_align_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, int n_maps,
                    const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose, int n_hits,
                    const bev_match_t *h_hits, const bev_align_params_t *params, bev_icp_result_t *results, int32_t *best,
                    bev_align_detail_t *detail)
{
    AlignShape as;
    if (!c || !align_call(c, params, &as) || n_frames < 0 || !host_clouds_ok(n_frames, clouds, n_pts)) return BEV_ERR_INVALID_ARG;
    bool maps = false;
    int rc = check_optional_maps(n_frames, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, &maps);
    if (rc != BEV_OK) return rc;
    const int n_db = maps ? n_maps : n_frames;
    if (n_hits < 0 || (n_hits > 0 && (!h_hits || !results || !best)) || !hits_ok(n_frames, n_db, n_hits, h_hits))
        return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if ((size_t)n_pts[f] > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_hits == 0) return BEV_OK;
    rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    std::vector<uint64_t> offs((size_t)n_frames + 1, 0);
    for (int f = 0; f < n_frames; ++f) offs[f + 1] = offs[f] + n_pts[f];
    const size_t cells = (size_t)as.G * (size_t)as.G;
    void *p_in = nullptr, *p_grids = nullptr, *p_energy = nullptr, *p_res = nullptr, *p_best = nullptr, *p_det = nullptr;
    const size_t sz[6] = {std::max<size_t>(offs[n_frames], 1) * sizeof(bev_point_t), std::max<size_t>(n_db, 1) * cells,
                          std::max<size_t>(n_db, 1) * sizeof(uint32_t), (size_t)2 * n_hits * sizeof(bev_icp_result_t),
                          (size_t)n_hits * sizeof(int32_t), (size_t)2 * n_hits * sizeof(bev_align_detail_t)};
    void **const dst[6] = {&p_in, &p_grids, &p_energy, &p_res, &p_best, &p_det};
    rc = c->align_io.grow(c, carve(nullptr, sz, dst));
    if (rc != BEV_OK) return rc;
    carve(c->align_io.p, sz, dst);
    const auto body = [&]() -> int {
        bev_point_t *d_in = static_cast<bev_point_t *>(p_in);
        for (int f = 0; f < n_frames; ++f)
            if (n_pts[f])
                HIPCK(c, hipMemcpyAsync(d_in + offs[f], clouds[f], (size_t)n_pts[f] * sizeof(bev_point_t), hipMemcpyHostToDevice,
                                        c->stream));
        if (n_db > 0) {
            const int rc_ = align_grids(c, as, n_frames, d_in, offs.data(), n_maps, h_map_offsets, h_entry_frame, h_entry_pose,
                                        static_cast<uint8_t *>(p_grids), static_cast<uint32_t *>(p_energy));
            if (rc_ != BEV_OK) return rc_;
        }
        const int rc_ = align_hits(c, as, d_in, offs.data(), static_cast<uint8_t *>(p_grids), static_cast<uint32_t *>(p_energy),
                                   n_hits, h_hits, static_cast<bev_icp_result_t *>(p_res), static_cast<int32_t *>(p_best),
                                   detail ? static_cast<bev_align_detail_t *>(p_det) : nullptr);
        if (rc_ != BEV_OK) return rc_;
        HIPCK(c, hipMemcpyAsync(results, p_res, sz[3], hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(best, p_best, sz[4], hipMemcpyDeviceToHost, c->stream));
        if (detail) HIPCK(c, hipMemcpyAsync(detail, p_det, sz[5], hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        return BEV_OK;
    };
    rc = body();
    if (rc != BEV_OK) (void)hipDeviceSynchronize();
    return rc;
}

} /* extern "C" */
