/*
 * bev_capi_place.hip — place retrieval of the boundary declared extern "C" in include/bev_mi355x.h: polar
 * max-height descriptors of frames or of submaps over packed frames, and the match list of queries against a database.
 * Host-side only; the kernels are bev_place.h's, the arithmetic bev_place_exact.h's, the maps' plan bev_submap_plan.h's (§6i);
 * the prologue of the descriptor call, the tables on their way up and both loops of bev_place_retrieval_batch are
 * bev_packed_host.h's, shared with the submap calls and the translation guess.
 */
#include <cstdlib>

#include "bev_packed_host.h"
#include "bev_place_exact.h"

using namespace bevh; /* (and through it bevk) */
using namespace bevx;

namespace {

/* the admitted parameters of a call as the kernels take them, and the ring edges */
struct PlaceCall {
    PlaceShape ps;
    float edge2[kPlaceMaxRings + 1];
    size_t cells;
};
bool place_call(const bev_ctx *c, const bev_place_params_t *params, PlaceCall *pc)
{
    const bev_place_params_t p = params ? *params : bev_place_defaults();
    if (!place_params_ok(p.n_rings, p.n_sectors, p.max_range, p.skip_label0)) return false;
    pc->ps = PlaceShape{p.n_rings, p.n_sectors, p.skip_label0, c ? c->geo.rp.lidar_to_ground : 0.0f};
    place_edges(p.n_rings, p.max_range, pc->edge2);
    pc->cells = (size_t)p.n_rings * (size_t)p.n_sectors;
    return true;
}

constexpr size_t kEdgeBytes = 256; /* the ring edges lead the block that goes up; the tables follow, 64-byte aligned */

/* rows [r0, r0 + nr) of the tables that went up behind the ring edges (TablesUp, bev_packed_host.h; the one launch group of a
 * plan over maps, or the frame table) splatted from d_clouds into planes (left out where they hold no point) */
void place_splat(bev_ctx *c, const TablesUp &u, const PlaceCall &pc, const bev_point_t *d_clouds, int r0, int nr, uint32_t *planes)
{
    const TablesUp::Slice s = u.slice(0, r0, nr);
    if (s.blocks == 0) return;
    ProfScope ps(c, K_PLACE_SPLAT, nr);
    launch_place_splat(d_clouds, s.rows, s.ent0, nr, s.blocks, s.entries, reinterpret_cast<const float *>(u.dev), pc.ps, planes,
                       c->stream);
}
void place_finish(bev_ctx *c, const PlaceCall &pc, const uint32_t *planes, int n_desc, uint8_t *d_desc, void *d_units)
{
    ProfScope ps(c, K_PLACE_FINISH, n_desc);
    launch_place_finish(planes, n_desc, pc.ps, d_desc, static_cast<PlaceHandle *>(d_units), c->stream);
}
/* the zeroed planes of n_desc descriptors on the context's stream */
int place_planes(bev_ctx *c, const PlaceCall &pc, int n_desc, uint32_t **planes)
{
    const size_t bytes = (size_t)n_desc * pc.cells * sizeof(uint32_t);
    const int rc = c->place_planes.grow(c, bytes);
    if (rc != BEV_OK) return rc;
    *planes = static_cast<uint32_t *>(c->place_planes.p);
    HIPCK(c, hipMemsetAsync(*planes, 0, bytes, c->stream));
    return BEV_OK;
}

/* The descriptors of nf frames (map_offs == nullptr), or of n_maps maps over them, in device memory, on the context's stream
 * (arguments checked by the caller; at least one descriptor) */
int place_descriptors(bev_ctx *c, const PlaceCall &pc, int nf, const bev_point_t *d_clouds, const uint64_t *offs, int n_maps,
                      const uint64_t *map_offs, const int32_t *entry_frame, const float *entry_pose, uint8_t *d_desc, void *d_units)
{
    TablesUp u;
    const int n_desc = map_offs ? n_maps : nf;
    if (map_offs ? !bevsub::plan_maps(u.plan, offs, map_offs, 0, n_maps, entry_frame, entry_pose, (size_t)n_maps) : !u.frames(nf, offs))
        return BEV_ERR_TOO_LARGE;
    uint32_t *planes = nullptr;
    int rc = place_planes(c, pc, n_desc, &planes); /* (a grow waits for the stream: before the tables go up) */
    if (rc != BEV_OK) return rc;
    rc = u.up(c, c->place_tab, kEdgeBytes, pc.edge2, sizeof pc.edge2);
    if (rc != BEV_OK) return rc;
    place_splat(c, u, pc, d_clouds, 0, u.plan.groups[0].n_rows, planes);
    place_finish(c, pc, planes, n_desc, d_desc, d_units);
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

constexpr size_t kPairGroupBytes = (size_t)64 << 20; /* the pairs of a group of queries: 8 bytes each */
constexpr int kMaxQueryGroup = 65535;                /* (a group's queries are the launch's y dimension) */

bool limits_ok(int n_queries, int n_db, const int32_t *h_limit)
{
    for (int q = 0; h_limit && q < n_queries; ++q)
        if (h_limit[q] < 0 || h_limit[q] > n_db) return false;
    return true;
}
/* The hits of n_queries > 0 queries on the context's stream (arguments checked by the caller): groups of queries over one
 * buffer of pairs, stream order handing it from group to group */
int place_match(bev_ctx *c, const PlaceCall &pc, int n_queries, const void *d_units_q, int n_db, const void *d_units_db,
                const int32_t *h_limit, int top_k, bev_place_hit_t *d_hits)
{
    size_t group = std::max<size_t>(1, kPairGroupBytes / (std::max<size_t>((size_t)n_db, 1) * sizeof(uint2)));
    if (const char *e = getenv("BEV_PLACE_QUERY_GROUP")) group = (size_t)std::max(1, atoi(e));
    group = std::min(group, (size_t)std::min(n_queries, kMaxQueryGroup));
    int rc = c->place_pairs.grow(c, std::max<size_t>(group * (size_t)n_db, 1) * sizeof(uint2));
    if (rc != BEV_OK) return rc;
    const int32_t *d_limit = nullptr;
    if (h_limit) {
        void *h = nullptr;
        rc = c->place_lim.begin(c, (size_t)n_queries * sizeof(int32_t), 4096, &h);
        if (rc != BEV_OK) return rc;
        memcpy(h, h_limit, (size_t)n_queries * sizeof(int32_t));
        d_limit = static_cast<const int32_t *>(c->place_lim.dev);
        rc = c->place_lim.push(c, (size_t)n_queries * sizeof(int32_t));
        if (rc != BEV_OK) return rc;
    }
    uint2 *pairs = static_cast<uint2 *>(c->place_pairs.p);
    const PlaceHandle *uq = static_cast<const PlaceHandle *>(d_units_q), *udb = static_cast<const PlaceHandle *>(d_units_db);
    for (int q0 = 0; q0 < n_queries; q0 += (int)group) {
        const int nq = std::min((int)group, n_queries - q0);
        {
            ProfScope ps(c, K_PLACE_PAIRS, nq);
            launch_place_pairs(uq, q0, nq, udb, n_db, d_limit, pc.ps, pairs, c->stream);
        }
        ProfScope ps(c, K_PLACE_TOPK, nq);
        launch_place_topk(pairs, q0, nq, n_db, d_limit, pc.ps, top_k, d_hits, c->stream);
    }
    HIPCK(c, hipGetLastError());
    return BEV_OK;
}

} // namespace

extern "C" {

bev_place_params_t bev_place_defaults(void) { return bev_place_params_t{20, 60, 80.0f, 1}; }

size_t bev_place_descriptor_bytes(const bev_place_params_t *params)
{
    PlaceCall pc;
    return place_call(nullptr, params, &pc) ? pc.cells : 0;
}

size_t bev_place_desc_handle_bytes(const bev_place_params_t *params)
{
    PlaceCall pc;
    return place_call(nullptr, params, &pc) ? sizeof(PlaceHandle) : 0;
}

int bev_place_descriptor_device_resident(bev_ctx_t *c, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                         int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                         const float *h_entry_pose, const bev_place_params_t *params, uint8_t *d_desc,
                                         void *d_units)
{
    PlaceCall pc;
    if (!c || !place_call(c, params, &pc)) return BEV_ERR_INVALID_ARG;
    const FramesAndMaps a{n_frames, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose};
    const bool outputs_ok = (d_desc || d_units) && reinterpret_cast<uintptr_t>(d_units) % 64 == 0;
    return resident_maps_call(c, a, true, BEV_OK, outputs_ok, [&] {
        return place_descriptors(c, pc, n_frames, d_clouds, h_offsets, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, d_desc,
                                 d_units);
    });
}

int bev_place_match_device_resident(bev_ctx_t *c, const bev_place_params_t *params, int n_queries, const void *d_units_q,
                                    int n_db, const void *d_units_db, const int32_t *h_limit, int top_k, bev_place_hit_t *d_hits)
{
    PlaceCall pc;
    if (!c || !place_call(c, params, &pc) || n_queries < 0 || n_db < 0 || top_k < 1 || top_k > BEV_PLACE_MAX_TOP_K ||
        !limits_ok(n_queries, n_db, h_limit))
        return BEV_ERR_INVALID_ARG;
    if (n_queries == 0) return BEV_OK;
    if (!d_hits || !d_units_q || (n_db > 0 && !d_units_db)) return BEV_ERR_INVALID_ARG;
    return resident_call(c, [&] { return place_match(c, pc, n_queries, d_units_q, n_db, d_units_db, h_limit, top_k, d_hits); });
}

/* The queries: the frames in chunks of max_batch through the input staging.  The maps: bev_submap_float_bev_batch's chunks of
 * one launch group of at most max_batch maps, the distinct frames a chunk names going up max_batch at a time, each such piece
 * splatted into the chunk's planes before the next goes up. */
int bev_place_retrieval_batch(bev_ctx_t *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, int n_maps,
                              const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                              const bev_place_params_t *params, const int32_t *h_limit, int top_k, bev_place_hit_t *hits)
{
    PlaceCall pc;
    if (!c || !place_call(c, params, &pc) || n_frames < 0 || !host_clouds_ok(n_frames, clouds, n_pts)) return BEV_ERR_INVALID_ARG;
    bool maps = false;
    int rc = check_optional_maps(n_frames, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, &maps);
    if (rc != BEV_OK) return rc;
    const int n_db = maps ? n_maps : n_frames;
    if (top_k < 1 || top_k > BEV_PLACE_MAX_TOP_K || !limits_ok(n_frames, n_db, h_limit) || (n_frames > 0 && !hits))
        return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if ((size_t)n_pts[f] > cloud_cap(c)) return BEV_ERR_TOO_LARGE;
    if (n_frames == 0) return BEV_OK;
    rc = begin_call(c, true);
    if (rc != BEV_OK) return rc;
    const size_t unit_bytes = ((size_t)n_frames + (maps ? (size_t)n_maps : 0)) * sizeof(PlaceHandle),
                 hit_bytes = (size_t)n_frames * (size_t)top_k * sizeof(bev_place_hit_t);
    rc = c->place_out.grow(c, unit_bytes + hit_bytes);
    if (rc != BEV_OK) return rc;
    PlaceHandle *units_q = static_cast<PlaceHandle *>(c->place_out.p), *units_db = maps ? units_q + n_frames : units_q;
    bev_place_hit_t *d_hits = reinterpret_cast<bev_place_hit_t *>(static_cast<char *>(c->place_out.p) + unit_bytes);
    const auto body = [&]() -> int {
        int rc_ = packed_chunks(c, n_frames, clouds, n_pts, [&](int f0, int nb, const uint64_t *off) {
            return place_descriptors(c, pc, nb, c->st_in, off, 0, nullptr, nullptr, nullptr, nullptr, units_q + f0);
        });
        if (rc_ != BEV_OK) return rc_;
        if (maps) {
            uint32_t *planes = nullptr;
            const HostMaps a{n_frames, clouds, n_pts, n_maps, h_map_offsets, h_entry_frame, h_entry_pose, &c->place_tab,
                             kEdgeBytes, pc.edge2, sizeof pc.edge2};
            rc_ = host_map_chunks(
                c, a, std::min(std::max(n_maps, 1), c->max_batch), [&](int, int nm) { return place_planes(c, pc, nm, &planes); },
                [&](const TablesUp &u, int r0, int nr) { place_splat(c, u, pc, c->st_in, r0, nr, planes); },
                [&](int m0, int nm) -> int {
                    place_finish(c, pc, planes, nm, nullptr, units_db + m0);
                    HIPCK(c, hipGetLastError());
                    return BEV_OK;
                });
            if (rc_ != BEV_OK) return rc_;
        }
        rc_ = place_match(c, pc, n_frames, units_q, n_db, units_db, h_limit, top_k, d_hits);
        if (rc_ != BEV_OK) return rc_;
        HIPCK(c, hipMemcpyAsync(hits, d_hits, hit_bytes, hipMemcpyDeviceToHost, c->stream));
        return BEV_OK;
    };
    return end_host_call(c, body());
}

} /* extern "C" */
