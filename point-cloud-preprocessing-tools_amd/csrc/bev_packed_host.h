/*
 * bev_packed_host.h — what the calls over packed frames and maps share across the files of the C ABI, over bev_ctx.h:
 * bev_capi_packed.hip (submap BEVs, float submap BEVs), bev_capi_place.hip (place retrieval; §6z) and
 * bev_capi_align.hip (the translation guess; §6ab).  The check of optional maps, the prologue of a device-resident call over
 * frames and maps, the tables of such a call on their way to the device (TablesUp), and the two loops of the host-buffer calls:
 * frames in chunks (packed_chunks) and maps in chunks whose frames go through the staging in pieces (host_map_chunks).
 * Short inline functions and templates, no state.  Private.
 */
#ifndef BEV_PACKED_HOST_H
#define BEV_PACKED_HOST_H

#include <cstring>
#include <vector>

#include "bev_ctx.h"
#include "bev_submap_plan.h"

namespace bevh {

static_assert(sizeof(ProjFrame) == sizeof(bevsub::Frame) && (uint32_t)kProjBlock == bevsub::kBlockPoints,
              "a frame table is read as ProjFrame rows of kProjBlock points a workgroup (bev_submap.h asserts the fields)");

/* ---- argument checks ---- */
/* The map arrays of a call whose maps are optional: all NULL with n_maps == 0 (*maps = false: the call is over the frames), or
 * what check_submap_entries asks for. */
inline int check_optional_maps(int n_frames, int n_maps, const uint64_t *map_offs, const int32_t *entry_frame,
                               const float *entry_pose, bool *maps)
{
    *maps = map_offs != nullptr;
    if (!map_offs) return (n_maps == 0 && !entry_frame && !entry_pose) ? BEV_OK : BEV_ERR_INVALID_ARG;
    return check_submap_entries(n_frames, n_maps, map_offs, entry_frame, entry_pose);
}

/* the arguments of a call over packed frames and maps, as the entry point got them */
struct FramesAndMaps {
    int n_frames;
    const bev_point_t *d_clouds;
    const uint64_t *offs;
    int n_maps;
    const uint64_t *map_offs; /* nullptr (where the call allows it): no maps, one output per frame */
    const int32_t *entry_frame;
    const float *entry_pose;
};
/* A device-resident call over frames and maps, behind the checks of the entry point's own parameters.  The order of the
 * statuses is the contract: the frames' BEV_ERR_INVALID_ARG; what the maps' check returns (optional: check_optional_maps, else
 * check_submap_entries); `behind_maps`, a status of the entry point's own (an interval that is not supported); a frame that is
 * too large; BEV_OK where there is no output to make; BEV_ERR_INVALID_ARG for !outputs_ok, and for a NULL d_clouds with
 * records to read.  Then body() inside resident_call. */
template <class Body>
int resident_maps_call(bev_ctx *c, const FramesAndMaps &a, bool optional, int behind_maps, bool outputs_ok, Body body)
{
    const int rc = check_packed_frames(c, a.n_frames, a.offs);
    if (rc == BEV_ERR_INVALID_ARG) return rc;
    bool maps = true;
    const int rc_maps = optional ? check_optional_maps(a.n_frames, a.n_maps, a.map_offs, a.entry_frame, a.entry_pose, &maps)
                                 : check_submap_entries(a.n_frames, a.n_maps, a.map_offs, a.entry_frame, a.entry_pose);
    if (rc_maps != BEV_OK) return rc_maps;
    if (behind_maps != BEV_OK) return behind_maps;
    if (rc != BEV_OK) return rc; /* (a frame that is too large: behind the arguments that are wrong) */
    if ((maps ? a.n_maps : a.n_frames) == 0) return BEV_OK;
    if (!outputs_ok) return BEV_ERR_INVALID_ARG;
    if (!a.d_clouds) { /* records to read */
        if (!maps && a.offs[a.n_frames] != a.offs[0]) return BEV_ERR_INVALID_ARG;
        for (uint64_t e = maps ? a.map_offs[0] : 0; maps && e < a.map_offs[a.n_maps]; ++e)
            if (a.offs[a.entry_frame[e] + 1] != a.offs[a.entry_frame[e]]) return BEV_ERR_INVALID_ARG;
    }
    return resident_call(c, body);
}

/* ---- the tables of a call on their way to the device ---- */
/* Either the frame table of a call without maps (frames) or the launch groups of a plan over maps (§6i), in ONE block of an
 * UploadTable of the caller's behind `lead` bytes of the call's own (a multiple of 64).  Each call has an UploadTable of its
 * own: a shared one would make a call wait for another call's upload event. */
struct TablesUp {
    bevsub::Plan plan; /* without maps: rows alone, one group of nf rows without entries */
    bool maps = true;
    std::vector<bevsub::GroupBytes> at; /* per group: where its tables lie in the block */
    const char *dev = nullptr;

    /* the frame table of nf frames [offs[f], offs[f + 1]): false for more workgroups than a launch can have */
    bool frames(int nf, const uint64_t *offs)
    {
        maps = false;
        plan.rows.resize((size_t)nf + 1);
        bevsub::Group g;
        g.n_rows = nf;
        uint32_t n_max;
        if (!bevsub::frame_table(plan.rows.data(), nf, offs, &n_max, &g.blocks)) return false;
        plan.groups.assign(1, g);
        return true;
    }
    bevsub::Frame *rows(size_t gi) { return plan.rows.data() + plan.groups[gi].row0; }
    /* Sends the block up the context's stream: lead_n bytes at lead_src, zeros up to `lead`, then the tables. */
    int up(bev_ctx *c, UploadTable &t, size_t lead = 0, const void *lead_src = nullptr, size_t lead_n = 0)
    {
        size_t bytes = lead;
        for (const bevsub::Group &g : plan.groups) {
            at.push_back(maps ? bevsub::group_bytes(g, bytes) : bevsub::GroupBytes{bytes, 0, 0, bytes + plan.rows.size() * sizeof(bevsub::Frame)});
            bytes = at.back().end;
        }
        char *h = nullptr;
        const int rc = t.begin(c, bytes, 64 * 1024, reinterpret_cast<void **>(&h));
        if (rc != BEV_OK) return rc;
        if (lead) memset(h, 0, lead);
        if (lead_n) memcpy(h, lead_src, lead_n);
        if (maps) bevsub::pack(plan, h + lead);
        else memcpy(h + lead, plan.rows.data(), bytes - lead);
        dev = static_cast<const char *>(t.dev);
        return t.push(c, bytes);
    }
    /* rows [r0, r0 + nr) of group gi as a launch takes them: device pointers (ent0, entries: nullptr without maps) and the
     * workgroups of the splat over them (0: nothing to launch) */
    struct Slice {
        const void *rows;
        const uint32_t *ent0;
        const void *entries;
        uint32_t blocks;
    };
    Slice slice(size_t gi, int r0, int nr) const
    {
        const bevsub::Frame *hr = plan.rows.data() + plan.groups[gi].row0;
        const bevsub::GroupBytes &b = at[gi];
        return Slice{dev + b.rows + (size_t)r0 * sizeof(bevsub::Frame),
                     maps ? reinterpret_cast<const uint32_t *>(dev + b.ent0) + r0 : nullptr, maps ? dev + b.entries : nullptr,
                     hr[r0 + nr].blk0 - hr[r0].blk0};
    }
};

/* ---- the host-buffer calls (after begin_call with the staging) ---- */
/* What ends a host-buffer call whose work on the context's stream returned rc: one synchronisation.  An error leaves nothing
 * in flight either: copies of earlier chunks into the caller's buffers may still be on their way. */
inline int end_host_call(bev_ctx *c, int rc)
{
    if (rc == BEV_OK) rc = [&]() -> int {
        HIPCK(c, hipStreamSynchronize(c->stream));
        return BEV_OK;
    }();
    if (rc != BEV_OK) (void)hipDeviceSynchronize();
    return rc;
}

/* Frames in chunks of max_batch clouds, which fit the input staging whatever their sizes.  A chunk's clouds are packed into
 * st_in, one copy per non-empty cloud; body(f0, nb, off) launches the chunk's nb frames [off[f], off[f + 1]) of st_in and
 * queues what becomes of their results; all of it follows the chunk before in the order of the context's stream. */
template <class Body>
int packed_chunks(bev_ctx *c, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, Body body)
{
    std::vector<uint64_t> off;
    for (int f0 = 0; f0 < n_frames; f0 += c->max_batch) {
        const int nb = std::min(c->max_batch, n_frames - f0);
        off.assign((size_t)nb + 1, 0);
        for (int f = 0; f < nb; ++f) {
            off[f + 1] = off[f] + n_pts[f0 + f];
            if (n_pts[f0 + f])
                HIPCK(c, hipMemcpyAsync(c->st_in + off[f], clouds[f0 + f], (size_t)n_pts[f0 + f] * sizeof(bev_point_t),
                                        hipMemcpyHostToDevice, c->stream));
        }
        const int rc = body(f0, nb, off.data());
        if (rc != BEV_OK) return rc;
    }
    return BEV_OK;
}

/* the host clouds and the maps of a host-buffer call over maps (checked by the caller), and the call's UploadTable */
struct HostMaps {
    int n_frames;
    const bev_point_t *const *clouds;
    const uint32_t *n_pts;
    int n_maps;
    const uint64_t *map_offs;
    const int32_t *entry_frame;
    const float *entry_pose;
    UploadTable *tab;
    size_t lead = 0; /* TablesUp::up's */
    const void *lead_src = nullptr;
    size_t lead_n = 0;
};
/* Maps in chunks of `chunk` (at most max_batch) maps, each ONE launch group; the distinct frames a chunk names go through the
 * input staging max_batch at a time, each such piece splatted before the next goes up.  Per chunk of maps [m0, m0 + nm):
 * begin(m0, nm) grows and zeroes what the chunk accumulates into (a grow waits for the stream: before the tables go up);
 * splat(u, r0, nr) launches rows [r0, r0 + nr) of u's group 0 from st_in; end(m0, nm) finishes the chunk and queues the copies
 * of its results. */
template <class Begin, class Splat, class End>
int host_map_chunks(bev_ctx *c, const HostMaps &a, int chunk, Begin begin, Splat splat, End end)
{
    std::vector<uint64_t> offs((size_t)a.n_frames + 1, 0); /* (only the counts matter: a row's offset is set per piece) */
    for (int f = 0; f < a.n_frames; ++f) offs[f + 1] = offs[f] + a.n_pts[f];
    for (int m0 = 0; m0 < a.n_maps; m0 += chunk) {
        const int nm = std::min(chunk, a.n_maps - m0);
        TablesUp u;
        if (!bevsub::plan_maps(u.plan, offs.data(), a.map_offs, m0, m0 + nm, a.entry_frame, a.entry_pose, (size_t)nm))
            return BEV_ERR_TOO_LARGE;
        const bevsub::Group &g = u.plan.groups[0];
        bevsub::Frame *rows = u.rows(0);
        for (int r = 0; r < g.n_rows; ++r) /* where the row's frame will lie in the staging while its piece is there */
            rows[r].off = r % c->max_batch ? rows[r - 1].off + rows[r - 1].n : 0;
        int rc = begin(m0, nm);
        if (rc != BEV_OK) return rc;
        rc = u.up(c, *a.tab, a.lead, a.lead_src, a.lead_n);
        if (rc != BEV_OK) return rc;
        for (int r0 = 0; r0 < g.n_rows; r0 += c->max_batch) {
            const int nr = std::min(c->max_batch, g.n_rows - r0);
            for (int r = r0; r < r0 + nr; ++r)
                if (rows[r].n)
                    HIPCK(c, hipMemcpyAsync(c->st_in + rows[r].off, a.clouds[u.plan.frame[g.row0 + r]],
                                            (size_t)rows[r].n * sizeof(bev_point_t), hipMemcpyHostToDevice, c->stream));
            splat(u, r0, nr);
        }
        rc = end(m0, nm);
        if (rc != BEV_OK) return rc;
    }
    return BEV_OK;
}

} // namespace bevh
#endif
