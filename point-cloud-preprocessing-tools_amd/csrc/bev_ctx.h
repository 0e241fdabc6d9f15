/*
 * bev_ctx.h — the context behind bev_ctx_t and what the seven files of the C ABI share: bev_capi.hip (the context, the BEV
 * pipeline and the single-cloud entry points), bev_capi_packed.hip (the batched calls over packed frames), bev_capi_reg.hip
 * (the registration entry points, frame against frame), bev_capi_submap_reg.hip (frames against submaps; what only these
 * two and bev_capi_verify.hip share: bev_reg_host.h), bev_capi_place.hip (place retrieval), bev_capi_verify.hip (verification of
 * registered matches) and bev_capi_align.hip (the translation guess of retrieved pairs; what it, bev_capi_place.hip and
 * bev_capi_packed.hip share over maps: bev_packed_host.h) — among it the prologue of every call outside the fused pipeline
 * (begin_call) and the bound on a cloud's points (cloud_cap).  Private, like bev_internal.h.  Named namespace: struct bev_ctx is one type in all of them.
 */
#ifndef BEV_CTX_H
#define BEV_CTX_H

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bev_internal.h"

struct bev_ctx;

namespace bevh {
using namespace bevk;

constexpr int kDescRing = 4; /* calls the host may run ahead of the device (2 and 12 measured the same) */
constexpr int kEventPairs = 2048;

struct ProfSlot {
    hipEvent_t a, b;
    int kid;
    int frames;
};

/* A sub-batch's workspace lives from its column walk to its rasters: four launches of its stream, and two streams take
 * sub-batches in turn (k_stage, see run_pipeline), so eight workspace sets ("lanes", the name rounds 2-5 gave them when
 * each also had a stream) go round.  Lane 0 doubles as
 * the workspace of the single-cloud entry points. */
constexpr int kMaxStageStreams = 4;
constexpr int kMaxLanes = 4 * kMaxStageStreams;
struct Lane {
    FrameInfo *info = nullptr;  /* per frame: how its points reach their slots (k_probe / k_verdict) */
    FrameDesc *desc = nullptr;  /* per frame: k_probe's device copy of the caller's descriptor */
    uint32_t *est = nullptr;    /* stream frames: estimated input position of every (row, strip)'s first slot */
    uint32_t *tail_list = nullptr, *tail_cnt = nullptr; /* ... and their tail points per (row, strip) (stream mode only) */
    int32_t *cm_par = nullptr;   /* firing-order frames: direction and row bases (k_probe) */
    uint32_t *cm_sync = nullptr; /* ... and what their strips tell each other and k_verdict about column 0 */
    uint32_t *winner = nullptr;
    uint32_t win_gen = 0; /* generation tag of the last sub-batch that used this set's winner table */
    uint2 *cand = nullptr; /* candidate key | height */
    uint32_t *ncand = nullptr;
    uint32_t *code_main = nullptr, *ncode = nullptr; /* per-(strip, band) lists of final BEV codes */
    float *avg = nullptr;
    int8_t *gm = nullptr; /* lazily allocated */
};

/* Device -> host side of bev_process_batch.  Copies into pageable host memory block the calling thread, so the
 * downloads of chunk k run on their own thread and stream while the main thread uploads and launches chunk k + 1:
 * PCIe is used in both directions at once.  The thread lives as long as the context (it used to be created and joined
 * by every call). */
struct Downloader {
    struct Task {
        int f0, nb, half;
        bev_point_t *const *ordered_out;
        uint8_t *const *multi_out;
        uint8_t *const *single_out;
        int8_t *const *gm_out;
        int half_frames;
    };
    bev_ctx *c = nullptr;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Task> queue;
    bool closing = false;
    int finished = 0; /* chunks of the current call whose outputs are in the caller's buffers */
    hipError_t err = hipSuccess;
    std::thread th;

    void run();
    void start(bev_ctx *ctx)
    {
        c = ctx;
        th = std::thread([this] { run(); });
    }
    void begin_call()
    {
        std::lock_guard<std::mutex> lk(mu);
        finished = 0;
        err = hipSuccess;
    }
    void push(Task t)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            queue.push_back(t);
        }
        cv.notify_all();
    }
    void wait_finished(int n)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return finished >= n; });
    }
    void close()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            closing = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};

/* ---- what the batched entry points keep between calls (defined in bev_capi.hip; used by all seven files) ---- */
/* a device buffer that grows when a call needs more */
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint64_t uses = 0; /* calls of grow: every call that lays the buffer out anew (GridRecord) */
    int grow(bev_ctx *c, size_t need); /* (waits for the context's stream first: the last call's kernels may still use it) */
    void release();
};
/* a pinned host block and its device copy: begin() waits until the last call's table has gone up, grows both blocks to
 * max(bytes, min_cap) where they are smaller and returns the host block to fill; push() sends it up the context's stream */
struct UploadTable {
    void *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int begin(bev_ctx *c, size_t bytes, size_t min_cap, void **host_out);
    int push(bev_ctx *c, size_t bytes);
    void release();
};
struct RegState {
    /* front end (bev_registration_front_device_resident & co.): one allocation on first use, max_batch frames of
     * max(max_points, S) points; the offsets of packed clouds go up through rf_offs */
    DevBuf rf_buf;
    RfWork rf{};
    float *rf_nrm = nullptr; /* P pcl::Normal records: bev_normals_2d's output */
    UploadTable rf_offs;
    /* coarse ICP (bev_coarse_registration_device_resident & co.): the grids and the transformed clouds; the problem tables;
     * bev_icp_point_to_plane's two clouds, their counts and the result */
    DevBuf icp_buf, icp_one;
    UploadTable icp_tab;
    /* fine stage (bev_fine_registration_device_resident & co.): the voxel clouds, grids and transformed clouds; the host
     * clouds of the per-cloud entries; the slot and problem tables */
    DevBuf fine_buf, fine_in;
    UploadTable fine_tab;
    /* scan-to-map fine ICP (bev_submap_registration_device_resident & co.) works in fine_buf and sends its plan
     * up fine_tab; sub_res: the results of bev_submap_registration_batch on the device */
    DevBuf sub_res;
    /* verification of registered matches (bev_capi_verify.hip) voxelises and builds its targets in fine_buf like
     * the fine calls; verify_buf: the moved queries and their grids of a launch group; verify_tab: the matches' table; verify_io:
     * what the host-buffer forms keep on the device (the transforms going in, the records coming out) */
    DevBuf verify_buf, verify_io;
    UploadTable verify_tab;
    /* Recorded on the context's stream behind the last batched registration call (front end, coarse, fine): the next BEV
     * call's stage streams wait for it.  One event serves all three: they record on the same stream, so the latest record
     * covers the earlier ones. */
    hipEvent_t tail_ev = nullptr;
    bool tail_pending = false;
    void release();
};

/* what bev_debug_get_submap_grid and bev_debug_get_pair_grid read (grid_record_read, bev_reg_host.h): the search grids that
 * the last call of a stage left in the stage's workspace.  An item is a map of the call's last launch group (scan-to-map) or a
 * match of the call (pair).  Each hook has its own rule for a record gone stale: scan-to-map holds while the workspace has not
 * moved (buf: its address then); pair while no later call has laid the buffer out (uses: DevBuf::uses behind the call's grow) */
struct GridRecord {
    const IcpGridHdr *hdr = nullptr;
    const uint32_t *cell_off = nullptr;
    struct Item {
        uint64_t hdr;   /* its header's index behind hdr */
        uint64_t off0;  /* its first offset word behind cell_off */
        uint64_t cells; /* the cells its offsets have room for */
    };
    std::vector<Item> items;
    const void *buf = nullptr;
    uint64_t uses = 0;
};

} // namespace bevh

struct bev_ctx {
    int device = -1;
    bev_params_t params{};
    bevk::Geometry geo{};
    int max_batch = 0;
    size_t max_points = 0;
    int win_shift = 32;  /* bits an input index + 1 needs; the rest of a winner entry is the generation tag */
    size_t multi_bytes = 0, single_bytes = 0;
    hipStream_t stream = nullptr;

    /* sub-batch workspace sets; the aliases below are lane 0's */
    bevh::Lane lanes[bevh::kMaxLanes];
    int n_lanes = 8; /* 4 * n_stage_streams */
    /* fused launches alternate between two streams: sub-batch s on stage_st[s % 2], its workspace set s % 8 (always the
     * same stream's), its later stages in that stream's next three launches — a launch's tail is filled by the other
     * stream's launch, and nothing but the order of launches on ONE stream ever orders two stages of one sub-batch */
    hipStream_t stage_st[bevh::kMaxStageStreams] = {};
    hipEvent_t stage_ev[bevh::kMaxStageStreams] = {};
    hipEvent_t fork_ev = nullptr, null_ev = nullptr;
    int n_stage_streams = 2;   /* BEV_STAGE_STREAMS=1 .. 4 (1: a launch's tail stands empty; 3, 4: measured like 2, with 12 / 16 workspace sets) */
    unsigned sub_seq = 0;      /* sub-batches so far */
    /* fused: a sub-batch's stages ride in consecutive k_stage launches beside the stages of its neighbours (run_pipeline);
     * serial (BEV_LANES=1, bev_set_lanes(ctx, 1)): every kernel a launch of its own, back to back — per-kernel durations */
    bool fused = true;
    int stage_lead = 0;        /* group slots by which a launch's walk workgroups precede its other stages' (0, 4, 12, 24, 32 measured the same) */
    uint32_t *hint = nullptr;  /* mapped host words (k_verdict): [0] frames of the last verdict's sub-batch that were NOT read in place, [1] the modes k_probe gave its frames (bit = mode) */
    int mode_absent[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* looks at hint[1] since it last showed the mode (see run_pipeline) */
    int mode_ttl = 8;          /* a mode's in-place walk stays launched for this many sub-batches after a verdict last showed the mode (BEV_MODE_TTL) */
    int layout_hint = 0;       /* bev_set_layout_hint: 0, kFrameStructured or kFrameColMajor */
    bool allow_stream = true;  /* sorted-prefix frames are read in place (k_probe); BEV_STREAM=0 turns it off, see bev_create */
    /* sub-batches whose later stages have not been launched yet, oldest first (see run_pipeline / flush_pending) */
    struct Pending {
        bevk::BatchPtrs b;
        int nf;
        bool want_multi, want_single;
        int8_t *gm_out; /* final ground_mat wanted (device), or nullptr */
        int next;       /* 1 phase B, 2 phase C, 3 rasters */
        int q;          /* which of the two streams its stages ride on */
    };
    std::deque<Pending> pending;
    uint32_t *winner = nullptr;
    uint32_t *codes = nullptr;
    size_t codes_elems = 0;
    uint32_t *ctx_tab = nullptr; /* per-context tables (BatchPtrs::ctx_tab) */
    float *last_avg = nullptr;
    uint32_t *last_ncode = nullptr;
    bevk::FrameInfo *last_info = nullptr;

    /* frame descriptors: ring of pinned host + device arrays */
    bevk::FrameDesc *h_desc[bevh::kDescRing] = {nullptr, nullptr, nullptr, nullptr};
    bevk::FrameDesc *d_desc[bevh::kDescRing] = {nullptr, nullptr, nullptr, nullptr}; /* the device's address of h_desc (mapped host memory) */
    size_t desc_cap[bevh::kDescRing] = {0, 0, 0, 0};
    hipEvent_t desc_done[bevh::kDescRing]{};
    bool desc_used[bevh::kDescRing] = {false, false, false, false};
    int desc_next = 0;

    /* staging for the host-buffer entry points (lazily allocated) */
    bev_point_t *st_in = nullptr;
    size_t st_in_elems = 0;
    bev_point_t *st_ordered = nullptr;
    uint8_t *st_multi = nullptr, *st_single = nullptr;
    int8_t *st_gm = nullptr;
    bool staging_ready = false;
    hipStream_t dl_stream = nullptr;             /* device -> host copies of bev_process_batch (own host thread) */
    bevh::Downloader *downloader = nullptr;            /* that thread, started with the staging buffers */
    hipEvent_t out_ready[2] = {nullptr, nullptr}; /* per half of the output staging: its chunk has been computed */
    /* projection of raw returns (project_frames, bev_capi_packed.hip): the frame table of a call; the KITTI workspace of one launch
     * group, allocated on first use and grown on demand; the raw staging of bev_process_batch_xyzi (lazily allocated) */
    bevh::UploadTable proj_tab;
    bevh::DevBuf kitti_ws;
    int kitti_group = bevk::kKittiGroup; /* BEV_PROJECT_GROUP=1 .. 64 (tests: results do not depend on it) */
    float *st_raw = nullptr;
    /* float BEV of a batch (float_bev_frames, bev_capi_packed.hip): the frame and pose table of a call; the grids of
     * bev_float_bev_batch's chunks (and of bev_submap_float_bev_batch's: both calls are synchronous), allocated on first use and
     * grown on demand */
    bevh::UploadTable manip_tab;
    bevh::DevBuf manip_grids;
    /* 24-layer and uint8 BEVs of a batch under per-frame poses (posed_bev_frames, bev_capi_packed.hip): the frame and pose table of
     * a call; the planes of one launch group; the images of bev_posed_bev_batch's chunks; all allocated on first use and
     * grown on demand */
    bevh::UploadTable posed_tab;
    bevh::DevBuf posed_ws, posed_imgs;
    /* ... of submaps (TablesUp, bev_packed_host.h; bev_capi_packed.hip): the plan of a call; the planes are posed_ws, the images of
     * bev_submap_bev_batch's chunks posed_imgs (both host-buffer calls are synchronous).  The float submap calls
     * (submap_float_frames) send their plan up the same table and have no planes: their output is the accumulator */
    bevh::UploadTable submap_tab;
    size_t submap_reg_group = 0; /* BEV_SUBMAP_REG_GROUP=<bytes>: the cap of a launch group of bev_submap_registration_* (tests: results do not depend on it); 0: kSubmapRegCap */
    /* bev_set_submap_search_grid: the cap of cells per axis of the maps' search grids, fine and coarse stage;
     * 0: the one-workgroup grids of 128 x 128 and 64 x 64 cells at most.  [0] fine, [1] coarse, as the records of the hook */
    int submap_grid_cap[2] = {0, 0};
    bevh::GridRecord submap_grid_rec[2];
    /* bev_set_pair_search_grid: the same for the pair calls' targets; neither setter reads the other's state */
    int pair_grid_cap[2] = {0, 0};
    bevh::GridRecord pair_grid_rec[2];
    /* place retrieval (bev_capi_place.hip): the frame table or plan and the ring edges of a descriptor call, the
     * limits of a match call; the descriptors' planes; the pairs of a group of queries; what bev_place_retrieval_batch keeps on
     * the device (unit records, hits); all allocated on first use and grown on demand */
    bevh::UploadTable place_tab, place_lim;
    bevh::DevBuf place_planes, place_pairs, place_out;
    /* translation guess of retrieved pairs (bev_capi_align.hip): the frame table or plan of a grid call, the
     * hits of a hits call; the grids' planes; the hypotheses of a launch group; what bev_align_batch keeps on the device (the
     * clouds, the grids, the records coming out); all allocated on first use and grown on demand */
    bevh::UploadTable align_tab, align_hits;
    bevh::DevBuf align_planes, align_hyp, align_io;
    int posed_group = 0; /* BEV_POSED_GROUP=1 .. 65535: grids per launch group (tests: results do not depend on it); 0: what fits kPosedWsCap */

    bevh::RegState reg;

    /* profiling */
    bool prof_on = false;
    std::vector<bevh::ProfSlot> prof_pool;
    size_t prof_used = 0;
    double prof_ms[bevk::K_COUNT]{};
    uint64_t prof_launches[bevk::K_COUNT]{};
    uint64_t prof_frames[bevk::K_COUNT]{};

    int last_sub_frames = 0;
    std::string last_error;
};

namespace bevh {

/* (file: __FILE__ of the caller) */
int hip_fail(bev_ctx *c, hipError_t e, const char *what, int line, const char *file = "bev_capi.hip");
#define HIPCK(ctx, expr)                                                             \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) return bevh::hip_fail((ctx), e_, #expr, __LINE__, __FILE__); \
    } while (0)

/* a kernel's events where profiling is on (bev_profile_enable) */
struct ProfScope {
    bev_ctx *c;
    ProfSlot *s = nullptr;
    hipStream_t st;
    ProfScope(bev_ctx *ctx, int kid, int frames, hipStream_t stream = nullptr);
    ~ProfScope();
};

/* the most points a cloud may have in every call but the pipeline's own (which take max_points): a structured cloud of S
 * records always fits */
inline size_t cloud_cap(const bev_ctx *c) { return std::max(c->max_points, (size_t)c->geo.S); }

/* launches what is left of every pending sub-batch, then joins the stage streams into the context's stream */
int flush_pending(bev_ctx *c);
/* How every entry point outside the fused pipeline begins, behind its argument checks: the calling thread's device;
 * flush_pending (the later stages of sub-batches still in flight use the workspace the call is about to use, and the call's
 * work on the context's stream comes behind theirs); staging: the staging buffers of the host-buffer calls (ensure_staging). */
int begin_call(bev_ctx *c, bool staging);
/* device pointers from the caller: whatever it has queued on the default stream up to now (the upload or the fill of these
 * very buffers, typically) comes before what the context's stream is given next */
int wait_default_stream(bev_ctx *c);
/* behind an asynchronous call on the context's stream (batched registration, projection): the next BEV call's stage streams
 * wait for it (run_pipeline) */
int record_tail(bev_ctx *c);
int ensure_staging(bev_ctx *c);
/* of the packed-frame calls (bev_capi_packed.hip), for bev_process_batch_xyzi as well: a BEV_PROJECT_* value; the projection */
inline bool project_kind_ok(int kind)
{
    return kind == BEV_PROJECT_MULRAN_OS1_64 || kind == BEV_PROJECT_OXFORD_HDL_32E || kind == BEV_PROJECT_KITTI_HDL_64E;
}
int project_frames(bev_ctx *c, int kind, int nf, const float *d_xyzi, const uint64_t *offs, bev_point_t *d_out);
/* What the submap entry points check of the maps (bev_capi_packed.hip): BEV_OK, or what the entry point returns.  The entry
 * arrays are read only when their length has passed. */
int check_submap_entries(int n_frames, int n_maps, const uint64_t *map_offs, const int32_t *entry_frame, const float *entry_pose);

/* ---- what the calls over packed frames share across files (more of it, over maps: bev_packed_host.h) ---- */
/* the arguments every call over packed frames of the caller's has: BEV_OK, or what the entry point returns */
inline int check_packed_frames(const bev_ctx *c, int n_frames, const uint64_t *h_offsets)
{
    if (!c || n_frames < 0 || !h_offsets) return BEV_ERR_INVALID_ARG;
    const uint64_t cap = cloud_cap(c);
    for (int f = 0; f < n_frames; ++f)
        if (h_offsets[f + 1] < h_offsets[f]) return BEV_ERR_INVALID_ARG;
    for (int f = 0; f < n_frames; ++f)
        if (h_offsets[f + 1] - h_offsets[f] > cap) return BEV_ERR_TOO_LARGE;
    return BEV_OK;
}
/* ... and the calls over host clouds: their arrays */
inline bool host_clouds_ok(int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts)
{
    if (n_frames > 0 && (!clouds || !n_pts)) return false;
    for (int f = 0; f < n_frames; ++f)
        if (n_pts[f] && !clouds[f]) return false;
    return true;
}
/* A call on packed frames in device memory of the caller's: asynchronous, on the context's stream.  flush_pending joins the
 * stage streams into it, so a BEV call that still reads or writes the caller's buffers (a bev_process_device_resident whose
 * d_ordered this call reads, say) has launched all its stages and comes first; then whatever the caller has queued on the
 * default stream (the upload or the fill of its input, typically); then the body; and the stage streams of the next BEV call
 * wait for what record_tail records: it may read this call's output, or overwrite its input, at once. */
template <class Body>
int resident_call(bev_ctx *c, Body body)
{
    int rc = begin_call(c, false);
    if (rc != BEV_OK) return rc;
    rc = wait_default_stream(c);
    if (rc != BEV_OK) return rc;
    rc = body();
    if (rc != BEV_OK) return rc;
    return record_tail(c);
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
/* one allocation in 256-byte aligned pieces: *dst[i] = the piece of sz[i] bytes (base == nullptr: nothing is written);
 * returns the bytes the pieces take */
template <size_t N>
size_t carve(void *base, const size_t (&sz)[N], void **const (&dst)[N])
{
    size_t off = 0;
    for (size_t i = 0; i < N; ++i) {
        if (base) *dst[i] = static_cast<char *>(base) + off;
        off += align256(sz[i]);
    }
    return off;
}

} // namespace bevh
#endif
