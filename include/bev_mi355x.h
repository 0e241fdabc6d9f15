/*
 * bev_mi355x.h — C ABI of the MI355X-native batch_multi_bev_gen hot path.
 *
 * This is the drop-in boundary ("lower face").  The reference
 * (soytony/Point-Cloud-Preprocessing-Tools) has no FFI layer of its own: its
 * hot path is four C++ free functions that read file-scope globals.  Every
 * entry point below names the reference interface it replaces (file:line are
 * relative to the reference tree).  Only POD types and plain pointers cross
 * this boundary; no C++/torch types.
 *
 * Conventions
 *   - return 0 (BEV_OK) on success, a negative bev_status_t otherwise;
 *     nothing throws, nothing calls exit().
 *   - the caller owns every buffer it passes; the context owns its device
 *     workspace, stream and events.
 *   - one context per GPU, used by one host thread at a time.
 *   - there is NO CPU fallback behind this ABI: if no HIP device is usable,
 *     bev_create() fails with BEV_ERR_NO_DEVICE.
 */
#ifndef BEV_MI355X_H
#define BEV_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEV_ABI_VERSION 1

/* Ground-height grid of getBelongingGrid (BatchMultiBevGen.h:73-99,
 * BatchMultiBevGen.cpp:25-26): 75 x 50 cells of 2 m. */
#define BEV_GROUND_GRID_ROWS 75
#define BEV_GROUND_GRID_COLS 50
#define BEV_GROUND_GRID_CELLS (BEV_GROUND_GRID_ROWS * BEV_GROUND_GRID_COLS)

typedef enum bev_status {
    BEV_OK = 0,
    BEV_ERR_INVALID_ARG = -1,
    BEV_ERR_NO_DEVICE = -2,     /* no usable HIP device: there is no CPU path */
    BEV_ERR_HIP = -3,           /* a HIP runtime call failed (see bev_last_error) */
    BEV_ERR_OOM = -4,
    BEV_ERR_UNSUPPORTED = -5,   /* parameter combination outside the built kernels */
    BEV_ERR_TOO_LARGE = -6      /* n_frames / n_points above what bev_create sized */
} bev_status_t;

/* In-memory layout of pcl::PointXYZIRCT (BatchMultiBevGen.h:43-54): 32 bytes,
 * 16-byte aligned; x@0 y@4 z@8 pad@12 intensity@16 row@20 col@22 t@24 label@28. */
typedef struct bev_point {
    float x, y, z, _pad0;
    float intensity;
    uint16_t row, col;
    uint32_t t;
    int16_t label;
    uint16_t _pad1;
} bev_point_t;

/* SensorParams (include/Utility.h:30-36) plus the constants the reference
 * hard-codes in computeAndSaveMultiBev / computeAndSaveSingleBev
 * (BatchMultiBevGen.cpp:266-269,336-338) and main (:738). */
typedef struct bev_params {
    int32_t n_scan;             /* SensorParams::N_SCAN */
    int32_t horizon_scan;       /* SensorParams::Horizon_SCAN */
    int32_t ground_upper_scan;  /* SensorParams::GROUND_UPPER_SCAN */
    float height_res;           /* SensorParams::HEIGHT_RES */
    float interval;             /* 1.0f  (main :738); others if M = (int)(2 * max_range / interval) is a multiple of 16 in
                                 * 16..512 other than 304, 336, 368, 400, 416, 432, 464, 480, 496 (no band of those
                                 * images fits a workgroup's LDS): bev_create returns BEV_ERR_UNSUPPORTED for the rest */
    int32_t max_range;          /* 112   (:266,:336) */
    int32_t n_layers;           /* 24    (:268,:271) */
    float lidar_to_ground;      /* 2.0f  (:269,:338) */
} bev_params_t;

typedef struct bev_ctx bev_ctx_t;

/* parseSensorType + getSensorParams (src/Utility.cpp:72-124) and the BEV
 * defaults above.  `sensor` is matched by substring like the reference
 * ("HDL_32E", "HDL_64E", "OS1_64").  Unknown sensor -> BEV_ERR_INVALID_ARG
 * (the reference leaves the struct uninitialised). */
int bev_params_for_sensor(const char *sensor, bev_params_t *out);

/* Slots of the ordered range image: n_scan * horizon_scan. */
size_t bev_num_slots(const bev_params_t *p);
/* Bytes of one multi-layer BEV (.bin payload, BatchMultiBevGen.cpp:307-314)
 * and of one single-layer BEV (cv::Mat single_bev, :340). */
size_t bev_multi_bytes(const bev_params_t *p);
size_t bev_single_bytes(const bev_params_t *p);

/* Replaces the global state the reference sets up in main()
 * (sensor_params_, four_neighbor_iterator_, BatchMultiBevGen.cpp:29,37,712-719).
 * device        : HIP device ordinal (>= 0).
 * max_batch     : frames processed per internal sub-batch (workspace is sized
 *                 for this many; any n_frames is accepted later and looped).
 * max_points    : largest per-frame input point count that will be passed. */
int bev_create(bev_ctx_t **ctx, int device, const bev_params_t *p,
               int max_batch, size_t max_points);
void bev_destroy(bev_ctx_t *ctx);

const char *bev_strerror(int status);
/* Text of the last HIP error seen by this context ("" if none). */
const char *bev_last_error(const bev_ctx_t *ctx);

/* ---- whole hot path, host buffers ------------------------------------
 * One call = the body of the per-file loop of main()
 * (BatchMultiBevGen.cpp:727-757) for n_frames clouds, minus file I/O:
 *   getOrderedCloud (:94-117) -> markGroundPoints (:119-252)
 *   -> computeAndSaveMultiBev raster (:266-292)
 *   -> computeAndSaveSingleBev raster (:336-356).
 * pts[f]         : n_pts[f] unordered input points of frame f.
 * ordered_out[f] : S points; labelled ordered cloud (what savePCDFileBinary
 *                  writes at :756).
 * multi_out[f]   : n_layers*M*M bytes, layer-major then row(x)-major — the
 *                  exact .bin payload.
 * single_out[f]  : M*M bytes, row(x)-major (cv::Mat single_bev).
 * ground_mat_out : optional (NULL or per-frame NULL allowed); S int8 values,
 *                  the final cv::Mat ground_mat of markGroundPoints. */
int bev_process_batch(bev_ctx_t *ctx, int n_frames,
                      const bev_point_t *const *pts, const uint32_t *n_pts,
                      bev_point_t *const *ordered_out,
                      uint8_t *const *multi_out,
                      uint8_t *const *single_out,
                      int8_t *const *ground_mat_out);

/* ---- whole hot path, device-resident ----------------------------------
 * Same computation, every data pointer is DEVICE memory; nothing crosses
 * PCIe except a few hundred bytes of launch metadata.
 * d_pts        : all frames' input points, packed; frame f occupies
 *                [h_offsets[f], h_offsets[f+1]) (element offsets, HOST array
 *                of n_frames+1 entries).
 * d_ordered    : n_frames * S points.
 * d_multi      : n_frames * bev_multi_bytes.
 * d_single     : n_frames * bev_single_bytes.
 * d_ground_mat : NULL or n_frames * S int8.
 * Asynchronous: call bev_synchronize() before reading results.  The stages of a
 * sub-batch ride in consecutive launches beside the stages of its neighbours
 * (see bev_set_lanes); the last stages of a call's last sub-batches are
 * launched by the NEXT call to this function — calls that follow each other
 * without a synchronisation keep the device busy across the call boundary —
 * or by bev_synchronize() (and by every other entry point of the context).
 * A bare hipDeviceSynchronize() is therefore NOT enough: bev_synchronize()
 * launches what is pending, then waits.  The buffers of a call must stay
 * valid until then.  Work the caller has queued on the DEFAULT stream before
 * the call (an upload or a fill of these buffers) is waited for on the device;
 * work on other streams of the caller's is the caller's to synchronise with:
 * the library's streams are non-blocking. */
int bev_process_device_resident(bev_ctx_t *ctx, int n_frames,
                                const bev_point_t *d_pts,
                                const uint64_t *h_offsets,
                                bev_point_t *d_ordered,
                                uint8_t *d_multi,
                                uint8_t *d_single,
                                int8_t *d_ground_mat);
int bev_synchronize(bev_ctx_t *ctx);

/* Page-locked host memory for the buffers handed to bev_process_batch (optional): copies from / to such memory
 * are DMA transfers without intermediate staging by the runtime.  Any host memory works (on the MI355X boxes
 * measured, pageable buffers reached 6.3 k frames/s and page-locked ones 6.5 k: the link, not the staging, is
 * the limit).  hipHostMalloc / hipHostFree. */
int bev_host_alloc(void **out, size_t bytes);
int bev_host_free(void *p);

/* ---- per-function entry points (host buffers, one cloud) ---------------
 * These let the reference-named C++ free functions be re-implemented as thin
 * callers, one ABI call each. */

/* getOrderedCloud (BatchMultiBevGen.cpp:94-117). out: S points. */
int bev_order_cloud(bev_ctx_t *ctx, const bev_point_t *pts, uint32_t n_pts,
                    bev_point_t *ordered_out);
/* markGroundPoints (BatchMultiBevGen.cpp:119-252). `ordered` holds S points;
 * labels are rewritten in place. ground_mat_out: NULL or S int8. */
int bev_mark_ground(bev_ctx_t *ctx, bev_point_t *ordered, int8_t *ground_mat_out);
/* Raster part of computeAndSaveMultiBev (:266-292) for any cloud of n points
 * (points with label == 0 are skipped). out: bev_multi_bytes. */
int bev_multi_bev(bev_ctx_t *ctx, const bev_point_t *cloud, uint32_t n,
                  uint8_t *multi_out);
/* Raster part of computeAndSaveSingleBev (:336-356). out: bev_single_bytes. */
int bev_single_bev(bev_ctx_t *ctx, const bev_point_t *cloud, uint32_t n,
                   uint8_t *single_out);

/* Float max-height BEV of the older tools: saveAsMat of batch_cloud_manip
 * (BatchCloudManip.cpp:201-225, skip_label0 = 1) and cloud_manip
 * (CloudManip.cpp:79-99, skip_label0 = 0): grid M x M, M = 200/interval + 1,
 * cell = max(0, max over points of z + 2.0f), float32.  out: M*M floats,
 * row index = x.  interval must give M <= 1024.  Bit-exact (a max has no
 * rounding), i.e. well inside the 1e-5 the float height channel is allowed. */
int bev_float_bev(bev_ctx_t *ctx, const bev_point_t *cloud, uint32_t n, float interval,
                  int skip_label0, float *out);
size_t bev_float_bev_size(float interval); /* M for a given interval (0 if unsupported) */

/* The rigid transform of cloud_manip (CloudManip.cpp:119-128, pcl::transformPointCloud with an Eigen::Affine3f):
 * out[i] = cloud[i] with xyz replaced by  col0 * x + (col1 * y + (col2 * z + col3))  of the 3 x 4 row-major
 * matrix m (12 floats) — the association of pcl::detail::Transformer<float>::se3 (PCL >= 1.10); every other field
 * is copied.  bev_yaw_translate_matrix builds the matrix the tool builds from its arguments
 * (translation tx ty tz, then rotate(AngleAxisf(yaw_deg / 180.0f * M_PI, UnitZ()))); host only, no device needed.
 * Eigen / PCL are third-party: restated from their published sources (parity unpinned). */
int bev_transform_cloud(bev_ctx_t *ctx, const bev_point_t *cloud, uint32_t n, const float *m /* 12 */,
                        bev_point_t *out);
void bev_yaw_translate_matrix(float tx, float ty, float tz, float yaw_deg, float *m /* 12 */);

/* The float BEV for a batch of frames in DEVICE memory, each under its own poses: what cloud_manip computes (the rigid
 * transform above, then saveAsMat) without the moved cloud ever being written.  One launch for the whole call, asynchronous
 * like bev_project_device_resident.
 * d_clouds  : frame f = records [h_offsets[f], h_offsets[f+1]) of d_clouds; h_offsets: HOST array of n_frames + 1 entries,
 *             non-decreasing.  With offsets f * S this is the d_ordered of bev_process_device_resident.
 * h_poses   : HOST array of n_frames * n_poses * 12 floats, frame f's pose k the row-major 3 x 4 matrix (what
 *             bev_yaw_translate_matrix builds) at (f * n_poses + k) * 12; NULL when n_poses == 0: the raw coordinates are
 *             rastered (NOT the same as an identity matrix: 0 * inf is NaN, and -0.0 becomes +0.0).
 * d_out     : n_frames * max(1, n_poses) grids of M * M floats, M = bev_float_bev_size(interval), row index = x; frame f's
 *             pose k is grid f * max(1, n_poses) + k and equals bev_float_bev(bev_transform_cloud(frame f, pose k)).  The
 *             call zeroes every grid itself (an empty frame gives an all-zero grid) and writes nothing else.  The host
 *             arrays may be reused as soon as the call returns.
 * Ordering  : a BEV call of this context issued before it (a bev_process_device_resident whose d_ordered it reads) is
 *             finished first; work queued on the DEFAULT stream before the call is waited for on the device; a BEV call
 *             issued right after it, which may overwrite d_clouds, waits for it.  bev_synchronize() before the host reads
 *             d_out.
 * Status    : BEV_ERR_INVALID_ARG for n_frames < 0, NULL or decreasing offsets, n_poses < 0 or > BEV_FLOAT_BEV_MAX_POSES,
 *             n_poses > 0 with NULL h_poses, a NULL data pointer with work to do; BEV_ERR_UNSUPPORTED when
 *             bev_float_bev_size(interval) == 0; BEV_ERR_TOO_LARGE for a frame of more than max(max_points, S) records;
 *             nothing is launched and d_out is untouched in every case.  n_frames == 0 returns BEV_OK.
 * Workspace : a table of 16 * (n_frames + 1) + 48 * n_frames * n_poses bytes, freed by bev_destroy. */
#define BEV_FLOAT_BEV_MAX_POSES 64
int bev_float_bev_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                  float interval, int skip_label0, int n_poses, const float *h_poses, float *d_out);
/* The same through HOST buffers, synchronous like bev_process_batch: clouds[f] holds n_pts[f] records (at most
 * max(max_points, S)), out[f] receives max(1, n_poses) * M * M floats.  The frames go up in chunks of max_batch through the
 * context's input staging; the chunks' grids live in a device buffer of the context that is allocated on first use, grown
 * when a call needs more and freed by bev_destroy. */
int bev_float_bev_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                        float interval, int skip_label0, int n_poses, const float *h_poses, float *const *out);

/* The 24-layer occupancy BEV and the uint8 max-height BEV (bev_multi_bev, bev_single_bev) for a batch of frames in DEVICE
 * memory, each under its own poses, without the moved clouds ever being written.  Asynchronous like
 * bev_float_bev_device_resident; the sensor and the grid are the context's (height_res, interval, max_range, n_layers).
 * d_clouds  : frame f = records [h_offsets[f], h_offsets[f+1]) of d_clouds; h_offsets: HOST array of n_frames + 1 entries,
 *             non-decreasing.  With offsets f * S this is the d_ordered of bev_process_device_resident.
 * h_poses   : HOST array of n_frames * n_poses * 12 floats, frame f's pose k the row-major 3 x 4 matrix (what
 *             bev_yaw_translate_matrix builds) at (f * n_poses + k) * 12; NULL when n_poses == 0: the raw coordinates are
 *             rastered (NOT the same as an identity matrix), and on d_ordered the images are exactly what
 *             bev_process_device_resident wrote to its own d_multi / d_single.
 * d_multi   : n_frames * max(1, n_poses) images of bev_multi_bytes, or NULL: not wanted.
 * d_single  : as many images of bev_single_bytes, or NULL: not wanted (not both).  Frame f's pose k is image
 *             f * max(1, n_poses) + k of either and equals bev_multi_bev / bev_single_bev of bev_transform_cloud(frame f,
 *             pose k) byte for byte.  Every byte of a wanted image is written (an empty frame gives all-zero images), nothing
 *             else is.  The host arrays may be reused as soon as the call returns.
 * Ordering  : as for bev_float_bev_device_resident: a BEV call of this context issued before it is finished first; work
 *             queued on the DEFAULT stream before the call is waited for on the device; a BEV call issued right after it,
 *             which may overwrite d_clouds, waits for it.  bev_synchronize() before the host reads the images.
 * Status    : BEV_ERR_INVALID_ARG for n_frames < 0, NULL or decreasing offsets, n_poses < 0 or > BEV_POSED_BEV_MAX_POSES,
 *             n_poses > 0 with NULL h_poses, d_multi and d_single both NULL, NULL d_clouds with records to read;
 *             BEV_ERR_TOO_LARGE for a frame of more than max(max_points, S) records; nothing is launched and the outputs are
 *             untouched in every case.  n_frames == 0 returns BEV_OK.
 * Workspace : the table of the float call, and two planes of M * M words per grid (8 * M * M bytes) for one launch group:
 *             the call is cut into groups of consecutive whole frames whose grids fit 256 MiB (BEV_POSED_GROUP=<grids>,
 *             1 .. 65535, in the environment of bev_create sets the cap in grids instead; results do not depend on it); a
 *             frame is never split: one whose poses alone exceed the cap is a group of its own.  Freed by bev_destroy. */
#define BEV_POSED_BEV_MAX_POSES 64
int bev_posed_bev_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                  int n_poses, const float *h_poses, uint8_t *d_multi, uint8_t *d_single);
/* The same through HOST buffers, synchronous like bev_float_bev_batch: clouds[f] holds n_pts[f] records (at most
 * max(max_points, S)); multi_out[f] receives max(1, n_poses) images of bev_multi_bytes, single_out[f] as many of
 * bev_single_bytes; a NULL array: not wanted (not both).  The frames go up in chunks of max_batch through the context's input
 * staging; the chunks' images live in a device buffer of the context that is allocated on first use, grown when a call
 * needs more and freed by bev_destroy. */
int bev_posed_bev_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                        int n_poses, const float *h_poses, uint8_t *const *multi_out, uint8_t *const *single_out);

/* The same two images of SUBMAPS: map g is a list of (frame, pose) entries, and its images are those of all its entries' moved
 * clouds together in ONE grid — bev_multi_bev / bev_single_bev of the concatenation of bev_transform_cloud(frame, pose) over
 * the map's entries, byte for byte (both rasters are idempotent stores and a maximum: the order of the entries does not
 * matter).  A local map around a key frame is the typical use: the key frame's neighbours, each under its pose relative to
 * the key frame.  Asynchronous like bev_posed_bev_device_resident.
 * d_clouds      : frames as for bev_posed_bev_device_resident: frame f = records [h_offsets[f], h_offsets[f+1]).
 * h_map_offsets : HOST array of n_maps + 1 entries, non-decreasing: map g owns entries [h_map_offsets[g], h_map_offsets[g+1])
 *                 of the two entry arrays (which are indexed from 0: h_map_offsets[0] is normally 0).
 * h_entry_frame : HOST array: the frame entry e names, 0 .. n_frames - 1.
 * h_entry_pose  : HOST array of 12 floats per entry: its row-major 3 x 4 matrix.  Every entry has one; the identity is
 *                 bev_yaw_translate_matrix(0, 0, 0, 0) (on finite clouds it gives the raw cloud's images).
 *                 A frame may feed any number of maps, appear several times in one map, or be named by none (it then costs no
 *                 workgroup); a map without entries gives all-zero images.  Only the call's total of entries is bounded:
 *                 BEV_SUBMAP_MAX_ENTRIES.
 * d_multi       : n_maps images of bev_multi_bytes, or NULL: not wanted.
 * d_single      : n_maps images of bev_single_bytes, or NULL: not wanted (not both).  Every byte of a wanted image is written,
 *                 nothing else is.  The host arrays may be reused as soon as the call returns.
 * Ordering      : as for bev_posed_bev_device_resident.
 * Status        : BEV_ERR_INVALID_ARG for a NULL context, n_frames < 0, n_maps < 0, NULL or decreasing h_offsets or
 *                 h_map_offsets, entries with a NULL entry array, an entry frame outside 0 .. n_frames - 1, d_multi and
 *                 d_single both NULL while n_maps > 0, NULL d_clouds while an entry names a frame that has records;
 *                 BEV_ERR_TOO_LARGE for a frame of more than max(max_points, S) records or more than BEV_SUBMAP_MAX_ENTRIES
 *                 entries (checked before the entry arrays are read); nothing is launched and the outputs are untouched in
 *                 every case.  n_maps == 0 returns BEV_OK.
 * Workspace     : the planes of the posed call, one grid per map of a launch group: the call is cut into groups of consecutive
 *                 maps that fit the same cap (256 MiB, or BEV_POSED_GROUP=<grids>; results do not depend on it), and per
 *                 group a table of 20 bytes per distinct frame of the group and 64 bytes per entry.  Freed by bev_destroy. */
#define BEV_SUBMAP_MAX_ENTRIES (1u << 20)   /* entries of one call */
int bev_submap_bev_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                   int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                   const float *h_entry_pose, uint8_t *d_multi, uint8_t *d_single);
/* The same through HOST buffers, synchronous and argument-checked like bev_posed_bev_batch: clouds[f] holds n_pts[f] records
 * (at most max(max_points, S)); multi_out[g] receives map g's image of bev_multi_bytes, single_out[g] its image of
 * bev_single_bytes; a NULL array: not wanted (not both).  The maps go in chunks of at most max_batch maps (and never more than
 * a launch group); the distinct frames a chunk names go up through the context's input staging max_batch at a time, each such
 * piece rastered into the chunk's planes before the next goes up, so a map may name more distinct frames than max_batch. */
int bev_submap_bev_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                         int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                         const float *h_entry_pose, uint8_t *const *multi_out, uint8_t *const *single_out);

/* The float max-height BEV (bev_float_bev, the "saveAsMat" grid) of SUBMAPS: map g is a list of (frame, pose) entries as for
 * bev_submap_bev_device_resident, and its grid is that of all its entries' moved clouds together — bev_float_bev of the
 * concatenation of bev_transform_cloud(frame, pose) over the map's entries, bit for bit (a maximum has no rounding and no
 * order).  Asynchronous like bev_float_bev_device_resident; ONE launch for the whole call.
 * d_clouds, h_map_offsets, h_entry_frame, h_entry_pose : exactly as for bev_submap_bev_device_resident: every entry has a
 *                 matrix; a frame may feed any number of maps, appear several times in one map, or be named by none (it then
 *                 costs no workgroup); the call's total of entries is bounded by BEV_SUBMAP_MAX_ENTRIES.
 * interval, skip_label0 : as for bev_float_bev.
 * d_out         : n_maps grids of M * M floats, M = bev_float_bev_size(interval), row index = x; map g's grid is grid g.  The
 *                 call zeroes every grid itself (a map without entries gives an all-zero grid) and accumulates in place:
 *                 every float of every grid is written, nothing else is.  The host arrays may be reused as soon as the call
 *                 returns.
 * Ordering      : as for bev_float_bev_device_resident: a BEV call of this context issued before it is finished first; work
 *                 queued on the DEFAULT stream before the call is waited for on the device; a BEV call issued right after it
 *                 waits for it.  bev_synchronize() before the host reads d_out.
 * Status        : the submap statuses: BEV_ERR_INVALID_ARG for a NULL context, n_frames < 0, n_maps < 0, NULL or decreasing
 *                 h_offsets or h_map_offsets, entries with a NULL entry array, an entry frame outside 0 .. n_frames - 1;
 *                 BEV_ERR_TOO_LARGE for more than BEV_SUBMAP_MAX_ENTRIES entries (checked before the entry arrays are read);
 *                 then BEV_ERR_UNSUPPORTED when bev_float_bev_size(interval) == 0; then BEV_ERR_TOO_LARGE for a frame of more
 *                 than max(max_points, S) records; then BEV_ERR_INVALID_ARG for NULL d_out while n_maps > 0 and for NULL
 *                 d_clouds while an entry names a frame that has records.  Nothing is launched and d_out is untouched in
 *                 every case.  n_maps == 0 returns BEV_OK.
 * Workspace     : no planes (the output is the accumulator): a table of 20 bytes per distinct named frame and 64 bytes per
 *                 entry, shared with bev_submap_bev_device_resident.  Freed by bev_destroy. */
int bev_submap_float_bev_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                         float interval, int skip_label0, int n_maps, const uint64_t *h_map_offsets,
                                         const int32_t *h_entry_frame, const float *h_entry_pose, float *d_out);
/* The same through HOST buffers, synchronous and argument-checked like bev_submap_bev_batch: clouds[f] holds n_pts[f] records
 * (at most max(max_points, S)); out[g] receives map g's M * M floats (NULL out while n_maps > 0, or a NULL out[g]:
 * BEV_ERR_INVALID_ARG).  The maps go in chunks of at most max_batch maps; the distinct frames a chunk names go up through the
 * context's input staging max_batch at a time, each such piece rastered into the chunk's grids before the next goes up, so a
 * map may name more distinct frames than max_batch.  The chunk's grids live in the device buffer of bev_float_bev_batch. */
int bev_submap_float_bev_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                               float interval, int skip_label0, int n_maps, const uint64_t *h_map_offsets,
                               const int32_t *h_entry_frame, const float *h_entry_pose, float *const *out);

/* Range-image projection of raw XYZI returns — the selectors' row / col assignment ("polar binning"):
 *   BEV_PROJECT_MULRAN_OS1_64   extractPointCloud, MulranPointCloudSelect.cpp:112-130:
 *                               xyzi = n * (x, y, z, intensity); row = k % 64, col from the azimuth (0..1024)
 *   BEV_PROJECT_OXFORD_HDL_32E  extractPointCloud, OxfordPointCloudSelect.cpp:172-218:
 *                               xyzi = x[n] y[n] z[n] intensity[n]; x and z are negated, row from the
 *                               elevation (0..31), col from the azimuth (0..1055)
 *   BEV_PROJECT_KITTI_HDL_64E   extractPointCloud, KittiPointCloudSelect.cpp:186-243 (after the file is read):
 *                               xyzi = n * (x, y, z, intensity); row = a counter of azimuth zero crossings (a new
 *                               ring needs more than 2083 * 0.60f points on the current one), col from the azimuth
 *                               (0..2082); out is the reference's STRUCTURED cloud of 64 * 2083 points, last
 *                               writer per slot, real points with intensity = -1, empty slots all-zero.  Point 0
 *                               is never stored (the reference's loop starts at 1).  n = 0 and NaN azimuths are
 *                               undefined behaviour in the reference; here: all-zero cloud / point dropped.
 * out: bev_project_out_points(kind, n) points (n, or 64 * 2083 for KITTI) with label = -2; t and padding are 0
 * (the reference leaves them uninitialised).  atan2f is evaluated on the device by a restatement of glibc's
 * algorithm (bit-identical, csrc/bev_libm.h). */
#define BEV_PROJECT_MULRAN_OS1_64 0
#define BEV_PROJECT_OXFORD_HDL_32E 1
#define BEV_PROJECT_KITTI_HDL_64E 2
int bev_project_xyzi(bev_ctx_t *ctx, int kind, const float *xyzi, uint32_t n, bev_point_t *out);
size_t bev_project_out_points(int kind, uint32_t n); /* 0 for an unknown kind */

/* The same projection for a batch of frames in DEVICE memory, asynchronous like bev_process_device_resident: what it writes
 * is what that call reads.
 * d_xyzi    : frames' raw returns, packed: frame f = returns [h_offsets[f], h_offsets[f+1]) of d_xyzi (16 bytes per return;
 *             Oxford: SoA inside the frame, x[n] y[n] z[n] intensity[n] from float 4 * h_offsets[f]).  h_offsets: HOST
 *             array of n_frames + 1 entries, non-decreasing.
 * d_out     : kinds 0 / 1: frame f's records at the same offsets (the same h_offsets array then serves
 *             bev_process_device_resident); MulRan's row = k % 64 counts k within the frame.  KITTI: frame f's structured
 *             cloud at f * 64 * 2083 (offsets f * 64 * 2083 for bev_process_device_resident; the call sets the structured
 *             layout hint, see bev_set_layout_hint).  bev_project_batch_out_points (host only) is the number of records
 *             d_out must hold: h_offsets[n_frames], or n_frames * 64 * 2083; 0 for an unknown kind or decreasing offsets.
 *             d_xyzi and d_out must not overlap.
 * Ordering  : work the caller has queued on the DEFAULT stream before the call (the upload or the fill of d_xyzi) is waited
 *             for on the device; a BEV call of this context issued before it, which may still read d_out, is finished
 *             first; a bev_process_device_resident issued right after it, with no synchronisation between, reads finished
 *             records.  bev_synchronize() before the host reads d_out.
 * Status    : BEV_ERR_INVALID_ARG for an unknown kind, decreasing offsets or a NULL pointer with work to do;
 *             BEV_ERR_TOO_LARGE for a frame of more than max(max_points, S) returns; nothing is launched in either case.
 * Workspace : kinds 0 / 1: a table of 16 * (n_frames + 1) bytes.  KITTI: the frames go through the four steps in launch
 *             groups of BEV_PROJECT_KITTI_GROUP; the group's workspace, allocated on first use, grown when a call needs more
 *             and freed by bev_destroy, is G * (288 + 4 * n_max + 516 * ceil(n_max / 256) + 4 * 64 * 2083) bytes (pieces
 *             rounded up to 256) for G = min(group, n_frames) and n_max the call's longest frame: 21 MB for 120 k-return
 *             sweeps.  Results do not depend on the group size. */
#define BEV_PROJECT_KITTI_GROUP 16
int bev_project_device_resident(bev_ctx_t *ctx, int kind, int n_frames, const float *d_xyzi,
                                const uint64_t *h_offsets, bev_point_t *d_out);
size_t bev_project_batch_out_points(int kind, int n_frames, const uint64_t *h_offsets);   /* host only */
/* bev_process_batch on raw returns: xyzi[f] holds n_returns[f] returns of `kind` (HOST memory, 16 bytes per return); they go
 * up as they are, are projected on the device and enter the pipeline there; the outputs are those of bev_process_batch on
 * the projected clouds.  The kind must be the context's sensor — MulRan: 64 x 1024, Oxford: 32 x 1056, KITTI: 64 x 2083 —
 * or the call returns BEV_ERR_UNSUPPORTED.  n_returns[f] <= max_points (KITTI: <= max(max_points, S), and max_points >= S). */
int bev_process_batch_xyzi(bev_ctx_t *ctx, int kind, int n_frames, const float *const *xyzi, const uint32_t *n_returns,
                           bev_point_t *const *ordered_out, uint8_t *const *multi_out, uint8_t *const *single_out,
                           int8_t *const *ground_mat_out);

/* ---- registration front end ----------------------------------------------------------------------------------------
 * What the reference's registration tools (top_part_registration, batch_top_part_registration, batch_whole_registration)
 * do to every cloud before ICP.  The contract — restated from PCL / FLANN / Eigen's published sources, parity with the
 * reference UNPINNED, the points the reference leaves open fixed — is DESIGN.md "Registration front end".  Layouts:
 * PointXYZ = 4 floats (x y z pad), pcl::Normal = 8 floats (nx ny nz pad curvature pad pad pad), pcl::PointNormal = 12
 * floats (x y z pad nx ny nz pad curvature pad pad pad); every pad the library writes is 0, every NaN it writes is
 * 0x7fc00000.  Clouds of up to max(max_points, S) points (bev_create); each entry first launches whatever the BEV path
 * has pending. */

/* extractTopAndFlatten (TopPartRegistration.cpp:79-136 = BatchTopPartRegistration.cpp:90-147 =
 * BatchWholeRegistration.cpp:90-147): label-0 and non-finite points are skipped; cell gx = round((x + 100) / 20), gy the
 * same from y, 0 <= gx, gy < 10; a cell of >= 20 points emits its round(0.2f * n) highest points (equal z: lower index
 * first) as (x, y, 0), cells in gx-major order.  out: capacity bev_regfront_max_out(n) PointXYZ. */
int bev_top_part_flatten(bev_ctx_t *ctx, const bev_point_t *cloud, uint32_t n, float *out, uint32_t *n_out);
/* pcl::VoxelGrid<pcl::PointXYZ> with one leaf size for x, y, z (BatchTopPartRegistration.cpp:342-343,405-409; PCL >= 1.10
 * defaults): voxels in ascending index order, centroids summed in input order.  Non-finite points are dropped.  When the
 * grid would have more than INT32_MAX voxels the output is the input.  out: capacity n PointXYZ. */
int bev_voxel_grid_xyz(bev_ctx_t *ctx, const float *xyz, uint32_t n, float leaf, float *out, uint32_t *n_out);
/* Normal2dEstimation::compute(PointCloud<Normal>) in radius mode with setViewPoint (src/Normal2dEstimation.cpp,
 * src/PCA2D.cpp; addNormal, BatchTopPartRegistration.cpp:155-172, uses radius 2 and the viewpoint (0, 0, 0)).
 * k_search != 0 (setKSearch) -> BEV_ERR_UNSUPPORTED.  viewpoint: 3 floats or NULL (origin; z is not used).  Every point
 * is scanned for every query (O(n^2) work: meant for clouds up to ~10^5 points).  out: n pcl::Normal records. */
int bev_normals_2d(bev_ctx_t *ctx, const float *xyz, uint32_t n, int k_search, float radius, const float *viewpoint,
                   float *out);
/* The three steps for a batch of clouds, device-resident: top part -> voxel grid (leaf) -> normals (radius, viewpoint)
 * -> pcl::concatenateFields into PointNormal (addNormal, BatchTopPartRegistration.cpp:155-172).
 * d_clouds   : h_offsets == NULL: the d_ordered output of bev_process_device_resident (n_frames * S points);
 *              else packed clouds, frame f = [h_offsets[f], h_offsets[f+1]) (HOST array of n_frames + 1 offsets).
 * d_out      : n_frames * out_stride PointNormal records (device); out_stride >= bev_regfront_max_out(largest cloud).
 * d_counts   : n_frames uint32 (device): records of frame f.
 * Asynchronous like bev_process_device_resident: bev_synchronize() before reading the results.  It starts behind every
 * BEV call made before it (including their pending stages) and behind the caller's default-stream work; the next
 * bev_process_device_resident starts behind it. */
int bev_registration_front_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds,
                                           const uint64_t *h_offsets, float leaf, float radius, const float *viewpoint,
                                           void *d_out, size_t out_stride, uint32_t *d_counts);
/* Records the top part (and so the chain) can emit for a cloud of n points: sum of round(0.2f * n_cell) <= n / 5 + 51.
 * Host only. */
size_t bev_regfront_max_out(size_t n);

/* ---- coarse point-to-plane ICP ---------------------------------------------------------------------------------------
 * pcl::IterativeClosestPointWithNormals<PointNormal, PointNormal> as the registration tools' performCoarseIcp runs it
 * (BatchTopPartRegistration.cpp:192-221; the tool's two yaw guesses and its choice, :415-466).  The contract — restated
 * from PCL's published sources, parity with the reference UNPINNED, exact 1-NN with the lowest index on ties, every sum
 * in a fixed order — is DESIGN.md §6c.  Clouds are pcl::PointNormal records (12 floats, as above); source normals are
 * never read.  The fine stage (VoxelGrid<PointXYZIRCT> + point-to-point ICP) is below. */
typedef struct {
    double max_correspondence_distance; /* D: a correspondence needs (double)dist <= D * D */
    double transformation_epsilon;
    double euclidean_fitness_epsilon;
    int32_t max_iterations;             /* 1 ... 1000 */
    int32_t _pad;                       /* 0 */
} bev_icp_params_t;
/* PCL's defaults plus the tool's two settings: D = 10, 10 iterations, transformation_epsilon 0,
 * euclidean_fitness_epsilon -DBL_MAX.  Host only. */
bev_icp_params_t bev_icp_coarse_defaults(void);

enum {
    BEV_ICP_NOT_CONVERGED = 0,
    BEV_ICP_ITERATIONS = 1,
    BEV_ICP_TRANSFORM = 2,
    BEV_ICP_ABS_MSE = 3,
    BEV_ICP_REL_MSE = 4,
    BEV_ICP_NO_CORRESPONDENCES = 5 /* fewer than 3 correspondences: converged 0 */
};
typedef struct {
    float T[16];        /* getFinalTransformation(), row-major; a NaN entry is 0x7fc00000 */
    double fitness;     /* getFitnessScore(): DBL_MAX when no source point has a finite nearest distance */
    int32_t converged;  /* hasConverged() */
    int32_t iterations;
    int32_t state;      /* BEV_ICP_* (DefaultConvergenceCriteria's enum) */
    int32_t _pad;       /* 0 */
} bev_icp_result_t;

/* the reference's MatchResult (BatchTopPartRegistration.cpp:83-88): query_idx is the source frame, match_idx the target */
typedef struct {
    int32_t query_idx;
    int32_t match_idx;
    float angle_guess; /* degrees */
} bev_match_t;

/* One problem on host clouds (synchronous).  guess16: row-major 4 x 4 initial guess (NULL: identity).  params NULL: the
 * coarse defaults.  Invalid parameters (max_iterations outside 1 ... 1000, D <= 0 or non-finite) -> BEV_ERR_INVALID_ARG. */
int bev_icp_point_to_plane(bev_ctx_t *ctx, const float *src, uint32_t n_src, const float *tgt, uint32_t n_tgt,
                           const float *guess16, const bev_icp_params_t *params, bev_icp_result_t *result);
/* The tool's coarse loop for a list of matches, device-resident: for match m, ICP of frame query_idx onto frame match_idx
 * from the guesses theta and theta + 180 (yaw about z, theta = angle_guess), and the better of the two.
 * d_pn, stride, d_counts : bev_registration_front_device_resident's output (n_frames * stride PointNormal records,
 *                          n_frames uint32 counts; a count above stride is read as stride)
 * h_matches              : n_matches HOST records; every index in 0 ... n_frames - 1
 * d_results              : 2 * n_matches results (device): [2m] guess theta, [2m + 1] guess theta + 180
 * d_best                 : n_matches int32 (device): 0 iff fitness[2m] < fitness[2m + 1], else 1 (ties, NaN)
 * Asynchronous like bev_process_device_resident: bev_synchronize() before reading the results.  It starts behind every
 * call made on the context before it and behind the caller's default-stream work; the next BEV call starts behind it.
 * Workspace, allocated on first use (grown when a call needs more) and freed by bev_destroy:
 *   U * (32 + 4 * 4097 + 16 * stride) + min(2 * n_matches, 1024) * 16 * stride + 80 * 2 * n_matches + 4 * U bytes,
 * U the number of distinct target frames; the problems run in launches of 1024 (the results do not depend on it).
 * Nothing is launched when an argument is invalid (BEV_ERR_INVALID_ARG). */
int bev_coarse_registration_device_resident(bev_ctx_t *ctx, int n_frames, const void *d_pn, size_t stride,
                                            const uint32_t *d_counts, int n_matches, const bev_match_t *h_matches,
                                            const bev_icp_params_t *params, bev_icp_result_t *d_results,
                                            int32_t *d_best);

/* ---- fine stage: VoxelGrid<PointXYZIRCT> and point-to-point ICP ------------------------------------------------------
 * performFineIcp of the registration tools (BatchTopPartRegistration.cpp:224-247, 480-497; BatchWholeRegistration.cpp:
 * 222-245, 372-389): pcl::VoxelGrid<PointXYZIRCT> (leaf 0.2) on the full labelled clouds, then
 * pcl::IterativeClosestPoint<PointXYZIRCT, PointXYZIRCT> (TransformationEstimationSVD, Umeyama without scaling).  The
 * contract — restated from PCL's and Eigen's published sources, parity with the reference UNPINNED, §6c's loop, exact
 * 1-NN and summation order — is DESIGN.md §6d. */
/* pcl::VoxelGrid<pcl::PointXYZIRCT> (BatchTopPartRegistration.cpp:345-346,483-487): x, y, z as bev_voxel_grid_xyz;
 * intensity the float sum in input order / float(n); label the majority (a tie: the smallest as uint32); row, col, t and
 * the pads 0.  out: capacity n records. */
int bev_voxel_grid_irct(bev_ctx_t *ctx, const bev_point_t *cloud, uint32_t n, float leaf, bev_point_t *out,
                        uint32_t *n_out);
/* the top-part tool's settings: D 1, transformation_epsilon 1e-6, euclidean_fitness_epsilon 0.01, 100 iterations.
 * Host only. */
bev_icp_params_t bev_icp_fine_defaults(void);
/* the whole tool's settings: D 4, 1e-6, 0.001, 200 iterations.  Host only. */
bev_icp_params_t bev_icp_whole_defaults(void);
/* One problem on host clouds (synchronous); only x, y, z are read.  guess16: row-major 4 x 4 (NULL: identity); params
 * NULL: the fine defaults.  Invalid parameters (as bev_icp_point_to_plane) -> BEV_ERR_INVALID_ARG. */
int bev_icp_point_to_point(bev_ctx_t *ctx, const bev_point_t *src, uint32_t n_src, const bev_point_t *tgt,
                           uint32_t n_tgt, const float *guess16, const bev_icp_params_t *params,
                           bev_icp_result_t *result);
/* The tools' fine stage for a list of matches, device-resident: the voxel grid (leaf) of every distinct frame the
 * matches name (once each), then ICP of frame query_idx onto frame match_idx per match.
 * d_clouds, h_offsets : as bev_registration_front_device_resident (h_offsets NULL: the d_ordered output of
 *                       bev_process_device_resident, S records per frame; else HOST offsets of packed clouds)
 * d_coarse, d_best    : bev_coarse_registration_device_resident's outputs: the guess of match m is
 *                       d_coarse[2m + d_best[m]].T (the top-part tool); both NULL: the yaw guess theta = angle_guess
 *                       (guess 0 of §6c; the whole tool).  One NULL and the other not: BEV_ERR_INVALID_ARG.
 * d_results           : n_matches results (device).  params NULL: the fine defaults.
 * Asynchronous like bev_process_device_resident: bev_synchronize() before reading the results.  It starts behind every
 * call made on the context before it and behind the caller's default-stream work; the next BEV call starts behind it.
 * Workspace, allocated on first use (grown when a call needs more) and freed by bev_destroy, with U the distinct frames
 * of the call, N the largest of their record counts and K the smallest power of two >= N:
 *   U * (48 N + 4 * 16385 + 36) + min(U, 256) * (8 K + 4 N + 4) + min(n_matches, 1024) * 20 N bytes,
 * i.e. per frame 48 N bytes of voxel records and the searchable points plus a 64 KiB grid (at most 128 x 128 cells);
 * plus the tables (16 bytes per frame, 80 per match).  Frames run in voxel launches of 256 and matches in ICP launches of
 * 1024 (the results do not depend on either).  Nothing is launched when an argument is invalid (BEV_ERR_INVALID_ARG). */
int bev_fine_registration_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds,
                                          const uint64_t *h_offsets, float leaf, int n_matches,
                                          const bev_match_t *h_matches, const bev_icp_result_t *d_coarse,
                                          const int32_t *d_best, const bev_icp_params_t *params,
                                          bev_icp_result_t *d_results);

/* ---- scan-to-map fine ICP: frames registered against submaps -----------------------------------------------------------
 * The fine stage with a MAP as its target: map g is a list of (frame, pose) entries, exactly as for
 * bev_submap_bev_device_resident, and
 *   target(g) = the concatenation, over g's entries e IN THE ORDER GIVEN, of
 *               bev_transform_cloud(bev_voxel_grid_irct(frame(e), leaf), pose(e));
 *   result(m) = bev_icp_point_to_point(bev_voxel_grid_irct(frame query_idx, leaf), target(match_idx), guess, params)
 * for match m = (query_idx, match_idx = a MAP's index, angle_guess), bit for bit.  Every frame is voxelised on
 * its own, once, and the voxel clouds are moved; there is no second voxel grid over the union.  A target point's index is its
 * position in the concatenation, and the search's "lowest index on ties" is over that index: unlike in the rasters, the
 * order of a map's entries matters.  Points a matrix makes non-finite keep their index and are never matched.  result.T takes
 * the query frame into the map's coordinates.  A map without entries or without a searchable point ends as
 * bev_icp_point_to_point ends on an empty target: BEV_ICP_NO_CORRESPONDENCES, fitness DBL_MAX.
 * d_clouds, h_offsets : as bev_fine_registration_device_resident (h_offsets NULL: d_ordered, S records per frame).
 * h_map_offsets, h_entry_frame, h_entry_pose : exactly as bev_submap_bev_device_resident: any number of entries per map; a
 *                       frame may appear several times in one map, feed many maps, or be named by none; the call's total of
 *                       entries is bounded by BEV_SUBMAP_MAX_ENTRIES, and the record counts of one map's entries' frames
 *                       together by BEV_SUBMAP_REG_MAX_TARGET.  A map no match names costs nothing.
 * h_matches           : n_matches HOST records; query_idx in 0 .. n_frames - 1, match_idx in 0 .. n_maps - 1.
 * d_coarse, d_best    : as bev_fine_registration_device_resident: both NULL: the yaw guess of angle_guess; both given: match m
 *                       starts from d_coarse[2m + d_best[m]].T; one NULL and the other not: BEV_ERR_INVALID_ARG.
 * d_results           : n_matches results (device); match m's at index m.  params NULL: the fine defaults.
 * Ordering  : asynchronous like bev_fine_registration_device_resident: it starts behind every call made on the context before
 *             it and behind the caller's default-stream work; the next BEV call starts behind it.  bev_synchronize() before
 *             reading the results.  The host arrays may be reused as soon as the call returns.
 * Status    : BEV_ERR_INVALID_ARG for a NULL context, a negative count, invalid parameters or leaf, and, with matches to run,
 *             a NULL array that would be read, decreasing offsets, an entry frame outside 0 .. n_frames - 1, a query_idx
 *             outside the frames, a match_idx outside the maps; BEV_ERR_TOO_LARGE for more than BEV_SUBMAP_MAX_ENTRIES
 *             entries (checked before the entry arrays are read) and for a map whose entries' frames total more than
 *             BEV_SUBMAP_REG_MAX_TARGET records.  Nothing is launched and d_results is untouched in every such case.
 *             n_matches == 0 returns BEV_OK.
 * Workspace : in the fine stage's buffer (allocated on first use, grown when a call needs more, freed by bev_destroy).  With U
 *             the distinct frames that queries and used maps' entries name, N the largest of their record counts, K the
 *             smallest power of two >= N, E the entries of the used maps and, of the launch group that needs most, T the sum
 *             of its maps' capacities (a map's capacity: the record counts of its entries' frames together) and M its maps:
 *               U * (32 N + 4) + min(U, 256) * (8 K + 4 N + 4) + min(n_matches, 1024) * 20 N + 4 E + 32 T + M * (4 * 16385 + 32)
 *             bytes (pieces rounded up to 256), plus the tables (16 bytes per frame and per map, 64 per entry, 80 per match).
 *             The used maps are cut into launch groups of consecutive maps whose 32 T + M * (4 * 16385 + 32) bytes fit 8 GiB
 *             (BEV_SUBMAP_REG_GROUP=<bytes> in the environment of bev_create sets the cap instead; results do not depend on
 *             it); a map above the cap is a group of its own.  Frames run in voxel launches of 256, a group's matches in ICP
 *             launches of 1024. */
#define BEV_SUBMAP_REG_MAX_TARGET (1u << 22)   /* records of one map's entries' frames together */
int bev_submap_registration_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                            float leaf, int n_maps, const uint64_t *h_map_offsets,
                                            const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                            const bev_match_t *h_matches, const bev_icp_result_t *d_coarse,
                                            const int32_t *d_best, const bev_icp_params_t *params,
                                            bev_icp_result_t *d_results);
/* The same through HOST buffers, synchronous: clouds[f] holds n_pts[f] records (NULL clouds[f] with n_pts[f] > 0:
 * BEV_ERR_INVALID_ARG); results receives n_matches records.  Yaw guesses only.  The clouds go up into the fine stage's input
 * buffer (grown on demand), the results come down from a device buffer of the context. */
int bev_submap_registration_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                                  float leaf, int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                  const float *h_entry_pose, int n_matches, const bev_match_t *h_matches,
                                  const bev_icp_params_t *params, bev_icp_result_t *results);

/* ---- scan-to-map fine ICP against THINNED maps: a voxel grid over the union ----------------------------------------------
 * bev_submap_registration_device_resident with a second leaf size.  With
 *   concat(g) = bev_submap_registration_device_resident's target(g) (above), and map_leaf > 0:
 *   target(g) = bev_voxel_grid_irct(concat(g), map_leaf), of which only x, y, z are ever read;
 *   result(m) = bev_icp_point_to_point(bev_voxel_grid_irct(frame query_idx, leaf), target(match_idx), guess, params),
 * bit for bit as a whole bev_icp_result_t.  So the target's points are in ascending voxel index of the UNION's grid, whose
 * bounds and divisions come from the finite points of concat(g); a centroid is the float sum of its voxel's points IN
 * CONCATENATION ORDER divided by float(n), without FMA; non-finite points of concat(g) (a matrix that overflows, NaN records
 * that a frame's own "leaf too small" branch copied) are dropped.  When the union's grid would have more than INT32_MAX voxels,
 * target(g) is concat(g) unchanged: non-finite points then keep their index and stay unsearchable.  The search's "lowest index
 * on ties" is over the thinned target's index; the order of a map's entries matters only through the order of the sums inside a
 * voxel.  An empty map, or one whose union has no finite point, ends as above: BEV_ICP_NO_CORRESPONDENCES, fitness DBL_MAX.
 * map_leaf == 0     : no second grid: bev_submap_registration_device_resident itself, byte for byte (that function is this
 *                     one with map_leaf = 0).
 * map_leaf < 0, NaN, infinite : BEV_ERR_INVALID_ARG.
 * Every other argument, status and bound, and the ordering, are bev_submap_registration_device_resident's; a refused call
 * launches nothing and leaves d_results untouched.
 * Workspace : with map_leaf > 0 a launch group also holds the concatenations, the padded sort keys, the voxel starts and a
 *             header per map: with T, M as above and K' the sum over the group's maps of the smallest power of two >= the map's
 *             capacity (0 for capacity 0), the formula above plus
 *               16 T + 8 K' + 4 (T + M) + 32 M
 *             bytes (pieces rounded up to 256), and 8 bytes per map in the tables.  The launch groups are cut so that
 *             48 T + 8 K' + 4 (T + M) + M * (4 * 16385 + 64) fits the cap.  The sort runs in tiles of 4096 keys per workgroup. */
int bev_submap_voxel_registration_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds,
                                                  const uint64_t *h_offsets, float leaf, float map_leaf, int n_maps,
                                                  const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                                  const float *h_entry_pose, int n_matches, const bev_match_t *h_matches,
                                                  const bev_icp_result_t *d_coarse, const int32_t *d_best,
                                                  const bev_icp_params_t *params, bev_icp_result_t *d_results);
/* The same through HOST buffers, synchronous, yaw guesses only: bev_submap_registration_batch with map_leaf (that function is
 * this one with map_leaf = 0). */
int bev_submap_voxel_registration_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                                        float leaf, float map_leaf, int n_maps, const uint64_t *h_map_offsets,
                                        const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                        const bev_match_t *h_matches, const bev_icp_params_t *params, bev_icp_result_t *results);
/* The local maps themselves: target(g) of EVERY map of the call (there are no matches), as PointXYZ records (x, y, z and a
 * pad of 0, 16 bytes).  Map g's records go to d_out + 4 * g * out_stride floats, its record count to d_counts[g]; records past
 * the count are not written.  map_leaf == 0 is allowed: concat(g).  Frames, maps, ordering and workspace as above (no ICP
 * scratch, no search grids).
 * Status    : as above; also BEV_ERR_INVALID_ARG for NULL d_out or d_counts with n_maps > 0, and for an out_stride (in
 *             records) smaller than the largest map's capacity (the record counts of its entries' frames together).
 *             n_maps == 0 returns BEV_OK.  A refused call launches nothing and leaves d_out and d_counts untouched. */
int bev_submap_voxel_cloud_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                           float leaf, float map_leaf, int n_maps, const uint64_t *h_map_offsets,
                                           const int32_t *h_entry_frame, const float *h_entry_pose, uint64_t out_stride,
                                           float *d_out, uint32_t *d_counts);

/* ---- scan-to-map coarse ICP: PointNormal frames registered point-to-plane against submaps ------------------------------
 * The coarse stage with a MAP as its target: bev_coarse_registration_device_resident's loop, the target of
 * match m being map match_idx instead of one frame.  Its two outputs are what the fine stages take as d_coarse / d_best, so
 * the top-part pipeline against local maps is: bev_registration_front_device_resident, this call,
 * bev_submap_voxel_registration_device_resident, with no synchronisation between them.
 * Frames    : PointNormal clouds, d_pn / stride / d_counts exactly as bev_coarse_registration_device_resident reads them (the
 *             output of bev_registration_front_device_resident; a count above stride is read as stride).
 * Maps      : h_map_offsets, h_entry_frame, h_entry_pose exactly as bev_submap_bev_device_resident (12 floats per entry, a
 *             row-major 3 x 4 matrix m); any number of entries per map; a frame may appear several times in one map, feed many
 *             maps, or be named by none; a map no match names costs nothing.
 * Moving a PointNormal record r under m, all in float, without FMA:
 *             position component i = m[i][0] * x + (m[i][1] * y + (m[i][2] * z + m[i][3]))   (bev_transform_cloud's association);
 *             normal component i   = m[i][0] * nx + (m[i][1] * ny + m[i][2] * nz)            (the same without the translation);
 *             the normal is neither renormalised nor flipped again, so a matrix that is no rotation gives what this formula
 *             gives; the curvature is copied, every pad is 0, every NaN written is 0x7fc00000; 48 bytes in the layout above.
 * target(g) : the concatenation, over g's entries e IN THE ORDER GIVEN, of the moved records of frame(e) under pose(e).  A
 *             target point's index is its position in the concatenation, and the search's "lowest index on ties" is over that
 *             index, so the order of a map's entries matters.  Points made non-finite keep their index and are never matched;
 *             a correspondence whose moved normal has a non-finite component adds nothing to the sums, but counts (§6c).
 * Results   : for match m = (query_idx, match_idx = a MAP's index, angle_guess) and guess k in {0, 1}
 *               d_results[2m + k] = bev_icp_point_to_plane(frame query_idx, target(match_idx), guess k of angle_guess, params)
 *             bit for bit as a whole bev_icp_result_t (guess 0: yaw theta, guess 1: theta + 180, as above);
 *             d_best[m] = 0 iff fitness[2m] < fitness[2m + 1], else 1.  result.T takes the query frame into the map's
 *             coordinates.  A map without entries or without a searchable point ends as bev_icp_point_to_plane ends on an
 *             empty target: BEV_ICP_NO_CORRESPONDENCES, fitness DBL_MAX.  params NULL: the coarse defaults.
 * Ordering  : asynchronous and ordered exactly like bev_coarse_registration_device_resident: it starts behind every call made
 *             on the context before it and behind the caller's default-stream work; the next BEV call starts behind it, so
 *             d_results / d_best can go straight into bev_submap_voxel_registration_device_resident (or any fine call) as
 *             d_coarse / d_best.  bev_synchronize() before reading them on the host.  The host arrays may be reused as soon as
 *             the call returns.
 * Status    : BEV_ERR_INVALID_ARG for a NULL context, a negative count, invalid parameters, and, with matches to run,
 *             stride == 0, a NULL array that would be read, decreasing offsets, an entry frame outside 0 .. n_frames - 1, a
 *             query_idx outside the frames, a match_idx outside the maps; BEV_ERR_TOO_LARGE for more than
 *             BEV_SUBMAP_MAX_ENTRIES entries (checked before the entry arrays are read) and for a map whose CAPACITY exceeds
 *             BEV_SUBMAP_COARSE_MAX_TARGET rows.  A map's capacity is n_entries * stride: the frames' true counts live on the
 *             device and the host does not wait for them, so a caller whose frames are short passes a tighter stride (any
 *             stride >= the largest count reads the same rows).  A refused call launches nothing and leaves d_results and
 *             d_best untouched.  n_matches == 0 returns BEV_OK.
 * Workspace : in the coarse stage's buffer (allocated on first use, grown when a call needs more, freed by bev_destroy; the
 *             pair call and this one hand it to each other in stream order).  With E the entries of the used maps and, of the
 *             launch group that needs most, T the sum of its maps' capacities and M its maps:
 *               min(2 * n_matches, 1024) * 16 * stride + 4 E + 64 T + M * (4 * 4097 + 32)
 *             bytes (pieces rounded up to 256), plus the tables (16 bytes per used map, 64 per entry, 80 per problem, two
 *             problems per match).  The used maps are cut into launch groups of consecutive maps whose
 *             64 T + M * (4 * 4097 + 32) bytes fit 8 GiB (BEV_SUBMAP_REG_GROUP=<bytes>, as above; results do not depend on
 *             it); a map above the cap is a group of its own.  A group's problems run in launches of 1024.  The search grid of
 *             a map has at most 64 x 64 cells, as a frame's has. */
#define BEV_SUBMAP_COARSE_MAX_TARGET (1u << 22)   /* rows of one map: its entries times the stride */
int bev_submap_coarse_registration_device_resident(bev_ctx_t *ctx, int n_frames, const void *d_pn, size_t stride,
                                                   const uint32_t *d_counts, int n_maps, const uint64_t *h_map_offsets,
                                                   const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                   const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                   bev_icp_result_t *d_results, int32_t *d_best);

/* ---- scan-to-map coarse ICP against THINNED maps: a voxel grid and 2-D normals over the union ----------------------------
 * bev_submap_coarse_registration_device_resident with a leaf size for the map: what the reference pipeline does
 * to every cloud it hands to coarse ICP (VoxelGrid<PointXYZ>, Normal2dEstimation, concatenateFields), done to the union of a
 * map's entries.  With concat(g) = bev_submap_coarse_registration_device_resident's target(g) (above; a frame's count cut at
 * stride), and pn_leaf > 0:
 *   V = bev_voxel_grid_xyz(positions of concat(g), pn_leaf): bounds and divisions from the finite positions of the union,
 *       voxels in ascending index, a centroid the float sum of its voxel's points IN CONCATENATION ORDER divided by float(n),
 *       without FMA; non-finite positions are dropped;
 *   N = bev_normals_2d(V, radius mode, radius, viewpoint): neighbours by the 3-D float distance in ascending index, the
 *       |N| = 0 / 1 / 2 / >= 3 branches, the flip towards the viewpoint (its x and y; NULL: the origin), every NaN 0x7fc00000;
 *   target(g)[i] = the PointNormal record  x y z 0 | nx ny nz 0 | curvature 0 0 0  of V[i] and N[i].
 * The moved normals and curvatures of concat(g) are NOT used: the rule for a merged voxel's normal is "recompute", so a
 * thinned map's normals have nz = 0 exactly, whatever its entries' poses.  When the union's grid would have more than INT32_MAX
 * voxels ("leaf too small"), target(g) is concat(g) unchanged, moved normals included, as §6l keeps the concatenation.  A map
 * without entries, or whose union has no finite position, ends as an empty target does.
 *   d_results[2m + k] = bev_icp_point_to_plane(frame query_idx, target(match_idx), guess k of angle_guess, params)
 * bit for bit as a whole bev_icp_result_t, d_best as above; both go straight into
 * bev_submap_voxel_registration_device_resident without a synchronisation.
 * pn_leaf == 0      : no grid over the union: bev_submap_coarse_registration_device_resident itself, byte for byte (that
 *                     function is this one with pn_leaf = 0); radius and viewpoint are not read.
 * pn_leaf < 0, NaN, infinite : BEV_ERR_INVALID_ARG.  With pn_leaf > 0 also a radius that bev_normals_2d refuses (not finite,
 *                     or <= 0).
 * Every other argument, status and bound, and the ordering, are bev_submap_coarse_registration_device_resident's
 * (BEV_SUBMAP_COARSE_MAX_TARGET applies to the capacity n_entries * stride); a refused call launches nothing and leaves
 * d_results and d_best untouched; n_matches == 0 returns BEV_OK.
 * Workspace : in the coarse stage's buffer.  With pn_leaf > 0 a launch group also holds the moved rows, the padded sort keys,
 *             the voxel starts, the voxel indices, the thinned positions and a header per map: with E, T, M as above and K' the
 *             sum over the group's maps of the smallest power of two >= the map's capacity (0 for capacity 0),
 *               min(2 * n_matches, 1024) * 16 * stride + 4 E + 136 T + 8 K' + M * (4 * 4097 + 32 + 4 + 32)
 *             bytes (pieces rounded up to 256), and 8 more bytes per used map in the tables.  The launch groups are cut so that
 *             136 T + 8 K' + M * (4 * 4097 + 68) fits the cap (BEV_SUBMAP_REG_GROUP; results do not depend on it).  The sort
 *             runs in tiles of 4096 keys per workgroup, the normals in workgroups of 256 thinned points. */
int bev_submap_coarse_voxel_registration_device_resident(bev_ctx_t *ctx, int n_frames, const void *d_pn, size_t stride,
                                                         const uint32_t *d_counts, float pn_leaf, float radius,
                                                         const float *viewpoint, int n_maps, const uint64_t *h_map_offsets,
                                                         const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                         const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                         bev_icp_result_t *d_results, int32_t *d_best);
/* The local maps themselves: target(g) of EVERY map of the call (there are no matches), as PointNormal records of 48 bytes.
 * Map g's records go to d_out + 12 * g * out_stride floats, its record count to d_counts_out[g]; records past the count are
 * not written.  pn_leaf == 0 is allowed: concat(g).  Frames, maps, ordering and workspace as above (no ICP scratch, no search
 * grids: 4 E + 120 T + 8 K' + M * (4 + 32) bytes with pn_leaf > 0, 4 E + 48 T + 32 M with pn_leaf == 0; the launch groups are
 * cut as above).
 * Status    : as above; with maps also BEV_ERR_INVALID_ARG for NULL d_pn, d_counts, d_out or d_counts_out, stride == 0, and an
 *             out_stride (in records) smaller than the largest map's capacity n_entries * stride.  n_maps == 0 returns BEV_OK.
 *             A refused call launches nothing and leaves d_out and d_counts_out untouched. */
int bev_submap_pn_cloud_device_resident(bev_ctx_t *ctx, int n_frames, const void *d_pn, size_t stride, const uint32_t *d_counts,
                                        float pn_leaf, float radius, const float *viewpoint, int n_maps,
                                        const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                                        uint64_t out_stride, float *d_out, uint32_t *d_counts_out);

/* ---- scan-to-map coarse ICP against the TOP PART OVER THE UNION of a map's moved full clouds ---------------------------------
 * What the reference hands coarse ICP is ONE cloud put through extractTopAndFlatten, VoxelGrid<PointXYZ> and Normal2dEstimation;
 * where the target is a local map, that cloud is the union of the map's moved full clouds.  The calls above
 * concatenate each sweep's own top part instead; these two build the top part over the union.  Maps: h_map_offsets,
 * h_entry_frame, h_entry_pose exactly as above.  Full labelled clouds: d_clouds / h_offsets exactly as
 * bev_submap_voxel_registration_device_resident takes them (h_offsets == NULL: d_ordered, S records per frame).
 *   union(g)  = the concatenation, over g's entries IN THE ORDER GIVEN, of bev_transform_cloud(frame(e), pose(e)): whole
 *               bev_point_t records, labels and the other fields carried; a record's index is its position in the concatenation;
 *   top(g)    = bev_top_part_flatten(union(g)), its contract unchanged: label 0 is skipped; a record whose MOVED x, y or z is
 *               not finite is skipped; the cell is taken from the moved x, y with round, in the 10 x 10 grid; a cell of fewer
 *               than 20 records is skipped; a kept cell emits round(0.2f * n) records, highest moved z first (-0 = +0), the
 *               lower union index first on equal z; output (x, y, 0), cells in gx-major then gy order.  Ties therefore go to the
 *               earlier entry: the order of a map's entries matters;
 *   V         = bev_voxel_grid_xyz(top(g), pn_leaf); in its "leaf too small" branch V = top(g) (and N is still computed);
 *   N         = bev_normals_2d(V, radius mode, radius, viewpoint);
 *   target(g)[i] = the PointNormal record  x y z 0 | nx ny nz 0 | curvature 0 0 0  of V[i] and N[i]: 48 bytes, pads 0, every
 *               NaN 0x7fc00000.
 * A map without entries, or whose cells all stay under 20 records, has an empty target and ends as an empty target does above.
 * Capacity  : a map's capacity is the sum of its entries' frames' record counts, at most BEV_SUBMAP_TOP_MAX_UNION = 2^24: the
 *             selection works on keys  cell (7 bits) | descending-z key (32) | union index (25)  and holds at most
 *             bev_submap_top_part_max_out(2^24) < 2^22 of them.
 * Ordering  : both calls are asynchronous and ordered exactly like bev_submap_coarse_voxel_registration_device_resident.
 * Workspace : in the coarse stage's buffer.  With U the union records, T' the sum of bev_submap_top_part_max_out(capacity) and
 *             K" the sum of the smallest powers of two >= these, over the maps of the launch group that needs most, and M its
 *             maps: 8 U (a key per record; the moved records are never written: a selected record is moved again) +
 *             M * (2816 + 25600) (the 100 cells' tables and histograms) + 136 T' + 8 K" + M * (4 * 4097 + 68) + the ICP scratch
 *             min(2 * n_matches, 1024) * 16 * stride, pieces rounded up to 256; the tables take 16 bytes per frame named and 16
 *             more per used map.  The launch groups are cut so that all but the scratch fits the cap (BEV_SUBMAP_REG_GROUP;
 *             results do not depend on it).
 *
 * The cloud call: target(g) of EVERY map as rows of 48 bytes at d_out + 12 * g * out_stride floats, its count in
 * d_counts_out[g]; rows past the count are not written.  out_stride is in records and must be at least
 * bev_submap_top_part_max_out of the largest capacity.  pn_leaf == 0 writes top(g) itself as rows
 * x y 0 0 | 0 0 0 0 | 0 0 0 0: no voxel stage and no normals; radius and viewpoint are not read.
 * Status    : BEV_ERR_INVALID_ARG for a NULL context, a negative count, a negative, NaN or infinite pn_leaf, with pn_leaf > 0 a
 *             radius that bev_normals_2d refuses, and, with maps, a NULL array that is needed, decreasing offsets, an entry frame
 *             outside the frames, a capacity above BEV_SUBMAP_TOP_MAX_UNION, a short out_stride; BEV_ERR_TOO_LARGE for more than
 *             BEV_SUBMAP_MAX_ENTRIES entries.  n_maps == 0 returns BEV_OK.  A refused call launches nothing and leaves d_out
 *             and d_counts_out untouched. */
#define BEV_SUBMAP_TOP_MAX_UNION (1u << 24) /* records of one map's union */
size_t bev_submap_top_part_max_out(size_t union_records); /* host only: bev_regfront_max_out of the union */
int bev_submap_top_part_cloud_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                              float pn_leaf, float radius, const float *viewpoint, int n_maps,
                                              const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                              const float *h_entry_pose, uint64_t out_stride, float *d_out, uint32_t *d_counts_out);
/* The registration call.  The QUERIES are d_pn / stride / d_counts, the front end's output for the same n_frames frames, exactly
 * as bev_submap_coarse_registration_device_resident reads them.  For match m = (query_idx, match_idx = a MAP's index,
 * angle_guess) and guess k in {0, 1}
 *   d_results[2m + k] = bev_icp_point_to_plane(d_pn rows of frame query_idx, target(match_idx), guess k of angle_guess, params)
 * bit for bit as a whole bev_icp_result_t; d_best as above; both go straight into
 * bev_submap_voxel_registration_device_resident as d_coarse / d_best without a synchronisation.  A map no match names costs
 * nothing.  params NULL: the coarse defaults.
 * Status    : as the cloud call's, and BEV_ERR_INVALID_ARG for a pn_leaf that is not finite and > 0 (0 too), invalid
 *             parameters, and, with matches, NULL h_matches, d_results, d_best, d_pn or d_counts, stride == 0, a query_idx
 *             outside the frames, a match_idx outside the maps.  n_matches == 0 returns BEV_OK.  A refused call launches nothing
 *             and leaves d_results and d_best untouched. */
int bev_submap_top_part_coarse_registration_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds,
                                                            const uint64_t *h_offsets, const void *d_pn, size_t stride,
                                                            const uint32_t *d_counts, float pn_leaf, float radius,
                                                            const float *viewpoint, int n_maps, const uint64_t *h_map_offsets,
                                                            const int32_t *h_entry_frame, const float *h_entry_pose, int n_matches,
                                                            const bev_match_t *h_matches, const bev_icp_params_t *params,
                                                            bev_icp_result_t *d_results, int32_t *d_best);

/* ---- scan-to-map search grids sized to the map ------------------------------------------------------------
 * The scan-to-map calls search a map's target on a uniform 2-D grid of at most dim x dim cells,
 *   dim = min(D, max(1, ceil(sqrtf(n)))),  n the target's points,
 * with D = 128 in the fine calls and D = 64 in the coarse ones: the cell counts of that build fit one workgroup's LDS.  This
 * call sets D per stage for the calls made after it (sticky per context):
 *   0          (default) the stage runs as it always has: the same kernels, launches and workspace;
 *   1 ... BEV_SUBMAP_SEARCH_GRID_MAX
 *              the stage's map targets get grids with that cap, built by several workgroups per map with the cell counts in
 *              global memory, and the ICP reads a map's cell offsets from there.  Values below 128 / 64 are allowed.
 * fine_dim governs bev_submap_registration_* and bev_submap_voxel_registration_* (both leaf branches, the batch forms too);
 * coarse_dim governs bev_submap_coarse_registration_device_resident, bev_submap_coarse_voxel_registration_device_resident and
 * bev_submap_top_part_coarse_registration_device_resident.  The cloud-writing calls build no grid; the pair calls keep theirs.
 * Results never depend on it: the search is an exact 1-NN with the lowest target index on equal distance whatever the cell
 * size, so every result is bit for bit what D = 0 gives.  Only time and workspace do: with D > 0 a map of capacity c takes
 * 8 (dim(c)^2 + 1) bytes of offsets and counters plus 5 KiB in place of the fixed grid's offsets.
 * No synchronisation is needed around it: a call made before it and not yet finished keeps its grids.
 * Status: BEV_ERR_INVALID_ARG for a NULL context or a value outside 0 ... BEV_SUBMAP_SEARCH_GRID_MAX; nothing changes then. */
#define BEV_SUBMAP_SEARCH_GRID_MAX 1024
int bev_set_submap_search_grid(bev_ctx_t *ctx, int fine_dim, int coarse_dim);

/* ---- pair registration search grids sized to the cloud ------------------------------------------------------
 * The pair calls search a target cloud on the same kind of grid, dim = min(D, max(1, ceil(sqrtf(n)))) cells per axis for a target
 * of n points, with D = 128 in the fine stage and D = 64 in the coarse one.  This call sets D per stage for the pair calls made
 * after it (sticky per context; host state read when a call is made):
 *   0          (default) the stage runs as it always has: the same kernels, launches and workspace layout;
 *   1 ... BEV_PAIR_SEARCH_GRID_MAX
 *              every cloud that a match names as a target gets a grid with that cap, built by several workgroups per target with
 *              the cell counts in global memory, and the ICP reads the target's cell offsets from there.  Values below 128 / 64
 *              are allowed.  A cloud that is a query only gets no grid.
 * fine_dim governs bev_icp_point_to_point and bev_fine_registration_device_resident (d_ordered or packed offsets, with or
 * without a coarse table); coarse_dim governs bev_icp_point_to_plane and bev_coarse_registration_device_resident.  No
 * bev_submap_* call reads it: those keep bev_set_submap_search_grid, and neither setter reads the other's state.
 * Results never depend on it: the search is an exact 1-NN with the lowest target index on equal distance whatever the cell size
 * or the order inside a cell, so every result is bit for bit what D = 0 gives.  Only time and workspace do.  With c the capacity
 * of a slot (the call's largest cloud in the fine stage, stride in the coarse one) and cells = dim(c)^2:
 *   a target slot      4 (cells + 1) bytes of offsets in place of the fixed grid's 4 * 16385 (fine) or 4 * 4097 (coarse), and
 *                      56 bytes of tables and point count;
 *   a build group      the grids are built in groups of at most 256 targets, one group behind the other in front of the ICP
 *                      launches; a slot of ONE group takes 4 (cells + 1) bytes of counters plus 5 KiB of partial bounds and sums;
 *   the coarse stage   keeps the searchable points (16 bytes a row) for every frame of the call, not for its targets alone.
 * No synchronisation is needed around it: a call made before it and not yet finished keeps its grids.
 * Status: BEV_ERR_INVALID_ARG for a NULL context or a value outside 0 ... BEV_PAIR_SEARCH_GRID_MAX; nothing changes then. */
#define BEV_PAIR_SEARCH_GRID_MAX 1024
int bev_set_pair_search_grid(bev_ctx_t *ctx, int fine_dim, int coarse_dim);

/* ---- layout hint -------------------------------------------------------
 * What the caller knows about how its clouds are laid out, so that the library need not look (k_probe reads every 63rd
 * record of a frame to find out: 0.36 MB and 0.07 us of an HDL_64E frame).  Sticky per context; applies to frames of
 * exactly S = n_scan * horizon_scan records, every other frame is probed as ever:
 *   BEV_LAYOUT_STRUCTURED    what kitti_point_cloud_select writes (KittiPointCloudSelect.cpp:206-207,240) and what
 *                            bev_project_xyzi(BEV_PROJECT_KITTI_HDL_64E) returns (that call sets this hint by itself):
 *                            record i is the point of slot i, or all-zero;
 *   BEV_LAYOUT_FIRING_ORDER  the plain sweep in firing order (BASELINE config 3): record k is beam k % n_scan of firing
 *                            k / n_scan, its column the firing's number + 0 .. 8 or >= horizon_scan.  (What
 *                            mulran_point_cloud_select writes for REAL sweeps — MulranPointCloudSelect.cpp:112-130: any
 *                            start azimuth, either direction, staggered beams, no-return records — needs the sweep's
 *                            direction and a base column per row, which k_probe measures: no hint for it.)
 *   BEV_LAYOUT_UNKNOWN       (default) the library looks.
 * The hint is a guess like the library's own: the walk checks every record it reads, a frame that is not what the hint
 * said is done again the general way — a wrong hint costs time, never results (tests/test_gpu_structured.py). */
#define BEV_LAYOUT_UNKNOWN 0
#define BEV_LAYOUT_STRUCTURED 3
#define BEV_LAYOUT_FIRING_ORDER 4
int bev_set_layout_hint(bev_ctx_t *ctx, int layout);

/* ---- measurement ------------------------------------------------------- */
/* Sub-batches (max_batch frames) run as FUSED launches: one launch holds the column walk of sub-batch t and, as further
 * workgroups of the same grid, phase B of an earlier sub-batch, phase C of the one before that and the rasters of the one
 * before that; the launches alternate between two streams of equal priority (a sub-batch's stages stay on its stream),
 * over eight workspace sets; every kernel has one workgroup shape (256 threads, a quarter of a CU's LDS and registers).
 * bev_set_lanes(ctx, 1) makes every kernel a launch of its own, back to back (clean per-kernel durations for
 * profiling; the same device code); bev_set_lanes(ctx, n > 1) switches back.  Returns the number of workspace sets now
 * in rotation (1 or 8), or a negative status.  Environment of bev_create: BEV_LANES=1 starts serial; BEV_STREAM=0
 * sends every frame through the general path (order scan + gather walk); BEV_MODE_TTL=n: sub-batches for which a
 * layout's walk stays launched after the workspace set last saw the layout (default 8); BEV_CODE_CAP=n: entries of a
 * raster-band code list (tests); BEV_STAGE_STREAMS=n (1 .. 4, default 2): streams the fused launches take turns on, with
 * 4 n workspace sets.  These are all the knobs the library reads. */
int bev_set_lanes(bev_ctx_t *ctx, int n);

#define BEV_MAX_KERNELS 16
typedef struct bev_kernel_stat {
    const char *name;      /* kernel symbol as rocprofv3 prints it */
    uint64_t launches;     /* launches timed since the last reset */
    double total_ms;       /* sum of HIP-event durations on the ctx stream */
    uint64_t frames;       /* frames those launches covered */
} bev_kernel_stat_t;
/* When enabled, every kernel launch of bev_process_* is bracketed by HIP
 * events recorded on the context's own stream. */
int bev_profile_enable(bev_ctx_t *ctx, int on);
int bev_profile_reset(bev_ctx_t *ctx);
/* Synchronises, then fills up to `cap` entries; returns the number of kernels
 * (or a negative status). */
int bev_profile_get(bev_ctx_t *ctx, bev_kernel_stat_t *out, int cap);

/* ---- test hooks (used by tests/ only; not part of the reference surface) - */
/* Per-cell average ground heights of the LAST sub-batch processed (bev_process_batch works in chunks of
 * max(1, max_batch / 2) frames, bev_process_device_resident in sub-batches of max_batch): copies
 * n_frames * 3750 floats (ground_grid_avg_heights after BatchMultiBevGen.cpp:210), first_frame counted
 * from the start of that sub-batch. */
int bev_debug_get_cell_avg(bev_ctx_t *ctx, int first_frame, int n_frames, float *out);
/* Test hook: how the frames of the LAST sub-batch reached their slots (getOrderedCloud, BatchMultiBevGen.cpp:94-117).
 * out[4 * i .. 4 * i + 3] = { T, mode, consumed, failed } of frame first_frame + i.  mode 0 = order scan over all points
 * (general path); 1 = the first T points were read in place (sorted prefix, verified: consumed == T, failed == 0);
 * 2 = read in place, verification failed, done again the general way; 3 = a structured cloud of S records (record i =
 * slot i's point or all-zero; KittiPointCloudSelect.cpp:206-207,240) read in place (consumed == T == S; failed bit 1: an
 * all-zero record after the first was seen, bit 2: k_probe expected one); 4 = S returns in firing order
 * (MulranPointCloudSelect.cpp:112-130) read in place.  Results never depend on the mode (reading in place is the default
 * for frames that qualify; BEV_STREAM=0 in the environment of bev_create turns it off). */
int bev_debug_get_frame_info(bev_ctx_t *ctx, int first_frame, int n_frames, uint32_t *out);
/* Test hook: out[i] = how many raster-band code lists of frame first_frame + i of the LAST sub-batch did not hold their
 * codes (those bands of the frame's images were computed from the ordered cloud instead; normally 0; BEV_CODE_CAP in the
 * environment of bev_create shrinks the lists). */
int bev_debug_get_code_overflow(bev_ctx_t *ctx, int first_frame, int n_frames, uint32_t *out);
/* Evaluates the phase-A angle predicate (BatchMultiBevGen.cpp:169-179) on the
 * device for n (dx,dy,dz) triples given as HOST arrays; out[i] = 1 if GROUND. */
int bev_debug_angle_predicate(bev_ctx_t *ctx, const float *dx, const float *dy,
                              const float *dz, uint8_t *out, size_t n);
/* Test hook: one function of the arithmetic that host and device share (csrc/bev_exact.h, bev_libm.h, bev_libm_f64.h),
 * named by id, evaluated on the device for n elements given as HOST arrays.  Synchronous; its allocations are its own, so
 * it moves no workspace and leaves the other hooks' state alone.  in0..in3: element i of each array the id reads (f: float,
 * u: uint32_t, d: double; arrays the id does not read may be NULL); params: the floats the id takes once per call (NULL
 * where it takes none); out: one 32-bit word per element (an int, or a float's bits), two for a double (low word first),
 * three floats for BEV_EVAL_TRANSFORM_XYZ.  BEV_ERR_INVALID_ARG, with out untouched, for a NULL context, out, needed array
 * or needed params, an unknown id, and n above BEV_EVAL_MAX_N; n == 0 is BEV_OK.
 *   FD_ATANF f(x) | FD_ATAN2F f(y) f(x) | KITTI_AZIMUTH f(x) f(y) | KITTI_COL f(az) | KITTI_CROSSING f(az_prev) f(az)
 *   PROJECT_MULRAN u(k) f(x) f(y) and PROJECT_OXFORD f(x) f(y) f(z): row | col << 16
 *   FD_SIN, FD_COS d(x) | CVTT_F32 f(v) | CVTT_F64 d(v) | FLOOR_HALF_TO_INT f(nx) | GROUND_CELL f(x) f(y)
 *   ROUND_HALF_UP_BIN f(v) | HEIGHT_TIMES4 f(t) | BIN_IN_RANGE, BIN_OF_SHIFTED f(v) u(M): bin | in << 31
 *   BEV_BIN f(p) f(MAX_RANGE) f(interval) | COUNT_ADVANCE f(c) u(n), c >= 0.01f finite and n < 2^24 | EXACT_RECIPROCAL f(v)
 *   ANGLE_NODIV, ANGLE f(dx) f(dy) f(dz) | TRANSFORM_XYZ f(x) f(y) f(z), params: 12 floats of a row-major [R | t]
 *   DEGREES_OF f(rad) | WRAP_AZIMUTH f(az) | TO_U16 f(v)
 *   BEV_CODE f(px) f(py) f(pz), params: MAX_RANGE, interval, HEIGHT_RES, lidar_to_ground, n_layers: the code of label 1
 *   KITTI_COL_XY f(x) f(y): KITTI_COL of KITTI_AZIMUTH */
enum {
    BEV_EVAL_FD_ATANF = 0, BEV_EVAL_FD_ATAN2F, BEV_EVAL_KITTI_AZIMUTH, BEV_EVAL_KITTI_COL, BEV_EVAL_KITTI_CROSSING,
    BEV_EVAL_PROJECT_MULRAN, BEV_EVAL_PROJECT_OXFORD, BEV_EVAL_FD_SIN, BEV_EVAL_FD_COS, BEV_EVAL_CVTT_F32, BEV_EVAL_CVTT_F64,
    BEV_EVAL_FLOOR_HALF_TO_INT, BEV_EVAL_GROUND_CELL, BEV_EVAL_ROUND_HALF_UP_BIN, BEV_EVAL_HEIGHT_TIMES4, BEV_EVAL_BIN_IN_RANGE,
    BEV_EVAL_BIN_OF_SHIFTED, BEV_EVAL_BEV_BIN, BEV_EVAL_COUNT_ADVANCE, BEV_EVAL_EXACT_RECIPROCAL, BEV_EVAL_ANGLE_NODIV,
    BEV_EVAL_ANGLE, BEV_EVAL_TRANSFORM_XYZ, BEV_EVAL_DEGREES_OF, BEV_EVAL_WRAP_AZIMUTH, BEV_EVAL_TO_U16, BEV_EVAL_BEV_CODE,
    BEV_EVAL_KITTI_COL_XY, BEV_EVAL_COUNT
};
#define BEV_EVAL_MAX_N ((size_t)1 << 24)
int bev_debug_exact_eval(bev_ctx_t *ctx, int id, size_t n, const void *in0, const void *in1, const void *in2,
                         const void *in3, const float *params, void *out);

/* Test hook: the search grids of the LAST launch group of the last fine (coarse == 0) or coarse (coarse == 1) scan-to-map call
 * with matches, whichever path built them.  Synchronises.  out[4 * i .. 4 * i + 3] = { nx, ny, searchable points, largest count
 * of one cell } of map first_map + i of that group, the maps in the plan's order (ascending map index among the maps that a
 * match names).  BEV_ERR_INVALID_ARG for a NULL context or out, a range outside that group, before any such call, and once
 * another call has moved the stage's workspace. */
int bev_debug_get_submap_grid(bev_ctx_t *ctx, int coarse, int first_map, int n_maps, uint32_t *out);

/* Test hook: the search grids of the targets of the last fine (coarse == 0) or coarse (coarse == 1) PAIR call with matches,
 * whichever path built them.  Synchronises.  out[4 * i .. 4 * i + 3] = { nx, ny, searchable points, largest count of one cell } of
 * the grid of the target of match first_match + i of that call; bev_icp_point_to_point and bev_icp_point_to_plane count as one
 * match, index 0.  BEV_ERR_INVALID_ARG for a NULL context or out, a range outside that call's matches, before any such call, and
 * once another call (a scan-to-map one included) has used the stage's workspace. */
int bev_debug_get_pair_grid(bev_ctx_t *ctx, int coarse, int first_match, int n_matches, uint32_t *out);

/* ---- place retrieval: polar max-height descriptors and a match list -----------------------------------
 * A rotation-searching polar descriptor in the manner of Scan Context (Kim and Kim, IROS 2018), and the brute-force search
 * over all (query, candidate) pairs and all rotations that turns descriptors into the match list the registration calls
 * start from.  The contract, whose arithmetic is csrc/bev_place_exact.h's on the host and on the device alike:
 *   cell      r2 = x * x + y * y in float; ring k holds edge2[k] <= r2 < edge2[k + 1], edge2[k] = (float)(((double)max_range *
 *             k / n_rings)^2); a point contributes iff 0 < r2 < edge2[n_rings] (not the origin's no-return records, NaN, inf)
 *             and, with skip_label0, label != 0; sector = floorf(a * (float)n_sectors / 360.0f) clamped to n_sectors - 1, with
 *             a = the azimuth of fd_atan2f(y, x) in degrees (degrees_of), + 360.0f where negative: counter-clockwise from +x;
 *   value     min(127, max(0, (int)((z + lidar_to_ground) * 4))), the single-layer BEV's height code saturated at 127
 *             (lidar_to_ground: the context's); a cell holds the maximum over its points, 0 when empty;
 *   descriptor n_rings x n_sectors bytes, ring-major.  Of a map: that of the concatenation of bev_transform_cloud(frame, pose)
 *             over its entries (the moved x, y, z);
 *   columns   n2 = the sum of column s's squared values; unit[s][r] = (int)(127.0 * v / sqrt((double)n2) + 0.5) in double, 0
 *             where n2 == 0; a column with n2 > 0 is "non-empty";
 *   shift n   S_n = sum over j, r of unit_q[j][r] * unit_c[(j + n) % n_sectors][r]; cnt_n = the number of j with both columns
 *             non-empty.  Score a beats score b iff S_a * cnt_b > S_b * cnt_a in 64-bit integers; cnt == 0 loses to every
 *             cnt > 0; ties go to the lower shift.  distance = 1.0 - (double)S / (16129.0 * (double)cnt) of the pair's best
 *             shift, 2.0 when every shift has cnt == 0 (the shift is 0 then);
 *   yaw       angle_guess = n * (360 / n_sectors) degrees, less 360 where that is >= 180: the yaw with p_match ~
 *             Rz(angle_guess) p_query, what the registration calls take as bev_match_t::angle_guess;
 *   ranking   query q's candidates are 0 .. limit[q] - 1, ranked by the same comparison of their best shifts, ties to the
 *             lower candidate index.
 * Every output is integer work or a maximum: bit for bit whatever the launch shape. */
typedef struct bev_place_params {
    int32_t n_rings;     /* 4 ... 32 */
    int32_t n_sectors;   /* 8 ... 64 */
    float max_range;     /* finite, > 0: metres */
    int32_t skip_label0; /* 0 or 1: as for bev_float_bev */
} bev_place_params_t;
typedef struct bev_place_hit { /* its first twelve bytes are a bev_match_t */
    int32_t query_idx;
    int32_t match_idx;  /* -1: the query has fewer candidates than top_k */
    float angle_guess;  /* degrees, in [-180, 180) */
    int32_t shift;      /* sectors */
    double distance;    /* 1 - the mean cosine of the common columns; 2.0: no common column */
} bev_place_hit_t;
#define BEV_PLACE_MAX_TOP_K 64
/* Host only.  The defaults: 20 rings, 60 sectors, 80.0f m, skip_label0 1.  The bytes of a descriptor, n_rings * n_sectors, and
 * of the opaque per-descriptor record that bev_place_descriptor_device_resident writes and bev_place_match_device_resident
 * reads (a multiple of 64); both 0 for parameters outside the admitted values (params NULL: the defaults). */
bev_place_params_t bev_place_defaults(void);
size_t bev_place_descriptor_bytes(const bev_place_params_t *params);
size_t bev_place_desc_handle_bytes(const bev_place_params_t *params);
/* The descriptors of frames or of maps over packed frames in device memory; asynchronous, on the context's stream.
 * d_clouds, h_offsets : as for bev_float_bev_device_resident (records in the d_ordered layout).
 * n_maps, h_map_offsets, h_entry_frame, h_entry_pose : as for bev_submap_float_bev_device_resident: descriptor g is map g's.
 *                 All three arrays NULL with n_maps == 0: one descriptor per frame, from its RAW coordinates (not an identity
 *                 pose, as in bev_float_bev_device_resident), n_frames descriptors.
 * params        : NULL: the defaults.
 * d_desc        : the descriptors, bev_place_descriptor_bytes each, one after the other; NULL: not wanted.
 * d_units       : per descriptor one record of bev_place_desc_handle_bytes bytes, 64-byte aligned; NULL: not wanted.  Every
 *                 byte of every record is written.
 * Ordering      : as for bev_submap_float_bev_device_resident.
 * Status        : that call's argument and status rules, with BEV_ERR_INVALID_ARG for parameters outside the admitted values
 *                 (checked first, behind the context), for map arrays of which only some are NULL, for n_maps > 0 with NULL
 *                 h_map_offsets, for both outputs NULL and for a misaligned d_units.  Nothing is launched in any of these
 *                 cases.  No descriptors to make: BEV_OK.
 * Workspace     : a plane of 4 bytes per cell and descriptor, and the tables of the submap calls.  Freed by bev_destroy. */
int bev_place_descriptor_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                         int n_maps, const uint64_t *h_map_offsets, const int32_t *h_entry_frame,
                                         const float *h_entry_pose, const bev_place_params_t *params, uint8_t *d_desc,
                                         void *d_units);
/* The best top_k candidates of every query; asynchronous, on the context's stream, ordered like the call above.
 * d_units_q, d_units_db : n_queries and n_db records of bev_place_descriptor_device_resident under the SAME params.
 * h_limit       : n_queries values 0 ... n_db, query q's candidates being 0 .. h_limit[q] - 1; NULL: all of the database.
 * top_k         : 1 ... BEV_PLACE_MAX_TOP_K.
 * d_hits        : n_queries * top_k records, query q's at q * top_k in rank order; rows past the number of its candidates
 *                 have match_idx -1, distance 2.0, shift 0 and angle_guess 0.
 * Status        : BEV_ERR_INVALID_ARG for a NULL context, parameters outside the admitted values, negative counts, top_k
 *                 outside its range, a limit outside 0 ... n_db, NULL d_hits or d_units_q with n_queries > 0, NULL d_units_db
 *                 with n_db > 0.  n_queries == 0: BEV_OK.
 * Workspace     : 8 bytes per pair of a group of queries (groups of at most 64 MiB; BEV_PLACE_QUERY_GROUP=<queries> sets the
 *                 group, the results do not depend on it).  Freed by bev_destroy. */
int bev_place_match_device_resident(bev_ctx_t *ctx, const bev_place_params_t *params, int n_queries, const void *d_units_q,
                                    int n_db, const void *d_units_db, const int32_t *h_limit, int top_k,
                                    bev_place_hit_t *d_hits);
/* Both calls through HOST clouds, synchronous: every frame alone (raw coordinates) is a query, query q = frame q; the database
 * is the maps (n_maps of them), or — all three map arrays NULL and n_maps == 0 — the frames themselves.  h_limit, top_k and
 * hits (n_frames * top_k records) as above.  The frames go up through the context's input staging max_batch at a time. */
int bev_place_retrieval_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, int n_maps,
                              const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                              const bev_place_params_t *params, const int32_t *h_limit, int top_k, bev_place_hit_t *hits);

/* ---- verification of registered matches: two-way inlier counts --------------------------------------------
 * What "retrieve, register" lacks: under the transform a registration returned, how many points of each cloud have a neighbour
 * in the other within a distance, in both directions.  bev_icp_result_t::fitness is a mean over all source points without a cap,
 * and says nothing of how much of the target the query explains; these counts do.  The contract, for match
 * m = (query_idx, match_idx, .) with T = d_results[m].T (rows 0 ... 2):
 *   query cloud  : Q = bev_voxel_grid_irct(frame query_idx, leaf);
 *   moved point  : q' = (T0 x + (T1 y + (T2 z + T3)), T4 x + (T5 y + (T6 z + T7)), T8 x + (T9 y + (T10 z + T11))): the ICP's own
 *                  association, the very point the fitness is measured at;
 *   target cloud : the pair call: P = bev_voxel_grid_irct(frame match_idx, leaf); the submap call: the target of
 *                  bev_submap_voxel_registration_device_resident for (leaf, map_leaf): the concatenation in entry order, thinned
 *                  over the union when map_leaf > 0;
 *   searchable   : a point whose x, y and z are finite.  n_query counts the searchable q', n_target the searchable p;
 *   distance     : d(a, B) = the minimum over searchable b of the float (dx dx + dy dy) + dz dz (the ICP's expression; the same
 *                  float in either direction of the subtraction);
 *   counting     : a point counts at k iff (double)d <= (double)threshold[k] * (double)threshold[k] (the form of the ICP's
 *                  correspondence rule).  query_within[k] counts the searchable q' with d(q', P) inside the rule,
 *                  target_within[k] the searchable p with d(p, Q') inside it;
 *   empty cases  : every count is 0 when the other side has no searchable point or the map is empty; a NaN in T gives
 *                  n_query = 0 and all sixteen counts 0; slots k >= n_thresholds are 0; every byte of the record is written.
 * The outputs are integers: no float sum appears anywhere, and no output depends on an atomic's order, on the launch shape, on
 * how a cloud is cut into slices or a match list into groups.  No inlier mean or RMSE is returned on purpose: the thresholds
 * give the distribution. */
#define BEV_VERIFY_MAX_THRESHOLDS 8
typedef struct bev_verify_params {   /* 40 bytes */
    float leaf;                      /* the voxel grid of every frame: as bev_fine_registration_device_resident's leaf */
    int32_t n_thresholds;            /* 1 ... 8 */
    float threshold[8];              /* metres; the first n_thresholds finite, > 0, strictly ascending; the rest 0 */
} bev_verify_params_t;
typedef struct bev_verify_result {   /* 72 bytes */
    uint32_t n_query, n_target;      /* searchable points of the moved query / of the target */
    uint32_t query_within[8];        /* moved query points whose nearest target point is within threshold[k] */
    uint32_t target_within[8];       /* target points whose nearest moved query point is within threshold[k] */
} bev_verify_result_t;
/* leaf 0.2; thresholds 0.1, 0.2, 0.5, 1.0.  Host only. */
bev_verify_params_t bev_verify_defaults(void);
/* One problem on host clouds (synchronous), no voxel grid: params->leaf is ignored; only x, y, z are read.  T16: row-major
 * 4 x 4, rows 0 ... 2 read (NULL: BEV_ERR_INVALID_ARG).  params NULL: the defaults.  Parameters outside the ranges above ->
 * BEV_ERR_INVALID_ARG before anything is launched. */
int bev_verify_clouds(bev_ctx_t *ctx, const bev_point_t *src, uint32_t n_src, const bev_point_t *tgt, uint32_t n_tgt,
                      const float *T16, const bev_verify_params_t *params, bev_verify_result_t *result);
/* The counts of a list of registered matches, frame against frame, device-resident.
 * d_clouds, h_offsets : as bev_fine_registration_device_resident (h_offsets NULL: d_ordered, S records per frame)
 * h_matches           : n_matches HOST records; angle_guess is not read
 * d_results           : n_matches bev_icp_result_t (device); only .T is read, so bev_fine_registration_device_resident's output
 *                       goes in as it is, with no synchronisation between the two calls
 * d_verify            : n_matches records (device).  params NULL: the defaults.
 * Asynchronous and ordered exactly like the fine call: it starts behind every earlier call on the context and behind the
 * caller's default-stream work; bev_synchronize() before reading.  Everything the fine call refuses (bad offsets, match indices
 * out of range, a leaf that is not finite and > 0) and every parameter outside its range is BEV_ERR_INVALID_ARG before anything
 * is launched.
 * Workspace, allocated on first use (grown when a call needs more) and freed by bev_destroy: the fine call's per frame, with U, N
 * and K as there, U * (48 N + 4 * 16385 + 36) + min(U, 256) * (8 K + 4 N + 4) bytes, plus min(n_matches, 1024) *
 * (32 N + 4 * 16385 + 32) bytes of moved queries and their grids, plus the tables (16 bytes per frame, 24 per match).  The call
 * voxelises the frames itself: reusing the voxel clouds a preceding fine call left in the workspace is out of scope.  It always
 * runs the default search grids (at most 128 x 128 cells, one workgroup's build): bev_set_pair_search_grid and
 * bev_set_submap_search_grid are not read.  Matches run in launches of 1024 and a cloud's points in workgroups of 256
 * (BEV_VERIFY_SLICE=<points> sets the latter); no result depends on either. */
int bev_verify_registration_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets,
                                            int n_matches, const bev_match_t *h_matches, const bev_icp_result_t *d_results,
                                            const bev_verify_params_t *params, bev_verify_result_t *d_verify);
/* The same against maps: match_idx is a MAP's index, the maps, map_leaf and the limits (BEV_SUBMAP_MAX_ENTRIES,
 * BEV_SUBMAP_REG_MAX_TARGET) those of bev_submap_voxel_registration_device_resident, whose d_results go in as they are.  The
 * workspace is that call's, plus the moved queries and their grids as above. */
int bev_submap_verify_registration_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds,
                                                   const uint64_t *h_offsets, int n_maps, const uint64_t *h_map_offsets,
                                                   const int32_t *h_entry_frame, const float *h_entry_pose, float map_leaf,
                                                   int n_matches, const bev_match_t *h_matches,
                                                   const bev_icp_result_t *d_results, const bev_verify_params_t *params,
                                                   bev_verify_result_t *d_verify);
/* The pair call through HOST buffers, synchronous: clouds / n_pts as the other _batch forms, results n_matches HOST records of
 * which .T is read, verify n_matches HOST records. */
int bev_verify_registration_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts,
                                  int n_matches, const bev_match_t *h_matches, const bev_icp_result_t *results,
                                  const bev_verify_params_t *params, bev_verify_result_t *verify);

/* ---- a translation guess for retrieved pairs: height-grid offset search ---------------------------------
 * Place retrieval hands a pair over on a yaw alone.  This stage adds the translation in the plane: both clouds become small
 * Cartesian height grids, the query's is rotated by the yaw hypotheses of the hit, and an exhaustive search over whole-cell
 * shifts picks the shift with the highest correlation.  The output is the table of initial transforms that the fine calls
 * already take as d_coarse / d_best.  The contract, whose arithmetic is csrc/bev_align_exact.h's on the host and on the
 * device alike:
 *   grid      G x G bytes, byte [iy * G + ix].  A point contributes iff x * x + y * y > 0 in float (not the origin's no-return
 *             records, NaN), label != 0 where skip_label0 is set, and fx = floorf(x / cell), fy = floorf(y / cell) both satisfy
 *             -(float)(G / 2) <= f < (float)(G / 2), compared in float before any conversion; then ix = (int)fx + G / 2, iy
 *             likewise.  Its value is §6z's: min(127, max(0, (int)((z + lidar_to_ground) * 4))); a cell holds the maximum;
 *   candidate of a frame: from its raw coordinates; of a map: every point moved by its entry's matrix (the moved x, y, z);
 *   hypotheses for flip in {0, 1} and k in -K ... K: theta = angle_guess + (float)k * yaw_step in float, T = the registration
 *             tools' initial guess of (theta, flip) (a yaw of theta, or theta + 180, degrees about z); the query's grid under
 *             the hypothesis is the grid of its points moved by rows 0 ... 2 of T;
 *   score     of a shift (dx, dy) in [-S, S]^2: the sum over ix, iy of q[iy][ix] * c[iy + dy][ix + dx], a candidate byte
 *             outside the grid being 0; a 32-bit unsigned integer;
 *   orders    among the shifts of a hypothesis: higher score, then smaller dx^2 + dy^2, then smaller dy, then smaller dx; among
 *             the k of a flip: higher best score, then smaller |k|, then smaller k; best = 0 iff the best score of flip 0 >=
 *             that of flip 1;
 *   offset    per axis, only where both neighbours of the winning shift lie inside the window: in double, den = S- - 2 S0 + S+,
 *             off = den < 0 ? 0.5 (S- - S+) / den : 0, clamped to [-0.5, 0.5];
 *   result    [2m + flip]: T of the winning hypothesis with T[3] = (float)(((double)dx + off_x) * (double)cell) and T[7] from dy:
 *             p_candidate ~ T p_query; fitness = 1 - S / sqrt((double)Eq * (double)Ec), Eq and Ec the grids' sums of squares,
 *             2.0 where S == 0; converged = S > 0; iterations 0; state BEV_ICP_NOT_CONVERGED; _pad 0;
 *   no match  a hit with match_idx < 0 reads an empty candidate: S = 0, Ec = 0, shift (0, 0), k = 0.
 * Everything but the last few double operations is integer work or a maximum: no output depends on the launch shape, on a
 * group's size or on an atomic's order. */
typedef struct bev_align_params {   /* 24 bytes */
    int32_t grid;        /* G: even, 16 ... 128 */
    float cell;          /* finite, > 0: metres */
    int32_t max_shift;   /* S: 1 ... 16, and 2 S <= G / 2 */
    int32_t yaw_steps;   /* K: 0 ... 3 */
    float yaw_step;      /* finite, >= 0: degrees */
    int32_t skip_label0; /* 0 or 1: as for bev_float_bev */
} bev_align_params_t;
typedef struct bev_align_detail {   /* 36 bytes */
    int32_t dx, dy, k, flip;        /* the winning shift and hypothesis of (hit, flip) */
    uint32_t score, eq, ec;         /* its score and the two grids' sums of squares */
    float off_x, off_y;             /* the sub-cell offsets, in cells */
} bev_align_detail_t;
/* Host only.  The defaults: G 128, cell 0.5f, S 16, K 1, yaw_step 2.0f, skip_label0 1.  The bytes of a grid, G * G; 0 for
 * parameters outside the admitted values (params NULL: the defaults). */
bev_align_params_t bev_align_defaults(void);
size_t bev_align_grid_bytes(const bev_align_params_t *params);
/* The candidate grids of frames (n_maps == 0, the three map arrays NULL) or of maps over packed frames in device memory;
 * asynchronous, on the context's stream.  Arguments, ordering and statuses are bev_place_descriptor_device_resident's.
 * d_grids  : bev_align_grid_bytes per grid, one after the other.
 * d_energy : one uint32 per grid: its sum of squares.  Both are required where there is a grid to make.
 * Workspace: a plane of 4 bytes per cell and grid, and the tables of the submap calls.  Freed by bev_destroy. */
int bev_align_grid_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets, int n_maps,
                                   const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose,
                                   const bev_align_params_t *params, uint8_t *d_grids, uint32_t *d_energy);
/* The translation guesses of a hit list; asynchronous, on the context's stream, ordered like the place calls.
 * d_clouds, h_offsets : the queries' packed frames, as above.
 * n_db, d_grids, d_energy : the candidates, as the call above left them under the SAME params.
 * h_hits    : n_hits HOST records; query_idx in 0 ... n_frames - 1; match_idx in 0 ... n_db - 1, or negative (a
 *             bev_place_hit_t that found nothing).
 * d_results : 2 * n_hits records (device); d_best: n_hits int32 (device).  Both go into bev_fine_registration_device_resident
 *             and bev_submap_voxel_registration_device_resident as d_coarse and d_best with no synchronisation in between.
 * d_detail  : 2 * n_hits records (device), or NULL.  Every byte of every record of all three is written.
 * Status    : BEV_ERR_INVALID_ARG for a NULL context, parameters outside the admitted values, bad offsets, negative counts,
 *             an index out of range, NULL h_hits, d_results or d_best with n_hits > 0, NULL d_grids or d_energy where a hit
 *             names a candidate, NULL d_clouds where a hit's query has records.  Nothing is launched then.  n_hits == 0: BEV_OK.
 * Workspace : 32 bytes per hypothesis of a launch group of hits (BEV_ALIGN_GROUP=<hits> sets the group, the results do not
 *             depend on it) and 24 bytes per hit.  Freed by bev_destroy. */
int bev_align_hits_device_resident(bev_ctx_t *ctx, int n_frames, const bev_point_t *d_clouds, const uint64_t *h_offsets, int n_db,
                                   const uint8_t *d_grids, const uint32_t *d_energy, int n_hits, const bev_match_t *h_hits,
                                   const bev_align_params_t *params, bev_icp_result_t *d_results, int32_t *d_best,
                                   bev_align_detail_t *d_detail);
/* Both calls through HOST buffers, synchronous: the frames are the queries; the candidates are the maps (n_maps of them), or —
 * all three map arrays NULL and n_maps == 0 — the frames themselves.  results: 2 * n_hits, best: n_hits, detail: 2 * n_hits
 * HOST records or NULL. */
int bev_align_batch(bev_ctx_t *ctx, int n_frames, const bev_point_t *const *clouds, const uint32_t *n_pts, int n_maps,
                    const uint64_t *h_map_offsets, const int32_t *h_entry_frame, const float *h_entry_pose, int n_hits,
                    const bev_match_t *h_hits, const bev_align_params_t *params, bev_icp_result_t *results, int32_t *best,
                    bev_align_detail_t *detail);

int bev_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BEV_MI355X_H */
