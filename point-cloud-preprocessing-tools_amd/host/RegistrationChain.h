/*
 * RegistrationChain.h — the one host program under the four batch registration tools (batch_top_part_registration,
 * batch_whole_registration, batch_submap_registration, batch_submap_top_part_registration).  A tool's main() reads
 * its arguments and says which file an index names; then, per chunk of matches (RegistrationChunks.h):
 *   load         the chunk's files, packed one behind the other
 *   runChunk     uploads, [front end, coarse ICP,] synchronise, fine ICP, synchronise, downloads — against the matches' target
 *                frames, or against their maps
 *   Tally        a match fails when its fitness exceeds 1.5; the report line of one that does not; the closing lines
 * registerChunk is the three in a row.  A HIP or library failure throws std::runtime_error naming the call; device memory is
 * owned, so every way out frees it.
 */
#ifndef BEV_HOST_REGISTRATIONCHAIN_H
#define BEV_HOST_REGISTRATIONCHAIN_H

#include <iosfwd>
#include <string>
#include <utility>
#include <vector>

#include "PointCloud.h"
#include "RegistrationChunks.h"

bev_ctx_t *bevhost_context(); /* BatchMultiBevGen.cpp: the free functions' context, created at the first call */

namespace regchain {

/* device memory that frees itself: hipMalloc / hipFree; move-only; default-constructed it holds nullptr */
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes);
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { return std::swap(p_, o.p_), *this; }
    ~DeviceBuffer();
    template <class T = void> T *as() const { return static_cast<T *>(p_); }
    void upload(const void *src, size_t bytes, size_t offset = 0);
    void download(void *dst, size_t bytes) const;

private:
    void *p_ = nullptr;
};

using Cloud = pcl::PointCloud<pcl::PointXYZIRCT>;

struct ChunkResult {
    std::vector<bev_icp_result_t> fine;   /* per match */
    std::vector<bev_icp_result_t> coarse; /* top part: per match, from the guess and from the guess + 180 */
    std::vector<int32_t> best;            /* top part: which of the two the fine stage started from */
    std::vector<bev_verify_result_t> verify; /* per match, where runChunk was handed verification parameters; else empty */
    /* where runChunk was handed alignment parameters (and not top_part): per match and flip the translation guess's detail;
     * coarse and best are then its table, what the fine stage started from; else empty */
    std::vector<bev_align_detail_t> align;
    double ms_first = 0.0; /* from before the first allocation to the synchronise behind coarse ICP (whole: the uploads) */
    double ms_fine = 0.0;  /* the fine stage and its synchronise */
};

/* The chain on one chunk: frame f is clouds[f], offs[f] its first point in the packed array.  entry_pose null: every match
 * against its target frame (chunk.matches[k].match_idx); else against its map (chunk.map_offs, chunk.entry_frame, 12 floats of
 * *entry_pose per entry), thinned by map_leaf if that is > 0.  top_part: front end (leaf 0.2, radius 2, viewpoint 0) and coarse
 * ICP, then fine ICP from the better coarse result; else fine ICP from the yaw guess.  pn_leaf > 0 (top_part against maps): the
 * coarse stage's maps are thinned over their union and their normals recomputed there, with the front end's radius and viewpoint
 * (bev_submap_coarse_voxel_registration_device_resident); with top_union as well, the coarse stage's maps are the
 * top part over the union of the entries' moved FULL clouds, thinned the same way, the front end's rows being the queries
 * (bev_submap_top_part_coarse_registration_device_resident).  verify not null: behind the fine stage and outside its
 * time, the two-way inlier counts of every match under its final transform, against the same targets; null, the
 * default: exactly the chain without them.  align not null and not top_part: ahead of the fine stage, the height grids of the
 * matches' targets (the frames, or the chunk's maps) and the translation guess of every match, whose table the
 * fine stage starts from in place of the yaw guess, with no synchronisation in between; null, the default: the chain as ever */
ChunkResult runChunk(bev_ctx_t *ctx, const std::vector<Cloud> &clouds, const std::vector<uint64_t> &offs, const Chunk &chunk,
                     const std::vector<float> *entry_pose, float map_leaf, bool top_part, const bev_icp_params_t &fine_prm,
                     float pn_leaf = 0.0f, bool top_union = false, const bev_verify_params_t *verify = nullptr,
                     const bev_align_params_t *align = nullptr);

/* what a successful match's "diff_xy diff_yaw" line compares its final transform with */
enum class ReportAgainst { Nothing, ChosenCoarse, YawGuess };

class Tally {
public:
    Tally(std::ostream *report, ReportAgainst against) : report_(report), against_(against) {}
    void add(const Chunk &chunk, const ChunkResult &r);
    /* the [TIME] lines (ms per match; the first only with coarse_line; fine_is_both: the fine line is both stages) and the summary */
    void print(std::ostream &out, bool coarse_line, bool fine_is_both) const;

private:
    std::ostream *report_;
    ReportAgainst against_;
    int success_ = 0, failure_ = 0;
    double ms_first_ = 0.0, ms_fine_ = 0.0;
};

/* The files paths[f] as the chunk's frames, the context (after the files: an unreadable one ends the tool first), runChunk, Tally::add.  0, or the tool's exit
 * status with the reason on stderr: 1 an unreadable cloud, 2 no context or a failed call.  verify, align: runChunk's; result not
 * null: it gets what runChunk returned */
int registerChunk(const std::vector<std::string> &paths, const Chunk &chunk, const std::vector<float> *entry_pose, float map_leaf,
                  bool top_part, const bev_icp_params_t &fine_prm, Tally &tally, float pn_leaf = 0.0f, bool top_union = false,
                  const bev_verify_params_t *verify = nullptr, ChunkResult *result = nullptr,
                  const bev_align_params_t *align = nullptr);

} // namespace regchain

#endif
