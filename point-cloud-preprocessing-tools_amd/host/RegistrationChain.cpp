/* RegistrationChain.cpp — see RegistrationChain.h */
#include "RegistrationChain.h"

#include <algorithm>
#include <chrono>
#include <iostream>
#include <stdexcept>

#include <hip/hip_runtime_api.h>

#include "../csrc/bev_libm_f64.h"
#include "FileFormats.h"
#include "Registration.h"

namespace regchain {

namespace {

void hip_check(hipError_t e, const char *call)
{
    if (e != hipSuccess) throw std::runtime_error(std::string(call) + ": " + hipGetErrorString(e));
}
void bev_check(bev_ctx_t *ctx, int rc, const char *call)
{
    if (rc != BEV_OK) throw std::runtime_error(std::string(call) + ": " + bev_strerror(rc) + " " + bev_last_error(ctx));
}
/* a library call on ctx that throws, under its own name, unless it returns BEV_OK */
#define BEV_CALL(fn, ...) bev_check(ctx, fn(ctx, ##__VA_ARGS__), #fn)

template <class T> std::vector<T> downloaded(const DeviceBuffer &b, size_t n)
{
    std::vector<T> v(n);
    b.download(v.data(), n * sizeof(T));
    return v;
}

} // namespace

DeviceBuffer::DeviceBuffer(size_t bytes) { hip_check(hipMalloc(&p_, bytes), "hipMalloc"); }
DeviceBuffer::~DeviceBuffer() { (void)hipFree(p_); /* (nullptr: a no-op) */ }
void DeviceBuffer::upload(const void *src, size_t bytes, size_t offset)
{
    hip_check(hipMemcpy(static_cast<char *>(p_) + offset, src, bytes, hipMemcpyHostToDevice), "hipMemcpy");
}
void DeviceBuffer::download(void *dst, size_t bytes) const { hip_check(hipMemcpy(dst, p_, bytes, hipMemcpyDeviceToHost), "hipMemcpy"); }

ChunkResult runChunk(bev_ctx_t *ctx, const std::vector<Cloud> &clouds, const std::vector<uint64_t> &offs, const Chunk &chunk,
                     const std::vector<float> *entry_pose, float map_leaf, bool top_part, const bev_icp_params_t &fine_prm,
                     float pn_leaf, bool top_union, const bev_verify_params_t *verify, const bev_align_params_t *align)
{
    using clk = std::chrono::steady_clock;
    const int F = (int)clouds.size(), n = (int)chunk.matches.size();
    const bev_match_t *cm = chunk.matches.data();
    const uint64_t *map_offs = chunk.map_offs.data();
    const int32_t *entry_frame = chunk.entry_frame.data();

    const auto t0 = clk::now();
    DeviceBuffer pts(std::max<uint64_t>(offs[F], 1) * sizeof(bev_point_t));
    for (int f = 0; f < F; ++f)
        if (!clouds[f].points.empty())
            pts.upload(clouds[f].points.data(), clouds[f].points.size() * sizeof(bev_point_t), offs[f] * sizeof(bev_point_t));
    DeviceBuffer fine((size_t)n * sizeof(bev_icp_result_t));
    DeviceBuffer pn, cnt, coarse, best; /* the top part's; the whole tools hand the fine stage nullptr for the last two */
    if (top_part) {
        size_t n_max = 1;
        for (int f = 0; f < F; ++f) n_max = std::max<size_t>(n_max, offs[f + 1] - offs[f]);
        const size_t stride = bev_regfront_max_out(n_max);
        pn = DeviceBuffer((size_t)F * stride * 48);
        cnt = DeviceBuffer((size_t)F * 4);
        coarse = DeviceBuffer((size_t)n * 2 * sizeof(bev_icp_result_t));
        best = DeviceBuffer((size_t)n * 4);
        const float vp[3] = {0.0f, 0.0f, 0.0f};
        BEV_CALL(bev_registration_front_device_resident, F, pts.as<bev_point_t>(), offs.data(), 0.2f, 2.0f, vp, pn.as(), stride,
                 cnt.as<uint32_t>());
        if (entry_pose && pn_leaf > 0.0f && top_union) /* the top part over the union of the moved full clouds, thinned */
            BEV_CALL(bev_submap_top_part_coarse_registration_device_resident, F, pts.as<bev_point_t>(), offs.data(), pn.as(), stride,
                     cnt.as<uint32_t>(), pn_leaf, 2.0f, vp, n, map_offs, entry_frame, entry_pose->data(), n, cm, nullptr,
                     coarse.as<bev_icp_result_t>(), best.as<int32_t>());
        else if (entry_pose && pn_leaf > 0.0f) /* the maps thinned over their union, under the front end's settings */
            BEV_CALL(bev_submap_coarse_voxel_registration_device_resident, F, pn.as(), stride, cnt.as<uint32_t>(), pn_leaf, 2.0f, vp,
                     n, map_offs, entry_frame, entry_pose->data(), n, cm, nullptr, coarse.as<bev_icp_result_t>(), best.as<int32_t>());
        else if (entry_pose)
            BEV_CALL(bev_submap_coarse_registration_device_resident, F, pn.as(), stride, cnt.as<uint32_t>(), n, map_offs, entry_frame,
                     entry_pose->data(), n, cm, nullptr, coarse.as<bev_icp_result_t>(), best.as<int32_t>());
        else
            BEV_CALL(bev_coarse_registration_device_resident, F, pn.as(), stride, cnt.as<uint32_t>(), n, cm, nullptr,
                     coarse.as<bev_icp_result_t>(), best.as<int32_t>());
        BEV_CALL(bev_synchronize);
    }
    DeviceBuffer grids, energy, detail; /* the translation guess's: it fills coarse and best, which the fine stage reads at once */
    const bool aligned = align && !top_part;
    if (aligned) {
        const size_t n_db = entry_pose ? (size_t)n : (size_t)F, grid_bytes = bev_align_grid_bytes(align);
        if (!grid_bytes) throw std::runtime_error("bev_align_grid_bytes: parameters outside the admitted values");
        grids = DeviceBuffer(std::max<size_t>(n_db, 1) * grid_bytes);
        energy = DeviceBuffer(std::max<size_t>(n_db, 1) * sizeof(uint32_t));
        coarse = DeviceBuffer((size_t)n * 2 * sizeof(bev_icp_result_t));
        best = DeviceBuffer((size_t)n * 4);
        detail = DeviceBuffer((size_t)n * 2 * sizeof(bev_align_detail_t));
        BEV_CALL(bev_align_grid_device_resident, F, pts.as<bev_point_t>(), offs.data(), entry_pose ? n : 0, entry_pose ? map_offs : nullptr,
                 entry_pose ? entry_frame : nullptr, entry_pose ? entry_pose->data() : nullptr, align, grids.as<uint8_t>(),
                 energy.as<uint32_t>());
        BEV_CALL(bev_align_hits_device_resident, F, pts.as<bev_point_t>(), offs.data(), (int)n_db, grids.as<uint8_t>(),
                 energy.as<uint32_t>(), n, cm, align, coarse.as<bev_icp_result_t>(), best.as<int32_t>(), detail.as<bev_align_detail_t>());
    }
    const auto t1 = clk::now();
    if (entry_pose) /* with map_leaf 0 this is bev_submap_registration_device_resident, which forwards here */
        BEV_CALL(bev_submap_voxel_registration_device_resident, F, pts.as<bev_point_t>(), offs.data(), 0.2f, map_leaf, n, map_offs,
                 entry_frame, entry_pose->data(), n, cm, coarse.as<bev_icp_result_t>(), best.as<int32_t>(), &fine_prm,
                 fine.as<bev_icp_result_t>());
    else
        BEV_CALL(bev_fine_registration_device_resident, F, pts.as<bev_point_t>(), offs.data(), 0.2f, n, cm,
                 coarse.as<bev_icp_result_t>(), best.as<int32_t>(), &fine_prm, fine.as<bev_icp_result_t>());
    BEV_CALL(bev_synchronize);
    const auto t2 = clk::now();
    ChunkResult r;
    r.ms_first = std::chrono::duration<double, std::milli>(t1 - t0).count();
    r.ms_fine = std::chrono::duration<double, std::milli>(t2 - t1).count();
    r.fine = downloaded<bev_icp_result_t>(fine, n);
    if (top_part || aligned) r.coarse = downloaded<bev_icp_result_t>(coarse, 2 * (size_t)n), r.best = downloaded<int32_t>(best, n);
    if (aligned) r.align = downloaded<bev_align_detail_t>(detail, 2 * (size_t)n);
    if (verify) { /* the fine results stay where they are: only their transforms are read */
        DeviceBuffer counts(std::max<size_t>((size_t)n, 1) * sizeof(bev_verify_result_t));
        if (entry_pose)
            BEV_CALL(bev_submap_verify_registration_device_resident, F, pts.as<bev_point_t>(), offs.data(), n, map_offs, entry_frame,
                     entry_pose->data(), map_leaf, n, cm, fine.as<bev_icp_result_t>(), verify, counts.as<bev_verify_result_t>());
        else
            BEV_CALL(bev_verify_registration_device_resident, F, pts.as<bev_point_t>(), offs.data(), n, cm, fine.as<bev_icp_result_t>(),
                     verify, counts.as<bev_verify_result_t>());
        BEV_CALL(bev_synchronize);
        r.verify = downloaded<bev_verify_result_t>(counts, n);
    }
    return r;
}

void Tally::add(const Chunk &chunk, const ChunkResult &r)
{
    ms_first_ += r.ms_first;
    ms_fine_ += r.ms_fine;
    for (size_t k = 0; k < r.fine.size(); ++k) {
        if (r.fine[k].fitness > 1.5f) {
            ++failure_;
            continue;
        }
        ++success_;
        if (against_ == ReportAgainst::Nothing) continue;
        float guess[16], xy, yaw;
        if (against_ == ReportAgainst::YawGuess) bevx::icp_tool_guess(chunk.matches[k].angle_guess, 0, guess);
        icpPrecisionReport(r.fine[k].T, against_ == ReportAgainst::YawGuess ? guess : r.coarse[2 * k + (r.best[k] ? 1 : 0)].T, xy, yaw);
        *report_ << xy << " " << yaw << "\n";
    }
}

void Tally::print(std::ostream &out, bool coarse_line, bool fine_is_both) const
{
    const size_t n_matches = (size_t)(success_ + failure_);
    if (coarse_line) out << "[TIME] Avg Tiempo for 1st Stage (coarse): " << ms_first_ / n_matches << "\n";
    out << "[TIME] Avg Tiempo for 2nd Stage (fine): " << (fine_is_both ? ms_first_ + ms_fine_ : ms_fine_) / n_matches << "\n";
    out << "count_success: " << success_ << ", count_failure: " << failure_ << ", SR: " << (1.0f * success_) / (success_ + failure_)
        << ". \n";
}

int registerChunk(const std::vector<std::string> &paths, const Chunk &chunk, const std::vector<float> *entry_pose, float map_leaf,
                  bool top_part, const bev_icp_params_t &fine_prm, Tally &tally, float pn_leaf, bool top_union,
                  const bev_verify_params_t *verify, ChunkResult *result, const bev_align_params_t *align)
{
    std::vector<Cloud> clouds(paths.size());
    std::vector<uint64_t> offs(paths.size() + 1, 0);
    for (size_t f = 0; f < paths.size(); ++f) {
        if (bevio::loadPCDFile(paths[f], clouds[f]) != 0) {
            std::cerr << "Cloud NOT load file: " << paths[f] << "\n";
            return 1;
        }
        offs[f + 1] = offs[f] + clouds[f].points.size();
    }
    bev_ctx_t *ctx = bevhost_context();
    if (!ctx) return 2;
    try {
        ChunkResult r = runChunk(ctx, clouds, offs, chunk, entry_pose, map_leaf, top_part, fine_prm, pn_leaf, top_union, verify, align);
        tally.add(chunk, r);
        if (result) *result = std::move(r);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 2;
    }
    return 0;
}

} // namespace regchain
