/*
 * batch_top_part_registration <match_list> <pcd_dir> [max_frames]     (BatchTopPartRegistration.cpp:311-571)
 * batch_whole_registration    <match_list> <pcd_dir> [max_frames]     (BatchWholeRegistration.cpp:310-436)
 *
 * One source, built twice (BEV_WHOLE_TOOL 0 / 1).  Same command line, input files and report file as the reference's
 * tools: the match list (loadMatchResults), the labelled clouds <pcd_dir>/%06d.pcd, the report in the working directory
 * (icp_precision_report.txt: one "diff_xy diff_yaw" line per successful match; the whole tool creates
 * icp_precision_report_3d_icp_directly.txt and writes nothing to it, as the reference does), and the reference's summary
 * line.  The chain runs on the GPU without a host round trip between its stages — top-part tool: front end (§6b), coarse
 * ICP (§6c), fine ICP (§6d); whole tool: fine ICP from the yaw guess — over chunks of consecutive matches that name at
 * most max_frames distinct frames (default 256; the results do not depend on it).
 *
 * Differs from the reference: no per-match chatter (the "Processing match", [TIME] and transform lines); the two
 * "[TIME] Avg Tiempo" lines are the chain's wall time per match in ms (coarse: file reading excluded, front end and
 * coarse ICP; fine: the fine stage), not the reference's per-match stopwatch; an unreadable file ends the tool with exit
 * status 1 before anything is written to the report.
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "BatchMultiBevGen.h"
#include "FileFormats.h"
#include "Registration.h"
#include "Utility.h"

#ifndef BEV_WHOLE_TOOL
#define BEV_WHOLE_TOOL 0
#endif

bev_ctx_t *bevhost_context(); /* BatchMultiBevGen.cpp (host) */

namespace {

void hip_or_die(hipError_t e, const char *what)
{
    if (e != hipSuccess) {
        std::cerr << what << ": " << hipGetErrorString(e) << "\n";
        std::exit(2);
    }
}

void bev_or_die(int rc, const char *what)
{
    if (rc != BEV_OK) {
        std::cerr << what << ": " << bev_strerror(rc) << "\n";
        std::exit(2);
    }
}

std::string cloud_path(const std::string &dir, int idx)
{
    char name[32];
    std::snprintf(name, sizeof(name), "%06d.pcd", idx);
    return (!dir.empty() && dir.back() == '/') ? dir + name : dir + "/" + name;
}

} // namespace

int main(int argc, char **argv)
{
    const char *tool = BEV_WHOLE_TOOL ? "batch_whole_registration" : "batch_top_part_registration";
    if (argc < 3) {
        std::cerr << "Usage: " << tool << " <match_list> <pcd_dir> [max_frames]\n";
        return 1;
    }
    const std::string match_list(argv[1]), pcd_dir(argv[2]);
    const int max_frames = argc > 3 ? std::atoi(argv[3]) : 256;
    if (max_frames < 2) {
        std::cerr << "max_frames must be at least 2\n";
        return 1;
    }
    std::ofstream report(BEV_WHOLE_TOOL ? "./icp_precision_report_3d_icp_directly.txt" : "./icp_precision_report.txt");
    std::vector<MatchResult> matches;
    try {
        matches = loadMatchResults(match_list);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    /* the free functions' context follows a sensor; the registration stages read no sensor setting (packed clouds) */
    sensor_params_ = getSensorParams(parseSensorType("HDL_64E"));
    const bev_icp_params_t fine_prm = BEV_WHOLE_TOOL ? bev_icp_whole_defaults() : bev_icp_fine_defaults();
    double t_coarse = 0.0, t_fine = 0.0;
    int count_success = 0, count_failure = 0;
    using clk = std::chrono::steady_clock;

    for (size_t m0 = 0; m0 < matches.size();) {
        /* the chunk: consecutive matches naming at most max_frames distinct frames */
        std::map<int, int> local;
        size_t m1 = m0;
        while (m1 < matches.size()) {
            const int add = (local.count(matches[m1].query_idx) ? 0 : 1) +
                            (local.count(matches[m1].match_idx) || matches[m1].match_idx == matches[m1].query_idx ? 0 : 1);
            if ((int)local.size() + add > max_frames) break;
            for (int f : {matches[m1].query_idx, matches[m1].match_idx})
                if (!local.count(f)) local.emplace(f, (int)local.size());
            ++m1;
        }
        const int F = (int)local.size();
        std::vector<int> frame_of(F);
        for (const auto &kv : local) frame_of[kv.second] = kv.first;
        std::vector<uint64_t> offs(F + 1, 0);
        std::vector<pcl::PointCloud<pcl::PointXYZIRCT>> clouds(F);
        for (int f = 0; f < F; ++f) {
            const std::string path = cloud_path(pcd_dir, frame_of[f]);
            if (bevio::loadPCDFile(path, clouds[f]) != 0) {
                std::cerr << "Cloud NOT load file: " << path << "\n";
                return 1;
            }
            offs[f + 1] = offs[f] + clouds[f].points.size();
        }
        bev_ctx_t *ctx = bevhost_context(); /* (after the first files: an unreadable one ends the tool first) */
        if (!ctx) return 2;
        std::vector<bev_match_t> cm(m1 - m0);
        for (size_t k = 0; k < cm.size(); ++k)
            cm[k] = bev_match_t{local[matches[m0 + k].query_idx], local[matches[m0 + k].match_idx], matches[m0 + k].angle_guess};
        const size_t n = cm.size();

        auto t0 = clk::now();
        void *d_pts = nullptr, *d_pn = nullptr, *d_cnt = nullptr, *d_coarse = nullptr, *d_best = nullptr, *d_fine = nullptr;
        hip_or_die(hipMalloc(&d_pts, std::max<uint64_t>(offs[F], 1) * sizeof(bev_point_t)), "hipMalloc");
        for (int f = 0; f < F; ++f)
            if (!clouds[f].points.empty())
                hip_or_die(hipMemcpy(static_cast<bev_point_t *>(d_pts) + offs[f], clouds[f].points.data(),
                                     clouds[f].points.size() * sizeof(bev_point_t), hipMemcpyHostToDevice),
                           "hipMemcpy");
        hip_or_die(hipMalloc(&d_fine, n * sizeof(bev_icp_result_t)), "hipMalloc");
        std::vector<bev_icp_result_t> coarse;
        std::vector<int32_t> best;
        if (!BEV_WHOLE_TOOL) {
            size_t n_max = 1;
            for (int f = 0; f < F; ++f) n_max = std::max<size_t>(n_max, offs[f + 1] - offs[f]);
            const size_t stride = bev_regfront_max_out(n_max);
            hip_or_die(hipMalloc(&d_pn, (size_t)F * stride * 48), "hipMalloc");
            hip_or_die(hipMalloc(&d_cnt, (size_t)F * 4), "hipMalloc");
            hip_or_die(hipMalloc(&d_coarse, n * 2 * sizeof(bev_icp_result_t)), "hipMalloc");
            hip_or_die(hipMalloc(&d_best, n * 4), "hipMalloc");
            const float vp[3] = {0.0f, 0.0f, 0.0f};
            bev_or_die(bev_registration_front_device_resident(ctx, F, static_cast<bev_point_t *>(d_pts), offs.data(), 0.2f,
                                                              2.0f, vp, d_pn, stride, static_cast<uint32_t *>(d_cnt)),
                       "bev_registration_front_device_resident");
            bev_or_die(bev_coarse_registration_device_resident(ctx, F, d_pn, stride, static_cast<uint32_t *>(d_cnt), (int)n,
                                                               cm.data(), nullptr, static_cast<bev_icp_result_t *>(d_coarse),
                                                               static_cast<int32_t *>(d_best)),
                       "bev_coarse_registration_device_resident");
            bev_or_die(bev_synchronize(ctx), "bev_synchronize");
        }
        auto t1 = clk::now();
        bev_or_die(bev_fine_registration_device_resident(ctx, F, static_cast<bev_point_t *>(d_pts), offs.data(), 0.2f, (int)n,
                                                         cm.data(), static_cast<bev_icp_result_t *>(d_coarse),
                                                         static_cast<int32_t *>(d_best), &fine_prm,
                                                         static_cast<bev_icp_result_t *>(d_fine)),
                   "bev_fine_registration_device_resident");
        bev_or_die(bev_synchronize(ctx), "bev_synchronize");
        auto t2 = clk::now();
        t_coarse += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t_fine += std::chrono::duration<double, std::milli>(t2 - t1).count();
        std::vector<bev_icp_result_t> fine(n);
        hip_or_die(hipMemcpy(fine.data(), d_fine, n * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
        if (!BEV_WHOLE_TOOL) {
            coarse.resize(2 * n);
            best.resize(n);
            hip_or_die(hipMemcpy(coarse.data(), d_coarse, 2 * n * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
            hip_or_die(hipMemcpy(best.data(), d_best, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        for (void *p : {d_pts, d_pn, d_cnt, d_coarse, d_best, d_fine})
            if (p) (void)hipFree(p);
        for (size_t k = 0; k < n; ++k) {
            if (fine[k].fitness > 1.5f) {
                ++count_failure;
                continue;
            }
            ++count_success;
            if (!BEV_WHOLE_TOOL) {
                float xy, yaw;
                icpPrecisionReport(fine[k].T, coarse[2 * k + (best[k] ? 1 : 0)].T, xy, yaw);
                report << xy << " " << yaw << "\n";
            }
        }
        m0 = m1;
    }
    t_coarse /= matches.size();
    t_fine /= matches.size();
    if (!BEV_WHOLE_TOOL) std::cout << "[TIME] Avg Tiempo for 1st Stage (coarse): " << t_coarse << "\n";
    std::cout << "[TIME] Avg Tiempo for 2nd Stage (fine): " << t_fine << "\n";
    std::cout << "count_success: " << count_success << ", count_failure: " << count_failure
              << ", SR: " << (1.0f * count_success) / (count_success + count_failure) << ". \n";
    report.close();
    return 0;
}
