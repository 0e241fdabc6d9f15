/*
 * batch_submap_registration          <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]
 * batch_submap_top_part_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]
 *
 * One source, built twice (BEV_SUBMAP_TOP_PART 0 / 1).  The first tool:
 *
 * Scan-to-map registration: batch_whole_registration with a LOCAL MAP as every match's target.  The match list
 * is batch_whole_registration's ("query match yaw" per line); the indices name the sorted files of
 * <root>/non_ground_point_cloud/, and row j of <root>/keyframe_pose.csv is file j's pose — what batch_submap_bev_gen and
 * batch_submap_cloud_manip read.  The map of match (q, m) holds the files j in [m - half_window, m + half_window], clipped to
 * the files, in ascending order, each under T_m^-1 T_j (submapwin::relativePose; j == m gets the exact identity); the query's
 * voxel cloud is registered against the map's moved voxel clouds from the yaw guess, with the whole tool's settings
 * (bev_icp_whole_defaults), by bev_submap_registration_device_resident.  half_window 0 is batch_whole_registration.
 * <map_leaf> > 0 thins every map by a voxel grid of that leaf over the union of its moved voxel clouds
 * (bev_submap_voxel_registration_device_resident); absent or 0: no second grid, the files as ever; negative or
 * not a finite number: refused with the usage line.
 *
 * Bookkeeping, summary line and [TIME] line are batch_whole_registration's (a match fails when its fitness exceeds 1.5); like
 * that tool it creates icp_precision_report_3d_icp_directly.txt in the working directory and writes nothing to it.  Beside
 * it, icp_precision_report_submap.txt gets one "diff_xy diff_yaw" line per successful match: the final transform against the
 * yaw guess it started from (the top-part tool's report arithmetic).  What the pose reader says goes to stderr: stdout is
 * batch_whole_registration's.  The matches go in chunks of consecutive matches
 * naming at most <chunk> distinct files (default 256, at least 2 * half_window + 2; the results do not depend on it).  Wrong
 * arguments, an unreadable match list or pose file, an index outside the files or an unreadable cloud exit 1.
 *
 * batch_submap_top_part_registration is batch_top_part_registration against the same windows: arguments, window
 * rule, chunking, refusals and the pose reader's redirection are those above.  Per chunk it runs the registration front end
 * on every file (leaf 0.2, radius 2, viewpoint 0), coarse point-to-plane ICP of the query's PointNormal cloud against the
 * window's moved PointNormal clouds from theta and theta + 180 (bev_submap_coarse_registration_device_resident, the coarse
 * defaults), then fine ICP from the better coarse result (bev_submap_voxel_registration_device_resident with the coarse table,
 * bev_icp_fine_defaults() and map_leaf).  Bookkeeping, both [TIME] lines, the summary line and the report file
 * (icp_precision_report.txt: the final transform against the chosen coarse one) are batch_top_part_registration's; with half_window
 * 0 and map_leaf 0 it is that tool.
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

#include "../csrc/bev_libm_f64.h"
#include "Registration.h"
#include "SubmapWindows.h"

#ifndef BEV_SUBMAP_TOP_PART
#define BEV_SUBMAP_TOP_PART 0
#endif

bev_ctx_t *bevhost_context(); /* BatchMultiBevGen.cpp (host) */

#if BEV_SUBMAP_TOP_PART
#define BEV_TOOL_NAME "batch_submap_top_part_registration"
#else
#define BEV_TOOL_NAME "batch_submap_registration"
#endif

namespace {

void hip_or_die(hipError_t e, const char *what)
{
    if (e != hipSuccess) {
        std::cerr << what << ": " << hipGetErrorString(e) << "\n";
        std::exit(2);
    }
}

#if BEV_SUBMAP_TOP_PART
void bev_or_die(int rc, const char *what)
{
    if (rc != BEV_OK) {
        std::cerr << what << ": " << bev_strerror(rc) << "\n";
        std::exit(2);
    }
}
#endif

const char kUsage[] = "Usage: " BEV_TOOL_NAME " <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]\n";

/* a finite number >= 0 and nothing else */
bool parse_map_leaf(const char *s, float *out)
{
    if (!s || !*s) return false;
    char *end = nullptr;
    const float v = std::strtof(s, &end);
    if (end == s || *end != '\0' || !std::isfinite(v) || v < 0.0f) return false;
    *out = v;
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::cerr << kUsage;
        return 1;
    }
    float map_leaf = 0.0f;
    if (argc > 5 && !parse_map_leaf(argv[5], &map_leaf)) {
        std::cerr << "map_leaf '" << argv[5] << "': expected a finite number >= 0\n" << kUsage;
        return 1;
    }
    std::string root(argv[2]);
    if (root.empty() || root.back() != '/') root.append("/");
    long half = 0, chunk = 256;
    if (!submapwin::parseCount(argv[3], 0, &half)) {
        std::cerr << "half_window '" << argv[3] << "': expected an integer >= 0\n";
        return 1;
    }
    if (argc > 4 && !submapwin::parseCount(argv[4], 2 * half + 2, &chunk)) {
        std::cerr << "chunk '" << argv[4] << "': expected an integer >= 2 * half_window + 2\n";
        return 1;
    }
    chunk = std::max(chunk, 2 * half + 2);
#if BEV_SUBMAP_TOP_PART
    std::ofstream report("./icp_precision_report.txt");
#else
    std::ofstream report("./icp_precision_report_3d_icp_directly.txt"), submap_report("./icp_precision_report_submap.txt");
#endif
    std::vector<MatchResult> matches;
    try {
        matches = loadMatchResults(argv[1]);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::vector<std::string> files;
    getPcdFileNames(root + "non_ground_point_cloud/", files);
    bool ok = false;
    std::streambuf *const out = std::cout.rdbuf(std::cerr.rdbuf()); /* the reader's chatter: off stdout, which is the whole tool's */
    const std::vector<Pose6f> pose = readKeyframePose(root + "keyframe_pose.csv", &ok);
    std::cout.rdbuf(out);
    if (!ok || pose.size() < files.size()) {
        std::cerr << "pose file " << root << "keyframe_pose.csv: can not be read, or fewer rows than clouds\n";
        return 1;
    }
    const long n_files = (long)files.size();
    for (const MatchResult &mt : matches)
        if (mt.query_idx < 0 || mt.query_idx >= n_files || mt.match_idx < 0 || mt.match_idx >= n_files) {
            std::cerr << "match " << mt.query_idx << " " << mt.match_idx << ": outside the " << n_files << " clouds\n";
            return 1;
        }
    sensor_params_ = getSensorParams(parseSensorType("HDL_64E")); /* (the context follows a sensor; packed clouds read none) */
    const bev_icp_params_t prm = BEV_SUBMAP_TOP_PART ? bev_icp_fine_defaults() : bev_icp_whole_defaults();
    double t_coarse = 0.0, t_fine = 0.0;
    int count_success = 0, count_failure = 0;
    using clk = std::chrono::steady_clock;

    for (size_t m0 = 0; m0 < matches.size();) {
        /* the chunk: consecutive matches whose queries and windows name at most `chunk` distinct files */
        std::map<long, int> local;
        size_t m1 = m0;
        while (m1 < matches.size()) {
            const long q = matches[m1].query_idx, m = matches[m1].match_idx;
            std::vector<long> add;
            if (!local.count(q)) add.push_back(q);
            for (long j = std::max(0L, m - half); j <= std::min(n_files - 1, m + half); ++j)
                if (!local.count(j) && j != q) add.push_back(j);
            if ((long)(local.size() + add.size()) > chunk) break;
            for (long f : add) local.emplace(f, (int)local.size());
            ++m1;
        }
        const int F = (int)local.size();
        std::vector<long> file_of(F);
        for (const auto &kv : local) file_of[kv.second] = kv.first;
        std::vector<uint64_t> offs(F + 1, 0);
        std::vector<pcl::PointCloud<pcl::PointXYZIRCT>> clouds(F);
        for (int f = 0; f < F; ++f) {
            if (bevio::loadPCDFile(files[file_of[f]], clouds[f]) != 0) {
                std::cerr << "Cloud NOT load file: " << files[file_of[f]] << "\n";
                return 1;
            }
            offs[f + 1] = offs[f] + clouds[f].points.size();
        }
        bev_ctx_t *ctx = bevhost_context();
        if (!ctx) return 2;
        /* one map per match (two matches of one key frame get two equal maps) */
        const size_t n = m1 - m0;
        std::vector<bev_match_t> cm(n);
        std::vector<uint64_t> map_offs(1, 0);
        std::vector<int32_t> entry_frame;
        std::vector<float> entry_pose;
        for (size_t k = 0; k < n; ++k) {
            const long m = matches[m0 + k].match_idx;
            cm[k] = bev_match_t{local[matches[m0 + k].query_idx], (int32_t)k, matches[m0 + k].angle_guess};
            for (long j = std::max(0L, m - half); j <= std::min(n_files - 1, m + half); ++j) {
                entry_frame.push_back(local[j]);
                entry_pose.resize(entry_pose.size() + 12);
                float *mat = entry_pose.data() + entry_pose.size() - 12;
                if (j == m) bev_yaw_translate_matrix(0.0f, 0.0f, 0.0f, 0.0f, mat); /* the exact identity */
                else submapwin::relativePose(pose[m], pose[j], mat);
            }
            map_offs.push_back(entry_frame.size());
        }
        auto t0 = clk::now();
        void *d_pts = nullptr, *d_fine = nullptr;
        hip_or_die(hipMalloc(&d_pts, std::max<uint64_t>(offs[F], 1) * sizeof(bev_point_t)), "hipMalloc");
        for (int f = 0; f < F; ++f)
            if (!clouds[f].points.empty())
                hip_or_die(hipMemcpy(static_cast<bev_point_t *>(d_pts) + offs[f], clouds[f].points.data(),
                                     clouds[f].points.size() * sizeof(bev_point_t), hipMemcpyHostToDevice),
                           "hipMemcpy");
        hip_or_die(hipMalloc(&d_fine, n * sizeof(bev_icp_result_t)), "hipMalloc");
#if BEV_SUBMAP_TOP_PART
        void *d_pn = nullptr, *d_cnt = nullptr, *d_coarse = nullptr, *d_best = nullptr;
        size_t n_max = 1;
        for (int f = 0; f < F; ++f) n_max = std::max<size_t>(n_max, offs[f + 1] - offs[f]);
        const size_t stride = bev_regfront_max_out(n_max);
        hip_or_die(hipMalloc(&d_pn, (size_t)F * stride * 48), "hipMalloc");
        hip_or_die(hipMalloc(&d_cnt, (size_t)F * 4), "hipMalloc");
        hip_or_die(hipMalloc(&d_coarse, n * 2 * sizeof(bev_icp_result_t)), "hipMalloc");
        hip_or_die(hipMalloc(&d_best, n * 4), "hipMalloc");
        const float vp[3] = {0.0f, 0.0f, 0.0f};
        bev_or_die(bev_registration_front_device_resident(ctx, F, static_cast<bev_point_t *>(d_pts), offs.data(), 0.2f, 2.0f, vp,
                                                          d_pn, stride, static_cast<uint32_t *>(d_cnt)),
                   "bev_registration_front_device_resident");
        bev_or_die(bev_submap_coarse_registration_device_resident(ctx, F, d_pn, stride, static_cast<uint32_t *>(d_cnt), (int)n,
                                                                  map_offs.data(), entry_frame.data(), entry_pose.data(), (int)n,
                                                                  cm.data(), nullptr, static_cast<bev_icp_result_t *>(d_coarse),
                                                                  static_cast<int32_t *>(d_best)),
                   "bev_submap_coarse_registration_device_resident");
        bev_or_die(bev_synchronize(ctx), "bev_synchronize");
        auto t1 = clk::now();
        bev_or_die(bev_submap_voxel_registration_device_resident(ctx, F, static_cast<bev_point_t *>(d_pts), offs.data(), 0.2f,
                                                                 map_leaf, (int)n, map_offs.data(), entry_frame.data(),
                                                                 entry_pose.data(), (int)n, cm.data(),
                                                                 static_cast<bev_icp_result_t *>(d_coarse),
                                                                 static_cast<int32_t *>(d_best), &prm,
                                                                 static_cast<bev_icp_result_t *>(d_fine)),
                   "bev_submap_voxel_registration_device_resident");
        bev_or_die(bev_synchronize(ctx), "bev_synchronize");
        auto t2 = clk::now();
        t_coarse += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t_fine += std::chrono::duration<double, std::milli>(t2 - t1).count();
        std::vector<bev_icp_result_t> fine(n), coarse(2 * n);
        std::vector<int32_t> best(n);
        hip_or_die(hipMemcpy(fine.data(), d_fine, n * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
        hip_or_die(hipMemcpy(coarse.data(), d_coarse, 2 * n * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
        hip_or_die(hipMemcpy(best.data(), d_best, n * 4, hipMemcpyDeviceToHost), "hipMemcpy");
        for (void *p : {d_pts, d_pn, d_cnt, d_coarse, d_best, d_fine}) (void)hipFree(p);
        for (size_t k = 0; k < n; ++k) {
            if (fine[k].fitness > 1.5f) {
                ++count_failure;
                continue;
            }
            ++count_success;
            float xy, yaw;
            icpPrecisionReport(fine[k].T, coarse[2 * k + (best[k] ? 1 : 0)].T, xy, yaw);
            report << xy << " " << yaw << "\n";
        }
#else
        int rc = map_leaf > 0.0f
                     ? bev_submap_voxel_registration_device_resident(ctx, F, static_cast<bev_point_t *>(d_pts), offs.data(), 0.2f,
                                                                     map_leaf, (int)n, map_offs.data(), entry_frame.data(),
                                                                     entry_pose.data(), (int)n, cm.data(), nullptr, nullptr,
                                                                     &prm, static_cast<bev_icp_result_t *>(d_fine))
                     : bev_submap_registration_device_resident(ctx, F, static_cast<bev_point_t *>(d_pts), offs.data(), 0.2f, (int)n,
                                                               map_offs.data(), entry_frame.data(), entry_pose.data(), (int)n,
                                                               cm.data(), nullptr, nullptr, &prm,
                                                               static_cast<bev_icp_result_t *>(d_fine));
        if (rc == BEV_OK) rc = bev_synchronize(ctx);
        if (rc != BEV_OK) {
            std::cerr << "bev_submap_registration_device_resident: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
            return 2;
        }
        t_fine += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        std::vector<bev_icp_result_t> fine(n);
        hip_or_die(hipMemcpy(fine.data(), d_fine, n * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
        (void)hipFree(d_pts);
        (void)hipFree(d_fine);
        for (size_t k = 0; k < n; ++k) {
            if (fine[k].fitness > 1.5f) {
                ++count_failure;
                continue;
            }
            ++count_success;
            float guess[16], xy, yaw;
            bevx::icp_tool_guess(cm[k].angle_guess, 0, guess);
            icpPrecisionReport(fine[k].T, guess, xy, yaw);
            submap_report << xy << " " << yaw << "\n";
        }
#endif
        m0 = m1;
    }
    t_coarse /= matches.size();
    t_fine /= matches.size();
    if (BEV_SUBMAP_TOP_PART) std::cout << "[TIME] Avg Tiempo for 1st Stage (coarse): " << t_coarse << "\n";
    std::cout << "[TIME] Avg Tiempo for 2nd Stage (fine): " << t_fine << "\n";
    std::cout << "count_success: " << count_success << ", count_failure: " << count_failure
              << ", SR: " << (1.0f * count_success) / (count_success + count_failure) << ". \n";
    report.close();
#if !BEV_SUBMAP_TOP_PART
    submap_report.close();
#endif
    return 0;
}
