/*
 * SubmapWindows.h — what the submap tools (batch_submap_bev_gen, batch_submap_cloud_manip) share: their
 * arguments, the sliding windows of key frames and the (frame, pose) entry lists of a batch of maps.  Host only, header only.
 *   windows    key index i = 0, stride, 2 * stride, ...: the files j in [i - half_window, i + half_window], clipped to the files
 *   matrix     of j in map i: T_i^-1 T_j, R = R_i^T R_j, t = R_i^T (t_j - t_i), evaluated in double from Pose6f's fields and
 *              rounded to float; j == i gets the exact identity
 */
#ifndef BEV_HOST_SUBMAPWINDOWS_H
#define BEV_HOST_SUBMAPWINDOWS_H

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "BatchMultiBevGen.h"
#include "FileFormats.h"
#include "LabelStep.h"

namespace submapwin {

/* a whole decimal integer of at least `least`, nothing behind it */
inline bool parseCount(const char *text, long least, long *out)
{
    char *end = nullptr;
    errno = 0;
    const long v = std::strtol(text, &end, 10);
    if (end == text || *end != '\0' || errno == ERANGE || v < least || v > 0x3fffffffL) return false;
    *out = v;
    return true;
}

/* T_i^-1 T_j as a row-major 3 x 4 float matrix */
inline void relativePose(const Pose6f &pi, const Pose6f &pj, float m[12])
{
    const double d[3] = {(double)pj.x - (double)pi.x, (double)pj.y - (double)pi.y, (double)pj.z - (double)pi.z};
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += pi.rotation_matrix[k][a] * pj.rotation_matrix[k][b];
            m[4 * a + b] = (float)r;
        }
        double t = 0.0;
        for (int k = 0; k < 3; ++k) t += pi.rotation_matrix[k][a] * d[k];
        m[4 * a + 3] = (float)t;
    }
}

/* file j's entry in the map of key file i, appended to entry_pose: T_i^-1 T_j, the key itself the exact identity.  The one rule
 * of every submap tool, BEV (loadBatch) and registration (batch_submap_registration_main.cpp) */
inline void appendEntryPose(const std::vector<Pose6f> &pose, long i, long j, std::vector<float> &entry_pose)
{
    entry_pose.resize(entry_pose.size() + 12);
    float *mat = entry_pose.data() + entry_pose.size() - 12;
    if (j == i) bev_yaw_translate_matrix(0.0f, 0.0f, 0.0f, 0.0f, mat); /* the exact identity */
    else relativePose(pose[i], pose[j], mat);
}

/* What a tool's command line and <root> say: argv[1 .. 4] = root, sensor, half_window, [stride] (argc >= 4 checked by the
 * caller, which prints its own usage), the sorted files of <root>/non_ground_point_cloud/ and row j of
 * <root>/keyframe_pose.csv for file j. */
struct Setup {
    std::string root; /* with its closing '/' */
    bev_params_t bp;
    long half = 0, stride = 1;
    std::vector<std::string> files;
    std::vector<Pose6f> pose;
    long n_files = 0, n_keys = 0;
};
/* false: a wrong argument, an unreadable pose file or one with fewer rows than there are clouds, said on stderr; no GPU
 * context exists yet */
inline bool readSetup(int argc, char **argv, Setup &s)
{
    s.root = argv[1];
    if (s.root.empty() || s.root.back() != '/') s.root.append("/");
    if (bev_params_for_sensor(argv[2], &s.bp) != BEV_OK) {
        std::cerr << "Unknown sensor type " << argv[2] << " (HDL_32E, HDL_64E or OS1_64)\n";
        return false;
    }
    if (!parseCount(argv[3], 0, &s.half)) {
        std::cerr << "half_window '" << argv[3] << "': expected an integer >= 0\n";
        return false;
    }
    if (argc > 4 && argv[4] != nullptr && !parseCount(argv[4], 1, &s.stride)) {
        std::cerr << "stride '" << argv[4] << "': expected an integer >= 1\n";
        return false;
    }
    getPcdFileNames(s.root + "non_ground_point_cloud/", s.files);
    bool ok = false;
    s.pose = readKeyframePose(s.root + "keyframe_pose.csv", &ok);
    if (!ok) {
        std::cerr << "pose file " << s.root << "keyframe_pose.csv: can not be read\n";
        return false;
    }
    if (s.pose.size() < s.files.size()) {
        std::cerr << "pose file " << s.root << "keyframe_pose.csv: " << s.pose.size() << " rows for " << s.files.size() << " clouds\n";
        return false;
    }
    s.n_files = (long)s.files.size();
    s.n_keys = (s.n_files + s.stride - 1) / s.stride;
    return true;
}
/* the maps of one call: BEV_BATCH (default 32), at most the keys; and the context for them, sized by BEV_MAX_POINTS (default
 * 4 Mi points per cloud).  nullptr: bev_create failed, said on stderr */
inline int batchSize(const Setup &s)
{
    return (int)std::max<long>(1, std::min<long>(std::max(1, std::atoi(std::getenv("BEV_BATCH") ? std::getenv("BEV_BATCH") : "32")), s.n_keys));
}
inline bev_ctx_t *createContext(const Setup &s, int batch)
{
    const long long max_pts_env = std::getenv("BEV_MAX_POINTS") ? std::atoll(std::getenv("BEV_MAX_POINTS")) : 0;
    bev_ctx_t *ctx = nullptr;
    const int rc0 = bev_create(&ctx, 0, &s.bp, batch, max_pts_env > 0 ? (size_t)max_pts_env : ((size_t)4 << 20));
    if (rc0 != BEV_OK) {
        std::cerr << "bev_create failed: " << bev_strerror(rc0) << "\n";
        return nullptr;
    }
    return ctx;
}

/* The maps of keys k0 .. k0 + nb - 1 as one submap call: the files they name, loaded as the call's frames (an unreadable PCD
 * is reported and goes on as an empty cloud), and the three entry arrays. */
struct Batch {
    std::vector<pcl::PointCloud<pcl::PointXYZIRCT>> in;
    std::vector<long> loaded; /* the files of the batch, ascending: frame f of the call is file loaded[f] */
    std::vector<const bev_point_t *> clouds;
    std::vector<uint32_t> n_pts;
    std::vector<uint64_t> map_offs;
    std::vector<int32_t> entry_frame;
    std::vector<float> entry_pose;
};
inline void loadBatch(const Setup &s, long k0, int nb, Batch &b)
{
    const long half = s.half, stride = s.stride, n_files = s.n_files;
    b.loaded.clear();
    for (int m = 0; m < nb; ++m) { /* (the windows ascend with the keys: what is new lies behind what is there) */
        const long i = (k0 + m) * stride;
        for (long j = std::max(std::max(0L, i - half), b.loaded.empty() ? 0L : b.loaded.back() + 1); j <= std::min(n_files - 1, i + half); ++j)
            b.loaded.push_back(j);
    }
    b.in.resize(b.loaded.size());
    b.clouds.resize(b.loaded.size());
    b.n_pts.resize(b.loaded.size());
    for (size_t f = 0; f < b.loaded.size(); ++f) {
        b.in[f].clear(); /* an unreadable file goes on as an empty cloud */
        if (bevio::loadPCDFile(s.files[b.loaded[f]], b.in[f]) != 0) std::cerr << "Can not read " << s.files[b.loaded[f]] << "\n";
        b.clouds[f] = b.in[f].size() ? reinterpret_cast<const bev_point_t *>(b.in[f].points.data()) : nullptr;
        b.n_pts[f] = (uint32_t)b.in[f].size();
    }
    b.map_offs.assign(1, 0);
    b.entry_frame.clear();
    b.entry_pose.clear();
    for (int m = 0; m < nb; ++m) {
        const long i = (k0 + m) * stride;
        for (long j = std::max(0L, i - half); j <= std::min(n_files - 1, i + half); ++j) {
            b.entry_frame.push_back((int32_t)(std::lower_bound(b.loaded.begin(), b.loaded.end(), j) - b.loaded.begin()));
            appendEntryPose(s.pose, i, j, b.entry_pose);
        }
        b.map_offs.push_back(b.entry_frame.size());
    }
}
/* the key frame's file name without directory and extension: what its outputs are called */
inline std::string keyName(const Setup &s, long key)
{
    const std::string &path = s.files[key * s.stride];
    const size_t start_pos = path.find_last_of('/') + 1, end_pos = path.find_last_of('.');
    return path.substr(start_pos, end_pos - start_pos);
}

} // namespace submapwin

#endif
