/*
 * batch_submap_bev_gen <keyframes_root_dir> <sensor_type> <half_window> [<stride>]
 *
 * The 24-layer occupancy BEV and the single-layer BEV of LOCAL MAPS: for key index i = 0, stride, 2 * stride, ... (stride
 * defaults to 1) the labelled clouds j in [i - half_window, i + half_window] (clipped to the files) that batch_multi_bev_gen
 * left in <root>/non_ground_point_cloud/, each moved into key frame i's coordinates and all rastered into one image pair
 * (DESIGN.md §6i).  The files are taken in sorted order; row j of <root>/keyframe_pose.csv (readKeyframePose) is file j's pose.
 *   matrix of j in map i   T_i^-1 T_j: R = R_i^T R_j, t = R_i^T (t_j - t_i), evaluated in double from Pose6f's fields and
 *                          rounded to float; j == i gets the exact identity
 *   writes                 <root>/output_submap_bev/binary/<key name>.bin  the .bin payload of batch_multi_bev_gen
 *                          <root>/output_submap_bev/csv/<key name>.csv     its single-layer CSV
 *                          (both directories are recreated; no PNGs)
 * The maps go BEV_BATCH at a time (default 32) through one bev_submap_bev_batch call; only the files a batch names are loaded.
 * Pose6f keeps positions as floats, as the reference does: with large coordinates (UTM) the relative translations are only
 * as fine as a float of that size.  Wrong arguments, an unreadable pose file or one with fewer rows than there are clouds
 * exit 1 before a GPU context is created; an unreadable PCD is reported and goes on as an empty cloud.
 * BEV_MAX_POINTS=P: points per cloud the context is sized for (default 4 Mi).
 */
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "BatchMultiBevGen.h"
#include "FileFormats.h"
#include "LabelStep.h"

void bevhost_recreate_dir(const std::string &dir); /* BatchMultiBevGen.cpp (host): rm -rf + mkdir -p */

namespace {

/* a whole decimal integer of at least `least`, nothing behind it */
bool parseCount(const char *text, long least, long *out)
{
    char *end = nullptr;
    errno = 0;
    const long v = std::strtol(text, &end, 10);
    if (end == text || *end != '\0' || errno == ERANGE || v < least || v > 0x3fffffffL) return false;
    *out = v;
    return true;
}

/* T_i^-1 T_j as a row-major 3 x 4 float matrix */
void relativePose(const Pose6f &pi, const Pose6f &pj, float m[12])
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

} // namespace

int main(int argc, char **argv)
{
    if (argc < 4 || argv[1] == nullptr || argv[2] == nullptr || argv[3] == nullptr) {
        std::cout << "Usage: " << (argc > 0 ? argv[0] : "batch_submap_bev_gen") << " [keyframes_root_dir] [sensor_type] [half_window] [stride]\n\n"
                  << "[keyframes_root_dir]/non_ground_point_cloud/ holds the labelled clouds batch_multi_bev_gen wrote,\n"
                  << "[keyframes_root_dir]/keyframe_pose.csv their poses, row j for file j in sorted order.\n"
                  << "[sensor_type] could be HDL_32E, HDL_64E or OS1_64. \n"
                  << "[half_window] h >= 0: the map of key frame i holds frames i - h .. i + h, each moved into frame i's coordinates.\n"
                  << "[stride] key frames 0, stride, 2 * stride, ...; default 1.\n\n"
                  << "Writes output_submap_bev/{binary,csv}/<key name>.{bin,csv} under [keyframes_root_dir].\n"
                  << "Positions are kept as floats, as the reference's Pose6f does: large coordinates (UTM) limit the precision\n"
                  << "of the relative translations.\n";
        return 1;
    }
    std::string root(argv[1]);
    if (root.empty() || root.back() != '/') root.append("/");
    bev_params_t bp;
    if (bev_params_for_sensor(argv[2], &bp) != BEV_OK) {
        std::cerr << "Unknown sensor type " << argv[2] << " (HDL_32E, HDL_64E or OS1_64)\n";
        return 1;
    }
    long half = 0, stride = 1;
    if (!parseCount(argv[3], 0, &half)) {
        std::cerr << "half_window '" << argv[3] << "': expected an integer >= 0\n";
        return 1;
    }
    if (argc > 4 && argv[4] != nullptr && !parseCount(argv[4], 1, &stride)) {
        std::cerr << "stride '" << argv[4] << "': expected an integer >= 1\n";
        return 1;
    }
    std::vector<std::string> files;
    getPcdFileNames(root + "non_ground_point_cloud/", files);
    bool ok = false;
    const std::vector<Pose6f> pose = readKeyframePose(root + "keyframe_pose.csv", &ok);
    if (!ok) {
        std::cerr << "pose file " << root << "keyframe_pose.csv: can not be read\n";
        return 1;
    }
    if (pose.size() < files.size()) {
        std::cerr << "pose file " << root << "keyframe_pose.csv: " << pose.size() << " rows for " << files.size() << " clouds\n";
        return 1;
    }
    const long n_files = (long)files.size(), n_keys = (n_files + stride - 1) / stride;

    const int batch = (int)std::max<long>(1, std::min<long>(std::max(1, std::atoi(std::getenv("BEV_BATCH") ? std::getenv("BEV_BATCH") : "32")), n_keys));
    const long long max_pts_env = std::getenv("BEV_MAX_POINTS") ? std::atoll(std::getenv("BEV_MAX_POINTS")) : 0;
    bev_ctx_t *ctx = nullptr;
    const int rc0 = bev_create(&ctx, 0, &bp, batch, max_pts_env > 0 ? (size_t)max_pts_env : ((size_t)4 << 20));
    if (rc0 != BEV_OK) {
        std::cerr << "bev_create failed: " << bev_strerror(rc0) << "\n";
        return 1;
    }

    const std::string bin_dir = root + "output_submap_bev/binary/", csv_dir = root + "output_submap_bev/csv/";
    bevhost_recreate_dir(bin_dir);
    bevhost_recreate_dir(csv_dir);

    const size_t multi_bytes = bev_multi_bytes(&bp), single_bytes = bev_single_bytes(&bp);
    const int M = (int)((float)(bp.max_range * 2) / bp.interval);
    std::vector<uint8_t> multi((size_t)batch * multi_bytes), single((size_t)batch * single_bytes);
    std::vector<uint8_t *> multi_out(batch), single_out(batch);
    for (int i = 0; i < batch; ++i) {
        multi_out[i] = multi.data() + (size_t)i * multi_bytes;
        single_out[i] = single.data() + (size_t)i * single_bytes;
    }
    std::vector<pcl::PointCloud<pcl::PointXYZIRCT>> in;
    std::vector<long> loaded; /* the files of the batch, ascending: frame f of the call is file loaded[f] */
    std::vector<const bev_point_t *> clouds;
    std::vector<uint32_t> n_pts;
    std::vector<uint64_t> map_offs;
    std::vector<int32_t> entry_frame;
    std::vector<float> entry_pose;
    long failed = 0;
    for (long k0 = 0; k0 < n_keys; k0 += batch) {
        const int nb = (int)std::min<long>(batch, n_keys - k0);
        loaded.clear();
        for (int m = 0; m < nb; ++m) { /* (the windows ascend with the keys: what is new lies behind what is there) */
            const long i = (k0 + m) * stride;
            for (long j = std::max(std::max(0L, i - half), loaded.empty() ? 0L : loaded.back() + 1); j <= std::min(n_files - 1, i + half); ++j)
                loaded.push_back(j);
        }
        in.resize(loaded.size());
        clouds.resize(loaded.size());
        n_pts.resize(loaded.size());
        for (size_t f = 0; f < loaded.size(); ++f) {
            in[f].clear(); /* an unreadable file goes on as an empty cloud */
            if (bevio::loadPCDFile(files[loaded[f]], in[f]) != 0) std::cerr << "Can not read " << files[loaded[f]] << "\n";
            clouds[f] = in[f].size() ? reinterpret_cast<const bev_point_t *>(in[f].points.data()) : nullptr;
            n_pts[f] = (uint32_t)in[f].size();
        }
        map_offs.assign(1, 0);
        entry_frame.clear();
        entry_pose.clear();
        for (int m = 0; m < nb; ++m) {
            const long i = (k0 + m) * stride;
            for (long j = std::max(0L, i - half); j <= std::min(n_files - 1, i + half); ++j) {
                entry_frame.push_back((int32_t)(std::lower_bound(loaded.begin(), loaded.end(), j) - loaded.begin()));
                entry_pose.resize(entry_pose.size() + 12);
                float *mat = entry_pose.data() + entry_pose.size() - 12;
                if (j == i) bev_yaw_translate_matrix(0.0f, 0.0f, 0.0f, 0.0f, mat); /* the exact identity */
                else relativePose(pose[i], pose[j], mat);
            }
            map_offs.push_back(entry_frame.size());
        }
        const int rc = bev_submap_bev_batch(ctx, (int)loaded.size(), clouds.data(), n_pts.data(), nb, map_offs.data(),
                                            entry_frame.data(), entry_pose.data(), multi_out.data(), single_out.data());
        if (rc != BEV_OK) {
            std::cerr << "bev_submap_bev_batch failed: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
            failed += nb;
            continue;
        }
        for (int m = 0; m < nb; ++m) {
            const std::string &path = files[(k0 + m) * stride];
            const size_t start_pos = path.find_last_of('/') + 1, end_pos = path.find_last_of('.');
            const std::string name = path.substr(start_pos, end_pos - start_pos);
            std::cout << "Converting file: " << name << "\n";
            const std::string bin = bin_dir + name + ".bin", csv = csv_dir + name + ".csv";
            if (!bevio::writeFile(bin, multi_out[m], multi_bytes)) std::cerr << "Can not open file: " << bin << "\n";
            const std::string text = bevio::formatCsvU8(single_out[m], M, M);
            if (!bevio::writeFile(csv, text.data(), text.size())) std::cerr << "Faied to export csv formatted BEV file: " << csv << "\n";
        }
    }
    bev_destroy(ctx);
    if (failed) {
        std::cerr << failed << " of " << n_keys << " maps failed on the GPU path\n";
        return 1;
    }
    std::cout << "Done. " << std::endl;
    return 0;
}
