/*
 * batch_posed_bev_gen <keyframes_root_dir> <sensor_type> <poses_file>
 *
 * The 24-layer occupancy BEV and the single-layer BEV of every labelled cloud batch_multi_bev_gen left in
 * the .pcd files of <root>/non_ground_point_cloud/, under every pose of <poses_file>: what cloud_manip's transform followed by
 * computeAndSaveMultiBev / computeAndSaveSingleBev would write, for training or evaluating the consumer of those images under
 * rigid motions of the sensor.  The files are taken in sorted order, BEV_BATCH at a time (default 32) through
 * one bev_posed_bev_batch call; the moved clouds are never written.
 *   <poses_file>  text, one pose per line: tx ty tz yaw_deg (cloud_manip's argument order; the matrix is
 *                 bev_yaw_translate_matrix's); blank lines and lines that start with '#' are skipped; 1 to 64 poses
 *   writes        <root>/output_posed_bev/binary/<name>_<kk>.bin  the .bin payload of batch_multi_bev_gen (24 * M * M bytes)
 *                 <root>/output_posed_bev/csv/<name>_<kk>.csv     its single-layer CSV; kk: the two-digit pose index
 *                 (both directories are recreated; no PNGs)
 * An unknown sensor, or an unreadable or malformed pose file, exits 1 before a GPU context is created; an unreadable PCD is
 * reported and goes on as an empty cloud.  BEV_MAX_POINTS=P: points per cloud the context is sized for (default 4 Mi).
 * Memory: min(BEV_BATCH, files) * poses images of 1.25 MB (M = 224) on the host and as many on the device: 2.5 GB each at 32
 * files and 64 poses; a smaller BEV_BATCH brings it down.
 */
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "BatchMultiBevGen.h"
#include "FileFormats.h"

void bevhost_recreate_dir(const std::string &dir); /* BatchMultiBevGen.cpp (host): rm -rf + mkdir -p */

namespace {

/* the poses of the file as 12 floats each; false (and why) for a file that cannot be read or is malformed */
bool readPoses(const std::string &path, std::vector<float> &matrices, std::string &why)
{
    std::ifstream in(path);
    if (!in.is_open()) {
        why = "can not be read";
        return false;
    }
    std::string line;
    int line_no = 0, n = 0;
    while (std::getline(in, line)) {
        ++line_no;
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        std::istringstream fields(line);
        std::string word;
        float v[4];
        int k = 0;
        while (fields >> word) {
            char *end = nullptr;
            errno = 0;
            const float x = std::strtof(word.c_str(), &end);
            if (k < 4 && (end == word.c_str() || *end != '\0' || errno == ERANGE)) {
                why = "line " + std::to_string(line_no) + ": bad number '" + word + "'";
                return false;
            }
            if (k < 4) v[k] = x;
            ++k;
        }
        if (k != 4) {
            why = "line " + std::to_string(line_no) + ": " + std::to_string(k) + " fields, expected tx ty tz yaw_deg";
            return false;
        }
        if (++n > BEV_POSED_BEV_MAX_POSES) {
            why = "more than " + std::to_string(BEV_POSED_BEV_MAX_POSES) + " poses";
            return false;
        }
        matrices.resize((size_t)n * 12);
        bev_yaw_translate_matrix(v[0], v[1], v[2], v[3], matrices.data() + (size_t)(n - 1) * 12);
    }
    if (in.bad()) {
        why = "can not be read";
        return false;
    }
    if (n == 0) {
        why = "no poses";
        return false;
    }
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 4 || argv[1] == nullptr || argv[2] == nullptr || argv[3] == nullptr) {
        std::cout << "Usage: " << (argc > 0 ? argv[0] : "batch_posed_bev_gen") << " [keyframes_root_dir] [sensor_type] [poses_file]\n\n"
                  << "[keyframes_root_dir]/non_ground_point_cloud/ holds the labelled clouds batch_multi_bev_gen wrote.\n"
                  << "[sensor_type] could be HDL_32E, HDL_64E or OS1_64. \n"
                  << "[poses_file] one pose per line: tx ty tz yaw_deg; 1 to " << BEV_POSED_BEV_MAX_POSES << " poses; '#' starts a comment line.\n\n"
                  << "Writes output_posed_bev/{binary,csv}/<name>_<pose>.{bin,csv} under [keyframes_root_dir].\n";
        return 1;
    }
    std::string root(argv[1]);
    if (root.empty() || root.back() != '/') root.append("/");
    bev_params_t bp;
    if (bev_params_for_sensor(argv[2], &bp) != BEV_OK) {
        std::cerr << "Unknown sensor type " << argv[2] << " (HDL_32E, HDL_64E or OS1_64)\n";
        return 1;
    }
    std::vector<float> matrices;
    std::string why;
    if (!readPoses(argv[3], matrices, why)) {
        std::cerr << "pose file " << argv[3] << ": " << why << "\n";
        return 1;
    }
    const int n_poses = (int)(matrices.size() / 12);

    std::vector<std::string> files;
    getPcdFileNames(root + "non_ground_point_cloud/", files);
    /* (no more than there are files: the host images and the library's device images are batch * n_poses * 1.25 MB each) */
    const int batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, std::atoi(std::getenv("BEV_BATCH") ? std::getenv("BEV_BATCH") : "32")), files.size()));
    const long long max_pts_env = std::getenv("BEV_MAX_POINTS") ? std::atoll(std::getenv("BEV_MAX_POINTS")) : 0;
    bev_ctx_t *ctx = nullptr;
    const int rc0 = bev_create(&ctx, 0, &bp, batch, max_pts_env > 0 ? (size_t)max_pts_env : ((size_t)4 << 20));
    if (rc0 != BEV_OK) {
        std::cerr << "bev_create failed: " << bev_strerror(rc0) << "\n";
        return 1;
    }

    const std::string bin_dir = root + "output_posed_bev/binary/", csv_dir = root + "output_posed_bev/csv/";
    bevhost_recreate_dir(bin_dir);
    bevhost_recreate_dir(csv_dir);

    const size_t multi_bytes = bev_multi_bytes(&bp), single_bytes = bev_single_bytes(&bp);
    const int M = (int)((float)(bp.max_range * 2) / bp.interval);
    std::vector<pcl::PointCloud<pcl::PointXYZIRCT>> in(batch);
    std::vector<uint8_t> multi((size_t)batch * n_poses * multi_bytes), single((size_t)batch * n_poses * single_bytes);
    std::vector<const bev_point_t *> clouds(batch);
    std::vector<uint32_t> n_pts(batch);
    std::vector<uint8_t *> multi_out(batch), single_out(batch);
    std::vector<float> poses((size_t)batch * matrices.size());
    for (int i = 0; i < batch; ++i) {
        std::copy(matrices.begin(), matrices.end(), poses.begin() + (size_t)i * matrices.size()); /* every cloud, every pose */
        multi_out[i] = multi.data() + (size_t)i * n_poses * multi_bytes;
        single_out[i] = single.data() + (size_t)i * n_poses * single_bytes;
    }
    int failed = 0;
    for (size_t b0 = 0; b0 < files.size(); b0 += (size_t)batch) {
        const int nb = (int)std::min<size_t>((size_t)batch, files.size() - b0);
        for (int i = 0; i < nb; ++i) {
            in[i].clear(); /* an unreadable file goes on as an empty cloud */
            if (bevio::loadPCDFile(files[b0 + i], in[i]) != 0) std::cerr << "Can not read " << files[b0 + i] << "\n";
            clouds[i] = in[i].size() ? reinterpret_cast<const bev_point_t *>(in[i].points.data()) : nullptr;
            n_pts[i] = (uint32_t)in[i].size();
        }
        const int rc = bev_posed_bev_batch(ctx, nb, clouds.data(), n_pts.data(), n_poses, poses.data(), multi_out.data(),
                                           single_out.data());
        if (rc != BEV_OK) {
            std::cerr << "bev_posed_bev_batch failed: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
            failed += nb;
            continue;
        }
        for (int i = 0; i < nb; ++i) {
            const std::string &path = files[b0 + i];
            const size_t start_pos = path.find_last_of('/') + 1, end_pos = path.find_last_of('.');
            const std::string name = path.substr(start_pos, end_pos - start_pos);
            std::cout << "Converting file: " << name << "\n";
            for (int k = 0; k < n_poses; ++k) {
                char kk[16];
                std::snprintf(kk, sizeof kk, "_%02d", k);
                const std::string bin = bin_dir + name + kk + ".bin", csv = csv_dir + name + kk + ".csv";
                if (!bevio::writeFile(bin, multi_out[i] + (size_t)k * multi_bytes, multi_bytes)) std::cerr << "Can not open file: " << bin << "\n";
                const std::string text = bevio::formatCsvU8(single_out[i] + (size_t)k * single_bytes, M, M);
                if (!bevio::writeFile(csv, text.data(), text.size())) std::cerr << "Faied to export csv formatted BEV file: " << csv << "\n";
            }
        }
    }
    bev_destroy(ctx);
    if (failed) {
        std::cerr << failed << " of " << files.size() << " clouds failed on the GPU path\n";
        return 1;
    }
    std::cout << "Done. " << std::endl;
    return 0;
}
