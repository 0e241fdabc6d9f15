/*
 * batch_submap_bev_gen <keyframes_root_dir> <sensor_type> <half_window> [<stride>]
 *
 * The 24-layer occupancy BEV and the single-layer BEV of LOCAL MAPS: for key index i = 0, stride, 2 * stride, ... (stride
 * defaults to 1) the labelled clouds j in [i - half_window, i + half_window] (clipped to the files) that batch_multi_bev_gen
 * left in <root>/non_ground_point_cloud/, each moved into key frame i's coordinates and all rastered into one image pair
 * (DESIGN.md §6i).  The files are taken in sorted order; row j of <root>/keyframe_pose.csv (readKeyframePose) is file j's pose.
 *   matrix of j in map i   T_i^-1 T_j, j == i the exact identity (SubmapWindows.h, shared with batch_submap_cloud_manip)
 *   writes                 <root>/output_submap_bev/binary/<key name>.bin  the .bin payload of batch_multi_bev_gen
 *                          <root>/output_submap_bev/csv/<key name>.csv     its single-layer CSV
 *                          (both directories are recreated; no PNGs)
 * The maps go BEV_BATCH at a time (default 32) through one bev_submap_bev_batch call; only the files a batch names are loaded.
 * Pose6f keeps positions as floats, as the reference does: with large coordinates (UTM) the relative translations are only
 * as fine as a float of that size.  Wrong arguments, an unreadable pose file or one with fewer rows than there are clouds
 * exit 1 before a GPU context is created; an unreadable PCD is reported and goes on as an empty cloud.
 * BEV_MAX_POINTS=P: points per cloud the context is sized for (default 4 Mi).
 */
#include <iostream>

#include "SubmapWindows.h"

void bevhost_recreate_dir(const std::string &dir); /* BatchMultiBevGen.cpp (host): rm -rf + mkdir -p */

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
    submapwin::Setup s;
    if (!submapwin::readSetup(argc, argv, s)) return 1;
    const bev_params_t &bp = s.bp;
    const long n_keys = s.n_keys;
    const int batch = submapwin::batchSize(s);
    bev_ctx_t *ctx = submapwin::createContext(s, batch);
    if (!ctx) return 1;

    const std::string bin_dir = s.root + "output_submap_bev/binary/", csv_dir = s.root + "output_submap_bev/csv/";
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
    submapwin::Batch b;
    long failed = 0;
    for (long k0 = 0; k0 < n_keys; k0 += batch) {
        const int nb = (int)std::min<long>(batch, n_keys - k0);
        submapwin::loadBatch(s, k0, nb, b);
        const int rc = bev_submap_bev_batch(ctx, (int)b.loaded.size(), b.clouds.data(), b.n_pts.data(), nb, b.map_offs.data(),
                                            b.entry_frame.data(), b.entry_pose.data(), multi_out.data(), single_out.data());
        if (rc != BEV_OK) {
            std::cerr << "bev_submap_bev_batch failed: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
            failed += nb;
            continue;
        }
        for (int m = 0; m < nb; ++m) {
            const std::string name = submapwin::keyName(s, k0 + m);
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
