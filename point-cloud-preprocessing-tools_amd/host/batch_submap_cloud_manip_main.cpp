/*
 * batch_submap_cloud_manip <keyframes_root_dir> <sensor_type> <half_window> [<stride>]
 *
 * The float max-height BEV (saveAsMat of batch_cloud_manip) of LOCAL MAPS: the windows, the matrices, the files read and the
 * knobs of batch_submap_bev_gen (SubmapWindows.h) — for key index i = 0, stride, 2 * stride, ... the labelled
 * clouds j in [i - half_window, i + half_window] of <root>/non_ground_point_cloud/, each moved into key frame i's coordinates
 * by T_i^-1 T_j of <root>/keyframe_pose.csv, all rastered into ONE grid.
 *   writes   <root>/output_submap_bvm/<key name>.csv and .png: the files batch_cloud_manip writes per cloud
 *            (BatchCloudManip::writeMat), at interval 1.0 and with label-0 points skipped (the directory is recreated)
 * The maps go BEV_BATCH at a time (default 32) through one bev_submap_float_bev_batch call; only the files a batch names are
 * loaded.  The sensor type is checked and sizes the context; the grid itself does not depend on it.  Wrong arguments, an
 * unreadable pose file or one with fewer rows than there are clouds exit 1 before a GPU context is created; an unreadable PCD is
 * reported and goes on as an empty cloud.  BEV_MAX_POINTS=P: points per cloud the context is sized for (default 4 Mi).
 */
#include <iostream>

#include "CloudManip.h"
#include "SubmapWindows.h"

void bevhost_recreate_dir(const std::string &dir); /* BatchMultiBevGen.cpp (host): rm -rf + mkdir -p */

int main(int argc, char **argv)
{
    if (argc < 4 || argv[1] == nullptr || argv[2] == nullptr || argv[3] == nullptr) {
        std::cout << "Usage: " << (argc > 0 ? argv[0] : "batch_submap_cloud_manip") << " [keyframes_root_dir] [sensor_type] [half_window] [stride]\n\n"
                  << "[keyframes_root_dir]/non_ground_point_cloud/ holds the labelled clouds batch_cloud_manip or batch_multi_bev_gen wrote,\n"
                  << "[keyframes_root_dir]/keyframe_pose.csv their poses, row j for file j in sorted order.\n"
                  << "[sensor_type] could be HDL_32E, HDL_64E or OS1_64. \n"
                  << "[half_window] h >= 0: the map of key frame i holds frames i - h .. i + h, each moved into frame i's coordinates.\n"
                  << "[stride] key frames 0, stride, 2 * stride, ...; default 1.\n\n"
                  << "Writes output_submap_bvm/<key name>.{csv,png} under [keyframes_root_dir]: the float max-height BEV at interval 1.0.\n"
                  << "Positions are kept as floats, as the reference's Pose6f does: large coordinates (UTM) limit the precision\n"
                  << "of the relative translations.\n";
        return 1;
    }
    submapwin::Setup s;
    if (!submapwin::readSetup(argc, argv, s)) return 1;
    const int batch = submapwin::batchSize(s);
    bev_ctx_t *ctx = submapwin::createContext(s, batch);
    if (!ctx) return 1;

    const std::string bvm_dir = s.root + "output_submap_bvm/";
    bevhost_recreate_dir(bvm_dir);

    const float interval_res = 1.0f; /* batch_cloud_manip's (BatchCloudManip.cpp:311) */
    const int M = (int)bev_float_bev_size(interval_res);
    std::vector<cv::Mat> grids(batch);
    std::vector<float *> out(batch);
    for (int i = 0; i < batch; ++i) {
        grids[i].create(M, M, cv::CV_32F);
        out[i] = grids[i].ptr<float>();
    }
    submapwin::Batch b;
    long failed = 0;
    for (long k0 = 0; k0 < s.n_keys; k0 += batch) {
        const int nb = (int)std::min<long>(batch, s.n_keys - k0);
        submapwin::loadBatch(s, k0, nb, b);
        const int rc = bev_submap_float_bev_batch(ctx, (int)b.loaded.size(), b.clouds.data(), b.n_pts.data(), interval_res, 1, nb,
                                                  b.map_offs.data(), b.entry_frame.data(), b.entry_pose.data(), out.data());
        if (rc != BEV_OK) {
            std::cerr << "bev_submap_float_bev_batch failed: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
            failed += nb;
            continue;
        }
        for (int m = 0; m < nb; ++m) {
            const std::string name = submapwin::keyName(s, k0 + m);
            std::cout << "Converting file: " << name << "\n";
            BatchCloudManip::writeMat(grids[m], bvm_dir + name);
        }
    }
    bev_destroy(ctx);
    if (failed) {
        std::cerr << failed << " of " << s.n_keys << " maps failed on the GPU path\n";
        return 1;
    }
    std::cout << "Done. " << std::endl;
    return 0;
}
