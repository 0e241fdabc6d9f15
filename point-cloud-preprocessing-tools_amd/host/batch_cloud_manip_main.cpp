/*
 * batch_cloud_manip <keyframes_root_dir>
 *
 * The older fork of the hot path (BatchCloudManip.cpp:269-335): HDL-64E constants hard-coded (N_SCAN = 64,
 * Horizon_SCAN = 2083, groundScanInd = 50; :13-14, :85), per file: load -> getOrderedCloud -> markGroundPoints ->
 * saveAsMat (float max-height BEV, 201 x 201 at interval 1.0: <root>/output_bvm/<name>.csv + .png) -> labelled cloud
 * to <root>/non_ground_point_cloud/<name>.pcd.  Same command line, directory tree and stdout lines; order, ground
 * segmentation and the raster run on MI355X through the C ABI, in batches: BEV_BATCH files (default 32, as in
 * batch_multi_bev_gen) are read, go through one bev_process_batch and one bev_float_bev_batch call and are written; the
 * figure on a file's [TIME] line is its batch's time divided by the batch's files.  BEV_MAX_POINTS=P: input points per
 * cloud the context is sized for (default 4 Mi, the knob and the default of batch_multi_bev_gen).
 * One difference is deliberate: the reference's getOrderedCloud of this tool has no bounds test (:55-62), so a point
 * with row >= 64 or col >= 2083 writes outside the cloud there; here such points are dropped.
 */
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iostream>

#include "BatchMultiBevGen.h"
#include "CloudManip.h"
#include "FileFormats.h"

void bevhost_recreate_dir(const std::string &dir); /* BatchMultiBevGen.cpp (host): rm -rf + mkdir -p */

int main(int argc, char **argv)
{
    if (argc < 2 || argv[1] == nullptr) {
        std::cout << "Usage: " << (argc > 0 ? argv[0] : "batch_cloud_manip") << " <keyframes_root_dir>" << std::endl; /* :271-274 */
        return 1;
    }
    std::string root(argv[1]);
    if (root.empty() || root.back() != '/') root.append("/");
    const std::string pcd_dir = root + "keyframe_point_cloud/";          /* :276-277 */
    const std::string non_ground_dir = root + "non_ground_point_cloud/"; /* :279-280 */
    bevhost_recreate_dir(non_ground_dir);                                /* :283-284 */

    std::vector<std::string> files;
    getPcdFileNames(pcd_dir, files);                                     /* :286-287 */
    setNeighbors();                                                      /* :289 */
    const std::string bvm_dir = root + "output_bvm/";                    /* :292-295 */
    bevhost_recreate_dir(bvm_dir);

    sensor_params_ = getSensorParams(SensorType::HDL_64E);               /* the tool's constants: 64 x 2083, 50 ground rings */
    const size_t S = (size_t)sensor_params_.N_SCAN * sensor_params_.Horizon_SCAN;
    const int batch = std::max(1, std::atoi(std::getenv("BEV_BATCH") ? std::getenv("BEV_BATCH") : "32"));
    const long long max_pts_env = std::getenv("BEV_MAX_POINTS") ? std::atoll(std::getenv("BEV_MAX_POINTS")) : 0;
    bev_params_t bp;
    bev_ctx_t *ctx = nullptr;
    int rc = bev_params_for_sensor("HDL_64E", &bp);
    if (rc == BEV_OK) rc = bev_create(&ctx, 0, &bp, batch, max_pts_env > 0 ? (size_t)max_pts_env : ((size_t)4 << 20));
    if (rc != BEV_OK) {
        std::cerr << "bev_create failed: " << bev_strerror(rc) << "\n";
        return 1;
    }

    const float interval_res = 1.0f;                                     /* :311 */
    double total_ms = 0;
    std::vector<pcl::PointCloud<pcl::PointXYZIRCT>> in(batch), ordered(batch);
    std::vector<cv::Mat> grids(batch);
    std::vector<std::string> names(batch);
    for (size_t b0 = 0; b0 < files.size(); b0 += (size_t)batch) {        /* :300-328, BEV_BATCH files at a time */
        const int nb = (int)std::min<size_t>((size_t)batch, files.size() - b0);
        for (int i = 0; i < nb; ++i) {
            const std::string &input_filename = files[b0 + i];
            in[i].clear(); /* an unreadable file goes on as an empty cloud */
            if (bevio::loadPCDFile(input_filename, in[i]) != 0) std::cerr << "Can not read " << input_filename << "\n";
            const size_t start_pos = input_filename.find_last_of('/') + 1;
            const size_t end_pos = input_filename.find_last_of('.');
            names[i] = input_filename.substr(start_pos, end_pos - start_pos);
        }

        const auto t0 = std::chrono::system_clock::now();
        rc = BatchCloudManip::processBatch(ctx, in, 0, nb, S, ordered, grids, interval_res);
        if (rc != BEV_OK) std::cerr << "saveAsMat: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
        for (int i = 0; i < nb; ++i) BatchCloudManip::writeMat(grids[i], bvm_dir + names[i]); /* :319 */
        const auto t1 = std::chrono::system_clock::now();
        const double ms = (double)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() * 1e-3 / nb;
        for (int i = 0; i < nb; ++i) {
            std::cout << "Converting file: " << names[i] << "\n";
            std::cout << "[TIME] Preprocessing and BEV generation: " << ms << "ms. \n" << std::endl; /* :323 */
            total_ms += ms;
        }

        for (int i = 0; i < nb; ++i) bevio::savePCDFileBinary(non_ground_dir + names[i] + ".pcd", ordered[i]); /* :327 */
    }
    std::cout << "[TIME] Average preprocessing and BEV generation: " << (files.empty() ? 0.0 : total_ms / (double)files.size())
              << "\n";
    std::cout << "Done. " << std::endl;
    bev_destroy(ctx);
    return 0;
}
