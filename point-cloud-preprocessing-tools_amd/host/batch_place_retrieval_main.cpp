/*
 * batch_place_retrieval <keyframes_root_dir> <sensor_type> <half_window> [<exclude_recent> [<top_k> [<max_distance>]]]
 *
 * Place retrieval over a directory of key frames: the match list the registration tools start from.  The files
 * read, the windows and the matrices are those of the submap tools at stride 1 (SubmapWindows.h): database entry i is the local
 * map of key file i — the labelled clouds j in [i - half_window, i + half_window] of <root>/non_ground_point_cloud/, each moved
 * into frame i's coordinates by T_i^-1 T_j of <root>/keyframe_pose.csv; half_window 0: the frame alone under the exact
 * identity — and query q is frame q alone.  Query q's candidates are the entries 0 .. q - exclude_recent (default 50): a place
 * is not recognised in what was just seen.
 *   writes   <root>/place_retrieval/match_result.txt: "query_idx match_idx angle_guess" per hit, a query's hits in rank order,
 *            what loadMatchResults reads (batch_top_part_registration, batch_submap_registration & co.); hits beyond the
 *            query's candidates or with a distance above max_distance (default 2: keep everything) are left out;
 *            <root>/place_retrieval/match_detail.csv: query, match, shift, angle, distance of the same hits
 *            (the directory is recreated)
 * One bev_place_retrieval_batch call over all the clouds: they are all held in host memory (32 bytes a point).  Wrong
 * arguments, an unreadable pose file or one with fewer rows than there are clouds exit 1 before a GPU context is created; an
 * unreadable PCD is reported and goes on as an empty cloud; a failed call exits 1.  BEV_BATCH=B: clouds per upload (default 32);
 * BEV_MAX_POINTS=P: points per cloud the context is sized for (default 4 Mi).
 */
#include <cmath>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>

#include "SubmapWindows.h"

void bevhost_recreate_dir(const std::string &dir); /* BatchMultiBevGen.cpp (host): rm -rf + mkdir -p */

int main(int argc, char **argv)
{
    if (argc < 4 || argv[1] == nullptr || argv[2] == nullptr || argv[3] == nullptr) {
        std::cout << "Usage: " << (argc > 0 ? argv[0] : "batch_place_retrieval")
                  << " [keyframes_root_dir] [sensor_type] [half_window] [exclude_recent] [top_k] [max_distance]\n\n"
                  << "[keyframes_root_dir]/non_ground_point_cloud/ holds the labelled clouds batch_cloud_manip or batch_multi_bev_gen wrote,\n"
                  << "[keyframes_root_dir]/keyframe_pose.csv their poses, row j for file j in sorted order.\n"
                  << "[sensor_type] could be HDL_32E, HDL_64E or OS1_64. \n"
                  << "[half_window] h >= 0: database entry i is the map of frames i - h .. i + h in frame i's coordinates.\n"
                  << "[exclude_recent] e >= 0: query q (frame q alone) searches entries 0 .. q - e; default 50.\n"
                  << "[top_k] 1 .. " << BEV_PLACE_MAX_TOP_K << " hits per query; default 1.\n"
                  << "[max_distance] hits above it are left out; default 2 (keep everything).\n\n"
                  << "Writes place_retrieval/match_result.txt (query_idx match_idx angle_guess) and match_detail.csv under [keyframes_root_dir].\n";
        return 1;
    }
    submapwin::Setup s;
    if (!submapwin::readSetup(4, argv, s)) return 1; /* (stride 1: every file is a key) */
    long exclude = 50, top_k = 1;
    double max_distance = 2.0;
    if (argc > 4 && !submapwin::parseCount(argv[4], 0, &exclude)) {
        std::cerr << "exclude_recent '" << argv[4] << "': expected an integer >= 0\n";
        return 1;
    }
    if (argc > 5 && (!submapwin::parseCount(argv[5], 1, &top_k) || top_k > BEV_PLACE_MAX_TOP_K)) {
        std::cerr << "top_k '" << argv[5] << "': expected an integer 1 .. " << BEV_PLACE_MAX_TOP_K << "\n";
        return 1;
    }
    if (argc > 6) {
        char *end = nullptr;
        max_distance = std::strtod(argv[6], &end);
        if (end == argv[6] || *end != '\0' || std::isnan(max_distance)) {
            std::cerr << "max_distance '" << argv[6] << "': expected a number\n";
            return 1;
        }
    }
    bev_ctx_t *ctx = submapwin::createContext(s, submapwin::batchSize(s));
    if (!ctx) return 1;

    const std::string out_dir = s.root + "place_retrieval/";
    bevhost_recreate_dir(out_dir);

    const int n = (int)s.n_files;
    submapwin::Batch b;
    submapwin::loadBatch(s, 0, n, b); /* every file a frame of the call, every key's window a map */
    std::vector<int32_t> limit((size_t)n);
    for (long q = 0; q < n; ++q) limit[(size_t)q] = (int32_t)std::max(0L, q - exclude + 1);
    std::vector<bev_place_hit_t> hits((size_t)n * (size_t)top_k);
    const bev_place_params_t prm = bev_place_defaults();
    const int rc = bev_place_retrieval_batch(ctx, n, b.clouds.data(), b.n_pts.data(), n, b.map_offs.data(), b.entry_frame.data(),
                                             b.entry_pose.data(), &prm, limit.data(), (int)top_k, hits.data());
    if (rc != BEV_OK) {
        std::cerr << "bev_place_retrieval_batch failed: " << bev_strerror(rc) << " " << bev_last_error(ctx) << "\n";
        bev_destroy(ctx);
        return 1;
    }
    bev_destroy(ctx);

    std::ofstream f_match(out_dir + "match_result.txt"), f_detail(out_dir + "match_detail.csv");
    f_match << std::setprecision(std::numeric_limits<float>::max_digits10);
    f_detail << std::setprecision(std::numeric_limits<double>::max_digits10) << "query_idx,match_idx,shift,angle_guess,distance\n";
    size_t kept = 0;
    for (const bev_place_hit_t &h : hits) {
        if (h.match_idx < 0 || h.distance > max_distance) continue;
        f_match << h.query_idx << " " << h.match_idx << " " << h.angle_guess << "\n";
        f_detail << h.query_idx << "," << h.match_idx << "," << h.shift << "," << h.angle_guess << "," << h.distance << "\n";
        ++kept;
    }
    if (!f_match.good() || !f_detail.good()) {
        std::cerr << "can not write under " << out_dir << "\n";
        return 1;
    }
    std::cout << kept << " matches of " << n << " queries\nDone. " << std::endl;
    return 0;
}
