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
 * most max_frames distinct frames (default 256; the results do not depend on it).  The chunks, the chain and the bookkeeping
 * are the four registration tools' own (RegistrationChunks.h, RegistrationChain.h): this file is the command
 * line and which file an index names.
 *
 * Differs from the reference: no per-match chatter (the "Processing match", [TIME] and transform lines); the two
 * "[TIME] Avg Tiempo" lines are the chain's wall time per match in ms (coarse: file reading excluded, front end and
 * coarse ICP; fine: the fine stage), not the reference's per-match stopwatch; an unreadable file ends the tool with exit
 * status 1 before anything is written to the report.
 *
 * BEV_PAIR_SEARCH_GRID=<fine>[,<coarse>] in the environment (both tools): the cap of cells per axis of the targets'
 * search grids in the fine and the coarse stage, handed to bev_set_pair_search_grid before the first chunk; a single number sets
 * both stages.  Integers 0 ... 1024; unset, empty or 0: the grids, the launches and the output as ever.  The output does not
 * depend on it.  Anything else: exit 1 with "BEV_PAIR_SEARCH_GRID '<text>': expected <fine>[,<coarse>], integers 0 ... 1024" and
 * the usage line, before any GPU work.
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "BatchMultiBevGen.h"
#include "Registration.h"
#include "RegistrationChain.h"
#include "SearchGridEnv.h"
#include "Utility.h"

#ifndef BEV_WHOLE_TOOL
#define BEV_WHOLE_TOOL 0
#endif

namespace {

constexpr bool kTopPart = !BEV_WHOLE_TOOL;
const char *const kTool = kTopPart ? "batch_top_part_registration" : "batch_whole_registration";

void usage() { std::cerr << "Usage: " << kTool << " <match_list> <pcd_dir> [max_frames]\n"; }

std::string cloud_path(const std::string &dir, long idx)
{
    char name[32];
    std::snprintf(name, sizeof(name), "%06d.pcd", (int)idx);
    return (!dir.empty() && dir.back() == '/') ? dir + name : dir + "/" + name;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) {
        usage();
        return 1;
    }
    int search_grid[2] = {0, 0};
    if (const char *env = std::getenv("BEV_PAIR_SEARCH_GRID"))
        if (*env && !parse_search_grid(env, BEV_PAIR_SEARCH_GRID_MAX, search_grid)) {
            std::cerr << "BEV_PAIR_SEARCH_GRID '" << env << "': expected <fine>[,<coarse>], integers 0 ... " << BEV_PAIR_SEARCH_GRID_MAX
                      << "\n";
            usage();
            return 1;
        }
    const std::string match_list(argv[1]), pcd_dir(argv[2]);
    const int max_frames = argc > 3 ? std::atoi(argv[3]) : 256;
    if (max_frames < 2) {
        std::cerr << "max_frames must be at least 2\n";
        return 1;
    }
    std::ofstream report(kTopPart ? "./icp_precision_report.txt" : "./icp_precision_report_3d_icp_directly.txt");
    std::vector<MatchResult> matches;
    try {
        matches = loadMatchResults(match_list);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    /* the free functions' context follows a sensor; the registration stages read no sensor setting (packed clouds) */
    sensor_params_ = getSensorParams(parseSensorType("HDL_64E"));
    const bev_icp_params_t fine_prm = kTopPart ? bev_icp_fine_defaults() : bev_icp_whole_defaults();
    regchain::Tally tally(&report, kTopPart ? regchain::ReportAgainst::ChosenCoarse : regchain::ReportAgainst::Nothing);
    if (search_grid[0] || search_grid[1]) {
        bev_ctx_t *ctx = bevhost_context();
        if (!ctx || bev_set_pair_search_grid(ctx, search_grid[0], search_grid[1]) != BEV_OK) return 2;
    }
    for (size_t m0 = 0; m0 < matches.size();) {
        /* the indices are file numbers: a window of the number alone, nothing to clip */
        const regchain::Chunk chunk =
            regchain::planChunk(matches.data(), matches.size(), m0, 0, regchain::kNoClipLo, regchain::kNoClipHi, max_frames, false);
        std::vector<std::string> paths;
        for (long f : chunk.files) paths.push_back(cloud_path(pcd_dir, f));
        if (const int rc = regchain::registerChunk(paths, chunk, nullptr, 0.0f, kTopPart, fine_prm, tally)) return rc;
        m0 = chunk.m1;
    }
    tally.print(std::cout, kTopPart, false);
    return 0;
}
