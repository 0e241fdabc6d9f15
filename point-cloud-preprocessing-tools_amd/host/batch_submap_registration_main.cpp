/*
 * batch_submap_registration          <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]
 * batch_submap_top_part_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]
 *
 * One source, built four times (BEV_SUBMAP_TOP_PART 0 / 1; BEV_VERIFY_TOOL, BEV_ALIGN_TOOL below).  The first tool:
 *
 * Scan-to-map registration: batch_whole_registration with a LOCAL MAP as every match's target.  The match list
 * is batch_whole_registration's ("query match yaw" per line); the indices name the sorted files of
 * <root>/non_ground_point_cloud/, and row j of <root>/keyframe_pose.csv is file j's pose — what batch_submap_bev_gen and
 * batch_submap_cloud_manip read.  The map of match (q, m) holds the files j in [m - half_window, m + half_window], clipped to
 * the files, in ascending order, each under T_m^-1 T_j (submapwin::relativePose; j == m gets the exact identity); the query's
 * voxel cloud is registered against the map's moved voxel clouds from the yaw guess, with the whole tool's settings
 * (bev_icp_whole_defaults), by bev_submap_voxel_registration_device_resident.  half_window 0 is batch_whole_registration.
 * <map_leaf> > 0 thins every map by a voxel grid of that leaf over the union of its moved voxel clouds; absent
 * or 0: no second grid, the files as ever (the call is then bev_submap_registration_device_resident's); negative
 * or not a finite number: refused with the usage line.
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
 * 0 and map_leaf 0 it is that tool.  BEV_SUBMAP_PN_LEAF in the environment (this tool alone): a finite number > 0
 * thins every coarse map by a voxel grid of that leaf over the union of its moved clouds and recomputes its 2-D normals there
 * (bev_submap_coarse_voxel_registration_device_resident, radius 2, viewpoint 0: the front end's settings); unset, empty or 0: the
 * output as ever; anything else: exit 1 with "BEV_SUBMAP_PN_LEAF '<text>': expected a finite number >= 0" before any GPU work.
 * BEV_SUBMAP_TOP_UNION in the environment (this tool alone): 1 sends every chunk's coarse stage against the top
 * part over the union of each window's moved FULL clouds, thinned by BEV_SUBMAP_PN_LEAF (which must then be > 0) with radius 2
 * and viewpoint 0 (bev_submap_top_part_coarse_registration_device_resident; the front end's rows are the queries); unset, empty
 * or 0: the output as ever; 1 without a leaf: exit 1 with "BEV_SUBMAP_TOP_UNION=1 needs BEV_SUBMAP_PN_LEAF > 0"; anything else:
 * exit 1 with "BEV_SUBMAP_TOP_UNION '<text>': expected 0 or 1"; both before any GPU work.
 *
 * BEV_SUBMAP_SEARCH_GRID=<fine>[,<coarse>] in the environment (both tools): the cap of cells per axis of the maps'
 * search grids in the fine and the coarse stage, handed to bev_set_submap_search_grid before the first chunk; a single number
 * sets both stages.  Integers 0 ... 1024; unset, empty or 0: the grids, the launches and the output as ever.  The output does
 * not depend on it.  Anything else: exit 1 with "BEV_SUBMAP_SEARCH_GRID '<text>': expected <fine>[,<coarse>], integers 0 ...
 * 1024" and the usage line, before any GPU work.
 *
 * batch_verified_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]] (a third build,
 * BEV_VERIFY_TOOL 1) is batch_submap_registration, stdout and reports included, with the third step of "retrieve,
 * register, verify" behind every chunk: bev_submap_verify_registration_device_resident on the chunk's fine results, at leaf 0.2
 * and one threshold.  Two values from the environment: BEV_VERIFY_THRESHOLD (metres, default 0.5) and BEV_VERIFY_MIN_OVERLAP
 * (default 0.3), finite and > 0, the overlap at most 1; anything else: exit 1 with the usage line before any GPU work.  Both
 * defaults are PLACEHOLDERS that nobody has tuned on real sweeps.  overlap = query_within / n_query, and at half_window 0 (a
 * frame against a frame) the smaller of that and target_within / n_target (a map is larger than a sweep by construction, so its
 * side says nothing); 0 where a count it divides by is 0.  A match is accepted iff converged && fitness <= 1.5 && overlap >=
 * min_overlap.  Into the working directory go verification_detail.csv (a header, then one row per input match in input order:
 * query, match, fitness, converged, n_query, n_target, query_within, target_within, overlap, accepted, the 12 entries of T) and
 * verified_match_result.txt (one line "query_idx match_idx yaw" per accepted match, yaw = atan2(T[4], T[0]) in degrees: a match
 * list that loadMatchResults reads back).
 *
 * batch_aligned_registration <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]] (a fourth build,
 * BEV_ALIGN_TOOL 1) is batch_submap_registration, stdout and reports included, with a translation guess ahead of
 * the fine stage of every chunk: the height grids of the chunk's maps (bev_align_grid_device_resident), the shift search of every
 * match (bev_align_hits_device_resident), and the fine stage from that table in place of the yaw guess.  BEV_ALIGN=<grid>,<cell>,
 * <max_shift>,<yaw_steps>,<yaw_step> in the environment overrides the defaults (bev_align_defaults; skip_label0 stays 1); unset or
 * empty: the defaults; anything but five numbers inside the admitted values: exit 1 with "BEV_ALIGN '<text>': expected
 * <grid>,<cell>,<max_shift>,<yaw_steps>,<yaw_step> ..." and the usage line before any GPU work.  Into the working directory goes
 * alignment_detail.csv: a header, then two rows per input match in input order, flip 0 and flip 1: query, match, flip, chosen (1
 * on the row the fine stage started from), dx, dy, k, score, eq, ec, off_x, off_y, fitness, tx, ty.
 *
 * The chunks, the chain and the bookkeeping are the four registration tools' own (RegistrationChunks.h, RegistrationChain.h;
 * DESIGN.md §6p), the entries' matrices every submap tool's (submapwin::appendEntryPose): this file is the command line, which
 * file an index names, and the poses.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "Registration.h"
#include "RegistrationChain.h"
#include "SearchGridEnv.h"
#include "SubmapWindows.h"

#ifndef BEV_SUBMAP_TOP_PART
#define BEV_SUBMAP_TOP_PART 0
#endif
#ifndef BEV_VERIFY_TOOL
#define BEV_VERIFY_TOOL 0
#endif
#ifndef BEV_ALIGN_TOOL
#define BEV_ALIGN_TOOL 0
#endif

namespace {

constexpr bool kTopPart = BEV_SUBMAP_TOP_PART, kVerify = BEV_VERIFY_TOOL, kAlign = BEV_ALIGN_TOOL;
static_assert(!(kTopPart && kVerify), "the verified tool is the whole tool's chain");
static_assert(!(kAlign && (kTopPart || kVerify)), "the aligned tool is the whole tool's chain");
const char *const kTool = kAlign    ? "batch_aligned_registration"
                          : kVerify ? "batch_verified_registration"
                          : kTopPart ? "batch_submap_top_part_registration"
                                     : "batch_submap_registration";

void usage()
{
    std::cerr << "Usage: " << kTool << " <match_result_text_file> <keyframes_root_dir> <half_window> [<chunk> [<map_leaf>]]\n";
    if (kVerify)
        std::cerr << "  environment: BEV_VERIFY_THRESHOLD=<metres> (default 0.5), BEV_VERIFY_MIN_OVERLAP=<share> (default 0.3): finite, > 0,\n"
                     "  the overlap <= 1.  Both defaults are placeholders that nobody has tuned on real sweeps.\n";
    if (kAlign)
        std::cerr << "  environment: BEV_ALIGN=<grid>,<cell>,<max_shift>,<yaw_steps>,<yaw_step> (default 128,0.5,16,1,2): grid even, 16 ... 128;\n"
                     "  cell > 0; max_shift 1 ... 16 and 2 * max_shift <= grid / 2; yaw_steps 0 ... 3; yaw_step >= 0.\n";
}

/* BEV_ALIGN: five numbers and nothing else, inside the admitted values (bev_align_grid_bytes says which) */
bool parse_align(const char *s, bev_align_params_t *out)
{
    bev_align_params_t p = *out;
    int used = 0;
    if (std::sscanf(s, "%d,%f,%d,%d,%f%n", &p.grid, &p.cell, &p.max_shift, &p.yaw_steps, &p.yaw_step, &used) != 5 || s[used] != '\0')
        return false;
    for (const char *c = s; *c; ++c) /* (sscanf reads "nan", "inf" and leading blanks: digits, signs, points and exponents only) */
        if (!std::strchr("0123456789+-.,eE", *c)) return false;
    if (bev_align_grid_bytes(&p) == 0) return false;
    *out = p;
    return true;
}

/* the two rows of a match in alignment_detail.csv */
void aligned_rows(std::FILE *csv, const MatchResult &mt, const bev_icp_result_t *table, const bev_align_detail_t *detail, int best)
{
    for (int flip = 0; flip < 2; ++flip) {
        const bev_align_detail_t &d = detail[flip];
        std::fprintf(csv, "%d,%d,%d,%d,%d,%d,%d,%u,%u,%u,%.9g,%.9g,%.17g,%.9g,%.9g\n", mt.query_idx, mt.match_idx, flip,
                     best == flip ? 1 : 0, d.dx, d.dy, d.k, d.score, d.eq, d.ec, (double)d.off_x, (double)d.off_y, table[flip].fitness,
                     (double)table[flip].T[3], (double)table[flip].T[7]);
    }
}

/* BEV_VERIFY_THRESHOLD, BEV_VERIFY_MIN_OVERLAP: unset or empty: the default; a finite number in (0, most]; else false */
bool verify_env(const char *name, float most, float *out)
{
    const char *s = std::getenv(name);
    if (!s || !*s) return true;
    char *end = nullptr;
    const float v = std::strtof(s, &end);
    if (end == s || *end != '\0' || !std::isfinite(v) || !(v > 0.0f) || v > most) return false;
    *out = v;
    return true;
}

/* a row of verification_detail.csv, and the match's line of verified_match_result.txt where it is accepted */
void verified_row(std::FILE *csv, std::FILE *list, const MatchResult &mt, const bev_icp_result_t &r, const bev_verify_result_t &v,
                  bool pair, float min_overlap)
{
    const double fwd = v.n_query && v.query_within[0] ? (double)v.query_within[0] / (double)v.n_query : 0.0;
    const double rev = v.n_target && v.target_within[0] ? (double)v.target_within[0] / (double)v.n_target : 0.0;
    const double overlap = pair ? std::min(fwd, rev) : fwd;
    const bool accepted = r.converged && r.fitness <= 1.5 && overlap >= (double)min_overlap;
    std::fprintf(csv, "%d,%d,%.17g,%d,%u,%u,%u,%u,%.17g,%d", mt.query_idx, mt.match_idx, r.fitness, r.converged, v.n_query, v.n_target,
                 v.query_within[0], v.target_within[0], overlap, accepted ? 1 : 0);
    for (int k = 0; k < 12; ++k) std::fprintf(csv, ",%.9g", (double)r.T[k]);
    std::fprintf(csv, "\n");
    if (accepted)
        std::fprintf(list, "%d %d %.9g\n", mt.query_idx, mt.match_idx,
                     (double)(float)(std::atan2((double)r.T[4], (double)r.T[0]) * 180.0 / 3.14159265358979323846));
}

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
        usage();
        return 1;
    }
    float map_leaf = 0.0f, pn_leaf = 0.0f, threshold = 0.5f, min_overlap = 0.3f;
    if (kVerify && !(verify_env("BEV_VERIFY_THRESHOLD", INFINITY, &threshold) && verify_env("BEV_VERIFY_MIN_OVERLAP", 1.0f, &min_overlap))) {
        std::cerr << "BEV_VERIFY_THRESHOLD / BEV_VERIFY_MIN_OVERLAP: expected finite numbers > 0, the overlap at most 1\n";
        usage();
        return 1;
    }
    bev_align_params_t aprm = bev_align_defaults();
    if (const char *env = kAlign ? std::getenv("BEV_ALIGN") : nullptr)
        if (*env && !parse_align(env, &aprm)) {
            std::cerr << "BEV_ALIGN '" << env << "': expected <grid>,<cell>,<max_shift>,<yaw_steps>,<yaw_step> inside the admitted values\n";
            usage();
            return 1;
        }
    if (const char *env = kTopPart ? std::getenv("BEV_SUBMAP_PN_LEAF") : nullptr)
        if (*env && !parse_map_leaf(env, &pn_leaf)) {
            std::cerr << "BEV_SUBMAP_PN_LEAF '" << env << "': expected a finite number >= 0\n";
            return 1;
        }
    bool top_union = false;
    if (const char *env = kTopPart ? std::getenv("BEV_SUBMAP_TOP_UNION") : nullptr)
        if (*env && std::string(env) != "0") {
            if (std::string(env) != "1") {
                std::cerr << "BEV_SUBMAP_TOP_UNION '" << env << "': expected 0 or 1\n";
                return 1;
            }
            if (!(pn_leaf > 0.0f)) {
                std::cerr << "BEV_SUBMAP_TOP_UNION=1 needs BEV_SUBMAP_PN_LEAF > 0\n";
                return 1;
            }
            top_union = true;
        }
    int search_grid[2] = {0, 0};
    if (const char *env = std::getenv("BEV_SUBMAP_SEARCH_GRID"))
        if (*env && !parse_search_grid(env, BEV_SUBMAP_SEARCH_GRID_MAX, search_grid)) {
            std::cerr << "BEV_SUBMAP_SEARCH_GRID '" << env << "': expected <fine>[,<coarse>], integers 0 ... " << BEV_SUBMAP_SEARCH_GRID_MAX
                      << "\n";
            usage();
            return 1;
        }
    if (argc > 5 && !parse_map_leaf(argv[5], &map_leaf)) {
        std::cerr << "map_leaf '" << argv[5] << "': expected a finite number >= 0\n";
        usage();
        return 1;
    }
    std::string root(argv[2]);
    if (root.empty() || root.back() != '/') root.append("/");
    long half = 0, limit = 256;
    if (!submapwin::parseCount(argv[3], 0, &half)) {
        std::cerr << "half_window '" << argv[3] << "': expected an integer >= 0\n";
        return 1;
    }
    if (argc > 4 && !submapwin::parseCount(argv[4], 2 * half + 2, &limit)) {
        std::cerr << "chunk '" << argv[4] << "': expected an integer >= 2 * half_window + 2\n";
        return 1;
    }
    limit = std::max(limit, 2 * half + 2); /* (the default too: a match's query and window always fit) */
    /* the whole tool's empty report and this tool's own beside it; the top-part tool's report */
    std::ofstream report(kTopPart ? "./icp_precision_report.txt" : "./icp_precision_report_3d_icp_directly.txt"), submap_report;
    if (!kTopPart) submap_report.open("./icp_precision_report_submap.txt");
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
    const bev_icp_params_t prm = kTopPart ? bev_icp_fine_defaults() : bev_icp_whole_defaults();
    bev_verify_params_t vprm{};
    vprm.leaf = 0.2f;
    vprm.n_thresholds = 1;
    vprm.threshold[0] = threshold;
    std::FILE *csv = kVerify ? std::fopen("./verification_detail.csv", "w") : nullptr;
    std::FILE *list = kVerify ? std::fopen("./verified_match_result.txt", "w") : nullptr;
    if (kVerify && (!csv || !list)) {
        std::cerr << "verification_detail.csv / verified_match_result.txt: can not be written\n";
        return 1;
    }
    if (kVerify)
        std::fprintf(csv, "query,match,fitness,converged,n_query,n_target,query_within,target_within,overlap,accepted,"
                          "t00,t01,t02,t03,t10,t11,t12,t13,t20,t21,t22,t23\n");
    std::FILE *align_csv = kAlign ? std::fopen("./alignment_detail.csv", "w") : nullptr;
    if (kAlign && !align_csv) {
        std::cerr << "alignment_detail.csv: can not be written\n";
        return 1;
    }
    if (kAlign) std::fprintf(align_csv, "query,match,flip,chosen,dx,dy,k,score,eq,ec,off_x,off_y,fitness,tx,ty\n");
    regchain::Tally tally(kTopPart ? &report : &submap_report,
                          kTopPart ? regchain::ReportAgainst::ChosenCoarse : regchain::ReportAgainst::YawGuess);
    if (search_grid[0] || search_grid[1]) {
        bev_ctx_t *ctx = bevhost_context();
        if (!ctx || bev_set_submap_search_grid(ctx, search_grid[0], search_grid[1]) != BEV_OK) return 2;
    }
    for (size_t m0 = 0; m0 < matches.size();) {
        /* the indices are places in the sorted listing: windows clipped to it, one map per match */
        const regchain::Chunk chunk = regchain::planChunk(matches.data(), matches.size(), m0, half, 0, n_files - 1, limit, true);
        std::vector<std::string> paths;
        for (long f : chunk.files) paths.push_back(files[f]);
        std::vector<float> entry_pose;
        for (size_t k = 0; k < chunk.matches.size(); ++k)
            for (uint64_t e = chunk.map_offs[k]; e < chunk.map_offs[k + 1]; ++e)
                submapwin::appendEntryPose(pose, matches[m0 + k].match_idx, chunk.files[chunk.entry_frame[e]], entry_pose);
        regchain::ChunkResult res;
        if (const int rc = regchain::registerChunk(paths, chunk, &entry_pose, map_leaf, kTopPart, prm, tally, pn_leaf, top_union,
                                                   kVerify ? &vprm : nullptr, kVerify || kAlign ? &res : nullptr,
                                                   kAlign ? &aprm : nullptr))
            return rc;
        for (size_t k = 0; kAlign && k < chunk.matches.size(); ++k)
            aligned_rows(align_csv, matches[m0 + k], &res.coarse[2 * k], &res.align[2 * k], res.best[k]);
        for (size_t k = 0; kVerify && k < chunk.matches.size(); ++k)
            verified_row(csv, list, matches[m0 + k], res.fine[k], res.verify[k], half == 0, min_overlap);
        m0 = chunk.m1;
    }
    /* batch_submap_registration's fine line is the whole visit of the device, uploads included */
    tally.print(std::cout, kTopPart, !kTopPart);
    if (kVerify && (std::fclose(csv) != 0 || std::fclose(list) != 0)) return 1;
    if (kAlign && std::fclose(align_csv) != 0) return 1;
    return 0;
}
