/*
 * submapfloatcheck.cpp — TEST HELPER (never shipped, never loaded by the product).
 *
 * Builds the plan of a float submap call (csrc/bev_submap_plan.h) the way bev_submap_float_bev_device_resident does — a cap of
 * all the call's maps, so ONE launch group whose grids are the maps —, packs it into the block the device would get, and
 * "executes" that block sequentially on the host the way k_submap_float_splat does: workgroup -> row of the frame table
 * (packed_place's binary search), the workgroup's 1024 points, per entry of the row transform_xyz (csrc/bev_exact.h) and the
 * float cell rule (float_bev_cell, csrc/bev_misc.h, restated here: that header is device code) into the entry's grid, the
 * maximum taken over the floats' bit patterns as the device's atomic does.  Every float of every map's grid is compared, as
 * bits, with oracle_float_bev of the concatenated oracle_transform_cloud outputs.  A stand-alone program: exit status 0 and a
 * last line "ok: submapfloatcheck: ..." when every case agrees, 1 and the failing cases otherwise.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bev_mi355x.h"
#include "../../oracle/bev_oracle.h"
#include "../../point-cloud-preprocessing-tools_amd/csrc/bev_exact.h"
#include "../../point-cloud-preprocessing-tools_amd/csrc/bev_submap_plan.h"

extern "C" size_t bev_synth_adversarial(const bev_params_t *p, uint64_t seed, uint32_t n_points, int with_nonfinite,
                                        bev_point_t *out, size_t cap);

using namespace bevx;
static_assert(sizeof(oracle_point_t) == sizeof(bev_point_t), "one record layout");

namespace {

/* float_bev_cell (csrc/bev_misc.h): the cell x * M + y of a point that counts and its height, or -1 */
int float_cell(float px, float py, float pz, int label, float interval, int M, int skip_label0, float &h)
{
    const int x = bev_bin(px, 100.0f, interval);
    const int y = bev_bin(py, 100.0f, interval);
    h = pz + 2.0f;
    if (x < 0 || x >= M || y < 0 || y >= M) return -1;
    if (skip_label0 && label == 0) return -1;
    return h > 0.0f ? x * M + y : -1;
}
/* bev_float_bev_size (csrc/bev_capi.hip) */
int float_size(float interval) { return cvtt_f32((float)200 / interval + 1); }

struct Pose { float tx, ty, tz, yaw; };
/* tests/submapcheck's poses: the identity, four general ones, one that pushes most points off the grid, a quarter turn */
const Pose kPoses[] = {{0, 0, 0, 0}, {1.5f, -2.25f, 0.125f, 30}, {-3, 4, 1, -45.5f}, {10, 20, -1, 180}, {0.1f, 0.2f, 0.3f, 359.9f},
                       {150, 0, 0, 10}, {-7.5f, 2, 0.5f, 90}};
constexpr int kNumPoses = (int)(sizeof kPoses / sizeof kPoses[0]);
/* two entries of map T of tests/raster_world_cases.py (frames 1 and 4 about a tilted origin): general rigid matrices, every one
 * of the 12 entries far from 0 and 1.  The Pose list above never has m[2], m[6], m[8], m[9] != 0 */
const float kGeneral[2][12] = {
    {0.9024916887283325f, 0.41009873151779175f, 0.13163472712039948f, -12.794914245605469f, -0.4304434359073639f, 0.8694769144058228f,
     0.24233940243721008f, 4.982234001159668f, -0.015070266090333462f, -0.27537062764167786f, 0.9612199664115906f, 1.820896863937378f},
    {0.9889324307441711f, -0.09149842709302902f, 0.11679299175739288f, -0.9883042573928833f, 0.05859272927045822f, 0.9640607237815857f,
     0.2591405510902405f, 3.9861388206481934f, -0.13630647957324982f, -0.24942927062511444f, 0.9587520956993103f, 0.1872139722108841f}};
/* pose index kNumPoses + g names kGeneral[g]; `bump` tells the entries of a scenario apart (added to tz) */
void pose_matrix(int index, float bump, float m[12])
{
    if (index < kNumPoses) {
        const Pose &q = kPoses[index];
        oracle_yaw_translate_matrix(q.tx, q.ty, q.tz + bump, q.yaw, m);
        return;
    }
    memcpy(m, kGeneral[index - kNumPoses], 12 * sizeof(float));
    m[11] += bump;
}

struct Scenario {
    const char *name;
    bool general = false;                               /* counted apart: the scenarios under kGeneral */
    std::vector<uint32_t> sizes;                        /* records per frame */
    std::vector<std::vector<std::pair<int, int>>> maps; /* per map its (frame, pose) entries */
};

/* what the device does with the packed block of the call's one group: the grids of its maps, as bit patterns */
void run_group(const char *block, const bevsub::GroupBytes &at, const bevsub::Group &g, const bev_point_t *clouds, float interval,
               int M, int skip_label0, std::vector<uint32_t> &grids)
{
    const size_t cells = (size_t)M * (size_t)M;
    grids.assign((size_t)g.n_maps * cells, 0u);
    const bevsub::Frame *tab = reinterpret_cast<const bevsub::Frame *>(block + at.rows);
    const uint32_t *ent0 = reinterpret_cast<const uint32_t *>(block + at.ent0);
    const bevsub::Entry *entries = reinterpret_cast<const bevsub::Entry *>(block + at.entries);
    for (uint32_t bid = 0; bid < g.blocks; ++bid) {
        int lo = 0, hi = g.n_rows; /* packed_place (csrc/bev_dev.h) */
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (tab[mid].blk0 <= bid) lo = mid;
            else hi = mid;
        }
        const uint32_t k0 = (bid - tab[lo].blk0) * bevsub::kBlockPoints, k1 = std::min(tab[lo].n, k0 + bevsub::kBlockPoints);
        for (uint32_t e = ent0[lo]; e < ent0[lo + 1]; ++e) {
            const bevsub::Entry &en = entries[e];
            uint32_t *grid = grids.data() + (size_t)en.grid * cells;
            for (uint32_t k = k0; k < k1; ++k) {
                const bev_point_t &q = clouds[tab[lo].off + k];
                float tx, ty, tz, h;
                transform_xyz(en.m, q.x, q.y, q.z, tx, ty, tz);
                const int cell = float_cell(tx, ty, tz, (int)q.label, interval, M, skip_label0, h);
                if (cell < 0) continue;
                uint32_t bits;
                memcpy(&bits, &h, sizeof bits);
                grid[cell] = std::max(grid[cell], bits);
            }
        }
    }
}

Scenario mixed()
{
    Scenario s;
    s.name = "mixed";
    s.sizes = {0, 1, 1024, 1025, 3000, 257, 5000, 2049}; /* frames 6 and 7: named by no map */
    s.maps = {{},
              {{4, 1}, {1, 2}, {4, 3}, {2, 0}}, /* frame 4 twice */
              {{2, 0}, {3, 4}},
              {},
              {{5, 6}, {4, 5}, {3, 2}, {2, 1}, {1, 3}, {0, 4}}, /* every frame with entries, not in frame order */
              {{2, 2}, {5, 1}, {0, 0}},
              {}};
    return s;
}
Scenario shared_frame()
{
    Scenario s;
    s.name = "a frame in every map";
    s.sizes = {700, 4097, 0, 1500};
    for (int m = 0; m < 5; ++m) {
        s.maps.push_back({{1, m}, {(m * 3) % 4, (m + 2) % kNumPoses}});
        if (m == 2) s.maps.back().push_back({1, 6});
    }
    return s;
}
/* the mixed frames under the general matrices, alone and next to yaw poses: one frame twice, a map of one matrix only */
Scenario general_matrices()
{
    Scenario s;
    s.name = "general matrices";
    s.general = true;
    s.sizes = {0, 1, 1024, 1025, 3000, 257, 5000, 2049};
    s.maps = {{{4, kNumPoses}, {1, kNumPoses + 1}, {4, kNumPoses + 1}, {2, 0}},
              {{6, kNumPoses}},
              {{3, kNumPoses + 1}, {5, 2}, {6, kNumPoses}, {7, kNumPoses + 1}, {0, kNumPoses}},
              {}};
    return s;
}
Scenario no_maps()
{
    Scenario s;
    s.name = "zero maps";
    s.sizes = {10, 2000};
    return s;
}
Scenario no_frames()
{
    Scenario s;
    s.name = "zero frames";
    s.maps = {{}, {}, {}};
    return s;
}

} // namespace

int main()
{
    bev_params_t bp{}; /* HDL_64E (bev_params_for_sensor): what the adversarial cloud is shaped by */
    bp.n_scan = 64;
    bp.horizon_scan = 2083;
    bp.ground_upper_scan = 50;
    bp.height_res = 0.25f;
    bp.interval = 1.0f;
    bp.max_range = 112;
    bp.n_layers = 24;
    bp.lidar_to_ground = 2.0f;
    std::vector<bev_point_t> adv(60000);
    adv.resize(bev_synth_adversarial(&bp, 3, 60000, 1, adv.data(), adv.size()));

    int cases = 0, general_cases = 0, bad = 0, bad_plans = 0;
    size_t set_floats = 0, groups_run = 0, skipped_by_label = 0, general_floats = 0;
    const Scenario scenarios[] = {mixed(), shared_frame(), no_maps(), no_frames(), general_matrices()};
    for (const Scenario &sc : scenarios) {
        /* the frames: slices of the adversarial cloud, one after the other */
        std::vector<bev_point_t> clouds;
        std::vector<uint64_t> offs(1, 0);
        for (size_t f = 0; f < sc.sizes.size(); ++f) {
            clouds.insert(clouds.end(), adv.begin() + 997 * (long)f, adv.begin() + 997 * (long)f + sc.sizes[f]);
            offs.push_back(clouds.size());
        }
        std::vector<uint64_t> map_offs(1, 0);
        std::vector<int32_t> entry_frame;
        std::vector<float> entry_pose;
        for (const auto &map : sc.maps) {
            for (const auto &fp : map) {
                entry_frame.push_back(fp.first);
                float m[12];
                /* (no two entries of a scenario share frame, map AND matrix: the entry's place tells them apart) */
                pose_matrix(fp.second, 0.001f * (float)entry_frame.size(), m);
                entry_pose.insert(entry_pose.end(), m, m + 12);
            }
            map_offs.push_back(entry_frame.size());
        }
        const int n_maps = (int)sc.maps.size();
        /* the plan of the call: a cap of all its maps */
        bevsub::Plan plan;
        if (!bevsub::plan_maps(plan, offs.data(), map_offs.data(), 0, n_maps, entry_frame.data(), entry_pose.data(), (size_t)n_maps) ||
            plan.groups.size() != (n_maps ? 1u : 0u) || (n_maps && (plan.groups[0].map0 != 0 || plan.groups[0].n_maps != n_maps))) {
            printf("PLAN %s: not one group of all maps\n", sc.name);
            ++bad_plans;
            continue;
        }
        if (n_maps)
            for (size_t e = 0; e < plan.groups[0].n_entries; ++e) bad_plans += plan.entries[e].grid >= (uint32_t)n_maps;
        std::vector<bevsub::Entry> block((bevsub::pack(plan, nullptr) + 63) / 64 + 1); /* 64-byte aligned storage */
        bevsub::pack(plan, reinterpret_cast<char *>(block.data()));
        for (const float interval : {1.0f, 2.0f, 0.5f})
            for (const int skip : {1, 0}) {
                const int M = float_size(interval);
                const size_t cells = (size_t)M * (size_t)M;
                std::vector<uint32_t> grids;
                if (n_maps) {
                    run_group(reinterpret_cast<const char *>(block.data()), bevsub::group_bytes(plan.groups[0], 0), plan.groups[0],
                              clouds.data(), interval, M, skip, grids);
                    groups_run += sc.general ? 0 : 1;
                }
                for (int m = 0; m < n_maps; ++m) {
                    std::vector<oracle_point_t> all(1); /* (never an empty vector's pointer) */
                    all.clear();
                    for (uint64_t e = map_offs[m]; e < map_offs[m + 1]; ++e) {
                        const int f = entry_frame[e];
                        const size_t n = sc.sizes[f], at = all.size();
                        all.resize(at + n);
                        if (n)
                            oracle_transform_cloud(reinterpret_cast<const oracle_point_t *>(clouds.data() + offs[f]), n,
                                                   entry_pose.data() + 12 * e, all.data() + at);
                    }
                    std::vector<float> want(cells, -1.0f);
                    oracle_float_bev(all.data(), all.size(), interval, skip, want.data());
                    ++(sc.general ? general_cases : cases);
                    size_t set = 0;
                    for (size_t i = 0; i < cells; ++i) set += grids[(size_t)m * cells + i] != 0u;
                    (sc.general ? general_floats : set_floats) += set;
                    if (all.empty() && set) {
                        ++bad;
                        printf("MISMATCH %s, interval %g, skip %d: map %d has no point and a grid that is not zero\n", sc.name,
                               (double)interval, skip, m);
                    }
                    if (memcmp(want.data(), grids.data() + (size_t)m * cells, cells * sizeof(float)) != 0) {
                        ++bad;
                        printf("MISMATCH %s, interval %g, skip %d: map %d\n", sc.name, (double)interval, skip, m);
                    }
                    if (skip == 0) { /* the label test does something: the grid under it differs somewhere in the run */
                        std::vector<float> with(cells);
                        oracle_float_bev(all.data(), all.size(), interval, 1, with.data());
                        skipped_by_label += memcmp(with.data(), want.data(), cells * sizeof(float)) != 0;
                    }
                }
            }
    }
    if (bad_plans || bad || set_floats == 0 || general_floats == 0 || skipped_by_label == 0) {
        printf("submapfloatcheck FAILED: %d plans, %d of %d grids\n", bad_plans, bad, cases + general_cases);
        return 1;
    }
    printf("ok: submapfloatcheck: %d grids in %zu launch groups, %zu non-zero floats compared, label 0 mattered in %zu; under general "
           "matrices %d more grids, %zu non-zero floats\n",
           cases, groups_run, set_floats, skipped_by_label, general_cases, general_floats);
    return 0;
}
