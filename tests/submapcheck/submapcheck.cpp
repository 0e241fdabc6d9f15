/*
 * submapcheck.cpp — TEST HELPER (never shipped, never loaded by the product).
 *
 * Builds the plan of a submap call (csrc/bev_submap_plan.h), packs it into the block the device would get, and "executes"
 * every launch group from that block sequentially on the host the way k_submap_splat does: workgroup -> row of the group's
 * frame table (packed_place's binary search), the workgroup's 1024 points, per entry of the row posed_code (csrc/bev_exact.h)
 * into the two planes of the entry's grid.  The planes are expanded as tests/posedcheck does and every byte of both images of
 * every map is compared with oracle_multi_bev / oracle_single_bev of the concatenated oracle_transform_cloud outputs.  The
 * plan's invariants are asserted on the way.  The packed-frame table that the calls without maps send up instead of a plan
 * (bevsub::frame_table) is checked from offsets alone: its rows, its closing row and the limit of a launch.  A stand-alone program: exit status 0 and a last line "submapcheck ok: ..." when
 * every case agrees, 1 and the failing cases otherwise.
 */
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <tuple>
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

RasterParams raster_params(float height_res, float interval)
{
    RasterParams rp{};
    rp.max_range_f = 112.0f; /* BatchMultiBevGen.cpp:266-269 */
    rp.interval = interval;
    rp.height_res = height_res;
    rp.lidar_to_ground = 2.0f;
    rp.mat_size = cvtt_f32(224.0f / interval);
    rp.n_layers = 24;
    rp.inv_interval = exact_reciprocal(interval);
    rp.inv_height_res = exact_reciprocal(height_res);
    /* (the bands cut the device's work, not the result: posed_code does not read them) */
    rp.coarse = rp.fine = rp.mat_size / 8;
    rp.z0 = rp.z1 = 0;
    rp.bands = 8;
    rp.coarse_magic = rp.fine_magic = small_div_magic(rp.coarse);
    return rp;
}

struct Pose { float tx, ty, tz, yaw; };
/* tests/posedcheck's first poses: the identity, four general ones, and one that pushes most points off the grid */
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

int g_bad = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_bad;                     \
            printf("PLAN " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

/* the plan's invariants for a call of n_maps maps under cap */
void check_plan(const bevsub::Plan &p, const Scenario &sc, const std::vector<uint64_t> &offs, const std::vector<uint64_t> &map_offs,
                const std::vector<int32_t> &entry_frame, const std::vector<float> &entry_pose, size_t cap, const char *tag)
{
    using Key = std::tuple<int, int, std::array<float, 12>>; /* map, frame, matrix */
    std::vector<Key> want, got;
    for (size_t m = 0; m < sc.maps.size(); ++m)
        for (uint64_t e = map_offs[m]; e < map_offs[m + 1]; ++e) {
            std::array<float, 12> a;
            memcpy(a.data(), entry_pose.data() + 12 * e, sizeof(float) * 12);
            want.emplace_back((int)m, entry_frame[e], a);
        }
    int next_map = 0;
    size_t next_row = 0, next_ent = 0;
    for (const bevsub::Group &g : p.groups) {
        CHECK(g.map0 == next_map && g.n_maps >= 1 && (size_t)g.n_maps <= cap, "%s: group of maps %d + %d, expected from %d, cap %zu", tag,
              g.map0, g.n_maps, next_map, cap);
        CHECK(g.row0 == next_row && g.ent_at == next_ent, "%s: group at map %d does not follow the one before", tag, g.map0);
        next_map = g.map0 + g.n_maps;
        next_row = g.row0 + (size_t)g.n_rows + 1;
        next_ent = g.ent_at + g.n_entries;
        const bevsub::Frame *rows = p.rows.data() + g.row0;
        const uint32_t *ent0 = p.ent0.data() + g.row0;
        const int32_t *frame = p.frame.data() + g.row0;
        CHECK(ent0[0] == 0 && ent0[g.n_rows] == g.n_entries && rows[0].blk0 == 0 && rows[g.n_rows].blk0 == g.blocks && frame[g.n_rows] == -1,
              "%s: closing values of the group at map %d", tag, g.map0);
        for (int r = 0; r < g.n_rows; ++r) {
            const int f = frame[r];
            CHECK(f >= 0 && f < (int)sc.sizes.size() && (r == 0 || f > frame[r - 1]), "%s: row %d names frame %d, not ascending", tag, r, f);
            if (f < 0 || f >= (int)sc.sizes.size()) continue;
            CHECK(rows[r].off == offs[f] && rows[r].n == sc.sizes[f], "%s: row %d: offset / count of frame %d", tag, r, f);
            CHECK(rows[r + 1].blk0 - rows[r].blk0 == (sc.sizes[f] + 1023u) / 1024u, "%s: row %d: %u workgroups for %u records", tag, r,
                  rows[r + 1].blk0 - rows[r].blk0, sc.sizes[f]);
            CHECK(ent0[r + 1] > ent0[r], "%s: row %d has no entry", tag, r); /* a frame without entries in the group has no row */
            for (uint32_t e = ent0[r]; e < ent0[r + 1]; ++e) {
                const bevsub::Entry &en = p.entries[g.ent_at + e];
                CHECK(en.grid < (uint32_t)g.n_maps, "%s: entry with grid %u of %d", tag, en.grid, g.n_maps);
                std::array<float, 12> a;
                memcpy(a.data(), en.m, sizeof en.m);
                got.emplace_back(g.map0 + (int)en.grid, f, a);
            }
        }
    }
    CHECK(next_map == (int)sc.maps.size(), "%s: the groups cover %d of %zu maps", tag, next_map, sc.maps.size());
    CHECK(next_row == p.rows.size() && p.rows.size() == p.ent0.size() && p.rows.size() == p.frame.size() && next_ent == p.entries.size(),
          "%s: rows or entries outside every group", tag);
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    CHECK(want == got, "%s: the plan's entries are not the call's, each once (%zu against %zu)", tag, got.size(), want.size());
}

/* what the device does with the packed block of one group: the planes of its maps */
void run_group(const char *block, const bevsub::GroupBytes &at, const bevsub::Group &g, const bev_point_t *clouds,
               const RasterParams &rp, std::vector<uint32_t> &planes)
{
    const size_t cells = (size_t)rp.mat_size * (size_t)rp.mat_size;
    planes.assign((size_t)g.n_maps * 2 * cells, 0u);
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
            uint32_t *hmax = planes.data() + (size_t)en.grid * 2 * cells, *mask = hmax + cells;
            for (uint32_t k = k0; k < k1; ++k) {
                const bev_point_t &q = clouds[tab[lo].off + k];
                const uint32_t c = posed_code(q.x, q.y, q.z, (int)q.label, en.m, rp);
                if (c == kSkip) continue;
                const size_t idx = (size_t)code_x(c) * (size_t)rp.mat_size + (size_t)code_y(c);
                if ((uint32_t)code_h(c) > hmax[idx]) hmax[idx] = (uint32_t)code_h(c);
                if (code_layer(c) != kNoLayer) mask[idx] |= 1u << code_layer(c);
            }
        }
    }
}

/* bevsub::frame_table from offsets alone (no clouds): every row, the closing row, the longest frame, and the limit of a launch;
 * returns the tables checked */
int check_frame_tables()
{
    int tables = 0;
    const auto run = [&](const std::vector<uint32_t> &sizes, bool want_ok, const char *tag) {
        const int nf = (int)sizes.size();
        std::vector<uint64_t> offs(1, 7); /* (a table need not start at record 0) */
        uint64_t want_blocks = 0;
        uint32_t want_max = 0;
        for (uint32_t n : sizes) {
            offs.push_back(offs.back() + n);
            want_blocks += ((uint64_t)n + 1023u) / 1024u;
            want_max = std::max(want_max, n);
        }
        const bevsub::Frame untouched{~0ull, ~0u, ~0u};
        std::vector<bevsub::Frame> rows((size_t)nf + 2, untouched); /* (one row behind the closing row: a guard) */
        uint32_t n_max = 12345u, blocks = 12345u;
        const bool ok = bevsub::frame_table(rows.data(), nf, offs.data(), &n_max, &blocks);
        ++tables;
        CHECK(ok == want_ok, "frame table %s: %s, %llu workgroups", tag, ok ? "accepted" : "refused", (unsigned long long)want_blocks);
        CHECK(rows[(size_t)nf + 1].off == untouched.off && rows[(size_t)nf + 1].n == untouched.n, "frame table %s: a row behind the table was written", tag);
        if (!ok || !want_ok) return;
        CHECK(n_max == want_max && blocks == want_blocks, "frame table %s: longest %u (%u), workgroups %u (%llu)", tag, n_max, want_max,
              blocks, (unsigned long long)want_blocks);
        uint64_t b = 0;
        for (int f = 0; f < nf; ++f) {
            CHECK(rows[f].off == offs[f] && rows[f].n == sizes[f] && rows[f].blk0 == b, "frame table %s: row %d", tag, f);
            b += ((uint64_t)sizes[f] + 1023u) / 1024u;
        }
        CHECK(rows[nf].off == offs[nf] && rows[nf].n == 0u && rows[nf].blk0 == want_blocks, "frame table %s: the closing row", tag);
    };
    run({}, true, "empty");
    run({0}, true, "0");
    run({1}, true, "1");
    run({1023}, true, "1023");
    run({1024}, true, "1024");
    run({1025}, true, "1025");
    run({0, 1, 1023, 1024, 1025, 0, 5000, 1}, true, "mixed"); /* 0 + 1 + 1 + 1 + 2 + 0 + 5 + 1 workgroups */
    /* a frame of 0xffffffff records is 4194304 workgroups: 511 of them are 2143289344 <= 2^31 - 1, 512 are exactly 2^31 */
    run(std::vector<uint32_t>(511, 0xffffffffu), true, "511 frames of 2^32 - 1");
    run(std::vector<uint32_t>(512, 0xffffffffu), false, "512 frames of 2^32 - 1");
    std::vector<uint32_t> edge(511, 0xffffffffu);
    edge.push_back(4194303u * 1024u); /* 2143289344 + 4194303 = 2^31 - 1 exactly: the most a launch can have */
    run(edge, true, "2^31 - 1 workgroups");
    edge.push_back(1u);
    run(edge, false, "2^31 workgroups");
    return tables;
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
    oracle_sensor_t sp;
    if (oracle_sensor_params(1 /* HDL_64E */, &sp) != 0) return 2;
    bev_params_t bp{};
    bp.n_scan = sp.n_scan;
    bp.horizon_scan = sp.horizon_scan;
    bp.ground_upper_scan = sp.ground_upper_scan;
    bp.height_res = sp.height_res;
    bp.interval = 1.0f;
    bp.max_range = 112;
    bp.n_layers = 24;
    bp.lidar_to_ground = 2.0f;
    std::vector<bev_point_t> adv(60000);
    adv.resize(bev_synth_adversarial(&bp, 3, 60000, 1, adv.data(), adv.size()));

    int cases = 0, general_cases = 0, bad_images = 0, prefix_sizes = 0;
    size_t set_bytes = 0, groups_run = 0, general_bytes = 0, general_groups = 0;
    const Scenario scenarios[] = {mixed(), shared_frame(), no_maps(), no_frames(), general_matrices()};
    for (const Scenario &sc : scenarios) {
        /* the frames: slices of the adversarial cloud, one after the other with a gap record between them */
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
        for (const float interval : {1.0f, 2.0f}) {
            const RasterParams rp = raster_params(sp.height_res, interval);
            const size_t M = (size_t)rp.mat_size, cells = M * M;
            /* the oracle's images of every map */
            std::vector<std::vector<uint8_t>> want_multi(sc.maps.size()), want_single(sc.maps.size());
            for (size_t m = 0; m < sc.maps.size(); ++m) {
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
                want_multi[m].assign(24 * cells, 0);
                want_single[m].assign(cells, 0);
                oracle_multi_bev(&sp, all.data(), all.size(), interval, want_multi[m].data());
                oracle_single_bev(all.data(), all.size(), interval, want_single[m].data());
                if (all.empty())
                    for (uint8_t v : want_multi[m]) bad_images += v != 0;
            }
            for (const size_t cap : {(size_t)1, (size_t)3, (size_t)1 << 40}) {
                char tag[128];
                snprintf(tag, sizeof tag, "%s, interval %g, cap %zu", sc.name, (double)interval, cap);
                bevsub::Plan plan;
                if (!bevsub::plan_maps(plan, offs.data(), map_offs.data(), 0, (int)sc.maps.size(), entry_frame.data(), entry_pose.data(), cap)) {
                    printf("PLAN %s: refused\n", tag);
                    ++g_bad;
                    continue;
                }
                check_plan(plan, sc, offs, map_offs, entry_frame, entry_pose, cap, tag);
                for (const bevsub::Group &g : plan.groups)
                    for (int r = 0; r < g.n_rows; ++r) {
                        const uint32_t n = plan.rows[g.row0 + r].n, b = plan.rows[g.row0 + r + 1].blk0 - plan.rows[g.row0 + r].blk0;
                        prefix_sizes |= (n == 0 && b == 0) | (n == 1 && b == 1) << 1 | (n == 1024 && b == 1) << 2 | (n == 1025 && b == 2) << 3;
                    }
                std::vector<bevsub::Entry> block((bevsub::pack(plan, nullptr) + 63) / 64 + 1); /* 64-byte aligned storage */
                bevsub::pack(plan, reinterpret_cast<char *>(block.data()));
                size_t at = 0;
                std::vector<uint32_t> planes;
                for (const bevsub::Group &g : plan.groups) {
                    const bevsub::GroupBytes gb = bevsub::group_bytes(g, at);
                    at = gb.end;
                    run_group(reinterpret_cast<const char *>(block.data()), gb, g, clouds.data(), rp, planes);
                    ++(sc.general ? general_groups : groups_run);
                    for (int m = 0; m < g.n_maps; ++m) {
                        const uint32_t *hmax = planes.data() + (size_t)m * 2 * cells, *mask = hmax + cells;
                        std::vector<uint8_t> multi(24 * cells), single(cells);
                        for (size_t i = 0; i < cells; ++i) {
                            single[i] = (uint8_t)hmax[i];
                            for (int l = 0; l < 24; ++l) multi[(size_t)l * cells + i] = (mask[i] >> l) & 1u ? 255 : 0;
                        }
                        ++(sc.general ? general_cases : cases);
                        for (uint8_t v : multi) (sc.general ? general_bytes : set_bytes) += v != 0;
                        if (multi != want_multi[g.map0 + m] || single != want_single[g.map0 + m]) {
                            ++bad_images;
                            printf("MISMATCH %s: map %d\n", tag, g.map0 + m);
                        }
                    }
                }
            }
        }
    }
    const int bad_before = g_bad, tables = check_frame_tables();
    printf("frame tables: %d checked, %d failed checks\n", tables, g_bad - bad_before);
    if (g_bad || bad_images || set_bytes == 0 || general_bytes == 0 || prefix_sizes != 15) /* (frames of 0, 1, 1024 and 1025 records were rows) */ {
        printf("submapcheck FAILED: %d plan checks, %d of %d images\n", g_bad, bad_images, cases + general_cases);
        return 1;
    }
    printf("submapcheck ok: %d map images in %zu launch groups, %zu occupied bytes compared; under general matrices %d more in %zu, %zu\n",
           cases, groups_run, set_bytes, general_cases, general_groups, general_bytes);
    return 0;
}
