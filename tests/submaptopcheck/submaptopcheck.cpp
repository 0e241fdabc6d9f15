/*
 * submaptopcheck — the plan of a scan-to-map coarse call whose maps are the thinned top part over the union of their entries'
 * moved full clouds (csrc/bev_submap_reg_plan.h with top_union beside point_normal and union_voxel) on seeded
 * random calls, at group caps from "every map alone" to "all maps together", for the eight combinations of the three older
 * options and for top_union with and without all_maps.  Checked per plan, against byte models RESTATED here in plain numbers (so
 * the existing combinations are pinned to what they were before this one came):
 *   bytes     a map's bytes under its options: fine 32 cap + 4 * 16385 + 32; its union grid + 16 cap + 8 K + 4 (cap + 1) + 32;
 *             PointNormal 64 cap + 4 * 4097 + 32; PointNormal thinned 136 cap + 8 K + 4 + 4 * 4097 + 32 + 32, K the smallest
 *             power of two >= cap (0 for cap 0); top_union, for a union of c records and r = c / 5 + 51 rows: 8 c (a key per
 *             record) + 2816 (100 cells of three words and two double words, four words) + 25600 (100 x 64 words of histogram)
 *             + the thinned PointNormal bytes of r rows, whose 8 K hold the padded selection first;
 *   groups    consecutive used maps, greedy: a group's bytes are within the cap unless it is one map, and the next map did not
 *             fit; a map's rows lie at pt0 = the capacities before it in its group (top_union: capacities in ROWS, r); with
 *             union_voxel its keys at key0 = the key slots before it, the group's keys and largest key array; top_union: its
 *             union keys at map_u0 = the union records before it, the group's union records and largest union; without
 *             top_union none of these exist;
 *   entries   top_union: an entry's pad words are its first index in the union and its record count, entry after entry; else 0;
 *   maxima    the largest group's rows, maps, keys and union records;
 *   used      all_maps: every map is used; else the maps that a match names;
 *   capacity  with frames counted at one stride (the PointNormal calls without top_union): entries * stride.
 * Prints one "ok:" line, or "PLAN ..." lines and exits 1.  Tests only.
 */
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../point-cloud-preprocessing-tools_amd/csrc/bev_submap_reg_plan.h"

using namespace bevsubreg;

static long g_bad = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("PLAN " __VA_ARGS__);  \
            std::printf("\n");                 \
            ++g_bad;                           \
        }                                      \
    } while (0)

static uint64_t pow2(uint64_t n)
{
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return n ? p : 0;
}

/* the byte models, restated */
static uint64_t rows_of(uint64_t c) { return c / 5 + 51; }
static uint64_t restated(const Options &o, uint64_t cap)
{
    if (o.top_union) return 8 * cap + 2816 + 25600 + 136 * rows_of(cap) + 8 * pow2(rows_of(cap)) + 4 + 4 * 4097 + 32 + 32;
    if (o.point_normal && o.union_voxel) return 136 * cap + 8 * pow2(cap) + 4 + 4 * 4097 + 32 + 32;
    if (o.point_normal) return 64 * cap + 4 * 4097 + 32;
    if (o.union_voxel) return 32 * cap + 4 * 16385 + 32 + 16 * cap + 8 * pow2(cap) + 4 * (cap + 1) + 32;
    return 32 * cap + 4 * 16385 + 32;
}

int main()
{
    std::mt19937_64 rng(20261020);
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    long plans = 0, groups = 0, oversize = 0, thinned = 0;
    Options top;
    top.point_normal = top.union_voxel = top.top_union = true;
    CHECK(kTopCellBytes == 2816 && kTopHistBytes == 25600 && kTopMaxUnion == (1ull << 24), "the select's tables");
    CHECK(top_max_out(0) == 51 && top_max_out(99) == 70 && top_max_out(1ull << 24) == 3355494 && top_max_out(1ull << 24) < (1ull << 22),
          "top_max_out");
    for (uint64_t c : {0ull, 1ull, 19ull, 20ull, 20224ull, 20225ull, 70000ull, 2800000ull, 1ull << 24})
        CHECK(map_top_union_bytes(c) == restated(top, c), "map_top_union_bytes(%llu)", (unsigned long long)c);
    CHECK(map_top_union_bytes(2800000) == 8 * 2800000ull + 28416 + 136 * 560051ull + 8 * 1048576ull + 16456, "a map of 21 sweeps");
    CHECK(kCoarseUnionRowBytes == 136, "a thinned PointNormal row costs %u bytes", kCoarseUnionRowBytes);
    for (uint64_t cap : {0ull, 1ull, 2ull, 4095ull, 4096ull, 4097ull, 8193ull, 1ull << 22}) {
        CHECK(map_coarse_union_bytes(cap) == restated(Options{true, false, true}, cap), "map_coarse_union_bytes(%llu)", (unsigned long long)cap);
        CHECK(map_coarse_bytes(cap) == restated(Options{false, false, true}, cap), "map_coarse_bytes(%llu)", (unsigned long long)cap);
        CHECK(map_bytes(cap, true) == restated(Options{true, false, false}, cap), "map_bytes(%llu, true)", (unsigned long long)cap);
        CHECK(map_bytes(cap) == restated(Options{}, cap), "map_bytes(%llu)", (unsigned long long)cap);
    }
    for (int call = 0; call < 50; ++call) {
        const int n_frames = (int)uni(1, 40), n_maps = (int)uni(0, 25), n_matches = n_maps ? (int)uni(0, 80) : 0;
        const uint64_t stride = uni(1, 3000);
        std::vector<uint64_t> map_offs(1, uni(0, 2));
        std::vector<int32_t> entry_frame((size_t)map_offs[0], 0);
        for (int g = 0; g < n_maps; ++g) {
            const int k = uni(0, 5) == 0 ? 0 : (int)uni(1, 9);
            for (int e = 0; e < k; ++e) entry_frame.push_back((int32_t)uni(0, n_frames - 1));
            map_offs.push_back(entry_frame.size());
        }
        std::vector<float> entry_pose(entry_frame.size() * 12 + 1, 0.5f);
        std::vector<bev_match_t> matches((size_t)n_matches);
        std::vector<int> named((size_t)n_maps, 0);
        for (int m = 0; m < n_matches; ++m) {
            matches[m] = bev_match_t{(int32_t)uni(0, n_frames - 1), (int32_t)uni(0, n_maps - 1), 0.0f};
            named[matches[m].match_idx] = 1;
        }
        for (int combo = 0; combo < 10; ++combo) {
            Options opt;
            opt.union_voxel = combo & 1;
            opt.all_maps = combo & 2;
            opt.point_normal = combo & 4;
            if (combo >= 8) {
                opt = top;
                opt.all_maps = combo == 9;
            }
            /* the PointNormal calls count every frame at the stride; the others have ragged frames */
            std::vector<uint64_t> off((size_t)n_frames, 0), cnt((size_t)n_frames, stride);
            std::mt19937_64 frng(77 + call);
            for (int f = 0; (!opt.point_normal || opt.top_union) && f < n_frames; ++f) {
                cnt[f] = frng() % 10 == 0 ? 0 : 1 + frng() % 5000;
                off[f] = f ? off[f - 1] + cnt[f - 1] : 0;
            }
            const Call desc{FrameTable{off, cnt}, n_maps, map_offs.data(), entry_frame.data(), entry_pose.data(), n_matches, matches.data()};
            std::vector<int> used_maps;
            for (int g = 0; g < n_maps; ++g)
                if (opt.all_maps || named[g]) used_maps.push_back(g);
            std::vector<uint64_t> caps;
            uint64_t all = 0;
            for (int g : used_maps) {
                uint64_t c = 0;
                for (uint64_t e = map_offs[g]; e < map_offs[g + 1]; ++e) c += cnt[entry_frame[e]];
                if (opt.point_normal && !opt.top_union) CHECK(c == (map_offs[g + 1] - map_offs[g]) * stride, "call %d: capacity of map %d", call, g);
                caps.push_back(c);
                all += restated(opt, c);
            }
            for (uint64_t cap : {(uint64_t)1, (uint64_t)150000, restated(opt, 12000), all / 3 + 1, all + 1}) {
                const Plan p = plan_call(desc, opt, cap);
                ++plans;
                thinned += opt.top_union;
                CHECK(p.map_union_cap.size() == (opt.top_union ? used_maps.size() : 0) && p.map_u0.size() == p.map_union_cap.size(),
                      "call %d combo %d: the union tables", call, combo);
                CHECK(p.maps.size() == used_maps.size() && p.map_cap.size() == used_maps.size() && p.map_key0.size() == used_maps.size(),
                      "call %d combo %d: %zu maps, expected %zu", call, combo, p.maps.size(), used_maps.size());
                if (p.maps.size() != used_maps.size()) continue;
                for (size_t u = 0; u < used_maps.size(); ++u)
                    CHECK(p.map_id[u] == used_maps[u] && p.map_cap[u] == (opt.top_union ? rows_of(caps[u]) : caps[u]) &&
                              (!opt.top_union || p.map_union_cap[u] == caps[u]),
                          "call %d combo %d: map %zu", call, combo, u);
                /* the entries' pad words */
                for (size_t u = 0; u < used_maps.size(); ++u) {
                    uint64_t at = 0;
                    for (uint32_t e = 0; e < p.maps[u].n_ent; ++e) {
                        const Entry &en = p.entries[p.maps[u].ent0 + e];
                        const uint64_t n = cnt[entry_frame[map_offs[used_maps[u]] + e]];
                        CHECK(en.pad[2] == 0 && (opt.top_union ? en.pad[0] == at && en.pad[1] == n && p.slots[en.slot].n == n
                                                               : en.pad[0] == 0 && en.pad[1] == 0),
                              "call %d combo %d: map %zu entry %u pad words %u %u", call, combo, u, e, en.pad[0], en.pad[1]);
                        at += n;
                    }
                }
                /* the greedy rule, restated */
                size_t u = 0, gi = 0;
                uint64_t max_pts = 0, max_keys = 0, max_union = 0;
                uint32_t max_maps = 0;
                while (u < used_maps.size()) {
                    uint64_t bytes = 0, pts = 0, keys = 0, max_slots = 0, upts = 0, largest = 0;
                    const size_t u0 = u;
                    while (u < used_maps.size()) {
                        const uint64_t b = restated(opt, caps[u]);
                        if (u > u0 && bytes + b > cap) break;
                        CHECK(p.maps[u].pt0 == pts, "call %d combo %d: map %zu lies at %llu, expected %llu", call, combo, u,
                              (unsigned long long)p.maps[u].pt0, (unsigned long long)pts);
                        CHECK(p.map_key0[u] == (opt.union_voxel ? keys : 0), "call %d combo %d: map %zu has its keys at %llu", call, combo, u,
                              (unsigned long long)p.map_key0[u]);
                        const uint64_t rows = opt.top_union ? rows_of(caps[u]) : caps[u];
                        if (opt.union_voxel) {
                            keys += pow2(rows);
                            max_slots = std::max(max_slots, pow2(rows));
                        }
                        if (opt.top_union) {
                            CHECK(p.map_u0[u] == upts, "call %d combo %d: map %zu has its union keys at %llu", call, combo, u,
                                  (unsigned long long)p.map_u0[u]);
                            upts += caps[u];
                            largest = std::max(largest, caps[u]);
                        }
                        pts += rows;
                        bytes += b;
                        ++u;
                    }
                    CHECK(gi < p.groups.size(), "call %d combo %d: group %zu is missing", call, combo, gi);
                    if (gi >= p.groups.size()) break;
                    const Group &g = p.groups[gi++];
                    ++groups;
                    CHECK(g.map0 == u0 && g.n_maps == u - u0, "call %d combo %d: a group of maps %u + %u, expected %zu + %zu", call, combo,
                          g.map0, g.n_maps, u0, u - u0);
                    CHECK(g.union_pts == upts && g.max_union == largest, "call %d combo %d: a group's union records %llu", call, combo,
                          (unsigned long long)g.union_pts);
                    max_union = std::max(max_union, upts);
                    CHECK(g.bytes == bytes && g.pts == pts && g.keys == keys && g.max_slots == max_slots,
                          "call %d combo %d: a group's bytes %llu rows %llu keys %llu", call, combo, (unsigned long long)g.bytes,
                          (unsigned long long)g.pts, (unsigned long long)g.keys);
                    CHECK(bytes <= cap || u - u0 == 1, "call %d combo %d: a group of %zu maps above the cap", call, combo, u - u0);
                    if (bytes > cap) ++oversize;
                    max_pts = std::max(max_pts, pts);
                    max_keys = std::max(max_keys, keys);
                    max_maps = std::max(max_maps, (uint32_t)(u - u0));
                }
                CHECK(gi == p.groups.size(), "call %d combo %d: %zu groups, expected %zu", call, combo, p.groups.size(), gi);
                CHECK(p.max_group_pts == max_pts && p.max_group_maps == max_maps && p.max_group_keys == max_keys &&
                          p.max_group_union == max_union,
                      "call %d combo %d: the largest group", call, combo);
                /* every match is in the group of its map */
                size_t n_probs = 0;
                for (const Group &g : p.groups) {
                    CHECK(g.prob0 == n_probs, "call %d combo %d: a group's problems start at %u", call, combo, g.prob0);
                    for (uint32_t k = g.prob0; k < g.prob0 + g.n_probs && k < p.probs.size(); ++k)
                        CHECK(p.probs[k].map >= g.map0 && p.probs[k].map < g.map0 + g.n_maps &&
                                  p.map_id[p.probs[k].map] == matches[p.probs[k].result].match_idx,
                              "call %d combo %d: match %u in the wrong group", call, combo, p.probs[k].result);
                    n_probs += g.n_probs;
                }
                CHECK(n_probs == (size_t)n_matches && p.probs.size() == (size_t)n_matches, "call %d combo %d: problems left over", call, combo);
                if (cap == 1) CHECK(p.groups.size() == p.maps.size(), "call %d combo %d: cap 1 must put every map alone", call, combo);
                if (cap == all + 1) CHECK(p.groups.size() == (p.maps.empty() ? 0u : 1u), "call %d combo %d: one group", call, combo);
            }
        }
    }
    if (g_bad) {
        std::printf("submaptopcheck: %ld failed checks\n", g_bad);
        return 1;
    }
    std::printf("ok: submaptopcheck: %ld plans, %ld of them top-part-over-the-union plans, %ld launch groups, %ld of them single maps above the cap\n",
                plans, thinned, groups, oversize);
    return 0;
}
