/*
 * submapregcheck — the plan of a scan-to-map registration call (csrc/bev_submap_reg_plan.h) on seeded random
 * calls, at group caps from "every map alone" to "all maps together".  Checked per plan:
 *   slots     every frame that a match's query or a used map's entry names has exactly one slot, with the frame's offset and
 *             count; no other frame has one; Pn is the largest count;
 *   maps      the used maps, ascending; a map's entries are the call's, IN MAP ORDER, each with its frame's slot and its
 *             matrix bit for bit; its capacity is the sum of its entries' record counts;
 *   groups    consecutive maps, all of them once; a group's bytes are within the cap unless it is one map; a map's points
 *             [pt0, pt0 + capacity) lie inside its group's points and overlap no other map's; max_cap is the largest
 *             capacity among the group's maps;
 *   problems  every match is in exactly one group, the group of its map, with its own index as the result and its query's
 *             slot; a group's problems are contiguous.
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

int main()
{
    std::mt19937_64 rng(20261019);
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    long plans = 0, groups = 0, oversize = 0;
    for (int call = 0; call < 60; ++call) {
        const int n_frames = (int)uni(1, 40), n_maps = (int)uni(0, 25), n_matches = n_maps ? (int)uni(0, 80) : 0;
        std::vector<uint64_t> off((size_t)n_frames), cnt((size_t)n_frames);
        uint64_t at = 0;
        for (int f = 0; f < n_frames; ++f) {
            off[f] = at;
            cnt[f] = uni(0, 9) == 0 ? 0 : uni(1, 5000);
            at += cnt[f] + uni(0, 3);
        }
        std::vector<uint64_t> map_offs(1, uni(0, 2)); /* (the entry arrays need not start at 0) */
        std::vector<int32_t> entry_frame((size_t)map_offs[0], 0);
        for (int g = 0; g < n_maps; ++g) {
            const int k = uni(0, 5) == 0 ? 0 : (int)uni(1, 9);
            for (int e = 0; e < k; ++e) entry_frame.push_back((int32_t)uni(0, n_frames - 1)); /* repeats within a map too */
            map_offs.push_back(entry_frame.size());
        }
        std::vector<float> entry_pose(entry_frame.size() * 12 + 1);
        for (float &v : entry_pose) v = (float)uni(0, 1000000) / 1000.0f;
        std::vector<int32_t> query((size_t)n_matches), match_map((size_t)n_matches);
        std::vector<bev_match_t> matches((size_t)n_matches);
        for (int m = 0; m < n_matches; ++m) {
            query[m] = (int32_t)uni(0, n_frames - 1);
            match_map[m] = (int32_t)uni(0, n_maps - 1);
            matches[m] = bev_match_t{query[m], match_map[m], 0.0f};
        }
        const Call desc{FrameTable{off, cnt}, n_maps, map_offs.data(), entry_frame.data(), entry_pose.data(), n_matches, matches.data()};
        uint64_t all = 0;
        for (int g = 0; g < n_maps; ++g) all += map_bytes(map_capacity(cnt.data(), map_offs.data(), entry_frame.data(), g));
        for (uint64_t cap : {(uint64_t)1, map_bytes(3000), map_bytes(12000), all / 3 + 1, all + 1}) {
            const Plan p = plan_call(desc, Options{}, cap);
            ++plans;
            /* slots */
            std::vector<int> named((size_t)n_frames, 0), used((size_t)n_maps, 0), slots_of((size_t)n_frames, 0);
            for (int m = 0; m < n_matches; ++m) {
                named[query[m]] = 1;
                used[match_map[m]] = 1;
            }
            for (int g = 0; g < n_maps; ++g)
                for (uint64_t e = map_offs[g]; used[g] && e < map_offs[g + 1]; ++e) named[entry_frame[e]] = 1;
            CHECK(p.slots.size() == p.slot_frame.size(), "call %d: slot tables differ in length", call);
            size_t Pn = 1;
            for (size_t s = 0; s < p.slots.size(); ++s) {
                const int f = p.slot_frame[s];
                CHECK(f >= 0 && f < n_frames && named[f], "call %d: slot %zu names frame %d", call, s, f);
                if (f < 0 || f >= n_frames) continue;
                ++slots_of[f];
                CHECK(p.slots[s].off == off[f] && p.slots[s].n == cnt[f], "call %d: slot %zu is not frame %d", call, s, f);
                Pn = std::max(Pn, (size_t)cnt[f]);
            }
            for (int f = 0; f < n_frames; ++f) CHECK(slots_of[f] == named[f], "call %d: frame %d has %d slots", call, f, slots_of[f]);
            CHECK(p.Pn == Pn, "call %d: Pn %zu, expected %zu", call, p.Pn, Pn);
            /* maps and their entries */
            size_t n_used = 0;
            for (int g = 0; g < n_maps; ++g) n_used += used[g];
            CHECK(p.maps.size() == n_used && p.map_id.size() == n_used && p.map_cap.size() == n_used, "call %d: %zu maps, expected %zu", call, p.maps.size(), n_used);
            for (size_t u = 0; u < p.maps.size() && u < p.map_id.size(); ++u) {
                const int g = p.map_id[u];
                CHECK(g >= 0 && g < n_maps && used[g] && (u == 0 || p.map_id[u - 1] < g), "call %d: map %zu is call map %d", call, u, g);
                if (g < 0 || g >= n_maps) continue;
                const Map &mp = p.maps[u];
                CHECK(mp.n_ent == map_offs[g + 1] - map_offs[g] && (size_t)mp.ent0 + mp.n_ent <= p.entries.size(), "call %d: map %d has %u entries", call, g, mp.n_ent);
                uint64_t capacity = 0;
                for (uint32_t k = 0; k < mp.n_ent && (size_t)mp.ent0 + k < p.entries.size(); ++k) {
                    const Entry &en = p.entries[mp.ent0 + k];
                    const uint64_t e = map_offs[g] + k;
                    CHECK(en.slot < p.slots.size() && p.slot_frame[en.slot] == entry_frame[e], "call %d: map %d entry %u is not frame %d", call, g, k, entry_frame[e]);
                    CHECK(memcmp(en.m, entry_pose.data() + 12 * e, 48) == 0, "call %d: map %d entry %u has another matrix", call, g, k);
                    capacity += cnt[entry_frame[e]];
                }
                CHECK(p.map_cap[u] == capacity, "call %d: map %d capacity", call, g);
            }
            /* groups */
            uint32_t next_map = 0, next_prob = 0;
            uint64_t max_pts = 0;
            uint32_t max_maps = 0;
            std::vector<int> seen((size_t)n_matches, 0);
            for (const Group &g : p.groups) {
                ++groups;
                CHECK(g.map0 == next_map && g.n_maps >= 1 && g.map0 + g.n_maps <= p.maps.size(), "call %d: a group starts at map %u", call, g.map0);
                CHECK(g.prob0 == next_prob && (size_t)g.prob0 + g.n_probs <= p.probs.size(), "call %d: a group's problems start at %u", call, g.prob0);
                uint64_t bytes = 0, pts = 0, largest = 0;
                for (uint32_t u = g.map0; u < g.map0 + g.n_maps && u < p.maps.size(); ++u) {
                    CHECK(p.maps[u].pt0 == pts, "call %d: map %u lies at %llu, expected %llu", call, u, (unsigned long long)p.maps[u].pt0, (unsigned long long)pts);
                    pts += p.map_cap[u];
                    bytes += map_bytes(p.map_cap[u]);
                    largest = std::max(largest, p.map_cap[u]);
                }
                CHECK(g.pts == pts && g.bytes == bytes, "call %d: a group's size", call);
                CHECK(g.max_cap == largest, "call %d: a group's largest map holds %llu, max_cap says %llu", call, (unsigned long long)largest, (unsigned long long)g.max_cap);
                CHECK(bytes <= cap || g.n_maps == 1, "call %d: a group of %u maps above the cap", call, g.n_maps);
                if (bytes > cap) ++oversize;
                /* greedy: the next map did not fit */
                if (g.map0 + g.n_maps < p.maps.size())
                    CHECK(bytes + map_bytes(p.map_cap[g.map0 + g.n_maps]) > cap, "call %d: a group ends early", call);
                for (uint32_t k = g.prob0; k < g.prob0 + g.n_probs && k < p.probs.size(); ++k) {
                    const Problem &pb = p.probs[k];
                    CHECK(pb.result < (uint32_t)n_matches, "call %d: problem %u has result %u", call, k, pb.result);
                    if (pb.result >= (uint32_t)n_matches) continue;
                    ++seen[pb.result];
                    CHECK(pb.map >= g.map0 && pb.map < g.map0 + g.n_maps && p.map_id[pb.map] == match_map[pb.result], "call %d: match %u in the wrong group", call, pb.result);
                    CHECK(pb.src_slot < p.slots.size() && p.slot_frame[pb.src_slot] == query[pb.result], "call %d: match %u has the wrong source", call, pb.result);
                }
                next_map = g.map0 + g.n_maps;
                next_prob = g.prob0 + g.n_probs;
                max_pts = std::max(max_pts, pts);
                max_maps = std::max(max_maps, g.n_maps);
            }
            CHECK(next_map == p.maps.size() && next_prob == p.probs.size() && p.probs.size() == (size_t)n_matches, "call %d: maps or problems left over", call);
            CHECK(p.max_group_pts == max_pts && p.max_group_maps == max_maps, "call %d: the largest group", call);
            for (int m = 0; m < n_matches; ++m) CHECK(seen[m] == 1, "call %d: match %d is in %d groups", call, m, seen[m]);
            if (cap == 1) CHECK(p.groups.size() == p.maps.size(), "call %d: cap 1 must put every map alone", call);
            if (cap == all + 1) CHECK(p.groups.size() == (p.maps.empty() ? 0u : 1u), "call %d: a cap of everything must give one group", call);
        }
    }
    if (g_bad) {
        std::printf("submapregcheck: %ld failed checks\n", g_bad);
        return 1;
    }
    std::printf("ok: submapregcheck: %ld plans, %ld launch groups, %ld of them single maps above the cap\n", plans, groups, oversize);
    return 0;
}
