/*
 * pairgridcheck — the byte model and the build groups of the pair calls' search grids sized to the cloud
 * (csrc/bev_pair_grid_plan.h), without a device.  Over seeded target counts, capacities and caps it prints one
 * line per layout for tests/test_pair_search_grid_cpu.py to compare with a Python restatement:
 *   targets capacity D cells off_words group off_bytes cnt_bytes bounds_bytes sums_bytes hdr_bytes map_bytes cell0_bytes parts
 *   tiles groups last_group_targets last_cell0
 * and checks on its own what the device relies on: the groups cover the targets once and in order, none is larger than the
 * group, every target's counters lie inside the group's, every target's offsets inside the table, the launch grids cover the
 * capacity and the cells and stay inside the partial results.  The last line: "ok: pairgridcheck: N layouts, G build groups".
 * Any violation: a line "PLAN ..." and exit status 1.
 */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../point-cloud-preprocessing-tools_amd/csrc/bev_pair_grid_plan.h"

namespace {

uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next()
{ /* splitmix64 */
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int fail(const char *what, uint64_t targets, uint64_t capacity, int D)
{
    std::printf("PLAN %s: targets %" PRIu64 " capacity %" PRIu64 " D %d\n", what, targets, capacity, D);
    return 1;
}

} // namespace

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 4000;
    const int caps[] = {0, 1, 2, 63, 64, 65, 128, 130, 256, 1000, 1024};
    const uint64_t sizes[] = {1, 2, 255, 256, 257, 511, 512, 513, 1000};
    uint64_t groups_total = 0;
    for (int i = 0; i < n; ++i) {
        const int D = caps[next() % (sizeof caps / sizeof *caps)];
        const uint64_t targets = i % 7 == 0 ? sizes[next() % (sizeof sizes / sizeof *sizes)] : i % 11 == 0 ? 0 : 1 + next() % 1200;
        const uint64_t capacity = i % 5 == 0 ? 1 + next() % 40 : i % 13 == 0 ? (1u << 20) + next() % (1u << 22) : 1 + next() % 200000;
        const bevpair::Layout l = bevpair::layout(targets, capacity, D);
        const std::vector<bevpair::Group> gs = bevpair::groups(targets, l);
        if (D == 0 || targets == 0) {
            if (l.cells || l.off_words || l.group || l.off_bytes || l.cnt_bytes || l.bounds_bytes || l.sums_bytes || l.hdr_bytes ||
                l.map_bytes || l.cell0_bytes || !gs.empty())
                return fail("something at D == 0", targets, capacity, D);
        } else {
            uint64_t at = 0;
            for (const bevpair::Group &g : gs) {
                if (g.t0 != at || g.n == 0 || g.n > l.group) return fail("groups", targets, capacity, D);
                at += g.n;
            }
            if (at != targets || l.group > bevpair::kBuildGroup) return fail("cover", targets, capacity, D);
            for (uint64_t t = 0; t < targets; ++t) {
                if ((bevpair::cell0(t, l) + l.off_words) * 4 > l.cnt_bytes) return fail("counters", targets, capacity, D);
                if ((t + 1) * l.off_words * 4 > l.off_bytes) return fail("offsets", targets, capacity, D);
            }
            const uint64_t dim = (uint64_t)bevsubreg::grid_dim((uint32_t)capacity, D);
            if (l.cells != dim * dim || l.off_words != l.cells + 1) return fail("cells", targets, capacity, D);
            if (l.parts < 1 || l.parts > bevsubreg::kGridParts || l.tiles < 1 || l.tiles > bevsubreg::kGridScanParts ||
                (uint64_t)l.tiles * bevsubreg::kGridScanTile < l.cells)
                return fail("launch grids", targets, capacity, D);
            if ((uint64_t)l.parts * bevpair::kPartPoints < capacity && l.parts != bevsubreg::kGridParts)
                return fail("parts", targets, capacity, D);
            if (l.bounds_bytes + l.sums_bytes != (uint64_t)l.group * bevsubreg::kGridPartBytes) return fail("5 KiB", targets, capacity, D);
        }
        groups_total += gs.size();
        std::printf("%" PRIu64 " %" PRIu64 " %d %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                    " %" PRIu64 " %" PRIu64 " %u %u %zu %u %" PRIu64 "\n",
                    targets, capacity, D, l.cells, l.off_words, l.group, l.off_bytes, l.cnt_bytes, l.bounds_bytes, l.sums_bytes,
                    l.hdr_bytes, l.map_bytes, l.cell0_bytes, l.parts, l.tiles, gs.size(), gs.empty() ? 0u : gs.back().n,
                    targets && D ? bevpair::cell0(targets - 1, l) : (uint64_t)0);
    }
    std::printf("ok: pairgridcheck: %d layouts, %" PRIu64 " build groups\n", n, groups_total);
    return 0;
}
