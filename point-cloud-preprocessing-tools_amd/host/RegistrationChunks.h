/*
 * RegistrationChunks.h — how the four batch registration tools cut a match list into chunks.  Host only, header
 * only, no HIP and no context: tests/hostcheck compiles it alone.
 *
 * A chunk is a run of consecutive matches whose files fit the device at once.  Match (q, m) names its query q and the window
 * [m - half, m + half] clipped to [lo, hi]; the frame tools have half 0 and no clip, so the window is m alone.  Starting at m0
 * with no files, a match adds q if the chunk does not hold it yet, then every window file that the chunk does not hold and that
 * is not q, ascending, and joins the chunk only if the files stay within `limit`; the first match that does not ends the chunk.
 * Files are numbered in the order they were added: that number is the frame index the device calls see.
 *
 * A first match that does not fit on its own would yield an empty chunk (m1 == m0) and a caller that never advances.  The tools
 * rule that out before they plan: the frame tools refuse a limit below 2 and a match names at most 2 files; the submap tools
 * raise the limit to 2 * half + 2, the most a match names.
 */
#ifndef BEV_HOST_REGISTRATIONCHUNKS_H
#define BEV_HOST_REGISTRATIONCHUNKS_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <vector>

#include "../../include/bev_mi355x.h"

namespace regchain {

constexpr long kNoClipLo = std::numeric_limits<long>::min() / 2, kNoClipHi = std::numeric_limits<long>::max() / 2;

struct Chunk {
    size_t m1 = 0;                    /* the chunk is matches [m0, m1) */
    std::vector<long> files;          /* frame f of the chunk is file files[f] */
    std::vector<bev_match_t> matches; /* query_idx: the query's frame; match_idx: the target's frame, or with maps the map k */
    /* with maps only: match k's map is entries [map_offs[k], map_offs[k + 1]), entry e the frame entry_frame[e].  One map per
     * match: two matches of one key frame get two equal maps */
    std::vector<uint64_t> map_offs;
    std::vector<int32_t> entry_frame;
};

/* Match: anything with query_idx, match_idx and angle_guess (MatchResult, bev_match_t) */
template <class Match>
Chunk planChunk(const Match *matches, size_t n_matches, size_t m0, long half, long lo, long hi, long limit, bool maps)
{
    Chunk c;
    std::map<long, int> local;
    const auto window = [&](long m) { return std::make_pair(std::max(lo, m - half), std::min(hi, m + half)); };
    for (c.m1 = m0; c.m1 < n_matches; ++c.m1) {
        const long q = matches[c.m1].query_idx;
        const auto w = window(matches[c.m1].match_idx);
        std::vector<long> add;
        if (!local.count(q)) add.push_back(q);
        for (long j = w.first; j <= w.second; ++j)
            if (!local.count(j) && j != q) add.push_back(j);
        if ((long)(local.size() + add.size()) > limit) break;
        for (long f : add) {
            local.emplace(f, (int)c.files.size());
            c.files.push_back(f);
        }
    }
    if (maps) c.map_offs.push_back(0);
    for (size_t k = m0; k < c.m1; ++k) {
        const long m = matches[k].match_idx;
        c.matches.push_back(bev_match_t{local[matches[k].query_idx], maps ? (int32_t)(k - m0) : local[m], matches[k].angle_guess});
        if (!maps) continue;
        const auto w = window(m);
        for (long j = w.first; j <= w.second; ++j) c.entry_frame.push_back(local[j]);
        c.map_offs.push_back(c.entry_frame.size());
    }
    return c;
}

} // namespace regchain

#endif
