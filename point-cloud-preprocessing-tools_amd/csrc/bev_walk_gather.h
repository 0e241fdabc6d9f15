/*
 * bev_walk_gather.h — the column walk's sources that read one point per slot: through the winner table (kSrcGather), an ordered cloud (kSrcIdentity), the caller's structured input (kSrcStructured)
 * Part of the device code of libbev_mi355x.so; included by bev_walk.h only, behind WalkCol and WalkLds.
 */
#ifndef BEV_WALK_GATHER_H
#define BEV_WALK_GATHER_H

namespace bevk {

/* raw winner words of rows r+2, r+3, r+4 (kSrcGather alone) */
template <bool kWinners>
struct WinnerRing {
    uint32_t wring[3][kStripThreads];
};
template <>
struct WinnerRing<false> {};

/* Winner words two steps before the points, points two steps before the row.  The ring holds the points of rows r, r+1,
 * r+2 by thread: low halves in a slot's first 4 KiB, high halves in the second.
 * kStructured: the identity source over the caller's INPUT (record i = slot i's point or an all-zero record), every
 * record checked; kIdentity covers both (no winner table, position = slot). */
template <int kSrc>
struct GatherSource {
    static constexpr bool kWinners = kSrc == kSrcGather, kStructured = kSrc == kSrcStructured, kIdentity = kSrc == kSrcIdentity || kStructured;
    static constexpr bool kIndexed = false, kChecked = kStructured;
    static constexpr bool kStrip0Last = false;
    static constexpr bool kAnyMode = kSrc == kSrcIdentity; /* handed an ordered cloud: no frame mode to match */
    static constexpr int kSlotBytes = 8192, kRingBytes = 3 * kSlotBytes;
    using Lds = WinnerRing<kWinners>;
    static __device__ __forceinline__ const bev_point_t *input(const BatchPtrs &b, const Geometry &g, int f)
    {
        return kSrc == kSrcIdentity ? (b.pts + (size_t)f * g.S) : (b.pts + b.frames[f].in_offset);
    }

    WalkLds<kSrc> &lds;
    const WalkCol &c;
    const uint32_t *const fwin;
    const uint32_t win_tag;
    const int win_shift;
    /* an empty slot loads a dummy (the first point of this frame's OUTPUT: always allocated, one cached line) and is
     * zeroed when the row is consumed: every step issues the same loads */
    const Half *const dummy;
    uint32_t wring_l = 0u;
    /* structured: the (row | col << 16) word the record of this thread's slot in row r must carry is (r - st_rowadj) | st_col
     * (the flat rule puts virtual columns < 0 into the previous row's tail); whether k_probe expects an all-zero record
     * after the first — slot 0 is all-zero then, whatever record 0 holds (BatchMultiBevGen.cpp:112-115, last writer) */
    const uint32_t st_rowadj, st_col;
    const bool st_zero_guess;
    uint32_t full = 0u; /* bit (row mod 3): the row's slot holds a point */
    uint32_t wraw = 0u; /* the raw winner word of row r + 2, read in arrive, used in issue */
    uint32_t consumed = 0u, failed = 0u;

    __device__ __forceinline__ GatherSource(WalkLds<kSrc> &lds_, const WalkCol &c_, const BatchPtrs &b, const Geometry &g, int f)
        : lds(lds_), c(c_), fwin(b.winner + (size_t)f * g.S), win_tag(b.win_tag), win_shift(b.win_shift),
          dummy(reinterpret_cast<const Half *>(b.ordered + (size_t)f * g.S)), st_rowadj(c_.v < 0 ? 1u : 0u),
          st_col((uint32_t)(c_.v < 0 ? c_.H + c_.v : c_.vcol) << 16), st_zero_guess(kStructured && (b.info[f].failed & kInfoZeroGuess) != 0u)
    {
        if constexpr (kWinners) wring_l = __builtin_amdgcn_readfirstlane(lds_addr(&lds.src.wring[0][0])) + (uint32_t)c.wv * 256u;
    }

    __device__ __forceinline__ bool has_slot(int r) const { return c.provider && r < c.N && r * c.H + c.vcol >= 0; }
    __device__ __forceinline__ void issue_winner(int q, int slot)
    {
        if constexpr (kWinners) {
            const int fl = has_slot(q) ? q * c.H + c.vcol : 0;
            glds4_nt(&fwin[fl], wring_l + (uint32_t)slot * 1024u);
        }
    }
    __device__ __forceinline__ void issue_points(uint32_t w, int slot) /* w: input index + 1, 0 = empty slot */
    {
        const Half *src = w != 0u ? reinterpret_cast<const Half *>(c.fbytes) + 2 * (size_t)(w - 1u) : dummy;
        const uint32_t at = c.ring_l + (uint32_t)slot * kSlotBytes + (uint32_t)c.wv * 1024u;
        glds16x2(src, at, src + 1, at + 4096u);
    }
    __device__ __forceinline__ uint32_t winner_of(int q, uint32_t raw) const /* input index + 1 of slot (q, this column), 0 = empty */
    {
        if (!has_slot(q)) return 0u;
        if (kIdentity) return (uint32_t)(q * c.H + c.vcol) + 1u;
        return winner_index(raw, win_tag, win_shift);
    }

    __device__ __forceinline__ void setup() {}
    /* the queue the row loop expects: the points of rows 0, 1, the winner words of rows 2, 3 */
    __device__ __forceinline__ void prologue()
    {
        issue_winner(0, 0);
        issue_winner(1, 1);
        wait_vm<0>();
        uint32_t r0 = 0u, r1 = 0u;
        if constexpr (kWinners) {
            r0 = lds.src.wring[0][c.tid];
            r1 = lds.src.wring[1][c.tid];
        }
        const uint32_t w0 = winner_of(0, r0), w1 = winner_of(1, r1);
        full = (w0 != 0u ? 1u : 0u) | (w1 != 0u ? 2u : 0u);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* the words have been read before their ring slots are refilled */
        issue_points(w0, 0);
        issue_winner(2, 2);
        issue_points(w1, 1);
        issue_winner(3, 0);
    }
    /* the thread's own piece of row r's slot (and the winner word of row r + 2) */
    template <int I>
    __device__ __forceinline__ void arrive(const int r, u32x4 &cur_lo, u32x4 &cur_hi WALK_PHA_PARAMS)
    {
        constexpr int s0 = RingSlots<I>::s0, s2 = RingSlots<I>::s2;
        wait_vm<kIdentity ? 2 : 3>();
        PHA(0);
        const char *mine = &lds.ring[s0 * kSlotBytes + c.tid * 16];
        cur_lo = *reinterpret_cast<const u32x4 *>(mine);
        cur_hi = *reinterpret_cast<const u32x4 *>(mine + 4096);
        if constexpr (kWinners) wraw = lds.src.wring[s2][c.tid];
        if (!((full >> s0) & 1u)) { /* untouched slot: value-initialised, BatchMultiBevGen.cpp:98 */
            cur_lo = u32x4{0u, 0u, 0u, 0u};
            cur_hi = u32x4{0u, 0u, 0u, 0u};
        }
        if constexpr (kStructured) {
            /* the record at flat position r * H + vcol: its slot's point (then the scatter leaves it where it is) or
             * all-zero (then it lands in slot 0 and its own slot stays value-initialised: all-zero as well); anything
             * else fails the frame.  Every record is seen by the owner of its column (counted) and by halo threads. */
            const bool rec = (full >> s0) & 1u;
            const uint32_t any = cur_lo.x | cur_lo.y | cur_lo.z | cur_lo.w | cur_hi.x | cur_hi.y | cur_hi.z | cur_hi.w;
            const bool real = cur_hi.y == (((uint32_t)r - st_rowadj) | st_col);
            const bool first = (r == 0) & (c.vcol == 0); /* flat position 0 */
            failed |= (rec & !real & (any != 0u)) ? kInfoFailed : 0u;
            failed |= (rec & (any == 0u) & !first) ? kInfoZeroSeen : 0u;
            consumed += (rec & c.outcol) ? 1u : 0u;
            if (first & st_zero_guess) {
                cur_lo = u32x4{0u, 0u, 0u, 0u};
                cur_hi = u32x4{0u, 0u, 0u, 0u};
            }
        }
    }
    template <int I>
    __device__ __forceinline__ void take(int, u32x4 &, u32x4 &) {}
    /* row r + 2's points, row r + 4's winner word */
    template <int I>
    __device__ __forceinline__ void issue(const int r)
    {
        constexpr int s2 = RingSlots<I>::s2, s1 = RingSlots<I>::s1;
        const uint32_t wn = winner_of(r + 2, wraw);
        full = (full & ~(1u << s2)) | (wn != 0u ? 1u << s2 : 0u);
        issue_points(wn, s2);
        issue_winner(r + 4, s1);
    }
    /* the slot of the row just consumed (this wave's two 1-KiB pieces, points 0..31 in the first) */
    template <int I>
    __device__ __forceinline__ int xpose() const { return RingSlots<I>::s0 * kSlotBytes; }
    __device__ __forceinline__ void upper_missing(int, float) {}
    __device__ __forceinline__ void finish() {}
#ifdef BEV_CS_CLOCK
    __device__ __forceinline__ void clk_print(int bid, int WALK_PHA_PARAMS)
    {
        PHA_PRINT("walk_gather vmwait - barrier acquire writeout issue status rest", c.lane == 0 && bid == 100);
    }
#endif
};
template <>
struct WalkSource<kSrcGather> : GatherSource<kSrcGather> {
    using GatherSource::GatherSource;
};
template <>
struct WalkSource<kSrcIdentity> : GatherSource<kSrcIdentity> {
    using GatherSource::GatherSource;
};
template <>
struct WalkSource<kSrcStructured> : GatherSource<kSrcStructured> {
    using GatherSource::GatherSource;
};

} /* namespace bevk */

#endif /* BEV_WALK_GATHER_H */
