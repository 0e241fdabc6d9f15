/*
 * bev_walk_inplace.h — the column walk's in-place source (kSrcInPlace): a sorted prefix read where it lies, through windows and an index row
 * Part of the device code of libbev_mi355x.so; included by bev_walk.h only, behind WalkCol and WalkLds.
 */
#ifndef BEV_WALK_INPLACE_H
#define BEV_WALK_INPLACE_H

namespace bevk {

/* kSrcInPlace: the input's first T points are in strictly ascending slot order (k_probe): they are read IN PLACE,
 * coalesced, once — no order scan, no winner table.  Row rho's points of this strip's 256 virtual columns are consecutive
 * in the input and start near est[rho][strip]; the workgroup DMAs a window of 256 positions (est - 12 ..., one per thread)
 * into LDS, every thread looks at the (row, col) its window position carries and enters the position into an index row at
 * the point's column offset; the points listed for the (row, strip) after the prefix ("tail", at most kTailCap, k_probe)
 * are DMAed beside the window and entered with a key that beats every prefix entry and every EARLIER tail point (LDS
 * atomicMax: the reference's scatter keeps the last writer, BatchMultiBevGen.cpp:112); after the step's barrier each
 * column's owner follows its index entry to its point; an entry whose (row, col) is not the slot's own is an empty slot.
 * Nothing of this is trusted: a position holding a point of the strip's OWN columns counts it and checks that its
 * predecessor in the input lies in the prefix and has a smaller slot; when all T prefix points of a frame have been
 * counted exactly once and no check has failed, the prefix is strictly ascending, every point was where its strip looked,
 * and the result is what getOrderedCloud's scatter gives; otherwise k_verdict sends the frame through the general kernels. */
constexpr int kWinPos = kStripThreads; /* window positions of a (row, strip), one per thread: est - kWinLead ... */
constexpr int kWinLead = 12;
constexpr int kWrapPos = 16;       /* ... the last strip's wrap-around halo: positions around the row's start */
constexpr int kWrapLead = 6;
/* bytes of one ring slot: the window's low halves (4 KiB), its high halves (4 KiB), then, 32 B each, the wrap-around
 * positions and the tail points */
constexpr int kInPlaceSlot = (kWinPos + kWrapPos + kTailCap) * 32;
constexpr uint32_t kIdxTail = 1u << 30;
static_assert(kWinPos == 256 && kStripVirt + 16 <= kWinPos && kTailCap == 64 && kWrapPos == 16, "DMA pieces of the in-place source");

template <>
struct WalkSource<kSrcInPlace> {
    static constexpr int kSrc = kSrcInPlace;
    static constexpr bool kIndexed = true, kChecked = true;
    static constexpr bool kStrip0Last = false, kAnyMode = false;
    /* the ring holds the points of rows r, r+1, r+2 by window position */
    static constexpr int kSlotBytes = kInPlaceSlot, kRingBytes = 3 * kSlotBytes;
    struct Lds {
        uint32_t idx[2][kStripThreads + 1]; /* column offset -> position + 1 | tail key ([256]: nowhere) */
        uint32_t tlist[3][64];              /* tail lists of rows r+2, r+3, r+4 */
        int est_l[2][kStreamMaxRows];
        uint8_t tcnt_l[kStreamMaxRows];
    };
    static __device__ __forceinline__ const bev_point_t *input(const BatchPtrs &b, const Geometry &, int f) { return b.pts + b.frames[f].in_offset; }

    WalkLds<kSrc> &lds;
    const WalkCol &c;
    const uint32_t *const fest, *const ftcnt; /* this frame's estimates and tail counts, [strip][row] */
    const uint32_t *const ftail;
    const int tail_stride;      /* words from one row's list to the next */
    const uint32_t tlist_l;
    uint32_t te[3] = {0u, 0u, 0u}; /* wave 3: this lane's tail entry of rows q at [q % 3] (column offset | input index << 8) */
    uint32_t consumed = 0u, failed = 0u;
    /* the check that index_row leaves for after the barrier */
    bool dneed = false;
    int dflat = 0, dq = 0;

    __device__ __forceinline__ WalkSource(WalkLds<kSrc> &lds_, const WalkCol &c_, const BatchPtrs &b, const Geometry &, int f)
        : lds(lds_), c(c_), fest(b.est + (size_t)f * c_.N * c_.strips), ftcnt(b.tail_cnt + (size_t)f * c_.N * c_.strips),
          ftail(b.tail_list + ((size_t)f * c_.N * c_.strips + c_.strip) * kTailCap), tail_stride(c_.strips * kTailCap),
          tlist_l(__builtin_amdgcn_readfirstlane(lds_addr(&lds_.src.tlist[0][0])))
    {
    }

    __device__ __forceinline__ int clamp_row(int q) const { return q < c.N ? q : c.N - 1; }
    __device__ __forceinline__ const char *pos_addr(int q) const /* the point at input position q, or position 0 outside the prefix */
    {
        return c.fbytes + (size_t)((unsigned)q < c.T ? q : 0) * 32u;
    }
    __device__ __forceinline__ void issue_window(int q, int slot) /* this wave's 64 positions of row q's window: low halves, high halves */
    {
        const int e = lds.src.est_l[0][clamp_row(q)] - kWinLead;
        const uint32_t at = c.ring_l + (uint32_t)slot * kSlotBytes + (uint32_t)c.wv * 1024u;
        /* (rows past the last one — the two steps that drain the pipeline and the two before them — still issue their
         * loads, so that every step counts the same: all lanes fetch position 0, one line instead of the last row's window again) */
        const char *src = q >= c.N ? c.fbytes
                                   : ((e >= 0 && e + kWinPos <= (int)c.T) ? c.fbytes + (size_t)(uint32_t)(e + c.tid) * 32u /* wave-uniform test */
                                                                          : pos_addr(e + c.tid));
        glds16x2(src, at, src + 16, at + 4096u);
    }
    __device__ __forceinline__ void issue_wrap(int q, int slot) /* last strip, wave 2: the positions around the row's start, 32 B each */
    {
        if (c.lane < 2 * kWrapPos)
            glds16(pos_addr(lds.src.est_l[1][clamp_row(q)] - kWrapLead + (c.lane >> 1)) + 16 * (c.lane & 1), c.ring_l + (uint32_t)slot * kSlotBytes + 8192u);
    }
    __device__ __forceinline__ void issue_tail_list(int q, int slot) /* wave 3: the (row, strip)'s list; lanes past its count fetch word 0 again (only the lines that hold entries move) */
    {
        const int qc = clamp_row(q);
        glds4_nt(ftail + (size_t)qc * tail_stride + (c.lane < (int)lds.src.tcnt_l[qc] ? c.lane : 0), tlist_l + (uint32_t)slot * 256u);
    }
    __device__ __forceinline__ void issue_tail_points(int q, int slot, int tslot) /* wave 3: the listed points of row q beside its window, 32 B each */
    {
        auto &tlist = lds.src.tlist;
        const int lane = c.lane;
        const int n = q < c.N ? (int)lds.src.tcnt_l[clamp_row(q)] : 0;
        te[tslot] = tlist[tslot][lane];
        const uint32_t ea = tlist[tslot][lane >> 1], eb = tlist[tslot][32 + (lane >> 1)];
        const uint32_t at = c.ring_l + (uint32_t)slot * kSlotBytes + 8192u + (uint32_t)kWrapPos * 32u;
        glds16x2(c.fbytes + (size_t)((lane >> 1) < n ? (ea >> 8) : 0u) * 32u + 16 * (lane & 1), at,
                 c.fbytes + (size_t)(32 + (lane >> 1) < n ? (eb >> 8) : 0u) * 32u + 16 * (lane & 1), at + 1024u);
    }
    __device__ __forceinline__ int slot_or_max(int q, uint32_t rcw) const /* slot of input position q, INT_MAX outside the prefix / the range image */
    {
        const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
        const bool valid = ((unsigned)q < c.T) & (row < (uint32_t)c.N) & (col < (uint32_t)c.H);
        return valid ? (int)(row * (uint32_t)c.H + col) : 0x7fffffff;
    }
    /* Row rho's positions -> idx[rho & 1].  Every thread enters ITS window position, counts and checks it: the predecessor
     * in the input must lie in the prefix and have a smaller slot (the lane to the left has it; window position 0 cannot
     * be checked: the estimate was too high).  The first lane of a wave follows a position that ANOTHER wave's DMA brings:
     * that check is made after the step's barrier.  Written without branches: an entry that belongs nowhere goes to the
     * spare word idx[.][256]. */
    __device__ __forceinline__ void index_row(int rho, int slot, int tslot)
    {
        const int tid = c.tid, lane = c.lane, H = c.H, first_col = c.first_col, row_span = c.row_span;
        const uint32_t T = c.T;
        if (rho >= c.N) return;
        const char *slot_b = &lds.ring[slot * kSlotBytes];
        uint32_t *irow = lds.src.idx[rho & 1];
        const uint32_t base = (uint32_t)(rho * H + first_col);
        {
            const int q = lds.src.est_l[0][rho] - kWinLead + tid;
            const u32x4 hi = *reinterpret_cast<const u32x4 *>(slot_b + 4096 + tid * 16); /* (conflict-free; only .y is used) */
            const int sflat = slot_or_max(q, hi.y);
            const uint32_t off = (uint32_t)sflat - base;
            /* (a window of the last strip runs into the next row: those points are not this row's wrap-around halo) */
            atomicMax(&irow[off < (uint32_t)row_span ? off : (uint32_t)kStripThreads], (uint32_t)tid + 1u);
            const bool own = (off - 2u) < (uint32_t)c.own_cols;
            consumed += own ? 1u : 0u;
            const int pflat = __builtin_amdgcn_update_dpp(0x7fffffff, sflat, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
            const bool chk = own & (q > 0);
            failed |= (chk & ((tid == 0) | ((lane != 0) & !(pflat < sflat)))) ? 1u : 0u;
            /* ... and the window must BRACKET the (row, strip)'s span of slots, halo columns included: the own columns are
             * proven found by the count, the two halo columns on either side are not — a halo point the window misses
             * would read as an empty slot and change phase A's fallbacks (BatchMultiBevGen.cpp:146-154) with nobody
             * noticing.  The prefix is strictly ascending (that is what the checks above prove), so it is enough that the
             * first position's slot is not past the span's first slot (or the window starts at the input's start) and the
             * last position's slot is the span's last or beyond (or the window reaches the prefix's end). */
            const int ibase = rho * H + first_col;
            failed |= (((tid == 0) & (q > 0) & (sflat > ibase)) |
                       ((tid == kWinPos - 1) & (q < (int)T - 1) & (sflat < ibase + row_span - 1))) ? 1u : 0u;
            dneed = chk & (lane == 0) & (tid != 0);
            dflat = sflat;
            dq = q;
        }
        if (c.last_strip && c.wv == 2) { /* wave-uniform: slots rho*H and rho*H + 1 as the halo columns H, H + 1 */
            const int k = lane & (kWrapPos - 1);
            const int q = lds.src.est_l[1][rho] - kWrapLead + k;
            const uint32_t rcw = *reinterpret_cast<const uint32_t *>(slot_b + 8192 + k * 32 + 20);
            const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
            const uint32_t off = (uint32_t)(H - first_col) + col;
            const bool ok = (lane < kWrapPos) & ((unsigned)q < T) & (row == (uint32_t)rho) & (col < 2u) & (off < (uint32_t)kStripVirt);
            atomicMax(&irow[ok ? off : (uint32_t)kStripThreads], (uint32_t)(kWinPos + k) + 1u);
            /* the same bracket for the 16 positions around the row's start: slots rho * H and rho * H + 1 lie inside */
            const int wflat = slot_or_max(q, rcw);
            failed |= (((lane == 0) & (q > 0) & (wflat > rho * H)) |
                       ((lane == kWrapPos - 1) & (q < (int)T - 1) & (wflat < rho * H + 1))) ? 1u : 0u;
        }
        if (c.wv == 3) { /* later input index beats earlier, any tail point beats the prefix */
            const uint32_t e = te[tslot];
            atomicMax(&irow[lane < (int)lds.src.tcnt_l[rho] ? (e & 0xffu) : (uint32_t)kStripThreads], kIdxTail | ((e >> 8) << 6) | (uint32_t)lane);
        }
    }
    __device__ __forceinline__ void deferred_check(const char *slot_b) /* after the barrier: every wave's pieces of the row have arrived */
    {
        const uint32_t rcp = *reinterpret_cast<const uint32_t *>(slot_b + 4096 + (c.tid > 0 ? c.tid - 1 : 0) * 16 + 4);
        failed |= (dneed && !(slot_or_max(dq - 1, rcp) < dflat)) ? 1u : 0u;
    }

    __device__ __forceinline__ void setup()
    {
        lds.src.idx[0][c.tid] = 0u;
        lds.src.idx[1][c.tid] = 0u;
        if (c.tid == 0) lds.zero16[0] = u32x4{0u, 0u, 0u, 0u};
        for (int r = c.tid; r < c.N; r += kStripThreads) {
            lds.src.est_l[0][r] = (int)fest[c.strip * c.N + r];
            lds.src.est_l[1][r] = (int)fest[r];
            lds.src.tcnt_l[r] = (uint8_t)ftcnt[c.strip * c.N + r];
        }
    }
    /* the queue the row loop expects: the windows and tail points of rows 0, 1, the tail lists of rows 2, 3 */
    __device__ __forceinline__ void prologue()
    {
        if (c.wv == 3) {
            issue_tail_list(0, 0);
            issue_tail_list(1, 1);
        }
        wait_vm<0>();
        issue_window(0, 0);
        if (c.last_strip && c.wv == 2) issue_wrap(0, 0);
        if (c.wv == 3) {
            issue_tail_points(0, 0, 0);
            issue_tail_list(2, 2);
        }
        issue_window(1, 1);
        if (c.last_strip && c.wv == 2) issue_wrap(1, 1);
        if (c.wv == 3) {
            issue_tail_points(1, 1, 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* list 0 has been read before its slot is refilled */
            issue_tail_list(3, 0);
        }
    }
    /* row r's window (and tail points) into its index row */
    template <int I>
    __device__ __forceinline__ void arrive(const int r, u32x4 &, u32x4 & WALK_PHA_PARAMS)
    {
        constexpr int s0 = RingSlots<I>::s0;
        if (c.wv == 3) wait_vm<5>();                        /* 2 window pieces, 1 list, 2 tail pieces */
        else if (c.last_strip && c.wv == 2) wait_vm<3>();   /* 2 window pieces, the wrap-around positions */
        else wait_vm<2>();
        PHA(0);
        index_row(r, s0, s0);
        PHA(1);
    }
    /* the column's owner follows its index entry: a window / wrap-around position, or a tail point; an entry
     * whose (row, col) is not the slot's own is an empty slot (value-initialised, BatchMultiBevGen.cpp:98) */
    template <int I>
    __device__ __forceinline__ void take(const int r, u32x4 &cur_lo, u32x4 &cur_hi)
    {
        constexpr int s0 = RingSlots<I>::s0;
        const int par = r & 1;
        if (c.lane == 0) deferred_check(&lds.ring[s0 * kSlotBytes]);
        const uint32_t e = lds.src.idx[par][c.tid];
        lds.src.idx[par][c.tid] = 0u; /* (the row after next enters here, two barriers from now) */
        const uint32_t pos = (e & kIdxTail) ? (uint32_t)(kWinPos + kWrapPos) + (e & 63u) : e - 1u;
        const bool inwin = pos < (uint32_t)kWinPos;
        const uint32_t lo_at = inwin ? pos * 16u : 8192u + (pos - (uint32_t)kWinPos) * 32u;
        const char *slot_b = &lds.ring[s0 * kSlotBytes];
        const bool have = (e != 0u) & (r < c.N);
        /* (an entry leads to a point whose (row, col) ARE this slot's: the offset it was entered at was computed from
         * them; in a frame where that fails — two prefix points of one slot — the order check fails as well) */
        cur_lo = *(have ? reinterpret_cast<const u32x4 *>(slot_b + lo_at) : &lds.zero16[0]);
        cur_hi = *(have ? reinterpret_cast<const u32x4 *>(slot_b + lo_at + (inwin ? 4096u : 16u)) : &lds.zero16[0]);
    }
    /* row r + 2's window, wrap-around positions and tail points, row r + 4's tail list */
    template <int I>
    __device__ __forceinline__ void issue(const int r)
    {
        constexpr int s2 = RingSlots<I>::s2, s1 = RingSlots<I>::s1;
        issue_window(r + 2, s2);
        if (c.last_strip && c.wv == 2) issue_wrap(r + 2, s2);
        if (c.wv == 3) {
            issue_tail_points(r + 2, s2, s2);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue_tail_list(r + 4, s1);
        }
    }
    /* this wave's two 1-KiB pieces of the slot row r-1 has left */
    template <int I>
    __device__ __forceinline__ int xpose() const { return RingSlots<I>::s2 * kSlotBytes; }
    __device__ __forceinline__ void upper_missing(int, float) {}
    __device__ __forceinline__ void finish() {}
#ifdef BEV_CS_CLOCK
    __device__ __forceinline__ void clk_print(int bid, int WALK_PHA_PARAMS)
    {
        PHA_PRINT("walk_inplace vmwait index barrier acquire writeout issue status rest", c.lane == 0 && bid == 100);
    }
#endif
};

} /* namespace bevk */

#endif /* BEV_WALK_INPLACE_H */
