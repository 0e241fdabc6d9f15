/*
 * bev_walk.h — the column walk: getOrderedCloud's gather + markGroundPoints phase A + BEV codes, six sources of the points
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_WALK_H
#define BEV_WALK_H

#include "bev_dev.h"

#ifndef BEV_SEENB
#define BEV_SEENB 8
#endif

namespace bevk {
using namespace bevx;

/* ------------------------------------------------------------------------- */
/* getOrderedCloud gather + markGroundPoints phase A, as a COLUMN WALK.
 *
 * A workgroup owns kStripCols (236) adjacent columns of one frame plus two halo columns on each side (240 virtual columns,
 * 256 threads) and walks the rows 0 .. N-1.  Thread tid sits on virtual column v = strip*236 + tid - 2 and, in row r, on flat slot
 * index r*H + v (v >= H wraps to v - H in the SAME row, v < 0 is the flat index r*H + v, i.e. the tail of row r-1 —
 * exactly the two index rules of BatchMultiBevGen.cpp:146-154).  Consequences:
 *   - every input point is loaded exactly once, rows arrive as 8 KiB coalesced pieces, two rows ahead;
 *   - the phase-A stencil needs no second pass: "upper" is the thread's own previous row (registers), its +-2
 *     fallbacks are the neighbours' previous rows (wave shuffles, LDS only across wave edges), row-2 is the thread's
 *     own row before that;
 *   - status s[r] is evaluated ONCE per slot; ground_mat(r-1) follows from s[r-1] and s[r] (closed form in
 *     bev_exact.h), so row r-1 is finished while row r is being evaluated, and row r-2 is written out.
 * Candidates of one (row, strip) are compacted in column order into their own segment; segments enumerate (row, strip)
 * in row-major order, so the concatenation of all segments is slot order — what phase B's accumulation order needs.
 *
 * Round 3 rebuilt the kernel around three measurements:
 *   1. hipcc drained the memory queue (s_waitcnt vmcnt(0)) at the top of EVERY row step: gfx9-family loads and stores
 *      retire out of order with respect to each other, so with stores pending the compiler cannot count, and the "two
 *      rows in flight" were one row in flight plus a full round trip per step.  Every global READ of the row loop is
 *      now an LDS-DMA load (global_load_lds: per-lane source address, the data lands in LDS, no VGPR destination the
 *      compiler could copy or spill while the load is in flight), issued two steps ahead and waited for with a COUNTED
 *      s_waitcnt: "a load has completed once at most as many operations are outstanding as loads were issued after it"
 *      holds whatever the stores in between do; the stores of a step are issued BEFORE its loads, so that the wait at
 *      the top of a step covers stores that are a whole step old and loads that are two.
 *   2. a fifth of the walk's vector instructions were v_readlane restores of spilled scalar registers: the raster
 *      constants came back as an 8-dword tuple for every multiplication, and pointers laundered through asm turned
 *      every store into a FLAT store (which also counts on lgkmcnt, the LDS counter).  The raster constants live in
 *      vector registers (they only feed VALU), the power-of-two / divide choice is a template parameter, stores go
 *      through address-space-1 pointers (global_store, scalar base + 32-bit lane offset).
 *   3. waves without a column (the last strip of a row holds 67 of 256 threads for HDL_64E, 16 for OS1_64) end before
 *      the row loop: an ended wave drops out of s_barrier.
 *
 * Where the points come from is a template parameter, a type WalkSource<kSrc> (the kSrc* names: bev_internal.h):
 *   bev_walk_gather.h   kSrcGather through the winner table of the order scan (any input); kSrcIdentity: b.pts already is an
 *                       ordered cloud (bev_mark_ground); kSrcStructured: the same over a structured input, every record checked;
 *   bev_walk_inplace.h  kSrcInPlace: a sorted prefix read where it lies, through windows and an index row;
 *   bev_walk_firing.h   kSrcColMajor, kSrcColMajorGen: firing order, read as bands of two rows, through an index row.
 * walk_body below is the part they share — the write-out of row r-2, the status of row r, the ground flag of row r-1, the BEV
 * code — and calls a source at fixed places of the step (see WalkSource). */
/* row record of the walk: flags = (status + 1) | (ground_mat + 1) << 2 | pred << 4 */
struct WalkRow {
    u32x4 lo, hi;
    uint32_t code, key, fl;
};
__device__ __forceinline__ int wr_status(uint32_t fl) { return (int)(fl & 3u) - 1; }
__device__ __forceinline__ int wr_gflag(uint32_t fl) { return (int)((fl >> 2) & 3u) - 1; }

/* A wave's candidates per cell quarter.  Every candidate lane holds a one in the byte of its quarter; an inclusive scan
 * over the wave's lanes (six DPP additions: four inside the rows of 16 lanes, two across rows) leaves in lane 63 the
 * wave's four counts (at most 64 each) and in every lane, in the byte of its quarter, its rank among the wave's candidates
 * of that quarter plus one.  No ballots, no 64-bit lane masks.  Returns the scan; *rank = this lane's rank. */
__device__ __forceinline__ uint32_t quarter_scan(bool c, uint32_t q, uint32_t *rank)
{
    const uint32_t sh = q << 3;
    const uint32_t one = c ? 1u << sh : 0u;
    uint32_t x = one;
    /* (a lane whose source lies outside its row / outside the row mask keeps the 0 given as the old value) */
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
    *rank = __builtin_amdgcn_ubfe(x - one, sh, 8u);
    return x;
}
constexpr int kFlRankShift = 8; /* WalkRow::fl bits 8..13: the lane's rank among its wave's candidates of its quarter */

/* ring slots of step I mod 3 */
template <int I>
struct RingSlots {
    static constexpr int s0 = I % 3;       /* ring slot of row r (and of row r + 3) */
    static constexpr int s2 = (I + 2) % 3; /* ... of row r + 2: the slot row r - 1 has left */
    static constexpr int s1 = (I + 1) % 3; /* winner / list ring: row r + 4 goes where row r + 1's was */
};

/* what a thread knows about its column and its strip, built once; the sources hold a reference */
struct WalkCol {
    const int N, H, strip, strips;
    const int tid, lane, wv;
    const int v;           /* virtual column */
    const int vcol;        /* wrap; v < 0 keeps the flat rule */
    const bool provider;   /* has a slot */
    const bool outcol;     /* owns column v's outputs */
    const int first_col;   /* virtual column of offset 0 */
    const int own_cols;    /* own columns of this strip */
    const int row_span;    /* offsets that belong to the row */
    /* the strips whose virtual columns reach past the row's end and wrap to its start: the last one — and the one before it
     * when the last strip owns a single column (H mod 236 == 1: column H - 2 then belongs to the strip before, and its
     * (c + 2) % H fallback is column 0).  Found by the round-4 property test on a 473-column sensor: until then only the
     * last strip fetched its wrap-around halo in the indexed sources. */
    const bool last_strip;
    const char *const fbytes; /* the frame's points as the source reads them */
    const uint32_t T;         /* indexed sources: length of the prefix k_probe took for sorted (FrameInfo::T) */
    const uint32_t ring_l;    /* LDS address of the ring, for LDS-DMA */
    __device__ __forceinline__ WalkCol(const Geometry &g, int strip_, const void *points, uint32_t T_, uint32_t ring_l_)
        : N(g.N), H(g.H), strip(strip_), strips(g.strips), tid((int)threadIdx.x), lane(tid & 63), wv(__builtin_amdgcn_readfirstlane(tid >> 6)),
          v(strip_ * kStripCols + tid - 2), vcol(v >= H ? v - H : v), provider(tid < kStripVirt && (v < H + 2) && (v >= 0 || strip_ == 0)),
          outcol(tid >= 2 && tid < 2 + kStripCols && v < H), first_col(strip_ * kStripCols - 2),
          own_cols((H - first_col - 2) < kStripCols ? (H - first_col - 2) : kStripCols), row_span((H - first_col) < kStripVirt ? (H - first_col) : kStripVirt),
          last_strip(strip_ * kStripCols - 2 + kStripVirt > H), fbytes(reinterpret_cast<const char *>(points)), T(T_), ring_l(ring_l_)
    {
    }
};

/* A source of the walk's points: a type that owns its per-thread state as members and its LDS arrays as the nested type Lds,
 * and that walk_body calls at these places (every hook force-inlined; I = step mod 3, see RingSlots):
 *   setup()                      fills its LDS tables, before the first barrier;
 *   prologue()                   issues the loads the first row steps expect to be under way;
 *   arrive<I>(r, lo, hi)         before step r's barrier: the counted wait for row r's loads, then the thread's own piece of the
 *                                row (-> lo, hi) or, kIndexed, row r's records into an index row;
 *   take<I>(r, lo, hi)           after the barrier: kIndexed: the column's owner follows its index entry to its point;
 *   issue<I>(r)                  the step's loads, behind its stores;
 *   xpose<I>()                   byte offset of the ring piece, idle right now, through which the write-out transposes;
 *   upper_missing(r, intensity)  in the status of row r, with the intensity of the point above (-1: none, a fallback is taken);
 *   finish()                     after the last step;
 * and these traits:
 *   kIndexed     the points reach their columns through an index row (LDS atomicMax) after the step's barrier: edges and
 *                wave counts are published at the END of a step, and no wave ends early;
 *   kChecked     the source counts and checks what it reads: `consumed` and `failed` go to FrameInfo;
 *   kAnyMode     the launch is not for the frames of one mode;  kStrip0Last  strip 0 is dispatched last;
 *   kRingBytes   bytes of the ring;  input(b, g, f)  the frame's points. */
template <int kSrc>
struct WalkSource;
/* (developer build with phase clocks: the hooks that hold a phase marker take the clock along) */
#ifdef BEV_CS_CLOCK
#define WALK_PHA_PARAMS , long long (&pha_)[8], long long &pha_t
#define WALK_PHA_ARGS , pha_, pha_t
#else
#define WALK_PHA_PARAMS
#define WALK_PHA_ARGS
#endif

/* The walk's LDS, one struct per source so that the same bytes can be another kernel body's in a fused launch (k_stage):
 * every body carves its arrays out of ONE arena; a workgroup runs one body.  What every source uses, then the source's own. */
template <int kSrc>
struct WalkLds {
    static constexpr int kWaves = kStripThreads / 64;
    static constexpr int kSeenB = WalkSource<kSrc>::kIndexed ? BEV_SEENB : kSeenBits; /* (the indexed sources need the LDS for their windows) */
    alignas(16) char ring[WalkSource<kSrc>::kRingBytes];      /* the points under way, as the source lays them out */
    alignas(16) u32x4 zero16[1];                              /* what an empty slot reads (indexed sources) */
    alignas(16) float4 edge[3][kWaves][4];                    /* rows r, r-1, (r-2): lanes 0, 1, 62, 63 of every wave */
    /* per-wave candidate counts of the row being written, at [.][kWaves + wave] behind kWaves words that stay zero: the
     * three words before a wave's own are the counts of the waves before it, whichever wave it is (no selects) */
    alignas(16) uint32_t wave_cnt[2][2 * kWaves];
    uint32_t band_cursor[kMaxBands];                          /* entries already in this strip's code list of each band */
    uint32_t seen[1 << kSeenB];                               /* direct-mapped memo of codes this strip has already listed */
    int edge_x[kGridRows], edge_y[kGridCols];                 /* BEV bin of every ground-grid row's / column's lower edge */
    uint8_t band_tab[512];                                    /* x bin -> raster band */
    typename WalkSource<kSrc>::Lds src;
};

} /* namespace bevk */

#include "bev_walk_gather.h"
#include "bev_walk_inplace.h"
#include "bev_walk_firing.h"

namespace bevk {

static_assert(sizeof(WalkLds<kSrcInPlace>) <= 32 * 1280 && sizeof(WalkLds<kSrcGather>) <= 32 * 1280 && sizeof(WalkLds<kSrcStructured>) <= 32 * 1280,
              "four column-walk workgroups per CU: 32 of the CU's 128 LDS granules (1,280 bytes) each");
static_assert(sizeof(WalkLds<kSrcColMajorGen>) <= 42 * 1280 && sizeof(WalkLds<kSrcColMajor>) <= 42 * 1280, "three firing-order workgroups per CU");

template <int kSrc, bool kPow2, bool kGm>
__device__ __forceinline__ void walk_body(char *arena, const BatchPtrs &b, const Geometry &g, const int f, int strip, uint32_t want_mode, int bid /* developer builds: which workgroup prints */)
{
    TL_BEGIN;
    using Source = WalkSource<kSrc>;
    using Lds = WalkLds<kSrc>;
    constexpr bool kIndexed = Source::kIndexed;
#ifdef BEV_CS_CLOCK
    const long long tl_t0 = wall_clock64();
#endif
    (void)bid;
    if (Source::kStrip0Last) strip = g.strips - 1 - strip;
    if (!Source::kAnyMode && b.info) { /* the launch for its mode has the frame; the general launch has every frame that is not read in place */
        const uint32_t fmode = b.info[f].mode;
        if (frame_read_in_place(want_mode) ? fmode != want_mode : frame_read_in_place(fmode)) return;
    }
    constexpr int kWaves = Lds::kWaves, kSeenB = Lds::kSeenB;
    Lds &lds_w = *reinterpret_cast<Lds *>(arena);
    const WalkCol c(g, strip, Source::input(b, g, f), kIndexed ? b.info[f].T : 0u, __builtin_amdgcn_readfirstlane(lds_addr(&lds_w.ring[0])));
    const int tid = c.tid, lane = c.lane, wv = c.wv, v = c.v;
    const bool outcol = c.outcol;
    const int N = g.N, H = g.H, lo_row = g.N - g.G, strips = g.strips;
    const size_t frame_off = (size_t)f * g.S;
    const int bands = g.raster_bands;

    /* the value two lanes to the right / left (wrapping inside the wave; the edge lanes are patched from LDS).  (Two DPP
     * wave shifts instead of each ds_bpermute measured the same.) */
    const int sh_right = ((lane + 2) & 63) << 2, sh_left = ((lane - 2) & 63) << 2;
    auto from_right2 = [&](float x) -> float { return __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(sh_right, (int)__float_as_uint(x))); };
    auto from_left2 = [&](float x) -> float { return __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(sh_left, (int)__float_as_uint(x))); };

    auto &ring = lds_w.ring;
    auto &edge = lds_w.edge;
    auto &wave_cnt = lds_w.wave_cnt;
    auto &band_cursor = lds_w.band_cursor;
    auto &band_tab = lds_w.band_tab;
    auto &seen = lds_w.seen;
    auto &edge_x = lds_w.edge_x;
    auto &edge_y = lds_w.edge_y;
    Source src(lds_w, c, b, g, f);
    if (tid < kMaxBands) band_cursor[tid] = 0u;
    if (tid < 4 * kWaves) (&wave_cnt[0][0])[tid] = 0u;
    if (tid < 3 * kWaves * 4) (&edge[0][0][0])[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = tid; k < (1 << kSeenB); k += kStripThreads) seen[k] = kSkip;
    for (int x = tid; x < g.rp.mat_size; x += kStripThreads) band_tab[x] = (uint8_t)raster_band_of_nodiv(x, g.rp);
    if (tid < kGridRows) edge_x[tid] = cell_edge_bin(tid, 75.0f, g.rp);
    else if (tid < kGridRows + kGridCols) edge_y[tid - kGridRows] = cell_edge_bin(tid - kGridRows, 50.0f, g.rp);
    src.setup();
    lds_barrier();
    /* a wave none of whose threads has a column ends here (its counts stay zero, nobody reads its edge lanes: the
     * threads that would are not output columns; an indexed source needs every wave for its windows) */
    if (!kIndexed && __ballot(c.provider) == 0ull) return;

    src.prologue();

    WalkRow pr[3] = {};
    PHA_DECL;
#ifdef BEV_CS_CLOCK
    if (lane == 0 && bid == 100) printf("walk_prologue %lld (x10 ns)\n", pha_t - tl_t0);
#endif
    float zref = __uint_as_float(0x7fc00000u); /* height of the column's last candidate taken for ground (NaN: none yet) */

    const size_t cand_base = (size_t)f * g.segs * kSeg;
    const gptr<u32x2> fcand = (gptr<u32x2>)(b.cand + cand_base);
    const gptr<uint32_t> fncand = (gptr<uint32_t>)(b.ncand + (size_t)f * g.segs);
    const uint32_t code_last = in_vgpr(g.code_cap - 1u), code_stride = in_vgpr(g.code_stride); /* (they only feed vector instructions) */
    const gptr<uint32_t> flist = (gptr<uint32_t>)(b.code_main + ((size_t)f * g.emitters + strip) * bands * (size_t)g.code_stride);
    const gptr<u32x4> fordered = (gptr<u32x4>)(b.ordered + frame_off);
    const gptr<int8_t> fgm = (gptr<int8_t>)(kGm ? b.gm + frame_off : nullptr);
    RasterParams rp = g.rp; /* the fields the BEV code needs, in vector registers */
    rp.max_range_f = in_vgpr(rp.max_range_f);
    rp.lidar_to_ground = in_vgpr(rp.lidar_to_ground);
    rp.mat_size = in_vgpr(rp.mat_size);
    rp.n_layers = in_vgpr(rp.n_layers);
    if (kPow2) {
        rp.inv_interval = in_vgpr(rp.inv_interval);
        rp.inv_height_res = in_vgpr(rp.inv_height_res);
    } else {
        rp.interval = in_vgpr(rp.interval);
        rp.height_res = in_vgpr(rp.height_res);
    }
    /* A wave's 64 finished points are 2 KiB of consecutive bytes of the output.  Stored as they sit in the registers — the
     * low halves with one instruction, the high halves with another — every 128-byte line leaves the CU in two
     * instalments and L2 writes some lines back in between (WRITE_SIZE 5.39 MB where 4.9 MB were stored).  Transposed
     * through 2 KiB of LDS each instruction stores 1 KiB of whole lines.  The 2 KiB are a piece of a ring slot that is
     * idle right now and that only this wave's own DMA refills: the source says which (xpose; this wave's two 1-KiB pieces
     * of it, points 0..31 in the first). */
    /* (a point's halves swap places in every second group of four points: eight lanes' 16-byte writes at a stride of
     * 32 B then fall into eight different bank quads instead of four — the writes were a two-way conflict) */
    const uint32_t xp_sw = ((uint32_t)lane >> 2) & 1u;
    const uint32_t xp_w = (uint32_t)wv * 1024u + (uint32_t)(lane & 31) * 32u + (lane < 32 ? 0u : 4096u);
    const uint32_t xp_wlo = xp_w + 16u * xp_sw, xp_whi = xp_w + 16u * (xp_sw ^ 1u);
    /* reader lane j wants 16-byte unit j of the KiB = half (j & 1) of point j >> 1 */
    const uint32_t xp_unit = ((uint32_t)lane & ~1u) | (((uint32_t)lane & 1u) ^ (((uint32_t)lane >> 3) & 1u));
    const uint32_t xp_r0 = (uint32_t)wv * 1024u + xp_unit * 16u, xp_r1 = xp_r0 + 4096u; /* first, second KiB */

    /* byte offset of this lane's 16-byte unit in the SECOND KiB of the wave's 64 columns of the ordered cloud's row r - 2
     * (128 units; the first KiB lies 1024 bytes before).  Modulo 2^32 while the row is negative: never used then; from row 0
     * on it is a true offset for every lane (the first strip's first wave starts two columns before the row: its first
     * KiB's first four units do not exist — those lanes do not store — but its second KiB does). */
    uint32_t ord_off = (uint32_t)((-2 * H + strip * kStripCols - 2 + 64 * wv) * 2 + 64 + lane) * 16u;
    const uint32_t row_bytes = (uint32_t)H * 32u;
    auto row_step = [&](auto I, const int r) {
        constexpr int kI = decltype(I)::value;
        WalkRow &p0 = pr[RingSlots<kI>::s0], &p1 = pr[RingSlots<kI>::s2], &p2 = pr[RingSlots<kI>::s1];
        const int par = r & 1;
        u32x4 cur_lo, cur_hi;
        PHA(7);
        /* Everything but the newest step's loads has arrived: what the source needs of row r.  A wave waits for as many
         * operations as it issues loads per step. */
        src.template arrive<kI>(r, cur_lo, cur_hi WALK_PHA_ARGS);
        /* What the waves exchange per step: row r's edge lanes (read by the NEXT step's status) and the per-wave counts of
         * row r-2's candidates (read by this step's write-out).  Published here, before the step's barrier — unless the
         * source is indexed: the point of row r is then known only after the barrier (it makes the index row visible), so
         * both are published at the END of the previous step instead (measured on the gather source, that order costs
         * 7 %: a wave reaches the barrier straight from its memory wait). */
        if constexpr (!kIndexed) {
            if (lane < 2 || lane >= 62)
                edge[r % 3][wv][lane < 2 ? lane : lane - 60] = make_float4(__uint_as_float(cur_lo.x), __uint_as_float(cur_lo.y), __uint_as_float(cur_lo.z), __uint_as_float(cur_hi.x));
            const bool c2 = outcol && wr_gflag(p2.fl) == 1;
            const uint32_t q2 = p2.key & 3u;
            uint32_t rank2;
            const uint32_t scan = quarter_scan(c2, q2, &rank2);
            if (lane == 63) wave_cnt[par][kWaves + wv] = scan;
            p2.fl |= rank2 << kFlRankShift;
        }
        lds_barrier();
        PHA(2);
        src.template take<kI>(r, cur_lo, cur_hi);
        const XYZI prev{__uint_as_float(p1.lo.x), __uint_as_float(p1.lo.y), __uint_as_float(p1.lo.z), __uint_as_float(p1.hi.x)};
        const XYZI prevprev{__uint_as_float(p2.lo.x), __uint_as_float(p2.lo.y), __uint_as_float(p2.lo.z), __uint_as_float(p2.hi.x)};
        const XYZI cur{__uint_as_float(cur_lo.x), __uint_as_float(cur_lo.y), __uint_as_float(cur_lo.z), __uint_as_float(cur_hi.x)};

        /* ---- write out row r-2 (first thing after the barrier: its stores are the oldest entries of the step) ---- */
        PHA(3);
        const bool cand2 = outcol && wr_gflag(p2.fl) == 1;
        if (r >= 2) {
            const int q = r - 2;
            const int rr = q - (lo_row - 1);        /* only rows lo-1 .. N-1 can hold candidates */
            if (rr >= 0) {
                /* Candidates of row r-2 by cell quarter (cell mod 4, the low bits of the key): a segment keeps its candidates
                 * as four consecutive runs, one per quarter, each in column order — phase B is four workgroups per frame that
                 * each read one run (cells are independent, only the order inside a cell matters).  A wave's four counts (at
                 * most 64 each; a segment's at most 236 each) travel in one word. */
                const uint32_t q2 = p2.key & 3u;
                static_assert(kWaves == 4, "the four counts are read as one 16-byte word");
                const u32x4 wc = *reinterpret_cast<const u32x4 *>(&wave_cnt[par][kWaves]);
                const uint32_t total = wc.x + wc.y + wc.z + wc.w; /* four byte-wide sums */
                const uint32_t *wb = &wave_cnt[par][wv + 1];
                const uint32_t before = wb[0] + wb[1] + wb[2];
                const uint32_t seg = (uint32_t)(rr * strips + strip);
                if (cand2) {
                    /* where the quarter's run starts (byte q of total * 0x01010100: the quarters below it) + the earlier
                     * waves' candidates of the quarter (no byte overflows: everything stays below the segment's total) +
                     * the earlier lanes' (the rank the scan left in the record) */
                    const uint32_t t8 = total << 8;
                    const uint32_t starts = t8 + (t8 << 8) + (t8 << 16) + before;
                    const uint32_t rank = __builtin_amdgcn_ubfe(starts, q2 << 3, 8u) + ((p2.fl >> kFlRankShift) & 63u);
                    fcand[seg * (uint32_t)kSeg + rank] = u32x2{p2.key, p2.lo.z}; /* key | height */
                }
                if (tid == 2) fncand[seg] = total;
            }
            {   /* BEV code of the slot.  A slot that is not a candidate has its final label, so its code is final too: it
                 * is appended to this strip's list of the raster band its x bin falls into (the order inside a list does
                 * not matter: an LDS cursor per band).  Candidates' codes travel in their keys.  A lane whose left
                 * neighbour appends the very same code skips (near the sensor dozens of consecutive returns share a bin),
                 * and so does one whose code this strip has listed before and still remembers (rings hit the same cells
                 * at the same heights again and again: a HDL_64E frame lists 74 k codes of which 24 k are distinct).  The
                 * rasters are idempotent, so a stale or racing memo entry only costs a duplicate. */
                bool has = outcol && !cand2 && p2.code != kSkip;
                /* (the left neighbour's code and flag by DPP: no LDS round trip) */
                const uint32_t left_code = (uint32_t)__builtin_amdgcn_update_dpp((int)kSkip, (int)p2.code, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                const bool left_has = __builtin_amdgcn_update_dpp(0, has ? 1 : 0, 0x138, 0xf, 0xf, false) != 0;
                has = has & !((lane > 0) & left_has & (left_code == p2.code));
                /* the memo entry and the band of the code are requested together, then one cursor atomic */
                const uint32_t slot = (p2.code * 0x9E3779B1u) >> (32 - kSeenB);
                const uint32_t remembered = seen[slot];
                const int band = band_tab[code_x(p2.code) & 511];
                has = has & (remembered != p2.code);
                if (has) seen[slot] = p2.code;
                /* (one cursor atomic per wave and band instead of one per code — a ballot loop — measured 2 % slower) */
                if (has) {
                    const uint32_t pos = atomicAdd(&band_cursor[band], 1u);
                    /* (a full list keeps counting and overwrites its last entry: k_bev_raster sees the count) */
                    flist[(uint32_t)band * code_stride + (pos < code_last ? pos : code_last)] = p2.code;
                }
            }
            {   /* the ordered cloud, as whole lines */
                u32x4 hi = p2.hi;
                const bool as_ground = cand2 && !((p2.fl >> 4) & 1u);
                if (as_ground) hi.w &= 0xffff0000u; /* label = 0, BatchMultiBevGen.cpp:245 (provisional) */
                char *xb = &ring[src.template xpose<kI>()];
                *reinterpret_cast<u32x4 *>(xb + xp_wlo) = p2.lo;
                *reinterpret_cast<u32x4 *>(xb + xp_whi) = hi;
                const u32x4 pa = *reinterpret_cast<const u32x4 *>(xb + xp_r0);
                const u32x4 pb = *reinterpret_cast<const u32x4 *>(xb + xp_r1);
                const unsigned long long owners = __ballot(outcol);
                /* (this lane's unit of row q: a byte offset into the frame kept per lane and advanced by one row per step —
                 * base register + 32-bit offset, no 64-bit address arithmetic) */
                const gptr<char> orow = (gptr<char>)fordered + ord_off;
                if ((owners >> (lane >> 1)) & 1ull) __builtin_nontemporal_store(pa, (gptr<u32x4>)(orow - 1024));
                if ((owners >> (32 + (lane >> 1))) & 1ull) __builtin_nontemporal_store(pb, (gptr<u32x4>)orow);
                if (kGm && outcol) fgm[(uint32_t)(q * H + v)] = (int8_t)wr_gflag(p2.fl);
            }
        }
        ord_off += row_bytes;
        /* ---- the loads of this step, behind its stores ---- */
        PHA(4);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* this wave is done reading the pieces it refills */
        src.template issue<kI>(r);

        /* ---- status of row r (BatchMultiBevGen.cpp:142-182) ---- */
        PHA(5);
        int s_r = kSteep;
        if (r >= lo_row && r < N) { /* workgroup-uniform */
            /* row r-1 of the threads two to the right / left */
            XYZI right{from_right2(prev.x), from_right2(prev.y), from_right2(prev.z), from_right2(prev.i)};
            XYZI left{from_left2(prev.x), from_left2(prev.y), from_left2(prev.z), from_left2(prev.i)};
            const float4(*pe)[4] = edge[(r + 2) % 3];
            if (lane >= 62) { /* (the last wave's two have no right neighbour: the value is never used, it is not an output column's) */
                const float4 q = pe[wv + 1 < kWaves ? wv + 1 : wv][lane - 62];
                right = XYZI{q.x, q.y, q.z, q.w};
            }
            if (lane < 2) {
                const float4 q = pe[wv > 0 ? wv - 1 : 0][lane + 2];
                left = XYZI{q.x, q.y, q.z, q.w};
            }
            {   /* (every thread evaluates it: only output columns' statuses are ever used) */
                XYZI up = prev;                                  /* (r-1, c)                  :143     */
                src.upper_missing(r, up.i);
                if (up.i == -1.0f) up = right;                   /* (r-1, (c+2) % H)          :146-149 */
                if (up.i == -1.0f) up = left;                    /* flat (r-1)*H + c - 2      :151-154 */
                if ((up.i == -1.0f) & (r >= 2)) up = prevprev;   /* (r-2, c)                  :157-160 */
                const bool ground = angle_is_ground_nodiv(up.x - cur.x, up.y - cur.y, up.z - cur.z); /* :169-182 */
                s_r = ((cur.i == -1.0f) | (up.i == -1.0f)) ? kInvalid : (ground ? kGround : kSteep); /* :162-167 */
            }
        }

        /* ---- ground_mat of row r-1 is now decided (closed form, see bev_exact.h) ---- */
        PHA(6);
        int gf = 0;
        {
            const int q = r - 1, st1 = wr_status(p1.fl);
            if (q >= lo_row) gf = (st1 == kInvalid) ? -1 : (st1 == kGround ? 1 : (s_r == kGround ? 1 : 0));
            else if (q == lo_row - 1) gf = (s_r == kGround) ? 1 : 0;
            if (!(q >= 0 && q < N)) gf = 0;
        }
        const bool cand1 = outcol && gf == 1;
        /* Provisional labels.  Phase C un-grounds a candidate that lies 0.30 m above a neighbour cell's average ground
         * height — known only after the whole frame has been summed.  The walk GUESSES: a candidate 0.30 m above the last
         * candidate of its column that it took for ground is written with its own label, every other candidate with
         * label 0; k_ground_resolve tests every candidate exactly and patches the wrong guesses in either direction.
         * The guess only decides how many sparse 2-byte patches are needed (benchmark frames: 1.3 k instead of 7.9 k per
         * frame).  A candidate whose label is not the -2 every producer writes (MulranPointCloudSelect.cpp:126) keeps its
         * label whatever the guess: phase C can then always patch without looking the input point up again (the key says
         * "-2" or the patch is a 0). */
        bool pred1;
        {
            const float zq = __uint_as_float(p1.lo.z);
            const bool plain = (p1.hi.w & 0xffffu) == 0xfffeu;
            pred1 = cand1 && (!plain || zq - zref >= 0.3f); /* (the comparison is false while zref is NaN) */
            if (cand1 && !pred1) zref = zq;
        }
        p1.fl = (p1.fl & 3u) | ((uint32_t)(gf + 1) << 2) | (pred1 ? 16u : 0u);
        if (cand1) {
            int cr, cc;
            const int cell = ground_cell_rc(__uint_as_float(p1.lo.x), __uint_as_float(p1.lo.y), &cr, &cc);
            p1.key = candidate_key_edges(cell, tid - 2, pred1, p1.code, (int)(int16_t)(p1.hi.w & 0xffffu), edge_x[cr], edge_y[cc]);
        }

        /* ---- row r's record (the one row r-3 has left) ---- */
        p0.lo = cur_lo;
        p0.hi = cur_hi;
        p0.fl = (uint32_t)(s_r + 1) | (1u << 2);
        p0.key = 0u;
        p0.code = code_t<kPow2>(cur.x, cur.y, cur.z, (int)(int16_t)(cur_hi.w & 0xffffu), rp);

        /* ---- indexed sources: published for the next step: row r's edge lanes, the candidates of row r-1 per wave ---- */
        if constexpr (kIndexed) {
            if (lane < 2 || lane >= 62) edge[r % 3][wv][lane < 2 ? lane : lane - 60] = make_float4(cur.x, cur.y, cur.z, cur.i);
            const uint32_t q1 = p1.key & 3u;
            uint32_t rank1;
            const uint32_t scan = quarter_scan(cand1, q1, &rank1);
            if (lane == 63) wave_cnt[par ^ 1][kWaves + wv] = scan;
            p1.fl |= rank1 << kFlRankShift;
        }
    };
    /* two extra iterations drain the pipeline */
    for (int r0 = 0; r0 < N + 2; r0 += 3) {
        row_step(std::integral_constant<int, 0>{}, r0);
        if (r0 + 1 < N + 2) row_step(std::integral_constant<int, 1>{}, r0 + 1);
        if (r0 + 2 < N + 2) row_step(std::integral_constant<int, 2>{}, r0 + 2);
    }
    wait_vm<0>(); /* no LDS-DMA may outlive the workgroup's LDS */
#ifdef BEV_CS_CLOCK
    src.clk_print(bid, f WALK_PHA_ARGS);
    /* where and when the workgroup ran: HW_ID (wave, SIMD, CU, SH, SE), XCC_ID; start and end on the 100 MHz clock */
    if (tid == 0 && kIndexed && bid < kWalkTlCap) {
        long long *rec = g_walk_tl[bid];
        rec[0] = tl_t0;
        rec[1] = wall_clock64();
        rec[2] = (long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        rec[3] = (long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
#endif
    lds_barrier();
    if (tid < bands) b.ncode[((size_t)f * g.emitters + strip) * bands + tid] = band_cursor[tid];
    src.finish();
    if constexpr (Source::kChecked) {
        uint32_t consumed = src.consumed, failed = src.failed;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            consumed += __shfl_xor(consumed, d);
            failed |= __shfl_xor(failed, d);
        }
        if (lane == 0) {
            atomicAdd(&b.info[f].consumed, consumed);
            if (failed) atomicOr(&b.info[f].failed, failed);
        }
    }
    TL_END(K_GATHER_GROUND);
}

template <int kSrc, bool kPow2, bool kGm>
__global__ __launch_bounds__(kStripThreads, (kSrc == kSrcColMajor || kSrc == kSrcColMajorGen) ? 3 : 4) void k_walk(BatchPtrs b, Geometry g, int nf, uint32_t want_mode)
{
    __shared__ __attribute__((aligned(16))) char arena[sizeof(WalkLds<kSrc>)];
    int f, strip;
    if (!map_block_xcd((int)blockIdx.x, nf, g.strips, f, strip)) return;
    walk_body<kSrc, kPow2, kGm>(arena, b, g, f, strip, want_mode, (int)blockIdx.x);
}

} /* namespace bevk */

#endif /* BEV_WALK_H */
