/*
 * bev_walk_firing.h — the column walk's firing-order sources: the plain sweep (kSrcColMajor) and the general form (kSrcColMajorGen), read as bands of two rows
 * Part of the device code of libbev_mi355x.so; included by bev_walk.h only, behind WalkCol and WalkLds.
 */
#ifndef BEV_WALK_FIRING_H
#define BEV_WALK_FIRING_H

namespace bevk {

/* Column-major source (kFrameColMajor): input position k holds the return of firing k / N, beam k % N — what the MulRan
 * selector writes (MulranPointCloudSelect.cpp:112-130: row = k % 64, col from the azimuth).  With u = +-firing mod H (the
 * sweep's direction) a return of row r sits in column (u + B[r] + 0 .. kColMaxDisp) mod H (k_probe found the direction and
 * the rows' bases B).  A strip's threads take one u each, from kColMaxDisp + the largest base before the strip's first
 * virtual column on (kCmExt more by wave 0: 272 firings cover 240 columns, the jitter and bases kCmSpread apart); the
 * records of kBandRows consecutive rows of a firing are 64 contiguous bytes of the input, fetched as one band. */
constexpr int kBandRows = 2;
/* the PLAIN sweep (kFrameColMajor: starts at azimuth 0, turns forward, column = firing + 0 .. 8, no no-return records; BASELINE
 * config 3) keeps round 4's walk: a thread per firing from kColLead firings before the strip's first own column, side windows of
 * the first / last kPlainSide firings, 50 KB of LDS.  Everything else in firing order takes the general form below (kFrameColMajorGen). */
constexpr int kColLead = 2 + kPlainDisp, kPlainSide = 16;
constexpr int kPlainBuf = kStripThreads * 32 * kBandRows + 2 * kPlainSide * 32 * kBandRows; /* one band buffer: the band, the flat-rule window, the wrap-around window */
static_assert(kPlainSide * 2 * kBandRows == 64 && kStripVirt + kPlainDisp <= kStripThreads && kPlainDisp + 2 <= kPlainSide, "the plain sweep's windows");
constexpr int kSideFirings = 32; /* firings of the side area: the wrap-around halo's window or strip 0's flat-index halo's */
constexpr int kBandBytes = kStripThreads * 32 * kBandRows;
constexpr int kExtBytes = kCmExt * 32 * kBandRows;
constexpr int kSideBytes = kSideFirings * 32 * kBandRows;
constexpr int kSpecialBytes = 32 * kBandRows;            /* strip 0: the last no-return record of either row that another strip owns */
constexpr int kColBuf = kBandBytes + kExtBytes + kSideBytes + kSpecialBytes; /* one band buffer */
/* where a record sits in a band buffer, as the index row remembers it: 0 .. 255 a thread's, then kCmExt extra firings,
 * kSideFirings side firings, the special record; all but the first 256 are 64-byte entries behind the band */
constexpr uint32_t kLocExt = kStripThreads, kLocSide = kLocExt + kCmExt, kLocSpecial = kLocSide + kSideFirings, kLocBits = 9;
static_assert(kLocSpecial < (1u << kLocBits) && kCmExt * 2 * kBandRows == 64, "location bits; the extra firings of a band are one LDS-DMA instruction");
static_assert(kStripVirt + kColMaxDisp + kCmSpread <= kStripThreads + kCmExt && 2 + kColMaxDisp + kCmSpread <= kSideFirings,
              "firings a strip's columns can come from");
constexpr uint32_t kCmSpins = 1u << 12; /* polls (a sleep and an agent-scope load each, a microsecond or two) before strip 0 gives up on the others' reports: milliseconds, where a walk workgroup lives a fifth of one */
/* What of a strip's place among its frame's strips the row loop needs it gets as ONE scalar word of flags and a handful of
 * per-lane values computed in setup() (the first form kept a dozen scalars alive across the loop: 52 spilled scalar
 * registers, the walk 8 % slower). */
enum : uint32_t { kCfExt = 2u, kCfReports = 4u, kCfListens = 8u, kCfQuiet = 16u, kCfFirst = 32u, kCfBoth = 64u, kCfFlat = 128u, kCfWrap = 256u };

template <bool kGen>
struct FiringLds {
    uint32_t idx[2][kStripThreads + 1]; /* column offset -> thread of the window + 1, or kStripThreads + side firing + 1 ([256]: nowhere) */
};
/* general form: the frame's row bases (k_probe), what the strips tell each other */
template <>
struct FiringLds<true> {
    uint32_t idx[2][kStripThreads + 1]; /* column offset -> (firing + 1) << kLocBits | where the record sits ([256]: nowhere) */
    uint32_t cm_nr_l[2];     /* no-return firings + 1 this strip owns, rows 2b, 2b + 1 of the band just arrived (LDS atomicMax) */
    uint32_t cm_spec_l[2][2]; /* strip 0: [band & 1][row & 1]: the last no-return firing + 1 of the row that another strip owns (0: none) */
    uint32_t cm_halo0_l[2];  /* [row & 1]: the index entry that the strip with the wrap-around halo found for virtual column H (= column 0) */
    uint32_t cm_poll_l[2][32];
    uint16_t cm_base_l[kCmMaxRows]; /* (LDS is what holds this source at three workgroups per CU: 42 allocation granules of 1,280 bytes and not one more) */
    uint16_t cm_win0_l[kCmMaxRows]; /* strip 0: per row, the firing + 1 whose record it put into column 0 (written out at the end) */
};

/* The two forms are ONE type: they share the band buffers, the index row and the step's shape (a band every other step,
 * waited for with nothing outstanding), and differ in which firing a thread takes and in what strips say to each other —
 * `if constexpr (kGen)` where they part, as many places as the plain form has lines of its own. */
template <bool kGen>
struct FiringSource {
    static constexpr int kSrc = kGen ? kSrcColMajorGen : kSrcColMajor;
    static constexpr bool kIndexed = true, kChecked = true;
    /* strip 0 listens to the other strips of its frame (no-return records, see listen_band): it is dispatched LAST of them,
     * and finds them under way (dispatched first it waited a quarter of its life for them to start: the walk 5 % slower) */
    static constexpr bool kStrip0Last = kGen;
    static constexpr bool kAnyMode = false;
    static constexpr int kCmBuf = kGen ? kColBuf : kPlainBuf; /* bytes of one band buffer */
    static constexpr int kRingBytes = 2 * kCmBuf + 8192;      /* two band buffers, then 8 KiB for the write-out's transposition */
    using Lds = FiringLds<kGen>;
    static __device__ __forceinline__ const bev_point_t *input(const BatchPtrs &b, const Geometry &, int f) { return b.pts + b.frames[f].in_offset; }

    WalkLds<kSrc> &lds;
    const WalkCol &c;
    const int32_t *const fpar; /* general form: the frame's direction, largest base, row bases, spread, kind (k_probe) */
    uint32_t consumed = 0u, failed = 0u;
    /* the plain sweep: this thread's firing */
    const int pl_firing;
    const bool pl_valid;
    const bool pl_own; /* counted by this strip */
    /* general form */
    bool cm_fwd = true;            /* the sweep's direction */
    uint32_t cm_f = 0u;            /* (wave-uniform) kCf* */
    int cm_u = 0;                  /* this thread's u = +-firing mod H */
    uint32_t cm_off = 0u, cm_key = 0u, cm_vf = 0u; /* byte offset of its firing's records in the frame; its index key; bit 0 valid, bit 1 counted by this strip */
    uint32_t cm_ext_off = 0u, cm_ext_key = 0u;     /* wave 0: lane = extra firing * 4 + piece: that piece's offset (row 0 of a band); lane < kCmExt: the extra firing's key (0: none) */
    uint32_t cm_side_off[2] = {0u, 0u}, cm_side_key = 0u; /* the side window's wave: the same for its firings (two instructions of 16); lane < 32: a side firing's key */
    const int cm_words_v; /* (<= 30: kCmMaxStrips) strip 0 listens to this many words per band (kept in a vector register: see cm_pub_v) */
    /* the frame's words of cm_sync: [band][strip][2], then the per-row words.  (The pointer lives in vector registers: these are
     * rare accesses, and every scalar register kept across the row loop is one more that the loop spills.) */
    const uint64_t cm_pub_v;
    int cm_waiting = -1; /* (wave 3 of strip 0) the band whose reports were not all in when asked */
#ifdef BEV_CS_CLOCK
    long long dbg_try_t = 0, dbg_block_t = 0;
    int dbg_fail_n = 0;
#endif

    __device__ __forceinline__ FiringSource(WalkLds<kSrc> &lds_, const WalkCol &c_, const BatchPtrs &b, const Geometry &, int f)
        : lds(lds_), c(c_), fpar(kGen ? b.cm_par + (size_t)f * kCmParWords : nullptr), pl_firing(c_.strip * kStripCols - kColLead + c_.tid),
          pl_valid((unsigned)pl_firing < (unsigned)c_.H), pl_own((unsigned)(pl_firing - c_.strip * kStripCols) < (unsigned)c_.own_cols),
          cm_words_v(in_vgpr((c_.strips - 1) * 2)), cm_pub_v(kGen ? in_vgpr((uint64_t)(uintptr_t)(b.cm_sync + (size_t)f * kCmSyncWords)) : 0ull)
    {
    }

    __device__ __forceinline__ gptr<uint32_t> cm_pub() const { return (gptr<uint32_t>)(uintptr_t)cm_pub_v; }
    __device__ __forceinline__ static uint32_t cm_buf(int band) { return (uint32_t)(band & 1) * (uint32_t)kCmBuf; }
    __device__ __forceinline__ int mod_h(int x) const /* x mod H for x in (-2 H, 2 H) */
    {
        const int H = c.H;
        x = x < 0 ? x + H : x;
        x = x < 0 ? x + H : x;
        return x >= H ? x - H : x;
    }
    __device__ __forceinline__ int firing_of(int u) const { return cm_fwd ? u : (u ? c.H - u : 0); } /* u = +-firing mod H */

    /* general form: the row bases, who counts what, this thread's firing and keys */
    __device__ __forceinline__ void setup()
    {
        const int tid = c.tid, lane = c.lane, wv = c.wv, H = c.H, N = c.N, first_col = c.first_col;
        lds.src.idx[0][tid] = 0u;
        lds.src.idx[1][tid] = 0u;
        if (tid == 0) lds.zero16[0] = u32x4{0u, 0u, 0u, 0u};
        if constexpr (kGen) {
            cm_fwd = fpar[0] > 0;
            const int cm_bmax = fpar[1];
            for (int r = tid; r < N; r += kStripThreads) lds.src.cm_base_l[r] = (uint16_t)fpar[2 + r];
            if (tid < 2) {
                lds.src.cm_nr_l[tid] = 0u;
                lds.src.cm_halo0_l[tid] = 0u;
                lds.src.cm_spec_l[0][tid] = lds.src.cm_spec_l[1][tid] = 0u;
            }
            const int kind = fpar[3 + kCmMaxRows]; /* 1 a sample was a no-return record, 0 none was */
            const bool first = c.strip == 0, both = first && c.last_strip, talk = c.strips > 1 && kind > 0;
            /* Do this frame's strips talk about no-return records (k_probe saw one)?  If not, a strip other than 0 that owns one
             * after all leaves the row's last in cm_sync and raises kInfoCmStray: k_verdict redoes the frame if it would have won.
             * The kCmExt firings behind the 256 threads' are needed only when the rows' bases lie far apart (staggered beams).
             * (A strip that is the first AND the last of its rows — a sensor of up to 237 columns — holds every firing in its
             * window: its threads enter columns 0, 1 a second time as the wrap-around halo, the side area is the flat-index halo's.) */
            const bool ext = kStripVirt + kColMaxDisp + fpar[2 + kCmMaxRows] > kStripThreads;
            cm_f = ((ext && wv == 0) ? kCfExt : 0u) | ((talk && !first) ? kCfReports : 0u) | ((talk && first && wv == 3) ? kCfListens : 0u) |
                   ((c.strips > 1 && !talk && !first) ? kCfQuiet : 0u) | (first ? kCfFirst : 0u) | (both ? kCfBoth : 0u) |
                   ((first && wv == 1) ? kCfFlat : 0u) | ((c.last_strip && !both && wv == 2) ? kCfWrap : 0u);
            cm_f = __builtin_amdgcn_readfirstlane(cm_f);
            /* this thread's u and firing; a window position past the circle's length repeats an earlier one */
            const int u0 = mod_h((first_col - cm_bmax - kColMaxDisp) % H);
            cm_u = mod_h(u0 + tid % H);
            const int firing = firing_of(cm_u);
            const bool valid = tid < H;
            /* every firing is counted by ONE strip: its window positions own_at .. own_at + own_cols - 1 (the strips' windows start
             * kStripCols apart, so these ranges tile the circle) */
            const int own_at = H >= kStripCols + 16 ? 16 : (H > kStripCols ? H - kStripCols : 0);
            cm_vf = (valid ? 1u : 0u) | (((unsigned)(tid - own_at) < (unsigned)c.own_cols) ? 2u : 0u);
            cm_off = (uint32_t)(valid ? firing : 0) * (uint32_t)N * 32u;
            cm_key = (((uint32_t)firing + 1u) << kLocBits) | (uint32_t)tid;
            const int i = lane >> 2, piece = lane & 3;
            if (cm_f & kCfExt) {
                const int w = kStripThreads + i, fr = firing_of(mod_h(u0 + w % H));
                cm_ext_off = (uint32_t)(w < H ? fr : 0) * (uint32_t)N * 32u + 16u * (uint32_t)(piece & 1);
                const int wl = kStripThreads + lane, frl = firing_of(mod_h(u0 + wl % H));
                cm_ext_key = (lane < kCmExt && wl < H) ? ((((uint32_t)frl + 1u) << kLocBits) | (kLocExt + (uint32_t)lane)) : 0u;
            }
            if (cm_f & (kCfFlat | kCfWrap)) {
                const int su0 = (cm_f & kCfFlat) ? mod_h((H - 2 - cm_bmax - kColMaxDisp) % H) : mod_h((-cm_bmax - kColMaxDisp) % H);
#pragma unroll
                for (int k0 = 0; k0 < 2; ++k0) {
                    const int k = 16 * k0 + i;
                    cm_side_off[k0] = (uint32_t)(k < H ? firing_of(mod_h(su0 + k % H)) : 0) * (uint32_t)N * 32u + 16u * (uint32_t)(piece & 1);
                }
                const int kl = lane & (kSideFirings - 1);
                cm_side_key = (lane < kSideFirings && kl < H) ? ((((uint32_t)firing_of(mod_h(su0 + kl % H)) + 1u) << kLocBits) | (kLocSide + (uint32_t)kl)) : 0u;
            }
        }
    }
    /* rows 2 * band, 2 * band + 1 of this thread's firing: four 16-byte pieces of one 64-byte sector -> piece j at
     * buffer + j * 4 KiB + thread * 16; wave 0: the same of the kCmExt firings behind the window; wave 1 of strip 0: the
     * rows LESS ONE of the firings whose returns can be columns H - 2, H - 1 (slots (r - 1, H - 2), (r - 1, H - 1) are
     * strip 0's virtual columns -2, -1 of row r); wave 2 of a strip with a wrap-around halo: the firings whose returns can
     * be columns 0, 1 (as H, H + 1); lane = firing * 4 + piece */
    __device__ __forceinline__ void issue_band(int band)
    {
        const int lane = c.lane, wv = c.wv, H = c.H, N = c.N;
        const char *fbytes = c.fbytes;
        const int r0 = band * kBandRows;
        if (r0 >= N) return; /* (uniform) */
        const uint32_t at = c.ring_l + cm_buf(band) + (uint32_t)wv * 1024u;
        if constexpr (!kGen) { /* the plain sweep: wave 1 of strip 0: the rows LESS ONE of the last kPlainSide firings; wave 2 of the last strip: the first kPlainSide firings */
            const char *src = fbytes + ((size_t)(pl_valid ? pl_firing : 0) * N + r0) * 32u;
            const bool two = r0 + 1 < N;
            glds16x2(src, at, src + 16, at + 4096u);
            glds16x2(src + (two ? 32 : 0), at + 8192u, src + (two ? 48 : 16), at + 12288u);
            if ((c.strip == 0 && wv == 1) || (c.last_strip && wv == 2)) {
                const bool flat = wv == 1;
                const int i = lane >> 2, piece = lane & 3;
                const int fr = flat ? H - kPlainSide + i : i;
                int row = r0 + (piece >> 1) - (flat ? 1 : 0);
                const bool ok = (unsigned)fr < (unsigned)H && (unsigned)row < (unsigned)N;
                glds16(fbytes + ((size_t)(ok ? fr : 0) * N + (ok ? row : 0)) * 32u + 16 * (piece & 1),
                       c.ring_l + cm_buf(band) + (uint32_t)kBandBytes + (flat ? 0u : (uint32_t)(kPlainSide * 32 * kBandRows)));
            }
            return;
        }
        const char *src = fbytes + cm_off + (uint32_t)r0 * 32u;
        /* (N odd or a last band of one row: the second row's pieces come from the next firing or past the frame's end —
         * never used; past the END of the input they would be out of bounds: clamp) */
        const bool two = r0 + 1 < N;
        glds16x2(src, at, src + 16, at + 4096u);
        glds16x2(src + (two ? 32 : 0), at + 8192u, src + (two ? 48 : 16), at + 12288u);
        const int ln = fresh(lane);
        const uint32_t second = ((ln & 2) && two) ? 32u : 0u; /* (piece >> 1: the band's second row) */
        if (cm_f & kCfExt) /* (uniform) the extra firings */
            glds16(fbytes + cm_ext_off + (uint32_t)r0 * 32u + second, c.ring_l + cm_buf(band) + (uint32_t)kBandBytes);
        if (cm_f & (kCfFlat | kCfWrap)) { /* (uniform) */
            const bool flat = (cm_f & kCfFlat) != 0u;
            /* the flat-index halo wants rows r0 - 1, r0: none before row 0 (that piece fetches row 0 and is not entered) */
            const int row = flat ? r0 - 1 + ((ln & 2) ? 1 : 0) : r0 + (((ln & 2) && two) ? 1 : 0);
            const uint32_t side_at = c.ring_l + cm_buf(band) + (uint32_t)(kBandBytes + kExtBytes);
            glds16(fbytes + cm_side_off[0] + (uint32_t)(row < 0 ? 0 : row) * 32u, side_at);
            glds16(fbytes + cm_side_off[1] + (uint32_t)(row < 0 ? 0 : row) * 32u, side_at + 16u * 64u);
        }
    }
    /* Strip 0, wave 3: what the other strips have reported for band `band` — the last no-return firing of either row —
     * and the two records themselves into the band buffer's special entry.  The others report when the band ARRIVES in
     * their LDS; strip 0 asks three steps before it uses the band, without waiting (the words come by LDS-DMA and are
     * looked at after the next step's memory wait): once it trails the others by that much it never stalls.  Only when
     * a report is still missing then does it wait for it (bounded), a step before the band is used. */
    __device__ __forceinline__ void ask_band(int band) /* (wave 3) */
    {
        if (band * kBandRows >= c.N) return; /* (uniform) */
        const int words = __builtin_amdgcn_readfirstlane(cm_words_v);
        if (fresh(c.lane) < words) glds4_nt((const uint32_t *)(uintptr_t)cm_pub_v + ((size_t)band * kCmMaxStrips + 1) * 2 + c.lane, __builtin_amdgcn_readfirstlane(lds_addr(&lds.src.cm_poll_l[band & 1][0])));
    }
    __device__ __forceinline__ void take_band(int band, uint32_t w) /* (wave 3) the reports are in: the larger firing per row, the records */
    {
        const int N = c.N;
        const int r0 = band * kBandRows, words = __builtin_amdgcn_readfirstlane(cm_words_v);
        /* even lanes: the band's first row, odd lanes: its second.  (The maxima by v_readlane and scalar compares: as lane
         * shuffles — five LDS round trips on a busy LDS — this cost strip 0 0.7 us at every other step.) */
        uint32_t v0 = 0u, v1 = 0u;
        for (int k = 0; k < words; k += 2) {
            const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)w, k) & 0xffffu, d = (uint32_t)__builtin_amdgcn_readlane((int)w, k + 1) & 0xffffu;
            v0 = a > v0 ? a : v0;
            v1 = d > v1 ? d : v1;
        }
        const int ln = fresh(c.lane);
        if (ln < 2) lds.src.cm_spec_l[band & 1][ln] = ln ? v1 : v0;
        if ((v0 | v1) != 0u && ln < 4) { /* (uniform test) the records (firing v - 1, row r0 + lane / 2); none: the frame's first record, never entered */
            const uint32_t vv = (ln >> 1) ? v1 : v0;
            const int row = r0 + (ln >> 1);
            const bool ok = vv != 0u && row < N;
            glds16(c.fbytes + ((size_t)(ok ? vv - 1u : 0u) * N + (ok ? row : 0)) * 32u + 16 * (ln & 1),
                   c.ring_l + cm_buf(band) + (uint32_t)(kBandBytes + kExtBytes + kSideBytes));
        }
    }
    __device__ __forceinline__ bool try_band(int band) /* (wave 3, after a memory wait) have all the others reported? */
    {
        if (band * kBandRows >= c.N) return true; /* (uniform) */
        const int ln = fresh(c.lane), words = __builtin_amdgcn_readfirstlane(cm_words_v);
        const uint32_t w = ln < words ? lds.src.cm_poll_l[band & 1][ln & 31] : kCmUsedBit;
        if (__ballot((w & kCmUsedBit) == 0u) != 0ull) return false;
        take_band(band, w);
        return true;
    }
    /* (wave 3) ... waiting for them — and for those of the band after the next (lanes 32 ..) as well: strip 0 then trails the
     * others by the four steps that asking without waiting needs, and stays there */
    __device__ __forceinline__ void listen_band(int band)
    {
        const int lane = c.lane;
        if (band * kBandRows >= c.N) return; /* (uniform) */
        const bool more = (band + 2) * kBandRows < c.N;
        const int words = __builtin_amdgcn_readfirstlane(cm_words_v);
        uint32_t w = 0u, spins = 0u;
        for (;;) {
            const int l = lane & 31;
            w = (l < words && (lane < 32 || more)) ? __hip_atomic_load(cm_pub() + ((size_t)(band + 2 * (lane >> 5)) * kCmMaxStrips + 1) * 2 + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                      : kCmUsedBit;
            if (__ballot((w & kCmUsedBit) == 0u) == 0ull) break;
            if (++spins > kCmSpins) { /* (never seen; the frame is redone the general way) and strip 0 stops listening: one
                                       * bounded wait per frame, not one per band (advisor, round 5) */
                failed |= 1u;
                cm_f &= ~(uint32_t)kCfListens;
                w = 0u;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
        take_band(band, w);
    }
    /* is column `col` of a return of row `row` where firing u's returns of that row lie? */
    __device__ __forceinline__ bool cm_regular(uint32_t col, int u, int row) const
    {
        const int d = mod_h((int)col - u - (int)lds.src.cm_base_l[row]); /* (col < H) */
        return d <= kColMaxDisp;
    }
    /* A band has arrived: the no-return records among the firings this strip owns (column 0, and not where the firing's
     * returns lie), both rows, for strip 0.  (Strip 0 finds its own in its window.) */
    __device__ __forceinline__ void report_band(int band)
    {
        const int r0 = band * kBandRows;
        const char *buf = &lds.ring[cm_buf(band)];
#pragma unroll
        for (int k = 0; k < kBandRows; ++k) {
            const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + (k * 2 + 1) * 4096 + c.tid * 16 + 4);
            const bool zero = cm_vf == 3u && r0 + k < c.N && rcw == (uint32_t)(r0 + k); /* (valid and counted here) row r0 + k, column 0 */
            if (__ballot(zero) == 0ull) continue; /* (wave-uniform: a sweep without no-return records pays two reads and a compare) */
            if (zero && !cm_regular(0u, cm_u, r0 + k)) atomicMax(&lds.src.cm_nr_l[k], cm_key >> kLocBits);
        }
    }
    /* Row rho's records -> idx[rho & 1], keyed by (firing + 1) << kLocBits | where the record sits: later firings are
     * later in the input, the larger key wins, as the reference's last writer does (BatchMultiBevGen.cpp:112-115).  Every
     * record this strip OWNS is checked: beam = position mod N, and its column is where its firing's returns lie, or out
     * of range (dropped by the scatter, :109-111), or 0 (a no-return record). */
    __device__ __forceinline__ void index_row_cm(int rho)
    {
        const int tid = c.tid, lane = c.lane, wv = c.wv, H = c.H, first_col = c.first_col, row_span = c.row_span;
        if (rho >= c.N) return;
        uint32_t *irow = lds.src.idx[rho & 1];
        const char *buf = &lds.ring[cm_buf(rho / kBandRows)];
        if constexpr (!kGen) { /* the plain sweep: column = firing + 0 .. kPlainDisp or out of range; keys are thread numbers (firings ascend with them) */
            {
                const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + ((rho & 1) * 2 + 1) * 4096 + tid * 16 + 4);
                const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
                const bool good = (row == (uint32_t)rho) & ((col >= (uint32_t)H) | ((col - (uint32_t)pl_firing) <= (uint32_t)kPlainDisp));
                failed |= (pl_valid & !good) ? 1u : 0u;
                consumed += (pl_valid & pl_own) ? 1u : 0u;
                const uint32_t off = col - (uint32_t)first_col;
                atomicMax(&irow[(pl_valid & (col < (uint32_t)H) & (off < (uint32_t)row_span)) ? off : (uint32_t)kStripThreads], (uint32_t)tid + 1u);
            }
            if ((c.strip == 0 && wv == 1) || (c.last_strip && wv == 2)) { /* wave-uniform */
                const bool flat = wv == 1;
                const int i = lane & (kPlainSide - 1);
                const int fr = flat ? H - kPlainSide + i : i;
                const int want_row = flat ? rho - 1 : rho;
                const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + kBandBytes + (flat ? 0 : kPlainSide * 32 * kBandRows) + i * 64 + (rho & 1) * 32 + 20);
                const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
                /* flat: columns H - 2, H - 1 of row rho - 1 at offsets 0, 1; wrap: columns 0, 1 of row rho at H - first_col + 0, 1 */
                const uint32_t off = flat ? col - (uint32_t)(H - 2) : (uint32_t)(H - first_col) + col;
                const bool ok = (lane < kPlainSide) & ((unsigned)fr < (unsigned)H) & (want_row >= 0) & (row == (uint32_t)want_row) &
                                (flat ? (col < (uint32_t)H) & (off < 2u) : (col < 2u) & (off < (uint32_t)kStripVirt));
                atomicMax(&irow[ok ? off : (uint32_t)kStripThreads], (uint32_t)(kStripThreads + (flat ? 0 : kPlainSide) + i) + 1u);
            }
            return;
        } else {
            {
                const int base = (int)lds.src.cm_base_l[rho]; /* (requested together with the record's word) */
                const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + ((rho & 1) * 2 + 1) * 4096 + tid * 16 + 4);
                const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
                const bool good = (row == (uint32_t)rho) && (col >= (uint32_t)H || col == 0u || mod_h((int)col - cm_u - base) <= kColMaxDisp);
                failed |= (cm_vf == 3u && !good) ? 1u : 0u;
                consumed += cm_vf == 3u ? 1u : 0u;
                const uint32_t off = col - (uint32_t)first_col;
                const bool here = (cm_vf & 1u) && row == (uint32_t)rho;
                atomicMax(&irow[(here & (col < (uint32_t)H) & (off < (uint32_t)row_span)) ? off : (uint32_t)kStripThreads], cm_key);
                if (cm_f & kCfBoth) { /* (uniform) columns 0, 1 once more, as the virtual columns H, H + 1 */
                    const uint32_t off2 = (uint32_t)(H - first_col) + col;
                    atomicMax(&irow[(here & (col < 2u) & (off2 < (uint32_t)kStripVirt)) ? off2 : (uint32_t)kStripThreads], cm_key);
                }
                if ((cm_f & kCfQuiet) && __ballot(cm_vf == 3u && rcw == (uint32_t)rho) != 0ull) { /* (wave-uniform, rare: a record of column 0)
                                                                                                 * a no-return record after all, in a frame whose strips do not talk? */
                    const bool stray = cm_vf == 3u && rcw == (uint32_t)rho && mod_h(-cm_u - base) > kColMaxDisp;
                    if (__ballot(stray) != 0ull) {
                        if (stray) atomicMax((uint32_t *)(uintptr_t)cm_pub_v + kCmPubWords + 2 * kCmMaxRows + rho, cm_key >> kLocBits);
                        failed |= kInfoCmStray;
                    }
                }
            }
            const int ln = fresh(lane);
            if ((cm_f & kCfExt) && ln < kCmExt) { /* (uniform per wave) the extra firings: never counted here */
                const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + kBandBytes + ln * 64 + (rho & 1) * 32 + 20);
                const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
                const uint32_t off = col - (uint32_t)first_col;
                atomicMax(&irow[((cm_ext_key != 0u) & (row == (uint32_t)rho) & (col < (uint32_t)H) & (off < (uint32_t)row_span)) ? off : (uint32_t)kStripThreads], cm_ext_key);
            }
            if (cm_f & (kCfFlat | kCfWrap)) { /* wave-uniform */
                const bool flat = (cm_f & kCfFlat) != 0u;
                const int e = ln & (kSideFirings - 1); /* entry of the side area */
                const int want_row = flat ? rho - 1 : rho;
                const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + kBandBytes + kExtBytes + e * 64 + (rho & 1) * 32 + 20);
                const uint32_t row = rcw & 0xffffu, col = rcw >> 16;
                /* flat: columns H - 2, H - 1 of row rho - 1 at offsets 0, 1; wrap: columns 0, 1 of row rho at H - first_col + 0, 1 */
                const uint32_t off = flat ? col - (uint32_t)(H - 2) : (uint32_t)(H - first_col) + col;
                const bool ok = (ln < kSideFirings) & (cm_side_key != 0u) & (want_row >= 0) & (row == (uint32_t)want_row) &
                                (flat ? (col < (uint32_t)H) & (off < 2u) : (col < 2u) & (off < (uint32_t)kStripVirt));
                atomicMax(&irow[ok ? off : (uint32_t)kStripThreads], cm_side_key);
            }
            if ((cm_f & kCfListens) && ln == 0) { /* the last no-return record of the row that another strip owns: column 0 = offset 2 */
                const uint32_t v = lds.src.cm_spec_l[(rho / kBandRows) & 1][rho & 1];
                const uint32_t rcw = *reinterpret_cast<const uint32_t *>(buf + kBandBytes + kExtBytes + kSideBytes + (rho & 1) * 32 + 20);
                if (v != 0u) {
                    if (rcw != (uint32_t)rho) failed |= 1u; /* (row rho, column 0: what its owner said it was) */
                    else atomicMax(&irow[2], (v << kLocBits) | kLocSpecial);
                }
            }
        }
    }

    /* the queue the row loop expects: band 0 (strip 0: the others' reports for it, and band 1's asked for) */
    __device__ __forceinline__ void prologue()
    {
        issue_band(0);
        if constexpr (kGen) {
            if (cm_f & kCfListens) {
                listen_band(0);
                ask_band(1); /* (looked at behind step 0's memory wait) */
            }
        }
    }
    /* a band's loads are the newest operations but the stores since: they have arrived when nothing is outstanding
     * (the stores of the step before are a step old, as for the other sources) */
    template <int I>
    __device__ __forceinline__ void arrive(const int r, u32x4 &, u32x4 & WALK_PHA_PARAMS)
    {
        if ((r % kBandRows) == 0) {
            wait_vm<0>();
            if constexpr (kGen) {
                if ((cm_f & kCfReports) && r < c.N) report_band(r / kBandRows);
            }
        }
        PHA(0);
        index_row_cm(r);
        PHA(1);
    }
    /* the column's owner follows its index entry to a record of the band: a thread's, an extra firing's, a side
     * window's, the special one */
    template <int I>
    __device__ __forceinline__ void take(const int r, u32x4 &cur_lo, u32x4 &cur_hi)
    {
        const int tid = c.tid, par = r & 1, N = c.N;
        const uint32_t e = lds.src.idx[par][tid];
        lds.src.idx[par][tid] = 0u;
        const char *buf = &lds.ring[cm_buf(r / kBandRows)];
        const uint32_t k = kGen ? e & ((1u << kLocBits) - 1u) : e - 1u; /* (the plain sweep: thread of the window, or kStripThreads + side firing) */
        const bool main = k < (uint32_t)kStripThreads;
        const uint32_t lo_at = main ? (uint32_t)((r & 1) * 2) * 4096u + k * 16u
                                    : (uint32_t)kBandBytes + (k - (uint32_t)kStripThreads) * 64u + (uint32_t)(r & 1) * 32u;
        const bool have = (e != 0u) & (r < N);
        cur_lo = *(have ? reinterpret_cast<const u32x4 *>(buf + lo_at) : &lds.zero16[0]);
        cur_hi = *(have ? reinterpret_cast<const u32x4 *>(buf + lo_at + (main ? 4096u : 16u)) : &lds.zero16[0]);
        if constexpr (kGen) {
            /* Column 0 can hold a no-return record of ANY firing.  Strip 0, which owns the column, hears of the other strips'
             * (listen_band) and says which firing's record it took; a strip whose wrap-around halo shows column 0 as virtual
             * column H sees only the firings of its side window: it remembers what it found there, and if column H - 2 falls
             * back on it (BatchMultiBevGen.cpp:146-149: the upper point's intensity is -1) says so: k_verdict compares. */
            if (r < N) {
                if ((cm_f & kCfFirst) && tid == 2) lds.src.cm_win0_l[r] = (uint16_t)(e >> kLocBits);
                if (c.last_strip && c.v == c.H) lds.src.cm_halo0_l[r & 1] = e >> kLocBits;
            }
            /* this strip's no-return records of the band that has just arrived, for strip 0: a word per row */
            if ((cm_f & kCfReports) && (r % kBandRows) == 0 && r < N && tid < kBandRows) {
                const uint32_t nr = lds.src.cm_nr_l[tid];
                lds.src.cm_nr_l[tid] = 0u;
                (void)nr;
#ifndef BEV_EXP_NO_REPORTS /* (developer build, scripts/cm_timeout_check.py: the reports never arrive — strip 0 must give up, once, and the frame be redone) */
                __hip_atomic_store(cm_pub() + ((size_t)(r / kBandRows) * kCmMaxStrips + c.strip) * 2 + tid, kCmUsedBit | nr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
            }
            if (cm_f & kCfListens) { /* (uniform) */
                if ((r % kBandRows) == 0) { /* after this step's memory wait: the reports asked for two steps ago, for the band two steps on;
                                             * and the next band's are asked for (a load asked for at an odd step was waited for half a
                                             * step later, by every wave at the barrier behind: strip 0 18 % slower) */
                    const int band = r / kBandRows + 1;
#ifdef BEV_CS_CLOCK
                    const long long t0_ = wall_clock64();
#endif
                    cm_waiting = try_band(band) ? -1 : band;
#ifdef BEV_CS_CLOCK
                    const long long t1_ = wall_clock64();
                    dbg_block_t += t1_ - t0_;
#endif
                    ask_band(band + 1);
#ifdef BEV_CS_CLOCK
                    dbg_try_t += wall_clock64() - t1_;
                    dbg_fail_n += cm_waiting >= 0 ? 1 : 0;
#endif
                } else if (cm_waiting >= 0) {
#ifdef BEV_CS_CLOCK
                    const long long t0_ = wall_clock64();
#endif
                    listen_band(cm_waiting);
#ifdef BEV_CS_CLOCK
                    dbg_block_t += wall_clock64() - t0_;
#endif
                }
            }
        }
    }
    /* every wave has passed this step's barrier: nobody reads the band before this one any more */
    template <int I>
    __device__ __forceinline__ void issue(const int r)
    {
        if ((r % kBandRows) == 0) issue_band(r / kBandRows + 1);
    }
    /* the 8 KiB behind the band buffers */
    template <int I>
    __device__ __forceinline__ int xpose() const { return 2 * kCmBuf; }
    /* general form: column H - 2 falls back on column 0 of row r - 1: which firing's record this strip took for it */
    __device__ __forceinline__ void upper_missing(const int r, const float up_i)
    {
        if constexpr (kGen) {
            if (c.last_strip && c.outcol && c.v == c.H - 2 && up_i == -1.0f) {
                cm_pub()[kCmPubWords + kCmMaxRows + (r - 1)] = kCmUsedBit | lds.src.cm_halo0_l[(r - 1) & 1];
                failed |= kInfoCmUsed;
            }
        }
    }
    /* general form, strip 0: which firing's record it put into column 0, per row */
    __device__ __forceinline__ void finish()
    {
        if constexpr (kGen) {
            if (cm_f & kCfFirst)
                for (int r = c.tid; r < c.N; r += kStripThreads) cm_pub()[kCmPubWords + r] = (uint32_t)lds.src.cm_win0_l[r];
        }
    }
#ifdef BEV_CS_CLOCK
    __device__ __forceinline__ void clk_print(int bid, int f WALK_PHA_PARAMS)
    {
        PHA_PRINT("walk_gather vmwait - barrier acquire writeout issue status rest", c.lane == 0 && bid == 100);
        PHA_PRINT("walk_cm_strip0 vmwait index barrier acquire writeout issue status rest", c.lane == 0 && c.strip == 0 && f == 12);
        if (c.lane == 0 && c.wv == 3 && c.strip == 0 && f == 12) printf("walk_cm_listen try_t %lld block_t %lld fails %d (x10 ns)\n", dbg_try_t, dbg_block_t, dbg_fail_n);
        PHA_PRINT("walk_cm_strip2 vmwait index barrier acquire writeout issue status rest", c.lane == 0 && c.strip == 2 && f == 12);
    }
#endif
};
template <>
struct WalkSource<kSrcColMajor> : FiringSource<false> {
    using FiringSource::FiringSource;
};
template <>
struct WalkSource<kSrcColMajorGen> : FiringSource<true> {
    using FiringSource::FiringSource;
};

} /* namespace bevk */

#endif /* BEV_WALK_FIRING_H */
