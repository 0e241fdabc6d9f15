/*
 * hostcheck.cpp — TEST HELPER (never shipped, never loaded by the product).
 *
 * Compiles csrc/bev_exact.h — the closed forms the HIP kernels evaluate per
 * slot — for the host and composes them the way the kernels do (max-index
 * winner table, phase-A closed form, slot-ordered candidates, per-cell
 * sequential sums, neighbour test, BEV codes, raster from codes).  The CPU
 * test-suite compares this composition with the sequential oracle, so a wrong
 * closed form is caught without a GPU.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/bev_mi355x.h"
#include "../../point-cloud-preprocessing-tools_amd/csrc/bev_exact.h"
#include "../../point-cloud-preprocessing-tools_amd/csrc/bev_libm.h"
#include "../../point-cloud-preprocessing-tools_amd/host/FileFormats.h"
#include "../../point-cloud-preprocessing-tools_amd/host/LabelStep.h"
#include "../../point-cloud-preprocessing-tools_amd/host/RegistrationChunks.h"

using namespace bevx;

namespace {
struct ArrayFetch {
    const bev_point_t *pts;
    XYZI operator()(long long i) const { return XYZI{pts[i].x, pts[i].y, pts[i].z, pts[i].intensity}; }
};
/* A COPY of raster_bands_for's loop (csrc/bev_raster.h is device code and is not compiled here) with its constants
 * (bev_internal.h: kRasterSplit, kRasterLdsCap = kSlotLdsBytes, kMaxStrips + kResolveParts + 2 tail words).
 * tests/test_raster_layout_cpu.py holds the sizes this admits against bev_multi_bytes of the product library. */
constexpr int kHcRasterSplit = 8, kHcRasterLdsCap = 32 * 1280, kHcRasterTailWords = 280 + 4 + 2;
int raster_bands_for_copy(int M)
{
    for (int bands = kHcRasterSplit; bands <= kBandMax; bands *= 2)
        if (M % bands == 0 && ((size_t)2 * (M / bands) * M + kHcRasterTailWords) * sizeof(uint32_t) <= (size_t)kHcRasterLdsCap) return bands;
    return 0;
}
/* what fill_geometry (bev_capi.hip) computes from the same two helpers; results do not depend on the band layout */
RasterParams raster_params(const bev_params_t *p)
{
    RasterParams rp;
    raster_scalars(p->max_range, p->interval, p->height_res, p->lidar_to_ground, p->n_layers, &rp);
    raster_band_layout(rp.mat_size, raster_bands_for_copy(rp.mat_size), &rp);
    return rp;
}
} // namespace

extern "C" {

void hc_angle(const float *dx, const float *dy, const float *dz, size_t n, uint8_t *out)
{
    for (size_t i = 0; i < n; ++i) out[i] = angle_is_ground(dx[i], dy[i], dz[i]) ? 1 : 0;
}

uint32_t hc_tan_threshold_bits(void) { return kTanThresholdBits; }

/* The reference's expression (BatchMultiBevGen.cpp:173-179, float overloads) on an
 * angle a = atan2f(...) that is already known. */
static inline bool ref_accepts_angle(float a)
{
    float angle = (float)((double)a * 180.0 / M_PI);
    return std::fabs(angle - 0.0f) <= 10.0f;
}

/* Re-derives, against the libm of THIS machine, the facts bev_exact.h relies on:
 *   out[0] = largest float bits a with ref_accepts_angle(a) (and the set is a prefix)
 *   out[1] = largest float bits q with ref_accepts_angle(atanf(q))
 *   out[2] = number of non-negative floats q (incl. +inf) where
 *            ref_accepts_angle(atanf(q)) != (q <= out[1])        (must be 0)
 *   out[3] = number of places where atanf decreases over the non-negative floats (must be 0)
 *   out[4] = number of non-negative floats a where ref_accepts_angle(a) != (a <= out[0]) (must be 0) */
void hc_derive_angle_threshold(uint64_t *out)
{
    uint32_t ta = 0;
    for (uint32_t u = 0; u <= 0x7f800000u; ++u) {
        if (ref_accepts_angle(bits_to_float(u))) ta = u; else break;
    }
    uint64_t bad_a = 0, bad_q = 0, nonmono = 0;
    uint32_t qs = 0;
#pragma omp parallel for reduction(+ : bad_a) schedule(static)
    for (int64_t u = 0; u <= 0x7f800000LL; ++u)
        if (ref_accepts_angle(bits_to_float((uint32_t)u)) != ((uint32_t)u <= ta)) ++bad_a;
    /* Q*: scan downwards from 1.0f (atan(1) = 45 deg is rejected) */
    for (uint32_t u = 0x3f800000u;; --u) {
        if (ref_accepts_angle(atanf(bits_to_float(u)))) { qs = u; break; }
        if (u == 0) break;
    }
#pragma omp parallel for reduction(+ : bad_q, nonmono) schedule(static)
    for (int64_t u = 0; u <= 0x7f800000LL; ++u) {
        const float a = atanf(bits_to_float((uint32_t)u));
        if (ref_accepts_angle(a) != ((uint32_t)u <= qs)) ++bad_q;
        if (u > 0 && a < atanf(bits_to_float((uint32_t)(u - 1)))) ++nonmono;
    }
    out[0] = ta; out[1] = qs; out[2] = bad_q; out[3] = nonmono; out[4] = bad_a;
}

/* Random + structured (dz, s) pairs around the threshold: the reference expression
 * with libm atan2f against angle_is_ground's ratio test.  Returns mismatches. */
uint64_t hc_angle_vs_libm(uint64_t n, uint64_t seed)
{
    uint64_t bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        uint64_t z = seed + 0x9e3779b97f4a7c15ULL * (uint64_t)(i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; z ^= z >> 31;
        uint64_t z2 = z * 0xd1b54a32d192ed03ULL + 0x2545f4914f6cdd1dULL;
        z2 = (z2 ^ (z2 >> 29)) * 0xbf58476d1ce4e5b9ULL; z2 ^= z2 >> 32;
        float dx, dy, dz;
        const int mode = (int)(z & 7);
        if (mode < 5) { /* near the threshold: dz = s * tan(10 deg) +- a few ulps */
            const int e = (int)((z >> 8) % 60) - 30;
            dx = std::ldexp(1.0f + (float)((z >> 16) & 0x7fffff) / 8388608.0f, e);
            dy = (mode & 1) ? 0.0f : dx * (float)((z >> 40) & 0xff) / 64.0f;
            const float s = std::sqrt(dx * dx + dy * dy);
            float t = (float)(0.17632698070846498 * (double)s);
            uint32_t ut; std::memcpy(&ut, &t, 4);
            ut += (uint32_t)((int)((z2 >> 3) % 33) - 16);
            std::memcpy(&dz, &ut, 4);
            if (z2 & 1) dz = -dz;
        } else if (mode < 7) { /* arbitrary bit patterns incl. denormals, inf, NaN */
            uint32_t a = (uint32_t)z2, b = (uint32_t)(z2 >> 32), c = (uint32_t)(z >> 32);
            std::memcpy(&dx, &a, 4); std::memcpy(&dy, &b, 4); std::memcpy(&dz, &c, 4);
        } else { /* plain small reals */
            dx = ((int)(z2 & 0xffff) - 32768) / 512.0f;
            dy = ((int)((z2 >> 16) & 0xffff) - 32768) / 512.0f;
            dz = ((int)((z2 >> 32) & 0xffff) - 32768) / 4096.0f;
        }
        const float horiz = std::sqrt(dx * dx + dy * dy);
        const float angle = (float)((double)std::atan2(dz, horiz) * 180.0 / M_PI); /* float overload = atan2f */
        const bool ref = std::fabs(angle - 0.0f) <= 10.0f;
        if (ref != angle_is_ground(dx, dy, dz)) ++bad;
    }
    return bad;
}

/* angle_is_ground_nodiv against angle_is_ground (the division form): n random bit patterns, n pairs of moderate
 * magnitude, and n pairs (a, s) with a within a few ulps of the cut M * s for s over 60 binades; returns mismatches */
uint64_t hc_angle_nodiv_check(uint64_t n)
{
    uint64_t bad = 0;
    const double mid = 0.5 * ((double)bits_to_float(kTanThresholdBits) + (double)bits_to_float(kTanThresholdBits + 1u));
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        uint64_t z = 0x243f6a8885a308d3ULL + 0x9e3779b97f4a7c15ULL * (uint64_t)(i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; z ^= z >> 31;
        uint64_t z2 = (z + 0x9e3779b97f4a7c15ULL); z2 = (z2 ^ (z2 >> 30)) * 0xbf58476d1ce4e5b9ULL; z2 ^= z2 >> 29;
        {   /* any bit patterns: dx, dy, dz */
            const float dx = bits_to_float((uint32_t)z), dy = bits_to_float((uint32_t)(z >> 32)), dz = bits_to_float((uint32_t)z2);
            if (angle_is_ground(dx, dy, dz) != angle_is_ground_nodiv(dx, dy, dz)) ++bad;
            if (angle_is_ground(dx, 0.0f, dz) != angle_is_ground_nodiv(dx, 0.0f, dz)) ++bad;
        }
        {   /* the walk's magnitudes */
            const float dx = ((int)((z >> 8) & 0xfffff) - 524288) / 4096.0f, dy = ((int)((z >> 28) & 0xfffff) - 524288) / 4096.0f;
            const float dz = ((int)(z2 & 0xfffff) - 524288) / 16384.0f;
            if (angle_is_ground(dx, dy, dz) != angle_is_ground_nodiv(dx, dy, dz)) ++bad;
        }
        {   /* straddling the cut: s = dx exactly (dy = 0), dz = fl32(M * s) +- k ulps */
            const float sc = std::ldexp(1.0f, (int)((z >> 4) % 60) - 30);
            const float s = sc * (1.0f + (float)((z >> 16) & 0x7fffff) / 8388608.0f);
            float a = (float)(mid * (double)s);
            int k = (int)((z2 >> 3) % 9) - 4;
            for (; k > 0; --k) a = std::nextafter(a, INFINITY);
            for (; k < 0; ++k) a = std::nextafter(a, -INFINITY);
            if (angle_is_ground(s, 0.0f, a) != angle_is_ground_nodiv(s, 0.0f, a)) ++bad;
            if (angle_is_ground(0.0f, -s, -a) != angle_is_ground_nodiv(0.0f, -s, -a)) ++bad;
        }
    }
    const float sp[] = {0.0f, -0.0f, 1.0f, -1.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 3.4e38f, -3.4e38f, 1e-38f, 2.0f, 0.5f, 0.17632698f};
    for (float x : sp) for (float y : sp) for (float zz : sp)
        if (angle_is_ground(x, y, zz) != angle_is_ground_nodiv(x, y, zz)) ++bad;
    return bad;
}

/* count_advance against the reference's step-by-step count: from 0.01f, every n up to n_max in one go, and chains of
 * random run lengths (the state after one call is the start of the next); returns mismatches */
uint64_t hc_count_advance_check(uint32_t n_max)
{
    uint64_t bad = 0;
    float seq = 0.01f;
    for (uint32_t n = 1; n <= n_max; ++n) {
        seq = seq + 1.0f;
        if (float_bits(count_advance(0.01f, n)) != float_bits(seq)) ++bad;
    }
    uint64_t z = 88172645463325252ULL;
    for (int chain = 0; chain < 200; ++chain) {
        float a = 0.01f, b = 0.01f;
        uint32_t total = 0;
        while (total < n_max) {
            z ^= z << 13; z ^= z >> 7; z ^= z << 17;
            const uint32_t run = 1u + (uint32_t)(z % ((chain & 1) ? 700u : 9u));
            a = count_advance(a, run);
            for (uint32_t k = 0; k < run; ++k) b = b + 1.0f;
            total += run;
            if (float_bits(a) != float_bits(b)) { ++bad; break; }
        }
    }
    return bad;
}

int hc_ground_cell(float x, float y) { return ground_cell(x, y); }

/* small_div against the division for every 0 <= x < 512, 1 <= d <= 512, and raster_band_of_nodiv against raster_band_of
 * for every image size fill_geometry lays out (M a multiple of 16 up to 512 that raster_bands_for admits: 8 to 64 coarse
 * bands, the middle cut twice finer or not — raster_band_layout, the helper fill_geometry itself calls): the number of
 * mismatches */
uint64_t hc_small_div_check(void)
{
    uint64_t bad = 0;
    for (int d = 1; d <= 512; ++d) {
        const uint32_t m = small_div_magic(d);
        for (int x = 0; x < 512; ++x) bad += small_div(x, m) != x / d;
    }
    int layouts = 0;
    for (int M = 16; M <= 512; M += 16) {
        const int u = raster_bands_for_copy(M);
        if (!u) continue;
        RasterParams rp{};
        rp.mat_size = M;
        raster_band_layout(M, u, &rp);
        ++layouts;
        for (int x = 0; x < M; ++x) bad += raster_band_of_nodiv(x, rp) != raster_band_of(x, rp);
    }
    return bad + (layouts == 0);
}

/* The band layout of image size M as the library computes it.  out[0..7] = u (0: M is refused), bands, coarse, fine, z0,
 * z1, LDS bytes of a band's workgroup (raster_lds_bytes), violations.  A violation is any of: more than kBandMax bands;
 * z0 not a multiple of coarse or z1 - z0 not a multiple of fine; fine above coarse (the LDS planes are sized for coarse
 * rows); the bands, walked with raster_band_x0 / raster_band_rows, not covering every row of [0, M) exactly once in
 * order; raster_band_of or raster_band_of_nodiv of a row differing from the band that covers it; the planes above the
 * LDS cap.  Returns the violations. */
int hc_band_layout(int M, int *out)
{
    const int u = raster_bands_for_copy(M);
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (!u) return 0;
    RasterParams rp{};
    rp.mat_size = M;
    raster_band_layout(M, u, &rp);
    int bad = 0;
    bad += rp.bands > kBandMax || rp.bands < 1;
    bad += rp.coarse < 1 || rp.fine < 1 || rp.fine > rp.coarse;
    bad += rp.z0 % rp.coarse != 0 || (rp.z1 - rp.z0) % rp.fine != 0 || (M - rp.z1) % rp.coarse != 0;
    int next = 0;
    for (int b = 0; b < rp.bands; ++b) {
        const int x0 = raster_band_x0(b, rp), rows = raster_band_rows(b, rp);
        bad += x0 != next || rows < 1;
        for (int x = x0; x < x0 + rows && x < M; ++x) bad += raster_band_of(x, rp) != b || raster_band_of_nodiv(x, rp) != b;
        next = x0 + rows;
    }
    bad += next != M;
    const size_t lds = ((size_t)2 * rp.coarse * M + kHcRasterTailWords) * sizeof(uint32_t);
    bad += lds > (size_t)kHcRasterLdsCap;
    out[0] = u; out[1] = rp.bands; out[2] = rp.coarse; out[3] = rp.fine; out[4] = rp.z0; out[5] = rp.z1; out[6] = (int)lds; out[7] = bad;
    return bad;
}

/* exact_reciprocal (bev_exact.h): for every power of two v it accepts, x / v == x * (1 / v) bit for bit over `samples`
 * pseudo-random bit patterns of x per v plus the extremes; everything that is not a power of two is refused.
 * Returns the number of violations. */
uint64_t hc_exact_reciprocal_check(uint64_t samples)
{
    uint64_t bad = 0;
    for (uint32_t e = 0; e < 256; ++e) {
        const float v = bits_to_float(e << 23);
        const float inv = exact_reciprocal(v);
        if (e == 0 || e >= 253) { bad += inv != 0.0f; continue; }
        if (inv == 0.0f || v * inv != 1.0f) { ++bad; continue; }
        uint64_t z = 0x9e3779b97f4a7c15ULL * (e + 1);
        for (uint64_t k = 0; k < samples + 8; ++k) {
            z += 0x9e3779b97f4a7c15ULL;
            uint64_t h = z; h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ULL; h = (h ^ (h >> 27)) * 0x94d049bb133111ebULL; h ^= h >> 31;
            static const uint32_t ext[8] = {0u, 0x80000000u, 1u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u};
            const float x = bits_to_float(k < 8 ? ext[k] : (uint32_t)h);
            const float a = x / v, b = x * inv;
            uint32_t ua, ub; std::memcpy(&ua, &a, 4); std::memcpy(&ub, &b, 4);
            if (ua != ub && !(a != a && b != b)) ++bad;
        }
    }
    const float no[] = {3.0f, 0.3f, -1.0f, -0.5f, 1.5f, 0.0f, 1e-40f, 6.0f};
    for (float v : no) bad += exact_reciprocal(v) != 0.0f;
    return bad;
}

/* candidate keys decoded / escaped by hc_process_frame since the last reset (test statistics) */
static uint64_t g_key_decodes = 0, g_key_escapes = 0;
void hc_key_stats(uint64_t *decodes, uint64_t *escapes, int reset)
{
    *decodes = g_key_decodes;
    *escapes = g_key_escapes;
    if (reset) g_key_decodes = g_key_escapes = 0;
}
/* candidate_key / candidate_code round trip on one point; returns 1 if the key reproduces bev_code (or escapes /
 * flags "no code" correctly), 0 otherwise */
int hc_key_roundtrip(const bev_params_t *p, float x, float y, float z, int label)
{
    const RasterParams rp = raster_params(p);
    const uint32_t code = bev_code(x, y, z, label, rp);
    const uint32_t key = candidate_key(ground_cell(x, y), 17, true, code, label, rp);
    if ((key & kKeyCellMask) != (uint32_t)ground_cell(x, y) || ((key >> kKeyColShift) & 0xffu) != 17u || !(key & kKeyPredBit)) return 0;
    if (((key & kKeyLabelM2Bit) != 0u) != (label == -2)) return 0;
    if (code == kSkip) return (key & kKeyNoCodeBit) ? 1 : 0;
    if (key & kKeyNoCodeBit) return 0;
    if (candidate_key_escapes(key)) return 2;
    return candidate_code(key, z, rp) == code ? 1 : 0;
}

uint32_t hc_bev_code(const bev_params_t *p, float x, float y, float z, int label)
{
    return bev_code(x, y, z, label, raster_params(p));
}

/* Exhaustive equivalence of the float-only forms in bev_exact.h with the reference's literal mixed
 * float/double expressions, over all 2^32 float bit patterns.  out[k] = number of mismatches:
 *   0: x + 75.0f            vs (float)((double)x + 75.0)         (bit patterns compared, NaN == NaN)
 *   1: floor_half_to_int(n) vs cvttsd2si(floor((double)n / 2.0))
 *   2: round_half_up_bin(v) vs cvttsd2si(round((double)v + 0.5))  (compared after mapping out-of-[0,4096) to -1)
 *   3: height_times4(t)     vs cvttsd2si((double)t * 4.0)
 *   4: d >= 0.3f            vs (double)d > 0.30
 *   5: bin_in_range(v, M)   vs round_half_up_bin(v) in [0, M), M = 2, 112, 224, 448, 512, 4096
 *   6: bin_of_shifted(p + R scaled by the interval, M) vs bin_in_range of the same value, for every coordinate p and a
 *      set of (MAX_RANGE, interval) from the smallest image validate_params admits (M = 16) to the largest, powers of
 *      two and not: the sum of two floats is never a tiny negative number */
void hc_exhaustive_exact_forms(uint64_t *out)
{
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0, m6 = 0;
    static const float kShift[][2] = {{112.0f, 1.0f}, {8.0f, 1.0f}, {50.0f, 0.25f}, {80.0f, 0.5f}, {100.0f, 0.4f}, {2048.0f, 8.0f}, {3.0f, 0.375f}};
#pragma omp parallel for reduction(+ : m0, m1, m2, m3, m4, m5, m6) schedule(static)
    for (int64_t u = 0; u <= 0xffffffffLL; ++u) {
        const float f = bits_to_float((uint32_t)u);
        {
            const float a = f + 75.0f, b = (float)((double)f + 75.0);
            uint32_t ua, ub; std::memcpy(&ua, &a, 4); std::memcpy(&ub, &b, 4);
            if (ua != ub && !(a != a && b != b)) ++m0;
            const float a2 = f + 50.0f, b2 = (float)((double)f + 50.0);
            std::memcpy(&ua, &a2, 4); std::memcpy(&ub, &b2, 4);
            if (ua != ub && !(a2 != a2 && b2 != b2)) ++m0;
        }
        if (floor_half_to_int(f) != cvtt_f64(std::floor((double)f / 2.0))) ++m1;
        {
            int a = round_half_up_bin(f), b = cvtt_f64(std::round((double)f + 0.5));
            if (a < 0 || a >= 4096) a = -1;
            if (b < 0 || b >= 4096) b = -1;
            if (a != b) ++m2;
        }
        if (height_times4(f) != cvtt_f64((double)f * 4.0)) ++m3;
        if ((f >= 0.3f) != ((double)f > 0.30)) ++m4;
        {
            const int full = round_half_up_bin(f);
            for (int M : {2, 112, 224, 448, 512, 4096}) {
                int b = -7;
                const bool in = bin_in_range(f, M, &b);
                const bool want = full >= 0 && full < M;
                if (in != want || (in && b != full)) ++m5;
            }
        }
        for (const auto &ri : kShift) {
            const float inv = exact_reciprocal(ri[1]);
            const float sh = f + ri[0];
            const float v = inv != 0.0f ? sh * inv : sh / ri[1];
            const int M = cvtt_f32((ri[0] * 2.0f) / ri[1]);
            int a = -7, b = -9;
            const bool ia = bin_in_range(v, M, &a), ib = bin_of_shifted(v, M, &b);
            if (ia != ib || (ia && a != b)) ++m6;
        }
    }
    out[0] = m0; out[1] = m1; out[2] = m2; out[3] = m3; out[4] = m4; out[5] = m5; out[6] = m6;
}

/* bev_libm.h against the host libm: out[0] = atanf mismatches over ALL 2^32 floats,
 * out[1] = atan2f mismatches over n random / structured pairs + special values (NaN == NaN). */
void hc_libm_vs_host(uint64_t n, uint64_t *out)
{
    uint64_t b0 = 0, b1 = 0;
#pragma omp parallel for reduction(+ : b0) schedule(static)
    for (int64_t u = 0; u <= 0xffffffffLL; ++u) {
        const float x = bits_to_float((uint32_t)u);
        const float a = atanf(x), b = fd_atanf(x);
        if (float_bits(a) != float_bits(b) && !(a != a && b != b)) ++b0;
    }
#pragma omp parallel for reduction(+ : b1) schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        uint64_t z = 0x243f6a8885a308d3ULL + 0x9e3779b97f4a7c15ULL * (uint64_t)(i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; z ^= z >> 31;
        uint64_t z2 = (z + 0x9e3779b97f4a7c15ULL); z2 = (z2 ^ (z2 >> 30)) * 0xbf58476d1ce4e5b9ULL; z2 ^= z2 >> 29;
        float y, x;
        switch (z & 3) {
        case 0: y = bits_to_float((uint32_t)(z >> 32)); x = bits_to_float((uint32_t)z2); break; /* any bit patterns */
        case 1: y = ((int)((z >> 8) & 0xfffff) - 524288) / 1024.0f; x = ((int)((z >> 28) & 0xfffff) - 524288) / 1024.0f; break;
        default: {
            const float sc = std::ldexp(1.0f, (int)((z >> 4) % 80) - 40);
            y = sc * ((int)((z >> 16) & 0xffff) - 32768) / 777.0f;
            x = ((int)((z >> 32) & 0xffff) - 32768) / 333.0f / sc;
        }
        }
        const float a = atan2f(y, x), b = fd_atan2f(y, x);
        if (float_bits(a) != float_bits(b) && !(a != a && b != b)) ++b1;
    }
    const float sp[] = {0.0f, -0.0f, 1.0f, -1.0f, INFINITY, -INFINITY, NAN, 1e-45f, -1e-45f, 3.4e38f, -3.4e38f, 1e-38f, 2.0f, 0.5f};
    for (float yy : sp)
        for (float xx : sp) {
            const float a = atan2f(yy, xx), b = fd_atan2f(yy, xx);
            if (float_bits(a) != float_bits(b) && !(a != a && b != b)) ++b1;
        }
    out[0] = b0; out[1] = b1;
}

/* the projection helpers of bev_libm.h on the host: kind 0 MulRan (interleaved), 1 Oxford (planes) */
void hc_project(int kind, const float *xyzi, uint32_t n, bev_point_t *out)
{
    for (uint32_t k = 0; k < n; ++k) {
        bev_point_t p;
        memset(&p, 0, sizeof p);
        if (kind == 0) {
            p.x = xyzi[4 * k]; p.y = xyzi[4 * k + 1]; p.z = xyzi[4 * k + 2]; p.intensity = xyzi[4 * k + 3];
            project_mulran(k, p.x, p.y, p.row, p.col);
        } else {
            p.x = -xyzi[k]; p.y = xyzi[(size_t)n + k]; p.z = -xyzi[2 * (size_t)n + k]; p.intensity = xyzi[3 * (size_t)n + k];
            project_oxford(p.x, p.y, p.z, p.row, p.col);
        }
        p.label = -2;
        out[k] = p;
    }
}


/* KITTI projection decomposed like the kernels k_kitti_* (crossing lists per block of 256 points, chain of
 * accepted crossings, ring by counting links, max-index winner per slot).  out: 64 * 2083 points. */
void hc_project_kitti(const float *xyzi, uint32_t n, bev_point_t *out)
{
    const size_t S = (size_t)kKittiRows * kKittiCols;
    memset(out, 0, S * sizeof *out);
    if (n == 0) return;
    const uint32_t nblocks = (n + kKittiBlock - 1u) / kKittiBlock;
    std::vector<float> az(n);
    std::vector<int32_t> col(n);
    std::vector<uint32_t> cnt(nblocks, 0), pos((size_t)nblocks * kKittiListCap);
    for (uint32_t i = 0; i < n; ++i) {
        az[i] = kitti_azimuth(xyzi[4 * (size_t)i], xyzi[4 * (size_t)i + 1]);
        col[i] = kitti_col(az[i]);
        if (i >= 1 && kitti_crossing(az[i - 1], az[i])) {
            const uint32_t b = i / kKittiBlock;
            pos[(size_t)b * kKittiListCap + cnt[b]++] = i;
        }
    }
    const int ring0 = az[0] > 0.0f ? 0 : -1;
    const uint32_t ring_min = kitti_ring_min();
    uint32_t link[kKittiMaxLinks], links = 0, last = 1;
    int ring = ring0;
    while (ring < kKittiRows && links < (uint32_t)kKittiMaxLinks) {
        const uint64_t target = ring == -1 ? 1ull : (uint64_t)last + ring_min;
        if (target >= n) break;
        uint32_t found = 0;
        const uint32_t b = (uint32_t)(target / kKittiBlock);
        for (uint32_t k = 0; k < cnt[b] && !found; ++k)
            if (pos[(size_t)b * kKittiListCap + k] >= target) found = pos[(size_t)b * kKittiListCap + k];
        for (uint32_t bb = b + 1; bb < nblocks && !found; ++bb)
            if (cnt[bb] > 0) found = pos[(size_t)bb * kKittiListCap];
        if (!found) break;
        ring = ring == -1 ? 0 : ring + 1;
        last = found;
        link[links++] = found;
    }
    std::vector<uint32_t> winner(S, 0);
    for (uint32_t i = 1; i < n; ++i) {
        const int r = kitti_ring_of(i, ring0, link, links);
        if (r >= 0 && r < kKittiRows && col[i] >= 0) {
            uint32_t &w = winner[(size_t)r * kKittiCols + col[i]];
            w = std::max(w, i + 1u);
        }
    }
    for (size_t s2 = 0; s2 < S; ++s2) {
        if (!winner[s2]) continue;
        const size_t i = winner[s2] - 1u;
        bev_point_t p;
        memset(&p, 0, sizeof p);
        p.x = xyzi[4 * i]; p.y = xyzi[4 * i + 1]; p.z = xyzi[4 * i + 2];
        p.intensity = -1.0f;
        p.row = (uint16_t)(s2 / kKittiCols);
        p.col = (uint16_t)(s2 % kKittiCols);
        p.label = -2;
        out[s2] = p;
    }
}

void hc_kitti_ring_min(uint32_t *out) { out[0] = kitti_ring_min(); }

/* host/LabelStep.cpp (row N1) for the CPU tests: positions in, major-frame indices / soft labels out */
static std::vector<Pose6f> poses_of(const float *xyz, uint32_t n)
{
    std::vector<Pose6f> p(n);
    for (uint32_t i = 0; i < n; ++i) {
        p[i] = Pose6f{};
        p[i].x = xyz[3 * i]; p[i].y = xyz[3 * i + 1]; p[i].z = xyz[3 * i + 2];
    }
    return p;
}
void hc_knn(const float *pts, uint32_t n, const float *q, uint32_t k, uint64_t *idx, float *d2)
{
    std::vector<std::vector<float>> set(n, std::vector<float>(3));
    for (uint32_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) set[i][d] = pts[3 * i + d];
    std::vector<size_t> ii;
    std::vector<float> dd;
    nearestPositions(set, std::vector<float>{q[0], q[1], q[2]}, k, ii, dd);
    for (uint32_t j = 0; j < k; ++j) { idx[j] = ii[j]; d2[j] = dd[j]; }
}
uint32_t hc_select_major_frames(const float *xyz, uint32_t n, int32_t *out)
{
    auto poses = poses_of(xyz, n);
    const std::vector<int32_t> major = selectMajorFrames(poses);
    for (size_t i = 0; i < major.size(); ++i) out[i] = major[i];
    return (uint32_t)major.size();
}
void hc_keyframe_labels(const float *xyz, uint32_t n, const int32_t *major, uint32_t m, float *out /* n * m */)
{
    auto poses = poses_of(xyz, n);
    std::vector<int32_t> mj(major, major + m);
    const std::vector<LabelType> labels = getKeyFrameLabel(poses, mj);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < m; ++j) out[(size_t)i * m + j] = labels[i][j];
}

/* Whole frame, composed like the kernels. gm_phase_a / gm_final / avg may be NULL. */
void hc_process_frame(const bev_params_t *p, const bev_point_t *in, uint32_t n_in, bev_point_t *ordered,
                      int8_t *gm_phase_a, int8_t *gm_final, float *avg_out, uint8_t *multi, uint8_t *single)
{
    const int N = p->n_scan, H = p->horizon_scan, G = p->ground_upper_scan;
    const size_t S = (size_t)N * H;
    const RasterParams rp = raster_params(p);
    const int M = rp.mat_size, L = rp.n_layers;

    /* order_scan: max (index + 1) per slot */
    std::vector<uint32_t> winner(S, 0u);
    for (uint32_t i = 0; i < n_in; ++i) {
        const uint32_t row = in[i].row, col = in[i].col;
        if (row >= (uint32_t)N || col >= (uint32_t)H) continue;
        uint32_t &w = winner[(size_t)row * H + col];
        if (i + 1 > w) w = i + 1;
    }
    for (size_t s = 0; s < S; ++s) {
        if (winner[s]) ordered[s] = in[winner[s] - 1];
        else memset(&ordered[s], 0, sizeof(bev_point_t));
    }

    /* gather_ground: phase-A closed form, codes, candidates in slot order */
    ArrayFetch fetch{ordered};
    std::vector<int8_t> g(S);
    std::vector<uint32_t> codes(S);
    struct Cand { uint32_t slot; float z; uint32_t key; int16_t label; };
    std::vector<Cand> cands;
    for (size_t s = 0; s < S; ++s) {
        const int row = (int)(s / H), col = (int)(s % H);
        const XYZI self{ordered[s].x, ordered[s].y, ordered[s].z, ordered[s].intensity};
        g[s] = (int8_t)phase_a_ground(row, col, N, H, G, self, fetch);
        codes[s] = bev_code(self.x, self.y, self.z, ordered[s].label, rp);
    }
    if (gm_phase_a) memcpy(gm_phase_a, g.data(), S);
    for (size_t s = 0; s < S; ++s) {
        if (g[s] != 1) continue;
        /* what the walk hands on per candidate: height + key (bev_exact.h); the column offset is not modelled here */
        cands.push_back(Cand{(uint32_t)s, ordered[s].z,
                             candidate_key(ground_cell(ordered[s].x, ordered[s].y), (int)(s % 252), false, codes[s],
                                           (int)ordered[s].label, rp),
                             ordered[s].label});
        codes[s] = kSkip;
        ordered[s].label = 0;
    }

    /* cell_sums: sequential float sums per cell in candidate (= slot) order */
    std::vector<float> sum(kGridCells, 0.0f), cnt(kGridCells, 0.01f), avg(kGridCells);
    for (const Cand &c : cands) {
        const int cell = (int)(c.key & kKeyCellMask);
        sum[cell] += c.z;
        cnt[cell] = cnt[cell] + 1.0f;
    }
    for (int k = 0; k < kGridCells; ++k) avg[k] = sum[k] / cnt[k];
    if (avg_out) memcpy(avg_out, avg.data(), sizeof(float) * kGridCells);

    /* ground_resolve */
    for (const Cand &c : cands) {
        if (above_neighbour_ground(c.z, (int)(c.key & kKeyCellMask), avg.data())) {
            ordered[c.slot].label = c.label;
            /* the code comes back from key + height, as in k_ground_resolve */
            if (c.key & kKeyNoCodeBit) codes[c.slot] = kSkip;
            else if (candidate_key_escapes(c.key))
                codes[c.slot] = bev_code(ordered[c.slot].x, ordered[c.slot].y, ordered[c.slot].z, 1, rp);
            else { codes[c.slot] = candidate_code(c.key, c.z, rp); ++g_key_decodes; }
            if (candidate_key_escapes(c.key)) ++g_key_escapes;
        }
    }
    /* ground_mat final */
    if (gm_final) {
        for (size_t s = 0; s < S; ++s) {
            const int cell = ground_cell(ordered[s].x, ordered[s].y);
            gm_final[s] = above_neighbour_ground(ordered[s].z, cell, avg.data()) ? (int8_t)0 : g[s];
        }
    }
    /* raster from codes */
    if (multi) memset(multi, 0, (size_t)L * M * M);
    if (single) memset(single, 0, (size_t)M * M);
    for (size_t s = 0; s < S; ++s) {
        const uint32_t c = codes[s];
        if (c == kSkip) continue;
        const int x = code_x(c), y = code_y(c);
        if (single) {
            uint8_t &h = single[(size_t)x * M + y];
            if (h < code_h(c)) h = (uint8_t)code_h(c);
        }
        if (multi && code_layer(c) != kNoLayer) multi[((size_t)code_layer(c) * M + x) * M + y] = 255;
    }
}

/* ---- host/FileFormats.cpp: the on-disk formats of the CLI (PCD in / out, PNG, CSV) ---- */
int hc_pcd_load(const char *path, bev_point_t *out, size_t cap, size_t *n, uint32_t *width, uint32_t *height)
{
    pcl::PointCloud<pcl::PointXYZIRCT> cloud;
    const int rc = bevio::loadPCDFile(path, cloud);
    *n = cloud.points.size();
    *width = cloud.width;
    *height = cloud.height;
    if (rc == 0 && out && !cloud.points.empty())
        std::memcpy(out, cloud.points.data(), std::min(cap, cloud.points.size()) * sizeof(bev_point_t));
    return rc;
}
int hc_pcd_save(const char *path, const bev_point_t *pts, size_t n)
{
    pcl::PointCloud<pcl::PointXYZIRCT> cloud;
    cloud.resize(n);
    if (n) std::memcpy(cloud.points.data(), pts, n * sizeof(bev_point_t));
    return bevio::savePCDFileBinary(path, cloud);
}
int hc_png_write(const char *path, const uint8_t *pixels, int rows, int cols)
{
    return bevio::writePngGray8(path, pixels, rows, cols) ? 0 : -1;
}
size_t hc_csv_u8(const uint8_t *pixels, int rows, int cols, char *out, size_t cap)
{
    const std::string s = bevio::formatCsvU8(pixels, rows, cols);
    if (out && cap) std::memcpy(out, s.data(), std::min(cap, s.size()));
    return s.size();
}

/* ---- host/RegistrationChunks.h: the chunk of the registration tools that starts at match m0 ---- */
/* counts[0..2] = m1, files, entries.  files has room for `limit` numbers, out_matches for n - m0 matches, map_offs for one more,
 * entry_frame for (n - m0) * (2 * half + 1) entries; without maps the last two are not written */
void hc_plan_chunk(const bev_match_t *matches, uint64_t n, uint64_t m0, int64_t half, int64_t lo, int64_t hi, int64_t limit, int maps,
                   uint64_t *counts, int64_t *files, bev_match_t *out_matches, uint64_t *map_offs, int32_t *entry_frame)
{
    const regchain::Chunk c = regchain::planChunk(matches, (size_t)n, (size_t)m0, (long)half, (long)lo, (long)hi, (long)limit, maps != 0);
    counts[0] = c.m1;
    counts[1] = c.files.size();
    counts[2] = c.entry_frame.size();
    std::copy(c.files.begin(), c.files.end(), files);
    std::copy(c.matches.begin(), c.matches.end(), out_matches);
    std::copy(c.map_offs.begin(), c.map_offs.end(), map_offs);
    std::copy(c.entry_frame.begin(), c.entry_frame.end(), entry_frame);
}

} /* extern "C" */
