/*
 * bev_place_exact.h — the arithmetic of place retrieval, written once for the HIP kernels (bev_place.h), the
 * host side of the C ABI (bev_capi_place.hip) and the sequential checker of the tests (tests/place/place_oracle.c): the
 * polar cell of a point, its height code, a column's unit values, the comparison of two scores, the distance and the yaw
 * guess of a shift.  bev_exact.h's rules hold: only correctly rounded IEEE operations, contraction off, fd_atan2f for the
 * azimuth (bev_libm.h) — every function gives the same bits on gfx950 and on x86-64.
 *
 * A descriptor is n_rings x n_sectors bytes, ring-major.  Ring k holds edge2[k] <= r2 < edge2[k + 1] with r2 = x * x + y * y
 * in float and edge2[k] = (float)(((double)max_range * k / n_rings)^2); sector s grows counter-clockwise from azimuth 0.
 */
#ifndef BEV_PLACE_EXACT_H
#define BEV_PLACE_EXACT_H

#include "bev_libm.h"

namespace bevx {

constexpr int kPlaceMinRings = 4, kPlaceMaxRings = 32, kPlaceMinSectors = 8, kPlaceMaxSectors = 64;
constexpr int kPlaceMaxTopK = 64;
constexpr int kPlaceUnit = 127;               /* the length of a non-empty unit column, and the largest height code */
constexpr double kPlaceUnit2 = 16129.0;       /* 127 * 127: the score of two equal one-ring columns */
constexpr double kPlaceNoDistance = 2.0;      /* the distance of a pair without a common non-empty column */

/* the admitted parameters (include/bev_mi355x.h: bev_place_params_t) */
BEVX_HD bool place_params_ok(int n_rings, int n_sectors, float max_range, int skip_label0)
{
    return n_rings >= kPlaceMinRings && n_rings <= kPlaceMaxRings && n_sectors >= kPlaceMinSectors &&
           n_sectors <= kPlaceMaxSectors && max_range > 0.0f && max_range <= 3.402823466e+38f && /* (false for NaN, inf) */
           (skip_label0 == 0 || skip_label0 == 1);
}
/* the n_rings + 1 squared ring edges */
BEVX_HD void place_edges(int n_rings, float max_range, float *edge2)
{
    for (int k = 0; k <= n_rings; ++k) {
        const double e = (double)max_range * (double)k / (double)n_rings;
        edge2[k] = (float)(e * e);
    }
}
BEVX_HD float place_r2(float x, float y) { return x * x + y * y; }
/* the ring of r2, -1 where the point does not contribute: 0 < r2 < edge2[n_rings] fails for the origin's no-return records,
 * NaN and inf.  A binary search of ceil(log2(32)) = 5 fixed steps over the table (edge2[0] = 0 <= r2 holds on entry). */
BEVX_HD int place_ring(const float *edge2, int n_rings, float r2)
{
    if (!(r2 > 0.0f && r2 < edge2[n_rings])) return -1;
    int lo = 0, hi = n_rings;
    for (int step = 0; step < 5; ++step) {
        const int mid = (lo + hi) >> 1;
        if (hi - lo > 1) {
            if (edge2[mid] <= r2) lo = mid;
            else hi = mid;
        }
    }
    return lo;
}
/* the sector of a contributing point (x, y finite, not both 0): a = degrees_of(fd_atan2f(y, x)), + 360.0f where negative,
 * then floorf(a * (float)n_sectors / 360.0f) in float, clamped to n_sectors - 1 (a tiny negative angle + 360.0f is 360.0f) */
BEVX_HD int place_sector(float x, float y, int n_sectors)
{
    float a = degrees_of(fd_atan2f(y, x));
    if (a < 0.0f) a = a + 360.0f;
    const int s = (int)floorf(a * (float)n_sectors / 360.0f);
    return s < 0 ? 0 : (s > n_sectors - 1 ? n_sectors - 1 : s);
}
/* the single-layer BEV's height code of a (moved) z, saturated at 127 */
BEVX_HD int place_value(float z, float lidar_to_ground)
{
    const int h = height_times4(z + lidar_to_ground);
    return h < 0 ? 0 : (h > kPlaceUnit ? kPlaceUnit : h);
}
/* ring * n_sectors + sector of a point, -1 where it does not contribute */
BEVX_HD int place_cell(const float *edge2, int n_rings, int n_sectors, float x, float y, int label, int skip_label0)
{
    const int ring = place_ring(edge2, n_rings, place_r2(x, y));
    if (ring < 0 || (skip_label0 && label == 0)) return -1;
    return ring * n_sectors + place_sector(x, y, n_sectors);
}
/* a value of a column whose squared values sum to n2 > 0, scaled to a column of length 127 */
BEVX_HD int place_unit(int v, int n2) { return (int)(127.0 * (double)v / sqrt((double)n2) + 0.5); }

/* Scores are (S, cnt): S / cnt the mean product of the columns both descriptors have.  a beats b iff S_a * cnt_b > S_b * cnt_a
 * in 64-bit integers; cnt == 0 loses to every cnt > 0; what is left goes to the lower index (a shift, or a candidate). */
BEVX_HD bool place_better(int32_t sa, int32_t cnta, int32_t ia, int32_t sb, int32_t cntb, int32_t ib)
{
    if (cnta == 0 || cntb == 0) {
        if ((cnta > 0) != (cntb > 0)) return cnta > 0;
    } else {
        const int64_t l = (int64_t)sa * (int64_t)cntb, r = (int64_t)sb * (int64_t)cnta;
        if (l != r) return l > r;
    }
    return ia < ib;
}
BEVX_HD double place_distance(int32_t s, int32_t cnt)
{
    return cnt > 0 ? 1.0 - (double)s / (kPlaceUnit2 * (double)cnt) : kPlaceNoDistance;
}
/* the yaw of shift n in degrees, in [-180, 180): p_match ~ Rz(angle) p_query */
BEVX_HD float place_angle(int n, int n_sectors)
{
    const float a = (float)n * (360.0f / (float)n_sectors);
    return a >= 180.0f ? a - 360.0f : a;
}
/* the columns of mask c (n_sectors bits) that meet the columns of mask q at shift n: bit j of the result = column j of q and
 * column (j + n) % n_sectors of c */
BEVX_HD uint64_t place_common(uint64_t q, uint64_t c, int n, int n_sectors)
{
    const uint64_t all = n_sectors == 64 ? ~(uint64_t)0 : (((uint64_t)1 << n_sectors) - 1u);
    const uint64_t rot = n == 0 ? c : ((c >> n) | (c << (n_sectors - n))) & all;
    return q & rot;
}

} /* namespace bevx */

#endif /* BEV_PLACE_EXACT_H */
