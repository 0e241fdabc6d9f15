/*
 * bev_align_exact.h — the arithmetic of the translation guess of retrieved pairs, written once for the HIP
 * kernels (bev_align.h), the host side of the C ABI (bev_capi_align.hip) and the sequential checker of the tests
 * (tests/align/align_oracle.c): the cell of a point in a Cartesian height grid, the hypotheses of a hit, the three orders, the
 * sub-cell offset of the winning shift and what goes into a result.  bev_exact.h's rules hold: only correctly rounded IEEE
 * operations, contraction off, no libm call beyond those the project already shares (floorf, sqrt; fd_sin / fd_cos through
 * icp_tool_guess) — every function gives the same bits on gfx950 and on x86-64.
 *
 * A height grid is G x G bytes, byte [iy * G + ix]; the value of a point is §6z's place_value, a cell holds the maximum.
 * The score of a shift (dx, dy) is the zero-padded correlation sum of q[iy][ix] * c[iy + dy][ix + dx], a 32-bit unsigned
 * integer (at most 128^2 * 127^2).
 */
#ifndef BEV_ALIGN_EXACT_H
#define BEV_ALIGN_EXACT_H

#include "bev_libm_f64.h"
#include "bev_place_exact.h"

namespace bevx {

constexpr int kAlignMinGrid = 16, kAlignMaxGrid = 128, kAlignMaxShift = 16, kAlignMaxYawSteps = 3;
constexpr double kAlignNoFitness = 2.0; /* the fitness of a hypothesis without a common cell (S == 0) */

/* the admitted parameters (include/bev_mi355x.h: bev_align_params_t) */
BEVX_HD bool align_params_ok(int grid, float cell, int max_shift, int yaw_steps, float yaw_step, int skip_label0)
{
    return grid >= kAlignMinGrid && grid <= kAlignMaxGrid && (grid & 1) == 0 && cell > 0.0f && cell <= 3.402823466e+38f &&
           max_shift >= 1 && max_shift <= kAlignMaxShift && 2 * max_shift <= grid / 2 && yaw_steps >= 0 &&
           yaw_steps <= kAlignMaxYawSteps && yaw_step >= 0.0f && yaw_step <= 3.402823466e+38f && /* (false for NaN, inf) */
           (skip_label0 == 0 || skip_label0 == 1);
}
/* iy * G + ix of a point, -1 where it does not contribute: the origin's no-return records and NaN fail r2 > 0; the range test
 * is made in float, before any conversion to int, so inf and what lies beyond int fail it */
BEVX_HD int align_cell(float x, float y, int label, int G, float cell, int skip_label0)
{
    if (!(place_r2(x, y) > 0.0f) || (skip_label0 && label == 0)) return -1;
    const float fx = floorf(x / cell), fy = floorf(y / cell), half = (float)(G / 2);
    if (!(-half <= fx && fx < half && -half <= fy && fy < half)) return -1;
    return ((int)fy + G / 2) * G + ((int)fx + G / 2);
}
/* the yaw of hypothesis k of a hit, in degrees, and its rotation: rows 0 ... 2 of T move the query's points */
BEVX_HD float align_theta(float angle_guess, int k, float yaw_step) { return angle_guess + (float)k * yaw_step; }

/* Among the shifts of a hypothesis: higher S, then smaller dx^2 + dy^2, then smaller dy, then smaller dx */
BEVX_HD bool align_shift_better(uint32_t sa, int dxa, int dya, uint32_t sb, int dxb, int dyb)
{
    if (sa != sb) return sa > sb;
    const int ra = dxa * dxa + dya * dya, rb = dxb * dxb + dyb * dyb;
    if (ra != rb) return ra < rb;
    if (dya != dyb) return dya < dyb;
    return dxa < dxb;
}
/* Among the k of a flip: higher best-S, then smaller |k|, then smaller k */
BEVX_HD bool align_k_better(uint32_t sa, int ka, uint32_t sb, int kb)
{
    if (sa != sb) return sa > sb;
    const int aa = ka < 0 ? -ka : ka, ab = kb < 0 ? -kb : kb;
    if (aa != ab) return aa < ab;
    return ka < kb;
}
/* best[m]: 0 iff the best-S of flip 0 >= that of flip 1 */
BEVX_HD int align_best_flip(uint32_t s0, uint32_t s1) { return s0 >= s1 ? 0 : 1; }

/* the sub-cell offset of the winning shift d along one axis from its neighbours' scores sm (d - 1) and sp (d + 1): a parabola
 * through the three, only where both neighbours lie inside the searched window [-S, S] */
BEVX_HD double align_offset(int d, int max_shift, uint32_t sm, uint32_t s0, uint32_t sp)
{
    if (d - 1 < -max_shift || d + 1 > max_shift) return 0.0;
    const double den = ((double)sm - 2.0 * (double)s0) + (double)sp;
    double off = den < 0.0 ? 0.5 * ((double)sm - (double)sp) / den : 0.0;
    if (off < -0.5) off = -0.5;
    if (off > 0.5) off = 0.5;
    return off;
}
/* a translation entry of T: the winning shift and its offset in metres */
BEVX_HD float align_translation(int d, double off, float cell) { return (float)(((double)d + off) * (double)cell); }
/* 1 - the cosine of the two grids at the winning shift; eq, ec: their sums of squares */
BEVX_HD double align_fitness(uint32_t s, uint32_t eq, uint32_t ec)
{
    return s > 0u ? 1.0 - (double)s / sqrt((double)eq * (double)ec) : kAlignNoFitness;
}

} /* namespace bevx */

#endif /* BEV_ALIGN_EXACT_H */
