/*
 * bev_libm_f64.h — double sin / cos for the coarse ICP: fdlibm's s_sin.c / s_cos.c over __kernel_sin,
 * __kernel_cos and the small / medium ranges of __ieee754_rem_pio2 (|x| <= 2^20 * pi/2), restated from the published
 * algorithm.  Beyond that range, and for non-finite x, the result is the quiet NaN 0x7ff8000000000000.  Host and device
 * (the kernel's increment, bev_icp.h; the tool's initial guesses, bev_capi_reg.hip and bev_capi_submap_reg.hip).  Only
 * IEEE + - * / and no FMA (see bev_exact.h), so both sides round alike; tests/test_icp_cpu.py bounds the checker's
 * independent restatement against the host libm and the GPU tests compare whole ICP results byte for byte.
 */
#ifndef BEV_LIBM_F64_H
#define BEV_LIBM_F64_H

#include "bev_exact.h"

namespace bevx {

BEVX_HD int32_t f64_hi(double x)
{
    union { double d; uint64_t u; } c;
    c.d = x;
    return (int32_t)(c.u >> 32);
}
BEVX_HD double f64_from_hi(int32_t hi)
{
    union { double d; uint64_t u; } c;
    c.u = (uint64_t)(uint32_t)hi << 32;
    return c.d;
}
BEVX_HD double f64_qnan() { return f64_from_hi(0x7ff80000); }

BEVX_HD double fd_kernel_sin(double x, double y, int iy)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    if ((f64_hi(x) & 0x7fffffff) < 0x3e400000 && (int)x == 0) return x; /* |x| < 2^-27 */
    const double z = x * x;
    const double v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

BEVX_HD double fd_kernel_cos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const int32_t ix = f64_hi(x) & 0x7fffffff;
    if (ix < 0x3e400000 && (int)x == 0) return 1.0;
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3FD33333) return 1.0 - (0.5 * z - (z * r - x * y)); /* |x| < 0.3 */
    const double qx = ix > 0x3fe90000 ? 0.28125 : f64_from_hi(ix - 0x00200000);
    const double hz = 0.5 * z - qx;
    const double a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}

/* n with y0 + y1 = x - n pi/2; returns 0x7fffffff (no reduction: the caller returns NaN) above 2^20 pi/2 */
BEVX_HD int fd_rem_pio2(double x, double &y0, double &y1)
{
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
                 pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
                 pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    /* high words of n * pi/2, n = 1..32: the medium range's "no cancellation" test */
    const int32_t npio2_hw[32] = {
        0x3FF921FB, 0x400921FB, 0x4012D97C, 0x401921FB, 0x401F6A7A, 0x4022D97C, 0x4025FDBB, 0x402921FB,
        0x402C463A, 0x402F6A7A, 0x4031475C, 0x4032D97C, 0x40346B9C, 0x4035FDBB, 0x40378FDB, 0x403921FB,
        0x403AB41B, 0x403C463A, 0x403DD85A, 0x403F6A7A, 0x40407E4C, 0x4041475C, 0x4042106C, 0x4042D97C,
        0x4043A28C, 0x40446B9C, 0x404534AC, 0x4045FDBB, 0x4046C6CB, 0x40478FDB, 0x404858EB, 0x404921FB};
    const int32_t hx = f64_hi(x), ix = hx & 0x7fffffff;
    if (ix <= 0x3fe921fb) { /* |x| <= pi/4 */
        y0 = x;
        y1 = 0.0;
        return 0;
    }
    if (ix < 0x4002d97c) { /* |x| < 3pi/4: n = +-1 */
        const double p2 = ix != 0x3ff921fb ? 0.0 : pio2_2, p2t = ix != 0x3ff921fb ? pio2_1t : pio2_2t;
        if (hx > 0) {
            double z = x - pio2_1;
            if (ix == 0x3ff921fb) z -= p2;
            y0 = z - p2t;
            y1 = (z - y0) - p2t;
            return 1;
        }
        double z = x + pio2_1;
        if (ix == 0x3ff921fb) z += p2;
        y0 = z + p2t;
        y1 = (z - y0) + p2t;
        return -1;
    }
    if (ix > 0x413921fb) return 0x7fffffff;
    double t = hx < 0 ? -x : x;
    const int n = (int)(t * invpio2 + 0.5);
    const double fn = (double)n;
    double r = t - fn * pio2_1;
    double w = fn * pio2_1t;
    y0 = r - w;
    if (!(n < 32 && ix != npio2_hw[n - 1])) {
        const int32_t j = ix >> 20;
        if (j - ((f64_hi(y0) >> 20) & 0x7ff) > 16) { /* second round, 118 bits */
            t = r;
            w = fn * pio2_2;
            r = t - w;
            w = fn * pio2_2t - ((t - r) - w);
            y0 = r - w;
            if (j - ((f64_hi(y0) >> 20) & 0x7ff) > 49) { /* third round, 151 bits */
                t = r;
                w = fn * pio2_3;
                r = t - w;
                w = fn * pio2_3t - ((t - r) - w);
                y0 = r - w;
            }
        }
    }
    y1 = (r - y0) - w;
    if (hx < 0) {
        y0 = -y0;
        y1 = -y1;
        return -n;
    }
    return n;
}

BEVX_HD double fd_sin(double x)
{
    const int32_t ix = f64_hi(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return fd_kernel_sin(x, 0.0, 0);
    if (ix >= 0x7ff00000) return f64_qnan();
    double y0, y1;
    const int n = fd_rem_pio2(x, y0, y1);
    if (n == 0x7fffffff) return f64_qnan();
    switch (n & 3) {
    case 0: return fd_kernel_sin(y0, y1, 1);
    case 1: return fd_kernel_cos(y0, y1);
    case 2: return -fd_kernel_sin(y0, y1, 1);
    default: return -fd_kernel_cos(y0, y1);
    }
}

BEVX_HD double fd_cos(double x)
{
    const int32_t ix = f64_hi(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return fd_kernel_cos(x, 0.0);
    if (ix >= 0x7ff00000) return f64_qnan();
    double y0, y1;
    const int n = fd_rem_pio2(x, y0, y1);
    if (n == 0x7fffffff) return f64_qnan();
    switch (n & 3) {
    case 0: return fd_kernel_cos(y0, y1);
    case 1: return -fd_kernel_sin(y0, y1, 1);
    case 2: return -fd_kernel_cos(y0, y1);
    default: return fd_kernel_sin(y0, y1, 1);
    }
}

/* the tool's initial guess (BatchTopPartRegistration.cpp:415-424): AngleAxisd(rad, UnitZ).toRotationMatrix() cast to
 * float in an identity 4 x 4 (row-major); which 0: rad = (double)(theta / 180.0f) * M_PI, 1: (theta + 180.0f) */
BEVX_HD void icp_tool_guess(float theta, int which, float T[16])
{
    const double pi = 3.14159265358979323846;
    const double rad = which ? (double)((theta + 180.0f) / 180.0f) * pi : (double)(theta / 180.0f) * pi;
    const double s = fd_sin(rad), c = fd_cos(rad);
    for (int k = 0; k < 16; ++k) T[k] = 0.0f;
    T[0] = (float)c;
    T[1] = (float)(0.0 - s);
    T[4] = (float)s;
    T[5] = (float)c;
    T[10] = (float)((1.0 - c) + c);
    T[15] = 1.0f;
}

} /* namespace bevx */

#endif
