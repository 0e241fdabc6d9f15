/*
 * bev_exact_eval.h — one dispatch from a function id to the shared host/device arithmetic of bev_exact.h, bev_libm.h and
 * bev_libm_f64.h, for the test hook bev_debug_exact_eval (k_exact_eval, bev_misc.h) and its host twin (tests/exacteval).
 * Both sides include THIS switch, and the switch calls the very inline functions the product kernels call: no body is
 * restated here.  What it proves is the claim the byte-for-byte GPU tests rest on — that each function rounds the same
 * on gfx950 as on x86-64 — one function at a time, on inputs no plausible sweep produces.
 *
 * An id takes up to four input arrays (element k of each is one evaluation) of 4-byte (float, uint32) or 8-byte
 * (double) words, up to 12 floats taken once per call, and writes `out_words` 32-bit words per element: an int or the
 * bits of a float (1), the two halves of a double, low word first (2), three floats (3).
 */
#ifndef BEV_EXACT_EVAL_H
#define BEV_EXACT_EVAL_H

#include <stddef.h>

#include "bev_libm.h"
#include "bev_libm_f64.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace bevx {

/* the ids are part of the test hook's contract (include/bev_mi355x.h: BEV_EVAL_*): append, never renumber */
enum : int {
    kEvFdAtanf = 0,        /* f(x)                  -> float  fd_atanf */
    kEvFdAtan2f,           /* f(y), f(x)            -> float  fd_atan2f */
    kEvKittiAzimuth,       /* f(x), f(y)            -> float  kitti_azimuth = degrees_of(fd_atan2f(y, x)) */
    kEvKittiCol,           /* f(az)                 -> int    kitti_col */
    kEvKittiCrossing,      /* f(az_prev), f(az)     -> int    kitti_crossing */
    kEvProjectMulran,      /* u(k), f(x), f(y)      -> row | col << 16 */
    kEvProjectOxford,      /* f(x), f(y), f(z)      -> row | col << 16 */
    kEvFdSin,              /* d(x)                  -> double fd_sin */
    kEvFdCos,              /* d(x)                  -> double fd_cos */
    kEvCvttF32,            /* f(v)                  -> int */
    kEvCvttF64,            /* d(v)                  -> int */
    kEvFloorHalfToInt,     /* f(nx)                 -> int */
    kEvGroundCell,         /* f(x), f(y)            -> int */
    kEvRoundHalfUpBin,     /* f(v)                  -> int */
    kEvHeightTimes4,       /* f(t)                  -> int */
    kEvBinInRange,         /* f(v), u(M)            -> bin | in << 31 */
    kEvBinOfShifted,       /* f(v), u(M)            -> bin | in << 31 */
    kEvBevBin,             /* f(p), f(R), f(interval) -> int */
    kEvCountAdvance,       /* f(c), u(n)            -> float  (c >= 0.01f finite, n < 2^24: the function's own domain) */
    kEvExactReciprocal,    /* f(v)                  -> float */
    kEvAngleNodiv,         /* f(dx), f(dy), f(dz)   -> int    angle_is_ground_nodiv */
    kEvAngle,              /* f(dx), f(dy), f(dz)   -> int    angle_is_ground */
    kEvTransformXyz,       /* f(x), f(y), f(z); prm = the 12 floats of [R | t] -> three floats */
    kEvDegreesOf,          /* f(rad)                -> float */
    kEvWrapAzimuth,        /* f(az)                 -> float */
    kEvToU16,              /* f(v)                  -> int */
    kEvBevCode,            /* f(px), f(py), f(pz); prm = MAX_RANGE, interval, HEIGHT_RES, lidar_to_ground, n_layers -> code (label 1) */
    kEvKittiColXy,         /* f(x), f(y)            -> int    kitti_col(kitti_azimuth(x, y)): a return's column as k_kitti_crossings computes it */
    kEvCount
};

enum : int { kEvNone = 0, kEvF32 = 1, kEvU32 = 2, kEvF64 = 3 };
constexpr size_t kEvMaxN = (size_t)1 << 24;
constexpr int kEvParams = 12;

struct ExactEvalSig {
    uint8_t in[4];      /* kEvNone: the array is not read */
    uint8_t out_words;  /* 0: no such id */
    uint8_t params;     /* floats of prm the id reads */
};

BEVX_HD ExactEvalSig exact_eval_sig(int id)
{
    switch (id) {
    case kEvFdAtanf: case kEvKittiCol: case kEvCvttF32: case kEvFloorHalfToInt: case kEvRoundHalfUpBin: case kEvHeightTimes4:
    case kEvExactReciprocal: case kEvDegreesOf: case kEvWrapAzimuth: case kEvToU16:
        return {{kEvF32, kEvNone, kEvNone, kEvNone}, 1, 0};
    case kEvFdAtan2f: case kEvKittiAzimuth: case kEvKittiCrossing: case kEvGroundCell: case kEvKittiColXy:
        return {{kEvF32, kEvF32, kEvNone, kEvNone}, 1, 0};
    case kEvProjectMulran:
        return {{kEvU32, kEvF32, kEvF32, kEvNone}, 1, 0};
    case kEvProjectOxford: case kEvBevBin: case kEvAngleNodiv: case kEvAngle:
        return {{kEvF32, kEvF32, kEvF32, kEvNone}, 1, 0};
    case kEvFdSin: case kEvFdCos:
        return {{kEvF64, kEvNone, kEvNone, kEvNone}, 2, 0};
    case kEvCvttF64:
        return {{kEvF64, kEvNone, kEvNone, kEvNone}, 1, 0};
    case kEvBinInRange: case kEvBinOfShifted: case kEvCountAdvance:
        return {{kEvF32, kEvU32, kEvNone, kEvNone}, 1, 0};
    case kEvTransformXyz:
        return {{kEvF32, kEvF32, kEvF32, kEvNone}, 3, 12};
    case kEvBevCode:
        return {{kEvF32, kEvF32, kEvF32, kEvNone}, 1, 5};
    default:
        return {{kEvNone, kEvNone, kEvNone, kEvNone}, 0, 0};
    }
}
BEVX_HD size_t exact_eval_word_bytes(int type) { return type == kEvF64 ? 8u : (type == kEvNone ? 0u : 4u); }

BEVX_HD void ev_put_f64(uint32_t *o, double v)
{
    union { double d; uint64_t u; } c;
    c.d = v;
    o[0] = (uint32_t)c.u;
    o[1] = (uint32_t)(c.u >> 32);
}

/* element i of id: in[k] are the arrays of exact_eval_sig(id), prm its kEvParams floats, o its out_words words */
BEVX_HD void exact_eval_one(int id, const void *const in[4], const float *prm, size_t i, uint32_t *o)
{
#define EV_F(k) (static_cast<const float *>(in[k])[i])
#define EV_U(k) (static_cast<const uint32_t *>(in[k])[i])
#define EV_D(k) (static_cast<const double *>(in[k])[i])
    switch (id) {
    case kEvFdAtanf: o[0] = float_bits(fd_atanf(EV_F(0))); break;
    case kEvFdAtan2f: o[0] = float_bits(fd_atan2f(EV_F(0), EV_F(1))); break;
    case kEvKittiAzimuth: o[0] = float_bits(kitti_azimuth(EV_F(0), EV_F(1))); break;
    case kEvKittiCol: o[0] = (uint32_t)kitti_col(EV_F(0)); break;
    case kEvKittiCrossing: o[0] = kitti_crossing(EV_F(0), EV_F(1)) ? 1u : 0u; break;
    case kEvProjectMulran: {
        uint16_t row, col;
        project_mulran(EV_U(0), EV_F(1), EV_F(2), row, col);
        o[0] = (uint32_t)row | ((uint32_t)col << 16);
        break;
    }
    case kEvProjectOxford: {
        uint16_t row, col;
        project_oxford(EV_F(0), EV_F(1), EV_F(2), row, col);
        o[0] = (uint32_t)row | ((uint32_t)col << 16);
        break;
    }
    case kEvFdSin: ev_put_f64(o, fd_sin(EV_D(0))); break;
    case kEvFdCos: ev_put_f64(o, fd_cos(EV_D(0))); break;
    case kEvCvttF32: o[0] = (uint32_t)cvtt_f32(EV_F(0)); break;
    case kEvCvttF64: o[0] = (uint32_t)cvtt_f64(EV_D(0)); break;
    case kEvFloorHalfToInt: o[0] = (uint32_t)floor_half_to_int(EV_F(0)); break;
    case kEvGroundCell: o[0] = (uint32_t)ground_cell(EV_F(0), EV_F(1)); break;
    case kEvRoundHalfUpBin: o[0] = (uint32_t)round_half_up_bin(EV_F(0)); break;
    case kEvHeightTimes4: o[0] = (uint32_t)height_times4(EV_F(0)); break;
    case kEvBinInRange: {
        int bin = 0;
        const bool ok = bin_in_range(EV_F(0), (int)EV_U(1), &bin);
        o[0] = ((uint32_t)bin & 0x7fffffffu) | (ok ? 0x80000000u : 0u);
        break;
    }
    case kEvBinOfShifted: {
        int bin = 0;
        const bool ok = bin_of_shifted(EV_F(0), (int)EV_U(1), &bin);
        o[0] = ((uint32_t)bin & 0x7fffffffu) | (ok ? 0x80000000u : 0u);
        break;
    }
    case kEvBevBin: o[0] = (uint32_t)bev_bin(EV_F(0), EV_F(1), EV_F(2)); break;
    case kEvCountAdvance: o[0] = float_bits(count_advance(EV_F(0), EV_U(1))); break;
    case kEvExactReciprocal: o[0] = float_bits(exact_reciprocal(EV_F(0))); break;
    case kEvAngleNodiv: o[0] = angle_is_ground_nodiv(EV_F(0), EV_F(1), EV_F(2)) ? 1u : 0u; break;
    case kEvAngle: o[0] = angle_is_ground(EV_F(0), EV_F(1), EV_F(2)) ? 1u : 0u; break;
    case kEvTransformXyz: {
        float tx, ty, tz;
        transform_xyz(prm, EV_F(0), EV_F(1), EV_F(2), tx, ty, tz);
        o[0] = float_bits(tx);
        o[1] = float_bits(ty);
        o[2] = float_bits(tz);
        break;
    }
    case kEvDegreesOf: o[0] = float_bits(degrees_of(EV_F(0))); break;
    case kEvWrapAzimuth: o[0] = float_bits(wrap_azimuth(EV_F(0))); break;
    case kEvToU16: o[0] = (uint32_t)to_u16(EV_F(0)); break;
    case kEvBevCode: {
        RasterParams rp{};
        raster_scalars((int)prm[0], prm[1], prm[2], prm[3], (int)prm[4], &rp);
        o[0] = bev_code(EV_F(0), EV_F(1), EV_F(2), 1, rp);
        break;
    }
    case kEvKittiColXy: o[0] = (uint32_t)kitti_col(kitti_azimuth(EV_F(0), EV_F(1))); break;
    default: break;
    }
#undef EV_F
#undef EV_U
#undef EV_D
}

} /* namespace bevx */
#endif
