/*
 * icp_oracle.c — sequential C checker of the coarse point-to-plane ICP: what
 * pcl::IterativeClosestPointWithNormals<PointNormal, PointNormal> does in performCoarseIcp
 * (BatchTopPartRegistration.cpp:192-221), restated from PCL's published sources, with the points the reference leaves
 * open fixed.  Tests only: it includes no header of the device code and shares none of its arithmetic.
 *
 * Records are pcl::PointNormal, 12 floats: x y z pad nx ny nz pad curvature pad pad pad.
 * Exact nearest neighbour: the searchable target points sorted by x (then index), a binary search for the query's x and
 * a scan outwards on both sides that stops once the float (dx * dx) alone exceeds the best distance (the float
 * ((dx² + dy²) + dz²) is never below it).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define REC 12

typedef struct {
    double max_correspondence_distance;
    double transformation_epsilon;
    double euclidean_fitness_epsilon;
    int32_t max_iterations;
    int32_t _pad;
} icp_params;

typedef struct {
    float T[16];
    double fitness;
    int32_t converged, iterations, state, _pad;
} icp_result;

enum { ST_NOT_CONVERGED, ST_ITERATIONS, ST_TRANSFORM, ST_ABS_MSE, ST_REL_MSE, ST_NO_CORRESPONDENCES };

/* ---- fdlibm sin / cos (s_sin.c, s_cos.c, k_sin.c, k_cos.c, e_rem_pio2.c medium range) -------------------------------- */
static int32_t hi_word(double x)
{
    uint64_t u;
    memcpy(&u, &x, 8);
    return (int32_t)(u >> 32);
}
static double with_hi(int32_t hi)
{
    uint64_t u = (uint64_t)(uint32_t)hi << 32;
    double x;
    memcpy(&x, &u, 8);
    return x;
}
static double qnan64(void) { return with_hi(0x7ff80000); }

static double k_sin(double x, double y, int iy)
{
    const double half = 5.00000000000000000000e-01, S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08,
                 S6 = 1.58969099521155010221e-10;
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix < 0x3e400000 && (int)x == 0) return x;
    const double z = x * x, v = z * x, r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (half * y - v * r) - y) - v * S1);
}

static double k_cos(double x, double y)
{
    const double one = 1.0, C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09,
                 C6 = -1.13596475577881948265e-11;
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix < 0x3e400000 && (int)x == 0) return one;
    const double z = x * x, r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3FD33333) return one - (0.5 * z - (z * r - x * y));
    const double qx = ix > 0x3fe90000 ? 0.28125 : with_hi(ix - 0x00200000);
    const double hz = 0.5 * z - qx, a = one - qx;
    return a - (hz - (z * r - x * y));
}

/* n, y[0] + y[1] = x - n * pi/2 for |x| <= 2^20 * pi/2; n = INT32_MIN beyond (the caller returns NaN) */
static int rem_pio2(double x, double *y)
{
    static const int32_t npio2_hw[32] = {
        0x3FF921FB, 0x400921FB, 0x4012D97C, 0x401921FB, 0x401F6A7A, 0x4022D97C, 0x4025FDBB, 0x402921FB,
        0x402C463A, 0x402F6A7A, 0x4031475C, 0x4032D97C, 0x40346B9C, 0x4035FDBB, 0x40378FDB, 0x403921FB,
        0x403AB41B, 0x403C463A, 0x403DD85A, 0x403F6A7A, 0x40407E4C, 0x4041475C, 0x4042106C, 0x4042D97C,
        0x4043A28C, 0x40446B9C, 0x404534AC, 0x4045FDBB, 0x4046C6CB, 0x40478FDB, 0x404858EB, 0x404921FB};
    const double half = 0.5, invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
                 pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
                 pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    const int32_t hx = hi_word(x), ix = hx & 0x7fffffff;
    if (ix <= 0x3fe921fb) {
        y[0] = x;
        y[1] = 0;
        return 0;
    }
    if (ix < 0x4002d97c) {
        double z;
        if (hx > 0) {
            z = x - pio2_1;
            if (ix != 0x3ff921fb) {
                y[0] = z - pio2_1t;
                y[1] = (z - y[0]) - pio2_1t;
            } else {
                z -= pio2_2;
                y[0] = z - pio2_2t;
                y[1] = (z - y[0]) - pio2_2t;
            }
            return 1;
        }
        z = x + pio2_1;
        if (ix != 0x3ff921fb) {
            y[0] = z + pio2_1t;
            y[1] = (z - y[0]) + pio2_1t;
        } else {
            z += pio2_2;
            y[0] = z + pio2_2t;
            y[1] = (z - y[0]) + pio2_2t;
        }
        return -1;
    }
    if (ix > 0x413921fb) return INT32_MIN;
    double t = fabs(x);
    const int n = (int)(t * invpio2 + half);
    const double fn = (double)n;
    double r = t - fn * pio2_1, w = fn * pio2_1t;
    if (n < 32 && ix != npio2_hw[n - 1]) {
        y[0] = r - w;
    } else {
        const int32_t j = ix >> 20;
        y[0] = r - w;
        int32_t i = j - ((hi_word(y[0]) >> 20) & 0x7ff);
        if (i > 16) {
            t = r;
            w = fn * pio2_2;
            r = t - w;
            w = fn * pio2_2t - ((t - r) - w);
            y[0] = r - w;
            i = j - ((hi_word(y[0]) >> 20) & 0x7ff);
            if (i > 49) {
                t = r;
                w = fn * pio2_3;
                r = t - w;
                w = fn * pio2_3t - ((t - r) - w);
                y[0] = r - w;
            }
        }
    }
    y[1] = (r - y[0]) - w;
    if (hx < 0) {
        y[0] = -y[0];
        y[1] = -y[1];
        return -n;
    }
    return n;
}

double icp_sin(double x)
{
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return k_sin(x, 0.0, 0);
    if (ix >= 0x7ff00000) return qnan64();
    double y[2];
    const int n = rem_pio2(x, y);
    if (n == INT32_MIN) return qnan64();
    switch (n & 3) {
    case 0: return k_sin(y[0], y[1], 1);
    case 1: return k_cos(y[0], y[1]);
    case 2: return -k_sin(y[0], y[1], 1);
    default: return -k_cos(y[0], y[1]);
    }
}

double icp_cos(double x)
{
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return k_cos(x, 0.0);
    if (ix >= 0x7ff00000) return qnan64();
    double y[2];
    const int n = rem_pio2(x, y);
    if (n == INT32_MIN) return qnan64();
    switch (n & 3) {
    case 0: return k_cos(y[0], y[1]);
    case 1: return -k_sin(y[0], y[1], 1);
    case 2: return -k_cos(y[0], y[1]);
    default: return k_sin(y[0], y[1], 1);
    }
}

/* ---- exact nearest neighbour ---------------------------------------------------------------------------------------- */
typedef struct {
    const float *pts; /* the target records */
    uint32_t *ord;    /* searchable indices, ascending x then index */
    uint32_t n;
} nn_index;

static int finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

/* stable merge sort of the indices by x (they come in ascending index order: equal x keeps that order) */
static void sort_by_x(const float *pts, uint32_t *a, uint32_t *tmp, uint32_t n)
{
    for (uint32_t w = 1; w < n; w *= 2) {
        for (uint32_t lo = 0; lo < n; lo += 2 * w) {
            const uint32_t mid = lo + w < n ? lo + w : n, hi = lo + 2 * w < n ? lo + 2 * w : n;
            uint32_t i = lo, j = mid, k = lo;
            while (i < mid && j < hi) tmp[k++] = pts[(size_t)a[j] * REC] < pts[(size_t)a[i] * REC] ? a[j++] : a[i++];
            while (i < mid) tmp[k++] = a[i++];
            while (j < hi) tmp[k++] = a[j++];
        }
        memcpy(a, tmp, sizeof(uint32_t) * n);
    }
}

static int nn_build(nn_index *ix, const float *pts, uint32_t n)
{
    ix->pts = pts;
    ix->n = 0;
    ix->ord = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    if (!ix->ord) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (finite3(pts + (size_t)i * REC)) ix->ord[ix->n++] = i;
    uint32_t *tmp = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    if (!tmp) return -1;
    sort_by_x(pts, ix->ord, tmp, ix->n);
    free(tmp);
    return 0;
}

static float sqdist(const float *q, const float *t)
{
    const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
    return (dx * dx + dy * dy) + dz * dz;
}

/* nearest searchable point of q (lowest index on ties): 1 and *idx, *dist, or 0.  limit2 >= 0: points whose float
 * distance, as double, exceeds it are of no interest (the search may then return 0 or a point beyond the limit) */
static int nn_query(const nn_index *ix, const float *q, double limit2, uint32_t *idx, float *dist)
{
    uint32_t lo = 0, hi = ix->n;
    while (lo < hi) { /* first point with x >= qx */
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ix->pts[(size_t)ix->ord[mid] * REC] < q[0]) lo = mid + 1;
        else hi = mid;
    }
    float best = INFINITY;
    uint32_t bi = UINT32_MAX;
    int have = 0;
    for (uint32_t k = lo; k < ix->n; ++k) { /* right: t.x >= q.x, dx grows */
        const uint32_t j = ix->ord[k];
        const float *t = ix->pts + (size_t)j * REC;
        const float dx = q[0] - t[0], dx2 = dx * dx;
        if ((have && dx2 > best) || (limit2 >= 0 && (double)dx2 > limit2)) break;
        const float d = sqdist(q, t);
        if (!have || d < best || (d == best && j < bi)) {
            best = d;
            bi = j;
            have = 1;
        }
    }
    for (uint32_t k = lo; k-- > 0;) { /* left: t.x < q.x */
        const uint32_t j = ix->ord[k];
        const float *t = ix->pts + (size_t)j * REC;
        const float dx = q[0] - t[0], dx2 = dx * dx;
        if ((have && dx2 > best) || (limit2 >= 0 && (double)dx2 > limit2)) break;
        const float d = sqdist(q, t);
        if (!have || d < best || (d == best && j < bi)) {
            best = d;
            bi = j;
            have = 1;
        }
    }
    *idx = bi;
    *dist = best;
    return have;
}

/* global nearest neighbour of every query (12-float records); idx UINT32_MAX when the target has no searchable point */
void icp_nn(const float *tgt, uint32_t n_tgt, const float *q, uint32_t nq, uint32_t *idx, float *dist)
{
    nn_index ix;
    if (nn_build(&ix, tgt, n_tgt)) return;
    for (uint32_t i = 0; i < nq; ++i) {
        if (!nn_query(&ix, q + (size_t)i * REC, -1.0, &idx[i], &dist[i])) {
            idx[i] = UINT32_MAX;
            dist[i] = INFINITY;
        }
    }
    free(ix.ord);
}

/* ---- fixed-order sums: chunks of 64 reduced as a tree, the chunks in ascending order -------------------------------- */
typedef struct {
    double s[64][28];
    int used, nv, first;
    double total[28];
} fsum;

static void fsum_init(fsum *f, int nv)
{
    memset(f, 0, sizeof(*f));
    f->nv = nv;
    f->first = 1;
}
static void fsum_flush(fsum *f)
{
    if (f->used == 0) return;
    for (int l = f->used; l < 64; ++l)
        for (int v = 0; v < f->nv; ++v) f->s[l][v] = 0.0;
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l)
            for (int v = 0; v < f->nv; ++v) f->s[l][v] = f->s[l][v] + f->s[l + off][v];
    for (int v = 0; v < f->nv; ++v) f->total[v] = f->first ? f->s[0][v] : f->total[v] + f->s[0][v];
    f->first = 0;
    f->used = 0;
}
/* term of source index i (called for every i in ascending order) */
static void fsum_add(fsum *f, const double *t)
{
    for (int v = 0; v < f->nv; ++v) f->s[f->used][v] = t[v];
    if (++f->used == 64) fsum_flush(f);
}

/* ---- the LLS system, its solve, the increment ------------------------------------------------------------------------ */
/* symmetric Gaussian elimination in unknown order 0..5, no pivoting; a non-positive (or NaN) pivot: unknown k is 0 */
void icp_solve(const double *ata, const double *atb, double *x)
{
    double M[6][6], v[6];
    int ok[6];
    for (int i = 0; i < 6; ++i) {
        v[i] = atb[i];
        for (int j = 0; j < 6; ++j) M[i][j] = ata[i * 6 + j];
    }
    for (int k = 0; k < 6; ++k) {
        ok[k] = M[k][k] > 0.0;
        if (!ok[k]) continue;
        for (int i = k + 1; i < 6; ++i) {
            const double f = M[i][k] / M[k][k];
            for (int j = k + 1; j < 6; ++j) M[i][j] -= f * M[k][j];
            v[i] -= f * v[k];
        }
    }
    for (int k = 5; k >= 0; --k) {
        if (!ok[k]) {
            x[k] = 0.0;
            continue;
        }
        double s = v[k];
        for (int j = k + 1; j < 6; ++j) s -= M[k][j] * x[j];
        x[k] = s / M[k][k];
    }
}

/* TransformationEstimationPointToPlaneLLS::constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz), row-major */
void icp_increment(const double *x, float *T)
{
    const double sa = icp_sin(x[0]), ca = icp_cos(x[0]), sb = icp_sin(x[1]), cb = icp_cos(x[1]), sg = icp_sin(x[2]),
                 cg = icp_cos(x[2]);
    memset(T, 0, 16 * sizeof(float));
    T[0] = (float)(cg * cb);
    T[1] = (float)(-sg * ca + cg * sb * sa);
    T[2] = (float)(sg * sa + cg * sb * ca);
    T[4] = (float)(sg * cb);
    T[5] = (float)(cg * ca + sg * sb * sa);
    T[6] = (float)(-cg * sa + sg * sb * ca);
    T[8] = (float)(-sb);
    T[9] = (float)(cb * sa);
    T[10] = (float)(cb * ca);
    T[3] = (float)x[3];
    T[7] = (float)x[4];
    T[11] = (float)x[5];
    T[15] = 1.0f;
}

/* Transformer::se3: col0 * x + (col1 * y + (col2 * z + col3)) */
static void se3(const float *T, const float *p, float *o)
{
    const float x = p[0], y = p[1], z = p[2];
    o[0] = T[0] * x + (T[1] * y + (T[2] * z + T[3]));
    o[1] = T[4] * x + (T[5] * y + (T[6] * z + T[7]));
    o[2] = T[8] * x + (T[9] * y + (T[10] * z + T[11]));
}

static void matmul4(const float *A, const float *B, float *C)
{
    float R[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            R[i * 4 + j] = ((A[i * 4] * B[j] + A[i * 4 + 1] * B[4 + j]) + A[i * 4 + 2] * B[8 + j]) + A[i * 4 + 3] * B[12 + j];
    memcpy(C, R, sizeof(R));
}

/* the tool's initial guesses (BatchTopPartRegistration.cpp:415-424): which 0 -> theta, 1 -> theta + 180 */
void icp_guess(float angle_deg, int which, float *T)
{
    const double rad = which ? (double)((angle_deg + 180.0f) / 180.0f) * M_PI : (double)(angle_deg / 180.0f) * M_PI;
    const double s = icp_sin(rad), c = icp_cos(rad);
    memset(T, 0, 16 * sizeof(float));
    T[0] = (float)c;
    T[1] = (float)(0.0 - s);
    T[4] = (float)s;
    T[5] = (float)c;
    T[10] = (float)((1.0 - c) + c);
    T[15] = 1.0f;
}

static float canon_f(float f)
{
    if (isnan(f)) {
        const uint32_t u = 0x7fc00000u;
        memcpy(&f, &u, 4);
    }
    return f;
}

/* ---- one problem ---------------------------------------------------------------------------------------------------- */
void icp_run(const float *src, uint32_t n_src, const float *tgt, uint32_t n_tgt, const float *guess, const icp_params *p,
             icp_result *res)
{
    memset(res, 0, sizeof(*res));
    nn_index ix;
    float *cur = (float *)malloc(sizeof(float) * 4 * (n_src ? n_src : 1));
    fsum *fs = (fsum *)malloc(sizeof(fsum));
    if (!cur || !fs || nn_build(&ix, tgt, n_tgt)) {
        free(cur);
        free(fs);
        res->state = -1;
        return;
    }
    static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int identity = 1;
    for (int k = 0; k < 16; ++k) identity &= guess[k] == I[k];
    float fin[16];
    memcpy(fin, guess, sizeof(fin));
    for (uint32_t i = 0; i < n_src; ++i) {
        if (identity) memcpy(cur + 4 * i, src + (size_t)i * REC, 3 * sizeof(float));
        else se3(guess, src + (size_t)i * REC, cur + 4 * i);
    }
    const double D = p->max_correspondence_distance, D2 = D * D;
    double prev = DBL_MAX;
    int iters = 0, state = ST_NOT_CONVERGED;
    while (state == ST_NOT_CONVERGED) {
        fsum_init(fs, 28);
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < n_src; ++i) {
            double t[28] = {0};
            const float *s = cur + 4 * i;
            uint32_t j;
            float d;
            if (finite3(s) && nn_query(&ix, s, D2, &j, &d) && (double)d <= D2) {
                ++cnt;
                const float *tp = tgt + (size_t)j * REC;
                const float sx = s[0], sy = s[1], sz = s[2], tx = tp[0], ty = tp[1], tz = tp[2];
                const float nx = tp[4], ny = tp[5], nz = tp[6];
                if (isfinite(nx) && isfinite(ny) && isfinite(nz)) {
                    const float a = nz * sy - ny * sz, b = nx * sz - nz * sx, c = ny * sx - nx * sy;
                    const float dd = ((((nx * tx + ny * ty) + nz * tz) - nx * sx) - ny * sy) - nz * sz;
                    const double r[6] = {a, b, c, nx, ny, nz};
                    int k = 0;
                    for (int u = 0; u < 6; ++u)
                        for (int v = u; v < 6; ++v) t[k++] = r[u] * r[v];
                    for (int u = 0; u < 6; ++u) t[21 + u] = r[u] * (double)dd;
                }
                t[27] = (double)d;
            }
            fsum_add(fs, t);
        }
        fsum_flush(fs);
        if (cnt < 3) {
            state = ST_NO_CORRESPONDENCES;
            break;
        }
        double ata[36], atb[6], x[6];
        int k = 0;
        for (int u = 0; u < 6; ++u)
            for (int v = u; v < 6; ++v) ata[u * 6 + v] = ata[v * 6 + u] = fs->total[k++];
        for (int u = 0; u < 6; ++u) atb[u] = fs->total[21 + u];
        icp_solve(ata, atb, x);
        float inc[16];
        icp_increment(x, inc);
        for (uint32_t i = 0; i < n_src; ++i) {
            float o[3];
            se3(inc, cur + 4 * i, o);
            memcpy(cur + 4 * i, o, sizeof(o));
        }
        matmul4(inc, fin, fin);
        ++iters;
        /* DefaultConvergenceCriteria::hasConverged (max similar iterations 0); the sums are in float, like Eigen's */
        const double cos_angle = 0.5 * (double)(((inc[0] + inc[5]) + inc[10]) - 1.0f);
        const double trans2 = (double)((inc[3] * inc[3] + inc[7] * inc[7]) + inc[11] * inc[11]);
        if (iters >= p->max_iterations) {
            state = ST_ITERATIONS;
        } else if (cos_angle >= 1.0 - p->transformation_epsilon && trans2 <= p->transformation_epsilon) {
            state = ST_TRANSFORM;
        } else {
            const double mse = fs->total[27] / (double)cnt;
            if (fabs(mse - prev) < 1e-12) state = ST_ABS_MSE;
            else if (fabs(mse - prev) / prev < p->euclidean_fitness_epsilon) state = ST_REL_MSE;
            else prev = mse;
        }
    }
    /* getFitnessScore(): the original source through final, every finite point's nearest distance if finite */
    fsum_init(fs, 1);
    uint32_t nr = 0;
    for (uint32_t i = 0; i < n_src; ++i) {
        double t = 0.0;
        float q[3], d;
        uint32_t j;
        se3(fin, src + (size_t)i * REC, q);
        if (finite3(q) && nn_query(&ix, q, -1.0, &j, &d) && isfinite(d)) {
            t = (double)d;
            ++nr;
        }
        fsum_add(fs, &t);
    }
    fsum_flush(fs);
    res->fitness = nr ? fs->total[0] / (double)nr : DBL_MAX;
    if (isnan(res->fitness)) res->fitness = qnan64();
    for (int k = 0; k < 16; ++k) res->T[k] = canon_f(fin[k]);
    res->iterations = iters;
    res->state = state;
    res->converged = state >= ST_ITERATIONS && state <= ST_REL_MSE;
    free(ix.ord);
    free(cur);
    free(fs);
}

/* the tool's choice (:464-466): guess 0 iff fitness0 < fitness1 */
int icp_best(double f0, double f1) { return f0 < f1 ? 0 : 1; }
