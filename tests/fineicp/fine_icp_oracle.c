/*
 * fine_icp_oracle.c — sequential C checker of the fine stage of the registration tools:
 * pcl::VoxelGrid<PointXYZIRCT>, point-to-point ICP with TransformationEstimationSVD (Umeyama, Eigen's JacobiSVD of a
 * 3 x 3 float matrix), and the tools' report maths.  Tests only; it includes no header of the device code.  Built with
 * -ffp-contract=off: no FMA anywhere.  The coarse checker (tests/icp/icp_oracle.c) is compiled in unchanged for the
 * tools' yaw guess (icp_guess) and its fixed-order conventions.
 *
 * Records are pcl::PointXYZIRCT as bev_point_t: 32 bytes, x y z pad intensity row col t label pad.
 */
#include "../icp/icp_oracle.c"

#include <float.h>

typedef struct {
    float x, y, z, pad0, intensity;
    uint16_t row, col;
    uint32_t t;
    int16_t label;
    uint16_t pad1;
} irct;

/* ---- VoxelGrid<PointXYZIRCT> ----------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t vox, idx;
} vkey;

static int vkey_cmp(const void *a, const void *b)
{
    const vkey *p = (const vkey *)a, *q = (const vkey *)b;
    if (p->vox != q->vox) return p->vox < q->vox ? -1 : 1;
    return p->idx < q->idx ? -1 : (p->idx > q->idx ? 1 : 0);
}

static int finite_rec(const irct *p) { return isfinite(p->x) && isfinite(p->y) && isfinite(p->z); }

/* out: capacity n records; returns the number written */
uint32_t fine_voxel_irct(const irct *in, uint32_t n, float leaf, irct *out)
{
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!finite_rec(&in[i])) continue;
        const float v[3] = {in[i].x, in[i].y, in[i].z};
        for (int d = 0; d < 3; ++d) {
            if (v[d] < mn[d]) mn[d] = v[d];
            if (v[d] > mx[d]) mx[d] = v[d];
        }
        ++nf;
    }
    if (nf == 0) return 0;
    const float inv = 1.0f / leaf;
    double prod = 1.0;
    int overflow = 0;
    for (int d = 0; d < 3; ++d) {
        const float e = (mx[d] - mn[d]) * inv;
        if (!(e < 9.0e18f)) overflow = 1;
        else prod *= (double)((int64_t)e + 1);
    }
    if (overflow || prod > 2147483647.0) { /* "leaf size is too small": the input, unchanged */
        memcpy(out, in, sizeof(irct) * n);
        return n;
    }
    int minb[3], div[3];
    for (int d = 0; d < 3; ++d) {
        minb[d] = (int)floorf(mn[d] * inv);
        div[d] = (int)floorf(mx[d] * inv) - minb[d] + 1;
    }
    vkey *k = (vkey *)malloc(sizeof(vkey) * nf);
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!finite_rec(&in[i])) continue;
        const uint32_t i0 = (uint32_t)(int)(floorf(in[i].x * inv) - (float)minb[0]);
        const uint32_t i1 = (uint32_t)(int)(floorf(in[i].y * inv) - (float)minb[1]);
        const uint32_t i2 = (uint32_t)(int)(floorf(in[i].z * inv) - (float)minb[2]);
        k[m].vox = i0 + i1 * (uint32_t)div[0] + i2 * ((uint32_t)div[0] * (uint32_t)div[1]);
        k[m].idx = i;
        ++m;
    }
    qsort(k, m, sizeof(vkey), vkey_cmp);
    uint32_t nv = 0;
    uint32_t *lab = (uint32_t *)malloc(sizeof(uint32_t) * (m ? m : 1));
    for (uint32_t a = 0; a < m;) {
        uint32_t b = a;
        while (b < m && k[b].vox == k[a].vox) ++b;
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, si = 0.0f;
        for (uint32_t q = a; q < b; ++q) {
            const irct *p = &in[k[q].idx];
            sx += p->x;
            sy += p->y;
            sz += p->z;
            si += p->intensity;
        }
        /* AccumulatorLabel: std::map<uint32_t, size_t>, ascending keys, the first strictly larger count wins */
        const uint32_t cnt = b - a;
        for (uint32_t q = 0; q < cnt; ++q) lab[q] = (uint32_t)(int32_t)in[k[a + q].idx].label;
        for (uint32_t q = 1; q < cnt; ++q) { /* insertion sort: voxels are small */
            const uint32_t v = lab[q];
            uint32_t r = q;
            while (r > 0 && lab[r - 1] > v) {
                lab[r] = lab[r - 1];
                --r;
            }
            lab[r] = v;
        }
        size_t best = 0;
        uint32_t best_lab = 0;
        for (uint32_t q = 0; q < cnt;) {
            uint32_t r = q;
            while (r < cnt && lab[r] == lab[q]) ++r;
            if ((size_t)(r - q) > best) {
                best = r - q;
                best_lab = lab[q];
            }
            q = r;
        }
        irct o;
        memset(&o, 0, sizeof(o));
        const float cf = (float)cnt;
        o.x = sx / cf;
        o.y = sy / cf;
        o.z = sz / cf;
        o.intensity = si / cf;
        o.label = (int16_t)best_lab;
        out[nv++] = o;
        a = b;
    }
    free(lab);
    free(k);
    return nv;
}

/* ---- exact 1-NN over a uniform 3-D grid ------------------------------------------------------------------------------ */
typedef struct {
    const irct *pts;
    double mn[3], h, mag;
    int dim[3];
    uint32_t *start; /* [cells + 1] */
    uint32_t *idx;   /* searchable indices by cell, ascending inside a cell */
    uint32_t n;
} grid3;

static int g_cell(const grid3 *g, double v, int d)
{
    double c = floor((v - g->mn[d]) / g->h);
    if (!(c >= 0.0)) c = 0.0; /* (NaN cannot occur: queries are finite) */
    if (c > (double)(g->dim[d] - 1)) c = (double)(g->dim[d] - 1);
    return (int)c;
}

static void grid_build(grid3 *g, const irct *pts, uint32_t n)
{
    memset(g, 0, sizeof(*g));
    g->pts = pts;
    double mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int d = 0; d < 3; ++d) g->mn[d] = INFINITY;
    for (uint32_t i = 0; i < n; ++i) {
        if (!finite_rec(&pts[i])) continue;
        const double v[3] = {pts[i].x, pts[i].y, pts[i].z};
        for (int d = 0; d < 3; ++d) {
            if (v[d] < g->mn[d]) g->mn[d] = v[d];
            if (v[d] > mx[d]) mx[d] = v[d];
        }
        ++g->n;
    }
    if (g->n == 0) {
        for (int d = 0; d < 3; ++d) g->mn[d] = 0.0, g->dim[d] = 1;
        g->h = 1.0;
    } else {
        double ext = 0.0;
        for (int d = 0; d < 3; ++d) {
            ext = fmax(ext, mx[d] - g->mn[d]);
            g->mag = fmax(g->mag, fmax(fabs(g->mn[d]), fabs(mx[d])));
        }
        g->h = ext > 0.0 && isfinite(ext) ? fmax(ext / 256.0, 0.25) : 1.0;
        for (int d = 0; d < 3; ++d) {
            const double c = floor((mx[d] - g->mn[d]) / g->h) + 1.0;
            g->dim[d] = c < 256.0 ? (int)c : 256;
        }
    }
    const size_t cells = (size_t)g->dim[0] * g->dim[1] * g->dim[2];
    g->start = (uint32_t *)calloc(cells + 1, sizeof(uint32_t));
    g->idx = (uint32_t *)malloc(sizeof(uint32_t) * (g->n ? g->n : 1));
    uint32_t *cell = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    for (uint32_t i = 0; i < n; ++i) {
        if (!finite_rec(&pts[i])) continue;
        cell[i] = (uint32_t)(((size_t)g_cell(g, pts[i].z, 2) * g->dim[1] + g_cell(g, pts[i].y, 1)) * g->dim[0] +
                             g_cell(g, pts[i].x, 0));
        g->start[cell[i] + 1]++;
    }
    for (size_t c = 0; c < cells; ++c) g->start[c + 1] += g->start[c];
    uint32_t *fill = (uint32_t *)malloc(sizeof(uint32_t) * (cells ? cells : 1));
    memcpy(fill, g->start, sizeof(uint32_t) * cells);
    for (uint32_t i = 0; i < n; ++i)
        if (finite_rec(&pts[i])) g->idx[fill[cell[i]]++] = i;
    free(fill);
    free(cell);
}

static void grid_free(grid3 *g)
{
    free(g->start);
    free(g->idx);
}

/* nearest searchable point of q (float distance ((dx^2 + dy^2) + dz^2), the lower index on ties): 1, or 0 when there is
 * none.  limit2 >= 0: points beyond it are of no interest (the search may stop) */
static int grid_nn(const grid3 *g, const float *q, double limit2, uint32_t *bi, float *bd)
{
    *bi = UINT32_MAX;
    *bd = INFINITY;
    if (g->n == 0) return 0;
    const int c[3] = {g_cell(g, q[0], 0), g_cell(g, q[1], 1), g_cell(g, q[2], 2)};
    int maxr = 0;
    for (int d = 0; d < 3; ++d) {
        if (c[d] > maxr) maxr = c[d];
        if (g->dim[d] - 1 - c[d] > maxr) maxr = g->dim[d] - 1 - c[d];
    }
    const double margin = 1e-4 * g->h + 1e-6 * g->mag;
    int have = 0;
    for (int r = 0; r <= maxr; ++r) {
        if (r >= 2) {
            const double lb = (double)(r - 1) * g->h - ((double)r * g->h * 1e-5 + margin);
            if (lb > 0.0) {
                const double lb2 = lb * lb * (1.0 - 1e-5);
                if ((have && lb2 > (double)*bd) || (limit2 >= 0.0 && lb2 > limit2)) break;
            }
        }
        for (int z = c[2] - r; z <= c[2] + r; ++z) {
            if (z < 0 || z >= g->dim[2]) continue;
            for (int y = c[1] - r; y <= c[1] + r; ++y) {
                if (y < 0 || y >= g->dim[1]) continue;
                const int shell = (z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r);
                for (int x = c[0] - r; x <= c[0] + r; x += (shell || r == 0) ? 1 : 2 * r) {
                    if (x < 0 || x >= g->dim[0]) continue;
                    const size_t cell = ((size_t)z * g->dim[1] + y) * g->dim[0] + x;
                    for (uint32_t k = g->start[cell]; k < g->start[cell + 1]; ++k) {
                        const uint32_t j = g->idx[k];
                        const irct *t = &g->pts[j];
                        const float dx = q[0] - t->x, dy = q[1] - t->y, dz = q[2] - t->z;
                        const float d = (dx * dx + dy * dy) + dz * dz;
                        if (!have || d < *bd || (d == *bd && j < *bi)) {
                            *bd = d;
                            *bi = j;
                            have = 1;
                        }
                    }
                }
            }
        }
    }
    return have;
}

/* global nearest neighbour of every query (3 floats each) */
void fine_nn(const irct *tgt, uint32_t n_tgt, const float *q, uint32_t nq, uint32_t *idx, float *dist)
{
    grid3 g;
    grid_build(&g, tgt, n_tgt);
    for (uint32_t i = 0; i < nq; ++i)
        if (!grid_nn(&g, q + 3 * (size_t)i, -1.0, &idx[i], &dist[i])) {
            idx[i] = UINT32_MAX;
            dist[i] = INFINITY;
        }
    grid_free(&g);
}

/* ---- Eigen's JacobiSVD<Matrix3f> (two-sided Jacobi, no preconditioner) ----------------------------------------------- */
static void rot_plane(float *x, float *y, float c, float s)
{
    const float a = *x, b = *y;
    *x = c * a + s * b;
    *y = -s * a + c * b;
}

static float det3(const float *M)
{
    const float h0 = M[0] * (M[4] * M[8] - M[5] * M[7]);
    const float h1 = M[1] * (M[3] * M[8] - M[5] * M[6]);
    const float h2 = M[2] * (M[3] * M[7] - M[4] * M[6]);
    return (h0 - h1) + h2;
}

#define SVD_SWEEPS 64

/* A (row-major, finite) = U diag(sv) V^T; U, V row-major; sv descending.  Returns the sweeps taken. */
int fine_svd3(const float *A, float *U, float *sv, float *V)
{
    const float kMin = FLT_MIN, kPrec = 2.0f * FLT_EPSILON;
    float scale = 0.0f, W[9];
    for (int k = 0; k < 9; ++k) scale = fabsf(A[k]) > scale ? fabsf(A[k]) : scale;
    if (scale == 0.0f) scale = 1.0f;
    for (int k = 0; k < 9; ++k) {
        W[k] = A[k] / scale;
        U[k] = V[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    }
    float maxd = fmaxf(fmaxf(fabsf(W[0]), fabsf(W[4])), fabsf(W[8]));
    int sweeps = 0;
    for (; sweeps < SVD_SWEEPS; ++sweeps) {
        int finished = 1;
        for (int p = 1; p < 3; ++p) {
            for (int q = 0; q < p; ++q) {
                const float thr = fmaxf(kMin, kPrec * maxd);
                if (!(fabsf(W[p * 3 + q]) > thr || fabsf(W[q * 3 + p]) > thr)) continue;
                finished = 0;
                const float m00 = W[p * 3 + p], m01 = W[p * 3 + q], m10 = W[q * 3 + p], m11 = W[q * 3 + q];
                const float t = m00 + m11, d = m10 - m01;
                float c1 = 1.0f, s1 = 0.0f;
                if (!(fabsf(d) < kMin)) {
                    const float u = t / d, tmp = sqrtf(1.0f + u * u);
                    s1 = 1.0f / tmp;
                    c1 = u / tmp;
                }
                float n00 = m00, n01 = m01, n10 = m10, n11 = m11;
                if (!(c1 == 1.0f && s1 == 0.0f)) {
                    rot_plane(&n00, &n10, c1, s1);
                    rot_plane(&n01, &n11, c1, s1);
                }
                float cr = 1.0f, sr = 0.0f;
                const float deno = 2.0f * fabsf(n01);
                if (!(deno < kMin)) {
                    const float tau = (n00 - n11) / deno, w = sqrtf(tau * tau + 1.0f);
                    const float tj = tau > 0.0f ? 1.0f / (tau + w) : 1.0f / (tau - w);
                    const float sign_t = tj > 0.0f ? 1.0f : -1.0f;
                    const float nn = 1.0f / sqrtf(tj * tj + 1.0f);
                    sr = ((-sign_t * (n01 / fabsf(n01))) * fabsf(tj)) * nn;
                    cr = nn;
                }
                const float cl = c1 * cr - s1 * (-sr), sl = c1 * (-sr) + s1 * cr;
                if (!(cl == 1.0f && sl == 0.0f)) {
                    for (int k = 0; k < 3; ++k) rot_plane(&W[p * 3 + k], &W[q * 3 + k], cl, sl);
                    for (int k = 0; k < 3; ++k) rot_plane(&U[k * 3 + p], &U[k * 3 + q], cl, sl);
                }
                if (!(cr == 1.0f && -sr == 0.0f)) {
                    for (int k = 0; k < 3; ++k) rot_plane(&W[k * 3 + p], &W[k * 3 + q], cr, -sr);
                    for (int k = 0; k < 3; ++k) rot_plane(&V[k * 3 + p], &V[k * 3 + q], cr, -sr);
                }
                maxd = fmaxf(maxd, fmaxf(fabsf(W[p * 3 + p]), fabsf(W[q * 3 + q])));
            }
        }
        if (finished) break;
    }
    for (int i = 0; i < 3; ++i) {
        const float a = W[i * 3 + i];
        sv[i] = fabsf(a);
        if (a < 0.0f)
            for (int k = 0; k < 3; ++k) U[k * 3 + i] = -U[k * 3 + i];
    }
    for (int i = 0; i < 3; ++i) sv[i] *= scale;
    for (int i = 0; i < 3; ++i) {
        int pos = i;
        for (int k = i + 1; k < 3; ++k)
            if (sv[k] > sv[pos]) pos = k;
        if (sv[pos] == 0.0f) break;
        if (pos != i) {
            float t = sv[i];
            sv[i] = sv[pos];
            sv[pos] = t;
            for (int k = 0; k < 3; ++k) {
                t = U[k * 3 + i], U[k * 3 + i] = U[k * 3 + pos], U[k * 3 + pos] = t;
                t = V[k * 3 + i], V[k * 3 + i] = V[k * 3 + pos], V[k * 3 + pos] = t;
            }
        }
    }
    return sweeps;
}

/* sigma -> R = U diag(1, 1, +-1) V^T; a non-finite sigma: NaN */
void fine_rotation(const float *sigma, float *R)
{
    for (int k = 0; k < 9; ++k)
        if (!isfinite(sigma[k])) {
            for (int j = 0; j < 9; ++j) R[j] = NAN;
            return;
        }
    float U[9], sv[3], V[9];
    fine_svd3(sigma, U, sv, V);
    const float sgn = det3(U) * det3(V) < 0.0f ? -1.0f : 1.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[i * 3 + j] = (U[i * 3] * V[j * 3] + U[i * 3 + 1] * V[j * 3 + 1]) + (U[i * 3 + 2] * sgn) * V[j * 3 + 2];
}

/* ---- fixed-order float / double sums (chunks of 64 as a tree, the chunks in ascending order) ------------------------- */
typedef struct {
    float f[64][9];
    double d[64];
    int used, nf, first;
    float tf[9];
    double td;
} fsum2;

static void f2_init(fsum2 *s, int nf)
{
    memset(s, 0, sizeof(*s));
    s->nf = nf;
    s->first = 1;
}
static void f2_flush(fsum2 *s)
{
    if (s->used == 0) return;
    for (int l = s->used; l < 64; ++l) {
        for (int v = 0; v < s->nf; ++v) s->f[l][v] = 0.0f;
        s->d[l] = 0.0;
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) {
            for (int v = 0; v < s->nf; ++v) s->f[l][v] = s->f[l][v] + s->f[l + off][v];
            s->d[l] = s->d[l] + s->d[l + off];
        }
    for (int v = 0; v < s->nf; ++v) s->tf[v] = s->first ? s->f[0][v] : s->tf[v] + s->f[0][v];
    s->td = s->first ? s->d[0] : s->td + s->d[0];
    s->first = 0;
    s->used = 0;
}
static void f2_add(fsum2 *s, const float *tf, double td)
{
    for (int v = 0; v < s->nf; ++v) s->f[s->used][v] = tf[v];
    s->d[s->used] = td;
    if (++s->used == 64) f2_flush(s);
}

/* one Umeyama step on n correspondence pairs (3 floats each, in order): the 4 x 4 increment, row-major */
void fine_umeyama(const float *src, const float *dst, uint32_t n, float *T)
{
    fsum2 *s = (fsum2 *)malloc(sizeof(fsum2));
    f2_init(s, 6);
    for (uint32_t i = 0; i < n; ++i) {
        const float t[6] = {src[3 * i], src[3 * i + 1], src[3 * i + 2], dst[3 * i], dst[3 * i + 1], dst[3 * i + 2]};
        f2_add(s, t, 0.0);
    }
    f2_flush(s);
    const float oon = 1.0f / (float)n;
    float mean[6];
    for (int k = 0; k < 6; ++k) mean[k] = s->tf[k] * oon;
    f2_init(s, 9);
    for (uint32_t i = 0; i < n; ++i) {
        float t[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) t[a * 3 + b] = (dst[3 * i + a] - mean[3 + a]) * (src[3 * i + b] - mean[b]);
        f2_add(s, t, 0.0);
    }
    f2_flush(s);
    float sigma[9], R[9];
    for (int k = 0; k < 9; ++k) sigma[k] = oon * s->tf[k];
    fine_rotation(sigma, R);
    memset(T, 0, 16 * sizeof(float));
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[i * 4 + j] = R[i * 3 + j];
        T[i * 4 + 3] = mean[3 + i] - ((R[i * 3] * mean[0] + R[i * 3 + 1] * mean[1]) + R[i * 3 + 2] * mean[2]);
    }
    T[15] = 1.0f;
    free(s);
}

/* ---- one problem ------------------------------------------------------------------------------------------------------ */
void fine_run(const irct *src, uint32_t n_src, const irct *tgt, uint32_t n_tgt, const float *guess, const icp_params *p,
              icp_result *res)
{
    memset(res, 0, sizeof(*res));
    grid3 g;
    grid_build(&g, tgt, n_tgt);
    float *cur = (float *)malloc(sizeof(float) * 3 * (n_src ? n_src : 1));
    uint32_t *corr = (uint32_t *)malloc(sizeof(uint32_t) * (n_src ? n_src : 1));
    fsum2 *fs = (fsum2 *)malloc(sizeof(fsum2));
    static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int identity = 1;
    for (int k = 0; k < 16; ++k) identity &= guess[k] == I[k];
    float fin[16];
    memcpy(fin, guess, sizeof(fin));
    for (uint32_t i = 0; i < n_src; ++i) {
        const float q[3] = {src[i].x, src[i].y, src[i].z};
        if (identity) memcpy(cur + 3 * i, q, sizeof(q));
        else {
            float o[4];
            const float q12[12] = {q[0], q[1], q[2]};
            se3(guess, q12, o);
            memcpy(cur + 3 * i, o, 3 * sizeof(float));
        }
    }
    const double D = p->max_correspondence_distance, D2 = D * D;
    double prev = DBL_MAX;
    int iters = 0, state = ST_NOT_CONVERGED;
    while (state == ST_NOT_CONVERGED) {
        f2_init(fs, 6);
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < n_src; ++i) {
            float t[6] = {0, 0, 0, 0, 0, 0};
            double td = 0.0;
            const float *s = cur + 3 * i;
            uint32_t j;
            float d;
            corr[i] = UINT32_MAX;
            if (isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]) && grid_nn(&g, s, D2, &j, &d) && (double)d <= D2) {
                corr[i] = j;
                ++cnt;
                t[0] = s[0], t[1] = s[1], t[2] = s[2];
                t[3] = tgt[j].x, t[4] = tgt[j].y, t[5] = tgt[j].z;
                td = (double)d;
            }
            f2_add(fs, t, td);
        }
        f2_flush(fs);
        if (cnt < 3) {
            state = ST_NO_CORRESPONDENCES;
            break;
        }
        const double mse_sum = fs->td;
        const float oon = 1.0f / (float)cnt;
        float mean[6];
        for (int k = 0; k < 6; ++k) mean[k] = fs->tf[k] * oon;
        f2_init(fs, 9);
        for (uint32_t i = 0; i < n_src; ++i) {
            float t[9] = {0};
            if (corr[i] != UINT32_MAX) {
                const float *s = cur + 3 * i;
                const irct *tp = &tgt[corr[i]];
                const float sd[3] = {s[0] - mean[0], s[1] - mean[1], s[2] - mean[2]};
                const float dd[3] = {tp->x - mean[3], tp->y - mean[4], tp->z - mean[5]};
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) t[a * 3 + b] = dd[a] * sd[b];
            }
            f2_add(fs, t, 0.0);
        }
        f2_flush(fs);
        float sigma[9], R[9], inc[16];
        for (int k = 0; k < 9; ++k) sigma[k] = oon * fs->tf[k];
        memset(inc, 0, sizeof(inc));
        fine_rotation(sigma, R);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) inc[i * 4 + j] = R[i * 3 + j];
            inc[i * 4 + 3] = mean[3 + i] - ((R[i * 3] * mean[0] + R[i * 3 + 1] * mean[1]) + R[i * 3 + 2] * mean[2]);
        }
        inc[15] = 1.0f;
        for (uint32_t i = 0; i < n_src; ++i) {
            float o[3];
            se3(inc, cur + 3 * i, o);
            memcpy(cur + 3 * i, o, sizeof(o));
        }
        matmul4(inc, fin, fin);
        ++iters;
        const double cos_angle = 0.5 * (double)(((inc[0] + inc[5]) + inc[10]) - 1.0f);
        const double trans2 = (double)((inc[3] * inc[3] + inc[7] * inc[7]) + inc[11] * inc[11]);
        if (iters >= p->max_iterations) {
            state = ST_ITERATIONS;
        } else if (cos_angle >= 1.0 - p->transformation_epsilon && trans2 <= p->transformation_epsilon) {
            state = ST_TRANSFORM;
        } else {
            const double mse = mse_sum / (double)cnt;
            if (fabs(mse - prev) < 1e-12) state = ST_ABS_MSE;
            else if (fabs(mse - prev) / prev < p->euclidean_fitness_epsilon) state = ST_REL_MSE;
            else prev = mse;
        }
    }
    f2_init(fs, 0);
    uint32_t nr = 0;
    for (uint32_t i = 0; i < n_src; ++i) {
        double t = 0.0;
        const float q12[12] = {src[i].x, src[i].y, src[i].z};
        float q[4], d;
        uint32_t j;
        se3(fin, q12, q);
        if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && grid_nn(&g, q, -1.0, &j, &d) && isfinite(d)) {
            t = (double)d;
            ++nr;
        }
        f2_add(fs, NULL, t);
    }
    f2_flush(fs);
    res->fitness = nr ? fs->td / (double)nr : DBL_MAX;
    if (isnan(res->fitness)) res->fitness = qnan64();
    for (int k = 0; k < 16; ++k) res->T[k] = canon_f(fin[k]);
    res->iterations = iters;
    res->state = state;
    res->converged = state >= ST_ITERATIONS && state <= ST_REL_MSE;
    grid_free(&g);
    free(cur);
    free(corr);
    free(fs);
}

/* ---- the tools' bookkeeping (BatchTopPartRegistration.cpp:290-309, 508-540) ------------------------------------------ */
/* rotationMatrixToEulerAngles: R row-major 3 x 3 -> (x, y, z) */
void fine_euler(const float *R, float *out)
{
    const float sy = sqrtf(R[0] * R[0] + R[3] * R[3]);
    if (!(sy < 1e-6)) {
        out[0] = atan2f(R[7], R[8]);
        out[1] = atan2f(-R[6], sy);
        out[2] = atan2f(R[3], R[0]);
    } else {
        out[0] = atan2f(-R[5], R[4]);
        out[1] = atan2f(-R[6], sy);
        out[2] = 0.0f;
    }
}

/* Eigen's cofactor inverse of a 3 x 3 (row-major in and out) */
void fine_inverse3(const float *m, float *r)
{
#define M(i, j) m[(i) * 3 + (j)]
#define COF(i, j) (M(((i) + 1) % 3, ((j) + 1) % 3) * M(((i) + 2) % 3, ((j) + 2) % 3) - M(((i) + 1) % 3, ((j) + 2) % 3) * M(((i) + 2) % 3, ((j) + 1) % 3))
    const float c00 = COF(0, 0), c10 = COF(1, 0), c20 = COF(2, 0);
    const float det = (c00 * M(0, 0) + c10 * M(1, 0)) + c20 * M(2, 0);
    const float inv = 1.0f / det;
    r[0] = c00 * inv;
    r[1] = c10 * inv;
    r[2] = c20 * inv;
    r[3] = COF(0, 1) * inv;
    r[4] = COF(1, 1) * inv;
    r[5] = COF(2, 1) * inv;
    r[6] = COF(0, 2) * inv;
    r[7] = COF(1, 2) * inv;
    r[8] = COF(2, 2) * inv;
#undef COF
#undef M
}

/* the top-part tool's report line of a successful match: out = (diff_xy, diff_yaw) */
void fine_report(const float *Tf, const float *Tc, float *out)
{
    const float dx = Tf[3] - Tc[3], dy = Tf[7] - Tc[7];
    out[0] = sqrtf(dx * dx + dy * dy);
    float Rf[9], Rc[9], Ri[9], rel[9], e[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Rf[i * 3 + j] = Tf[i * 4 + j];
            Rc[i * 3 + j] = Tc[i * 4 + j];
        }
    fine_inverse3(Rf, Ri);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            rel[i * 3 + j] = (Ri[i * 3] * Rc[j] + Ri[i * 3 + 1] * Rc[3 + j]) + Ri[i * 3 + 2] * Rc[6 + j];
    fine_euler(rel, e);
    float yaw = (float)((double)e[2] / M_PI * 180.0f);
    if (yaw > 180.0f) yaw -= 360.0f;
    if (yaw < -180.0f) yaw += 360.0f;
    out[1] = yaw;
}
