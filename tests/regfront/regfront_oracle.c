/*
 * regfront_oracle.c — plain sequential restatement of the registration front end of the reference's registration
 * tools (TopPartRegistration.cpp / BatchTopPartRegistration.cpp / BatchWholeRegistration.cpp):
 *   extractTopAndFlatten (TopPartRegistration.cpp:79-136)
 *   -> pcl::VoxelGrid<pcl::PointXYZ> (BatchTopPartRegistration.cpp:342-343,405-409)
 *   -> addNormal: Normal2dEstimation in radius mode + concatenateFields (BatchTopPartRegistration.cpp:155-172,
 *      src/Normal2dEstimation.cpp, src/PCA2D.cpp).
 * It follows the contract written in DESIGN.md ("Registration front end") line by line; the GPU must match it bit
 * for bit.  Deliberately naive: O(n^2) neighbour scan, insertion-free qsort on unique keys.
 * Layouts: input points are the 32-byte pcl::PointXYZIRCT records (x@0 y@4 z@8 label@28); PointXYZ is 4 floats
 * (x y z pad), pcl::Normal 8 floats (nx ny nz pad curvature pad pad pad), pcl::PointNormal 12 floats
 * (x y z pad nx ny nz pad curvature pad pad pad); every pad is written as 0.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define RF_GRID 10
#define RF_CELLS (RF_GRID * RF_GRID)
#define RF_MIN_CELL_POINTS 20

typedef struct {
    float x, y, z, pad0, intensity;
    uint16_t row, col;
    uint32_t t;
    int16_t label;
    uint16_t pad1;
} rf_point_t;

static uint32_t canon_nan(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return isnan(f) ? 0x7fc00000u : u;
}
static float fcanon(float f)
{
    uint32_t u = canon_nan(f);
    memcpy(&f, &u, 4);
    return f;
}

static int cmp_u64(const void *a, const void *b)
{
    uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

/* z -> 32-bit key whose ascending order is DESCENDING z (-0 and +0 are one value) */
static uint32_t z_desc_key(float z)
{
    if (z == 0.0f) z = 0.0f;
    uint32_t u;
    memcpy(&u, &z, 4);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

/* the cell of a point, or -1 (label 0, non-finite coordinate, outside the 10 x 10 grid) */
static int top_cell(const rf_point_t *p)
{
    if (p->label == 0) return -1;
    if (!isfinite(p->x) || !isfinite(p->y) || !isfinite(p->z)) return -1;
    const float gx = roundf((p->x + 100.0f) / 20.0f);
    const float gy = roundf((p->y + 100.0f) / 20.0f);
    if (!(gx >= 0.0f && gx < (float)RF_GRID && gy >= 0.0f && gy < (float)RF_GRID)) return -1;
    return (int)gx * RF_GRID + (int)gy;
}

/* extractTopAndFlatten.  out: capacity n/5 + 51 PointXYZ.  Returns the number written. */
uint32_t rf_top_part(const rf_point_t *pts, uint32_t n, float *out)
{
    uint32_t cnt[RF_CELLS] = {0};
    int *cell = (int *)malloc(sizeof(int) * (n ? n : 1));
    for (uint32_t i = 0; i < n; ++i) {
        cell[i] = top_cell(&pts[i]);
        if (cell[i] >= 0) ++cnt[cell[i]];
    }
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * (n ? n : 1));
    uint32_t w = 0;
    for (int c = 0; c < RF_CELLS; ++c) {
        if (cnt[c] < RF_MIN_CELL_POINTS) continue;
        const uint32_t k = (uint32_t)roundf(0.2f * (float)cnt[c]);
        uint32_t m = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (cell[i] == c) keys[m++] = ((uint64_t)z_desc_key(pts[i].z) << 32) | i;
        qsort(keys, m, sizeof(uint64_t), cmp_u64);
        for (uint32_t r = 0; r < k; ++r) {
            const rf_point_t *p = &pts[(uint32_t)keys[r]];
            out[4 * w + 0] = p->x;
            out[4 * w + 1] = p->y;
            out[4 * w + 2] = 0.0f;
            out[4 * w + 3] = 0.0f;
            ++w;
        }
    }
    free(keys);
    free(cell);
    return w;
}

uint32_t rf_max_out(uint64_t n) { return (uint32_t)(n / 5 + 51); }

static int finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

/* pcl::VoxelGrid<PointXYZ>::applyFilter, one leaf size for x, y, z.  Non-finite points are dropped (getMinMax3D and
 * the index loop of a cloud that is not dense).  out: capacity n PointXYZ.  Returns the number written.
 * info (optional, 4 words): overflow flag, div_x, div_y, div_z. */
uint32_t rf_voxel(const float *in, uint32_t n, float leaf, float *out, int64_t *info)
{
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t nf = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float *p = in + 4 * i;
        if (!finite3(p)) continue;
        ++nf;
        for (int d = 0; d < 3; ++d) {
            if (p[d] < mn[d]) mn[d] = p[d];
            if (p[d] > mx[d]) mx[d] = p[d];
        }
    }
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (nf == 0) return 0;
    const float inv = 1.0f / leaf;
    int64_t dd[3];
    int overflow = 0;
    for (int d = 0; d < 3; ++d) {
        const float e = (mx[d] - mn[d]) * inv;
        if (!(e < 9.0e18f)) overflow = 1;
        dd[d] = overflow ? 0 : (int64_t)e + 1;
    }
    if (!overflow) {
        /* (dx * dy * dz) > INT32_MAX, evaluated without wrapping */
        const double prod = (double)dd[0] * (double)dd[1] * (double)dd[2];
        overflow = prod > 2147483647.0;
    }
    if (overflow) {
        memcpy(out, in, sizeof(float) * 4 * (size_t)n);
        if (info) info[0] = 1;
        return n;
    }
    int minb[3], divb[3];
    for (int d = 0; d < 3; ++d) {
        minb[d] = (int)floorf(mn[d] * inv);
        const int maxb = (int)floorf(mx[d] * inv);
        divb[d] = maxb - minb[d] + 1;
    }
    const uint32_t mul1 = (uint32_t)divb[0], mul2 = (uint32_t)divb[0] * (uint32_t)divb[1];
    if (info) {
        info[1] = divb[0];
        info[2] = divb[1];
        info[3] = divb[2];
    }
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * nf);
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float *p = in + 4 * i;
        if (!finite3(p)) continue;
        const uint32_t ijk0 = (uint32_t)(int)(floorf(p[0] * inv) - (float)minb[0]);
        const uint32_t ijk1 = (uint32_t)(int)(floorf(p[1] * inv) - (float)minb[1]);
        const uint32_t ijk2 = (uint32_t)(int)(floorf(p[2] * inv) - (float)minb[2]);
        const uint32_t idx = ijk0 + ijk1 * mul1 + ijk2 * mul2; /* modulo 2^32 */
        keys[m++] = ((uint64_t)idx << 32) | i;
    }
    qsort(keys, m, sizeof(uint64_t), cmp_u64); /* unique keys: (voxel, input index) — a stable sort by voxel */
    uint32_t w = 0;
    for (uint32_t a = 0; a < m;) {
        uint32_t b = a + 1;
        while (b < m && (keys[b] >> 32) == (keys[a] >> 32)) ++b;
        float s[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t q = a; q < b; ++q) {
            const float *p = in + 4 * (uint32_t)keys[q];
            s[0] += p[0];
            s[1] += p[1];
            s[2] += p[2];
        }
        const float cntf = (float)(b - a);
        out[4 * w + 0] = s[0] / cntf;
        out[4 * w + 1] = s[1] / cntf;
        out[4 * w + 2] = s[2] / cntf;
        out[4 * w + 3] = 0.0f;
        ++w;
        a = b;
    }
    free(keys);
    return w;
}

/* Normal2dEstimation::compute(PointCloud<Normal>), radius mode.  out: n pcl::Normal records (8 floats).
 * nn_out (optional): |N| per point. */
void rf_normals(const float *in, uint32_t n, float radius, float vpx, float vpy, float *out, uint32_t *nn_out)
{
    const float r2 = (float)((double)radius * (double)radius);
    uint32_t *nb = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    for (uint32_t q = 0; q < n; ++q) {
        const float qx = in[4 * q], qy = in[4 * q + 1], qz = in[4 * q + 2];
        uint32_t cnt = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const float dx = in[4 * j] - qx, dy = in[4 * j + 1] - qy, dz = in[4 * j + 2] - qz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d <= r2) nb[cnt++] = j;
        }
        if (nn_out) nn_out[q] = cnt;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = 0.0f;
        if (cnt == 1) {
            nx = ny = nz = curv = NAN;
        } else if (cnt == 2) {
            const double vx = (double)(float)(in[4 * nb[0]] - in[4 * nb[1]]);
            const double vy = (double)(float)(in[4 * nb[0] + 1] - in[4 * nb[1] + 1]);
            const double norm = sqrt(vx * vx + vy * vy);
            nx = (float)(-vy / norm);
            ny = (float)(vx / norm);
        } else if (cnt >= 3) {
            float sx = 0.0f, sy = 0.0f;
            for (uint32_t t = 0; t < cnt; ++t) {
                sx += in[4 * nb[t]];
                sy += in[4 * nb[t] + 1];
            }
            const float mx = sx / (float)cnt, my = sy / (float)cnt;
            float a = 0.0f, b = 0.0f, c = 0.0f;
            for (uint32_t t = 0; t < cnt; ++t) {
                const float dx = in[4 * nb[t]] - mx, dy = in[4 * nb[t] + 1] - my;
                a += dx * dx;
                b += dx * dy;
                c += dy * dy;
            }
            double vx, vy;
            const double h = 0.5 * ((double)c - (double)a);
            const double s = sqrt(h * h + (double)b * (double)b);
            if (b == 0.0f) {
                vx = a <= c ? 1.0 : 0.0;
                vy = a <= c ? 0.0 : 1.0;
            } else if (h >= 0.0) {
                vx = h + s;
                vy = -(double)b;
            } else {
                vx = (double)b;
                vy = h - s;
            }
            const double len = sqrt(vx * vx + vy * vy);
            nx = (float)(vx / len);
            ny = (float)(vy / len);
            const float lx = -ny, ly = nx; /* the large eigenvector (-n.y, n.x) */
            curv = ly / (lx + ly);
        }
        if (cnt >= 2) {
            const float cs = (float)((double)(vpx - qx) * (double)nx + (double)(vpy - qy) * (double)ny);
            if (cs < 0.0f) {
                nx = -nx;
                ny = -ny;
                nz = -nz;
            }
        }
        float *o = out + 8 * q;
        o[0] = fcanon(nx);
        o[1] = fcanon(ny);
        o[2] = fcanon(nz);
        o[3] = 0.0f;
        o[4] = fcanon(curv);
        o[5] = o[6] = o[7] = 0.0f;
    }
    free(nb);
}

/* the whole chain for one cloud: top part -> voxel grid -> normals -> PointNormal (12 floats).  out: capacity
 * rf_max_out(n).  Returns the number of records. */
uint32_t rf_chain(const rf_point_t *pts, uint32_t n, float leaf, float radius, float vpx, float vpy, float *out)
{
    const uint32_t cap = rf_max_out(n);
    float *flat = (float *)calloc((size_t)cap * 4, sizeof(float));
    float *vox = (float *)calloc((size_t)cap * 4, sizeof(float));
    const uint32_t m = rf_top_part(pts, n, flat);
    const uint32_t v = rf_voxel(flat, m, leaf, vox, NULL);
    float *nrm = (float *)calloc((size_t)(v ? v : 1) * 8, sizeof(float));
    rf_normals(vox, v, radius, vpx, vpy, nrm, NULL);
    for (uint32_t i = 0; i < v; ++i) {
        float *o = out + 12 * i;
        memcpy(o, vox + 4 * i, 3 * sizeof(float));
        o[3] = 0.0f;
        memcpy(o + 4, nrm + 8 * i, 3 * sizeof(float));
        o[7] = 0.0f;
        o[8] = nrm[8 * i + 4];
        o[9] = o[10] = o[11] = 0.0f;
    }
    free(flat);
    free(vox);
    free(nrm);
    return v;
}
