/*
 * align_oracle.c — sequential checker of the translation guess of retrieved pairs: the contract of
 * include/bev_mi355x.h restated point by point, shift by shift, cell by cell and hypothesis by hypothesis, with plain loops.
 * Tests only.  Of the product it includes csrc/bev_align_exact.h (the cell of a point, the orders, the offset, the entries of a
 * result) and csrc/bev_libm_f64.h (the rotation of a hypothesis) alone, and shares nothing else with the device code: no LDS
 * plane, no packed words, no padding, no reductions.
 *
 * Records are bev_point_t, 32 bytes: x y z at 0 4 8, the int16 label at 28.  A grid is G * G bytes, byte [iy * G + ix].
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bev_align_exact.h"
#include "bev_libm_f64.h"

#define REC 32

typedef struct {
    int32_t grid;
    float cell;
    int32_t max_shift, yaw_steps;
    float yaw_step;
    int32_t skip_label0;
} align_params;

typedef struct {
    float T[16];
    double fitness;
    int32_t converged, iterations, state, _pad;
} icp_result;

typedef struct {
    int32_t dx, dy, k, flip;
    uint32_t score, eq, ec;
    float off_x, off_y;
} align_detail;

extern "C" {

int align_params_admitted(const align_params *p)
{
    return bevx::align_params_ok(p->grid, p->cell, p->max_shift, p->yaw_steps, p->yaw_step, p->skip_label0) ? 1 : 0;
}

/* the points of one cloud, moved by rows 0 ... 2 of pose (12 floats; NULL: the raw coordinates), into grid: a running maximum,
 * so that a map is one call per entry over the same grid (zeroed by the caller) */
void align_accumulate(const uint8_t *pts, uint32_t n, const float *pose12, const align_params *p, float lidar_to_ground,
                      uint8_t *grid)
{
    for (uint32_t i = 0; i < n; ++i) {
        float xyz[3], x, y, z;
        int16_t label;
        memcpy(xyz, pts + (size_t)i * REC, sizeof xyz);
        memcpy(&label, pts + (size_t)i * REC + 28, sizeof label);
        if (pose12) bevx::transform_xyz(pose12, xyz[0], xyz[1], xyz[2], x, y, z);
        else x = xyz[0], y = xyz[1], z = xyz[2];
        const int cell = bevx::align_cell(x, y, label, p->grid, p->cell, p->skip_label0);
        if (cell < 0) continue;
        const int v = bevx::place_value(z, lidar_to_ground);
        if (v > grid[cell]) grid[cell] = (uint8_t)v;
    }
}

uint32_t align_energy(const uint8_t *grid, int G)
{
    uint32_t e = 0;
    for (int i = 0; i < G * G; ++i) e += (uint32_t)grid[i] * grid[i];
    return e;
}

/* score[(dy + S) * (2S + 1) + (dx + S)] of every shift: a candidate byte outside the grid is 0 */
void align_scores(const uint8_t *q, const uint8_t *c, int G, int S, uint32_t *score)
{
    const int side = 2 * S + 1;
    memset(score, 0, (size_t)side * side * sizeof(uint32_t));
    for (int iy = 0; iy < G; ++iy)
        for (int ix = 0; ix < G; ++ix) {
            const uint32_t v = q[iy * G + ix];
            if (!v) continue; /* (an empty cell adds nothing to any shift) */
            for (int dy = -S; dy <= S; ++dy) {
                const int cy = iy + dy;
                if (cy < 0 || cy >= G) continue;
                for (int dx = -S; dx <= S; ++dx) {
                    const int cx = ix + dx;
                    if (cx < 0 || cx >= G) continue;
                    score[(dy + S) * side + (dx + S)] += v * c[cy * G + cx];
                }
            }
        }
}

/* the rotation of hypothesis (k, flip) of a hit: 16 floats */
void align_guess(float angle_guess, int k, float yaw_step, int flip, float *T)
{
    bevx::icp_tool_guess(bevx::align_theta(angle_guess, k, yaw_step), flip, T);
}

/* One hit: the query's records against the candidate's grid (NULL: no candidate, an empty grid).  results[2], detail[2], *best.
 * scores (NULL: not wanted): 2 * (2K + 1) tables of (2S + 1)^2 scores, [flip][k + K]; qgrids (NULL: not wanted): as many grids
 * of the query under each hypothesis. */
void align_hit(const uint8_t *qpts, uint32_t nq, const uint8_t *cgrid, const align_params *p, float lidar_to_ground,
               float angle_guess, icp_result *results, int32_t *best, align_detail *detail, uint32_t *scores, uint8_t *qgrids)
{
    const int G = p->grid, S = p->max_shift, K = p->yaw_steps, side = 2 * S + 1, nk = 2 * K + 1;
    uint8_t *q = (uint8_t *)malloc((size_t)G * G), *c = (uint8_t *)calloc((size_t)G * G, 1);
    uint32_t *sc = (uint32_t *)malloc((size_t)side * side * sizeof(uint32_t));
    if (cgrid) memcpy(c, cgrid, (size_t)G * G);
    const uint32_t ec = align_energy(c, G);
    uint32_t top[2];
    for (int flip = 0; flip < 2; ++flip) {
        int have = 0, bk = 0;
        uint32_t bs = 0, beq = 0, nb[4] = {0, 0, 0, 0};
        int bdx = 0, bdy = 0;
        for (int k = -K; k <= K; ++k) {
            float T[16];
            align_guess(angle_guess, k, p->yaw_step, flip, T);
            memset(q, 0, (size_t)G * G);
            align_accumulate(qpts, nq, T, p, lidar_to_ground, q);
            align_scores(q, c, G, S, sc);
            if (scores) memcpy(scores + ((size_t)flip * nk + (k + K)) * side * side, sc, (size_t)side * side * sizeof(uint32_t));
            if (qgrids) memcpy(qgrids + ((size_t)flip * nk + (k + K)) * G * G, q, (size_t)G * G);
            int dx = -S, dy = -S;
            for (int y = -S; y <= S; ++y)
                for (int x = -S; x <= S; ++x)
                    if (bevx::align_shift_better(sc[(y + S) * side + (x + S)], x, y, sc[(dy + S) * side + (dx + S)], dx, dy))
                        dx = x, dy = y;
            const uint32_t s = sc[(dy + S) * side + (dx + S)];
            if (!have || bevx::align_k_better(s, k, bs, bk)) {
                have = 1, bk = k, bs = s, bdx = dx, bdy = dy, beq = align_energy(q, G);
                nb[0] = dx > -S ? sc[(dy + S) * side + (dx + S - 1)] : 0;
                nb[1] = dx < S ? sc[(dy + S) * side + (dx + S + 1)] : 0;
                nb[2] = dy > -S ? sc[(dy + S - 1) * side + (dx + S)] : 0;
                nb[3] = dy < S ? sc[(dy + S + 1) * side + (dx + S)] : 0;
            }
        }
        const double ox = bevx::align_offset(bdx, S, nb[0], bs, nb[1]), oy = bevx::align_offset(bdy, S, nb[2], bs, nb[3]);
        icp_result *r = results + flip;
        memset(r, 0, sizeof *r);
        align_guess(angle_guess, bk, p->yaw_step, flip, r->T);
        r->T[3] = bevx::align_translation(bdx, ox, p->cell);
        r->T[7] = bevx::align_translation(bdy, oy, p->cell);
        r->fitness = bevx::align_fitness(bs, beq, ec);
        r->converged = bs > 0;
        align_detail *d = detail + flip;
        d->dx = bdx, d->dy = bdy, d->k = bk, d->flip = flip;
        d->score = bs, d->eq = beq, d->ec = ec;
        d->off_x = (float)ox, d->off_y = (float)oy;
        top[flip] = bs;
    }
    *best = bevx::align_best_flip(top[0], top[1]);
    free(q), free(c), free(sc);
}

} /* extern "C" */
