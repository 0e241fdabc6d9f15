/*
 * place_oracle.c — sequential checker of place retrieval: the contract of include/bev_mi355x.h restated point
 * by point, column by column, shift by shift and candidate by candidate, with plain loops and a sort.  Tests only.  Of the
 * product it includes csrc/bev_place_exact.h alone — the cell and the value of a point, a unit value, the comparison of two
 * scores, the distance and the angle — and shares nothing else with the device code: no LDS plane, no packed dot products, no
 * masks, no reductions.
 *
 * Records are bev_point_t, 32 bytes: x y z at 0 4 8, the int16 label at 28.  A descriptor is n_rings * n_sectors bytes,
 * ring-major.  A handle is the product's opaque record, restated: 64 columns of 32 bytes (ring r of column s at s * 32 + r),
 * the 64-bit mask of non-empty columns at 2048, zeros to 2112.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bev_place_exact.h"

#define REC 32
#define HANDLE 2112

typedef struct {
    int32_t n_rings, n_sectors;
    float max_range;
    int32_t skip_label0;
} place_params;

typedef struct {
    int32_t query_idx, match_idx;
    float angle_guess;
    int32_t shift;
    double distance;
} place_hit;

extern "C" {

/* the points of one cloud, moved by pose12 (NULL: the raw coordinates), into desc: a running maximum, so that a map is one call
 * per entry over the same descriptor (zeroed by the caller) */
void place_accumulate(const uint8_t *pts, uint32_t n, const float *pose12, const place_params *p, float lidar_to_ground,
                      uint8_t *desc)
{
    float edge2[bevx::kPlaceMaxRings + 1];
    bevx::place_edges(p->n_rings, p->max_range, edge2);
    for (uint32_t i = 0; i < n; ++i) {
        float xyz[3], x, y, z;
        int16_t label;
        memcpy(xyz, pts + (size_t)i * REC, sizeof xyz);
        memcpy(&label, pts + (size_t)i * REC + 28, sizeof label);
        if (pose12) bevx::transform_xyz(pose12, xyz[0], xyz[1], xyz[2], x, y, z);
        else x = xyz[0], y = xyz[1], z = xyz[2];
        const int cell = bevx::place_cell(edge2, p->n_rings, p->n_sectors, x, y, label, p->skip_label0);
        if (cell < 0) continue;
        const int v = bevx::place_value(z, lidar_to_ground);
        if (v > desc[cell]) desc[cell] = (uint8_t)v;
    }
}

/* unit[s * n_rings + r] of a descriptor's columns, nonempty[s] */
static void unit_columns(const uint8_t *desc, int R, int C, int32_t *unit, int32_t *nonempty)
{
    for (int s = 0; s < C; ++s) {
        int n2 = 0;
        for (int r = 0; r < R; ++r) n2 += (int)desc[r * C + s] * (int)desc[r * C + s];
        nonempty[s] = n2 > 0;
        for (int r = 0; r < R; ++r) unit[s * R + r] = n2 > 0 ? bevx::place_unit(desc[r * C + s], n2) : 0;
    }
}

void place_handle(const uint8_t *desc, int R, int C, uint8_t *handle)
{
    int32_t unit[64 * 32], nonempty[64];
    uint64_t mask = 0;
    unit_columns(desc, R, C, unit, nonempty);
    memset(handle, 0, HANDLE);
    for (int s = 0; s < C; ++s) {
        for (int r = 0; r < R; ++r) handle[s * 32 + r] = (uint8_t)unit[s * R + r];
        if (nonempty[s]) mask |= (uint64_t)1 << s;
    }
    memcpy(handle + 2048, &mask, sizeof mask);
}

/* every shift of a pair: S[n], cnt[n] (n_sectors values each) */
static void pair_shifts(const int32_t *uq, const int32_t *eq, const int32_t *uc, const int32_t *ec, int R, int C, int32_t *S,
                        int32_t *cnt)
{
    for (int n = 0; n < C; ++n) {
        int64_t s = 0;
        int32_t k = 0;
        for (int j = 0; j < C; ++j) {
            const int jc = (j + n) % C;
            for (int r = 0; r < R; ++r) s += (int64_t)uq[j * R + r] * uc[jc * R + r];
            k += eq[j] && ec[jc];
        }
        S[n] = (int32_t)s;
        cnt[n] = k;
    }
}
void place_pair_shifts(const uint8_t *dq, const uint8_t *dc, int R, int C, int32_t *S, int32_t *cnt)
{
    int32_t uq[64 * 32], uc[64 * 32], eq[64], ec[64];
    unit_columns(dq, R, C, uq, eq);
    unit_columns(dc, R, C, uc, ec);
    pair_shifts(uq, eq, uc, ec, R, C, S, cnt);
}

typedef struct {
    int32_t s, cnt, shift, idx;
} score;
static int by_rank(const void *a, const void *b)
{
    const score *x = (const score *)a, *y = (const score *)b;
    if (bevx::place_better(x->s, x->cnt, x->idx, y->s, y->cnt, y->idx)) return -1;
    return bevx::place_better(y->s, y->cnt, y->idx, x->s, x->cnt, x->idx) ? 1 : 0;
}

/* hits[q * top_k + k]: descriptors n_rings * n_sectors bytes each; limit NULL: all of the database */
void place_match(const uint8_t *dq, int nq, const uint8_t *ddb, int ndb, const int32_t *limit, int top_k, int R, int C,
                 place_hit *hits)
{
    const size_t cells = (size_t)R * C;
    int32_t *udb = (int32_t *)malloc(((size_t)ndb + 1) * cells * sizeof(int32_t));
    int32_t *edb = (int32_t *)malloc(((size_t)ndb + 1) * 64 * sizeof(int32_t));
    score *sc = (score *)malloc(((size_t)ndb + 1) * sizeof(score));
    for (int c = 0; c < ndb; ++c) unit_columns(ddb + c * cells, R, C, udb + c * cells, edb + (size_t)c * 64);
    for (int q = 0; q < nq; ++q) {
        int32_t uq[64 * 32], eq[64], S[64], cnt[64];
        const int lim = limit ? limit[q] : ndb;
        unit_columns(dq + q * cells, R, C, uq, eq);
        for (int c = 0; c < lim; ++c) {
            pair_shifts(uq, eq, udb + c * cells, edb + (size_t)c * 64, R, C, S, cnt);
            int best = 0;
            for (int n = 1; n < C; ++n)
                if (bevx::place_better(S[n], cnt[n], n, S[best], cnt[best], best)) best = n;
            sc[c].s = S[best], sc[c].cnt = cnt[best], sc[c].shift = best, sc[c].idx = c;
        }
        qsort(sc, (size_t)lim, sizeof(score), by_rank);
        for (int k = 0; k < top_k; ++k) {
            place_hit *h = hits + (size_t)q * top_k + k;
            memset(h, 0, sizeof *h);
            h->query_idx = q;
            if (k < lim) {
                h->match_idx = sc[k].idx;
                h->angle_guess = bevx::place_angle(sc[k].shift, C);
                h->shift = sc[k].shift;
                h->distance = bevx::place_distance(sc[k].s, sc[k].cnt);
            } else {
                h->match_idx = -1;
                h->distance = 2.0;
            }
        }
    }
    free(udb), free(edb), free(sc);
}

} /* extern "C" */
