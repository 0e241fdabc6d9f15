/*
 * verify_oracle.c — the contract of the verification calls (include/bev_mi355x.h) restated sequentially, with
 * plain loops: the moved query, a brute-force nearest neighbour in both directions, the counts.  No grid, no ballot, no
 * parallelism: what the kernels must equal, byte for byte.  Points are float x, y, z at a stride given in floats.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bev_mi355x.h"

static int searchable(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

/* the smallest float (dx dx + dy dy) + dz dz from a to the searchable points of b (nb of them marked in ok); 0: there is none */
static int nearest(const float *a, const float *b, const uint8_t *ok, uint32_t nb, float *out)
{
    int found = 0;
    float best = INFINITY;
    for (uint32_t j = 0; j < nb; ++j) {
        if (!ok[j]) continue;
        const float dx = a[0] - b[3 * (size_t)j], dy = a[1] - b[3 * (size_t)j + 1], dz = a[2] - b[3 * (size_t)j + 2];
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (!found || d < best) best = d;
        found = 1;
    }
    *out = best;
    return found;
}

/* the points of side a counted against side b */
static void count(const float *a, const uint8_t *aok, uint32_t na, const float *b, const uint8_t *bok, uint32_t nb,
                  const bev_verify_params_t *prm, uint32_t *within)
{
    for (uint32_t i = 0; i < na; ++i) {
        float d;
        if (!aok[i] || !nearest(a + 3 * (size_t)i, b, bok, nb, &d)) continue;
        for (int k = 0; k < prm->n_thresholds; ++k)
            if ((double)d <= (double)prm->threshold[k] * (double)prm->threshold[k]) ++within[k];
    }
}

/* src, tgt: n_src and n_tgt points at src_stride and tgt_stride floats; T: row-major, rows 0 ... 2 read */
void verify_oracle(const float *src, uint32_t n_src, size_t src_stride, const float *tgt, uint32_t n_tgt, size_t tgt_stride,
                   const float *T, const bev_verify_params_t *prm, bev_verify_result_t *out)
{
    float *q = malloc((size_t)(n_src + 1) * 12), *p = malloc((size_t)(n_tgt + 1) * 12);
    uint8_t *qok = malloc((size_t)n_src + 1), *pok = malloc((size_t)n_tgt + 1);
    memset(out, 0, sizeof *out);
    for (uint32_t i = 0; i < n_src; ++i) {
        const float x = src[i * src_stride], y = src[i * src_stride + 1], z = src[i * src_stride + 2];
        for (int r = 0; r < 3; ++r) q[3 * (size_t)i + r] = T[4 * r] * x + (T[4 * r + 1] * y + (T[4 * r + 2] * z + T[4 * r + 3]));
        qok[i] = (uint8_t)searchable(q + 3 * (size_t)i);
        out->n_query += qok[i];
    }
    for (uint32_t j = 0; j < n_tgt; ++j) {
        for (int r = 0; r < 3; ++r) p[3 * (size_t)j + r] = tgt[j * tgt_stride + r];
        pok[j] = (uint8_t)searchable(p + 3 * (size_t)j);
        out->n_target += pok[j];
    }
    count(q, qok, n_src, p, pok, n_tgt, prm, out->query_within);
    count(p, pok, n_tgt, q, qok, n_src, prm, out->target_within);
    free(q);
    free(p);
    free(qok);
    free(pok);
}
