/* Host build of csrc/bev_exact_eval.h: the dispatch the device hook k_exact_eval runs, on the CPU.  Tests only.
 * Built twice from this one source (Makefile): libexacteval.so as the product's host code is built (-ffp-contract=off), and
 * libexacteval_fma.so with -ffp-contract=fast -mfma — the mutant of the sharpness test, loaded by nothing else. */
#include <cstddef>
#include <cstdint>
#include <xmmintrin.h>

#include "bev_exact_eval.h"

using namespace bevx;

extern "C" {

int ee_count(void) { return kEvCount; }

/* out[0..3] = input kinds (0 none, 1 float, 2 uint32, 3 double), out[4] = 32-bit words per element, out[5] = params; 0 for an unknown id */
int ee_sig(int id, uint8_t *out)
{
    const ExactEvalSig s = exact_eval_sig(id);
    for (int k = 0; k < 4; ++k) out[k] = s.in[k];
    out[4] = s.out_words;
    out[5] = s.params;
    return s.out_words != 0;
}

int ee_eval(int id, size_t n, const void *const *in, const float *prm, uint32_t *out)
{
    const ExactEvalSig s = exact_eval_sig(id);
    if (s.out_words == 0) return -1;
    const float zeros[kEvParams] = {};
    for (size_t i = 0; i < n; ++i) exact_eval_one(id, in, prm ? prm : zeros, i, out + i * s.out_words);
    return 0;
}

/* the same with flush-to-zero (MXCSR bit 15) and denormals-are-zero (bit 6) set for the duration of the call */
int ee_eval_ftz(int id, size_t n, const void *const *in, const float *prm, uint32_t *out)
{
    const unsigned csr = _mm_getcsr();
    _mm_setcsr(csr | 0x8040u);
    const int rc = ee_eval(id, n, in, prm, out);
    _mm_setcsr(csr);
    return rc;
}

/* the plain references of fd_atanf / fd_atan2f: this machine's libm, element by element */
void ee_libm_atanf(size_t n, const float *x, float *out)
{
    for (size_t i = 0; i < n; ++i) out[i] = ::atanf(x[i]);
}
void ee_libm_atan2f(size_t n, const float *y, const float *x, float *out)
{
    for (size_t i = 0; i < n; ++i) out[i] = ::atan2f(y[i], x[i]);
}

/* 1 if this CPU can run libexacteval_fma.so */
int ee_cpu_has_fma(void) { return __builtin_cpu_supports("fma") ? 1 : 0; }

} /* extern "C" */
