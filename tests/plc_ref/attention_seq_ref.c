/* Long-sequence restatement of orc_attention (oracle/c/oracle.c) for the full-sequence attention tests: the same loop, the
 * same order (score = one fma chain over d ascending from +0, divided by sqrtf(dh); m = max_j; p_j = om_exp(s_j - m); l summed
 * over j ascending; p_j / l; ctx[d] = one fma chain over j ascending), with the probability row in a caller-sized buffer
 * instead of orc_attention's float p[64].  Built by tests/test_gpu_plc.py with the oracle's flags (-ffp-contract=off).
 * Q, ctx [B, H*dh, Tq]; K, V [B, H*dh, Tk]; contiguous. */
#include <math.h>
#include <stdlib.h>
#include <stddef.h>
#include "det_math.h"

int ref_attention_seq(const float* Q, const float* Kx, const float* V, float* ctx, int B, int H, int dh, int Tq, int Tk)
{
    const size_t C = (size_t)H * dh;
    const float rs = sqrtf((float)dh);
    int bad = 0;
#pragma omp parallel for collapse(3) reduction(|:bad)
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < H; ++h)
            for (int i = 0; i < Tq; ++i) {
                float* p = (float*)malloc(sizeof(float) * (size_t)(Tk > 0 ? Tk : 1));
                if (!p) { bad = 1; continue; }
                const float* q = Q + ((size_t)b * C + (size_t)h * dh) * Tq + i;
                const float* kb = Kx + ((size_t)b * C + (size_t)h * dh) * Tk;
                const float* vb = V + ((size_t)b * C + (size_t)h * dh) * Tk;
                float m = -INFINITY;
                for (int j = 0; j < Tk; ++j) {
                    float a = 0.0f;
                    for (int d = 0; d < dh; ++d) a = om_fma(q[(size_t)d * Tq], kb[(size_t)d * Tk + j], a);
                    p[j] = a / rs;
                    m = fmaxf(m, p[j]);
                }
                float l = 0.0f;
                for (int j = 0; j < Tk; ++j) { p[j] = om_exp(p[j] - m); l = l + p[j]; }
                for (int j = 0; j < Tk; ++j) p[j] = p[j] / l;
                for (int d = 0; d < dh; ++d) {
                    float a = 0.0f;
                    for (int j = 0; j < Tk; ++j) a = om_fma(p[j], vb[(size_t)d * Tk + j], a);
                    ctx[((size_t)b * C + (size_t)h * dh + d) * Tq + i] = a;
                }
                free(p);
            }
    return bad ? -1 : 0;
}
