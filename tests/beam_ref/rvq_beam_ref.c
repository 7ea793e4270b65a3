/* rvq_beam_ref.c -- C restatement of the sender's beam search over the books (include/mvq.h: mvq_rvq_beam_f32), straight from the
 * rule: every candidate pair is keyed and the whole list is sorted; nothing of the kernel's tiling or its running selection.
 * Build with -ffp-contract=off: every fused multiply-add is an explicit fmaf, every other step one fp32 operation.
 *
 *   z[B, D, T] contiguous, books[nb, K, D] -> idx int32 [nb, B*T], slot uint8 [B*T], energy float [B*T]; 0, or -1 on a bad shape. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BEAM_MAX 8

typedef struct { float key; int j, k; } cand_t;

static float energy(const float* r, int D)
{
    float E = 0.0f;
    for (int d = 0; d < D; ++d) { const float p = r[d] * r[d]; E = E + p; }
    return E;
}

static float half_norm(const float* e, int D)
{
    float s = 0.0f;
    for (int d = 0; d < D; ++d) s = fmaf(e[d], e[d], s);
    return 0.5f * s;
}

static float score(const float* r, const float* e, float h, int D)
{
    float dot = 0.0f;
    for (int d = 0; d < D; ++d) dot = fmaf(r[d], e[d], dot);
    return dot - h;
}

/* a number before a NaN, then key ascending, then slot, then code */
static int before(const void* pa, const void* pb)
{
    const cand_t* a = (const cand_t*)pa; const cand_t* b = (const cand_t*)pb;
    const int an = isnan(a->key), bn = isnan(b->key);
    if (an != bn) return an ? 1 : -1;
    if (!an && a->key != b->key) return a->key < b->key ? -1 : 1;
    if (a->j != b->j) return a->j < b->j ? -1 : 1;
    return a->k < b->k ? -1 : (a->k > b->k ? 1 : 0);
}

int ref_rvq_beam(const float* z, const float* books, int32_t* idx, uint8_t* slot, float* energy_out, int B, int D, int T, int nb,
                 int K, int beam)
{
    if (beam < 1 || beam > BEAM_MAX || D <= 0 || K <= 0 || nb < 0 || B < 0 || T < 0) return -1;
    const int M = beam;
    const long long N = (long long)B * T;
    cand_t* cand = (cand_t*)malloc(sizeof(cand_t) * (size_t)BEAM_MAX * (size_t)K);
    float* R = (float*)malloc(sizeof(float) * 2 * BEAM_MAX * (size_t)D);
    int* path = (int*)malloc(sizeof(int) * 2 * BEAM_MAX * (size_t)(nb > 0 ? nb : 1));
    float* hn = (float*)malloc(sizeof(float) * (size_t)(nb > 0 ? nb : 1) * (size_t)K);
    if (!cand || !R || !path || !hn) { free(cand); free(R); free(path); free(hn); return -1; }
    for (size_t i = 0; i < (size_t)nb * K; ++i) hn[i] = half_norm(books + i * D, D);
    for (long long n = 0; n < N; ++n) {
        const int b = (int)(n / T), t = (int)(n % T);
        float* rc = R; float* rn = R + (size_t)BEAM_MAX * D;
        int* pc = path; int* pn = path + (size_t)BEAM_MAX * (nb > 0 ? nb : 1);
        float J[BEAM_MAX], Jn[BEAM_MAX];
        for (int d = 0; d < D; ++d) rc[d] = z[((size_t)b * D + d) * T + t];
        J[0] = energy(rc, D);
        int L = 1;
        for (int m = 0; m < nb; ++m) {
            const float* emb = books + (size_t)m * K * D;
            /* slot 0: the greedy lineage */
            float best = -INFINITY; int ks = 0;
            for (int k = 0; k < K; ++k) {
                const float s = score(rc, emb + (size_t)k * D, hn[(size_t)m * K + k], D);
                if (s > best) { best = s; ks = k; }
            }
            /* the other slots: every pair except (0, k*), keyed and sorted */
            int nc = 0;
            for (int j = 0; j < L; ++j)
                for (int k = 0; k < K; ++k) {
                    if (j == 0 && k == ks) continue;
                    const float s = score(rc + (size_t)j * D, emb + (size_t)k * D, hn[(size_t)m * K + k], D);
                    const float two = 2.0f * s;
                    cand[nc].key = J[j] - two; cand[nc].j = j; cand[nc].k = k;
                    ++nc;
                }
            qsort(cand, (size_t)nc, sizeof(cand_t), before);
            const long long lk = (long long)L * K;
            const int Ln = lk < M ? (int)lk : M;
            for (int s = 0; s < Ln; ++s) {
                const int j = s == 0 ? 0 : cand[s - 1].j, k = s == 0 ? ks : cand[s - 1].k;
                const float* e = emb + (size_t)k * D;
                for (int d = 0; d < D; ++d) rn[(size_t)s * D + d] = rc[(size_t)j * D + d] - e[d];
                Jn[s] = energy(rn + (size_t)s * D, D);
                memcpy(pn + (size_t)s * nb, pc + (size_t)j * nb, sizeof(int) * (size_t)m);
                pn[(size_t)s * nb + m] = k;
            }
            float* tr = rc; rc = rn; rn = tr;
            int* tp = pc; pc = pn; pn = tp;
            memcpy(J, Jn, sizeof(float) * (size_t)Ln);
            L = Ln;
        }
        int w = 0; float Jw = J[0];
        for (int s = 1; s < L; ++s) if (J[s] < Jw) { Jw = J[s]; w = s; }
        for (int m = 0; m < nb; ++m) idx[(size_t)m * N + n] = pc[(size_t)w * nb + m];
        if (slot) slot[n] = (uint8_t)w;
        if (energy_out) energy_out[n] = Jw;
    }
    free(cand); free(R); free(path); free(hn);
    return 0;
}
