// attention_seq.hip -- full-sequence cross-attention (forward and backward) for the packet-loss-concealment predictor
// (PLC/PLC1.py:349-422: CrossPredictor called once over the whole latent sequence, Tq = Tk = T_lat up to 8192).
//
// Forward: the arithmetic of attention_kernel (kernels_small.hip) and oracle/c/oracle.c::orc_attention, for any length:
//   s_j = (one fma chain over d ascending from +0) / sqrtf(dh);  m = max_j s_j;  e_j = det_exp(s_j - m);
//   l = e_0 + e_1 + ... (j ascending);  p_j = e_j / l;  ctx[d] = one fma chain over j ascending of p_j * V[d][j].
// No MFMA: a matrix core would change the summation order.  So on every shape attention_kernel accepts the two are bit-equal.
// Structure: one block per (batch, head, query tile of QT rows).  The QT probability rows stay resident in LDS (row pitch
// TkP); K and V go through one [dh][KT] LDS tile, K in the score pass and V in the value pass.  QT is the largest of 16, 8, 4,
// 2, 1 whose footprint fits the 160 KiB of a CU (attn_seq_plan); at Tk = 8192, dh = 128 that is QT = 4.
// MASKED (mvq_attention_seq_masked_f32; its backward is below): key j of item b is present when kmask[b*msb + j] != 0.  P keeps its
// pitch and the plan its footprint; absent columns are not staged, the max / exp / value passes skip them and their e_j is
// written as +0, whose addition to l is exact; the value chain is predicated by the tile's ballot of the mask, never
// multiplied.  So the result is the plain kernel's on the compacted K / V, bit for bit, and no present key gives +0.
//
// Backward (not part of the bit-exact contract; checked against float64 autograd): four launches over a caller scratch of
// 2 * B*H*Tq*Tk floats (P and dS), for Tq, Tk <= 512:
//   scores   : one thread per (i, j) pair of a 16x16 tile, Q/G/K/V head slices staged in LDS -> S = QK^T/sqrt(dh), dP = G V^T
//   softmax  : one thread per query row -> P, dS = P * (dP - sum_j dP P) / sqrt(dh)
//   gq       : gQ[d][i] = sum_j dS[i][j] K[d][j]
//   gkv      : gK[d][j] = sum_i dS[i][j] Q[d][i],  gV[d][j] = sum_i P[i][j] G[d][i]
//
// Masked fill (PLC1.py:401-410): zt_in = zt * (~mask) (an IEEE multiply by 1 or 0: -0, NaN and inf behave as in torch),
// z_filled = where(mask, z_pred, zt_in); backward g_zpred = where(mask, g, 0) (torch.where's backward).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "det_math.hpp"
#include "kernels_small.hpp"

namespace mvq {

constexpr int ATT_SEQ_THREADS = 256;
constexpr size_t ATT_SEQ_LDS_FLOATS = 160 * 1024 / sizeof(float);

static inline int attn_seq_pitch(int tk)
{
    int p = (tk + 3) & ~3;                         // 16-byte rows (float4 reads of the l chain)
    if (p % 32 == 0) p += 4;                       // rows of a query tile on different banks in the value pass
    return p;
}

// Query-tile rows, key-tile columns and LDS floats of one launch; false when no tile fits.
bool attn_seq_plan(int dh, int tk, int* qt, int* kt, size_t* lds_floats)
{
    const size_t tkp = (size_t)attn_seq_pitch(tk);
    for (int q = 16; q >= 1; q >>= 1) {
        if ((size_t)dh * q > (size_t)ATT_SEQ_THREADS * 8) continue;          // value-pass outputs: at most 8 per thread
        for (int k = 64; k >= 32; k -= 32) {
            const size_t n = (size_t)dh * q + (size_t)dh * k + (size_t)q * tkp + 16;
            if (n <= ATT_SEQ_LDS_FLOATS) { *qt = q; *kt = k; *lds_floats = n; return true; }
        }
    }
    return false;
}

template <int NPT, bool MASKED>
__global__ __launch_bounds__(ATT_SEQ_THREADS) void attention_seq_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, float* __restrict__ ctx,
    int H, int dh, int Tq, int Tk, int QT, int KT, int TkP, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
    const uint8_t* __restrict__ kmask, size_t msb)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* P = sm;                                 // [QT][TkP]
    float* Ls = P + (size_t)QT * TkP;              // [16] row sums
    float* Qs = Ls + 16;                           // [dh][QT]
    float* T = Qs + dh * QT;                       // [dh][KT]  K tile, then V tile
    const int tid = threadIdx.x;
    const int b = blockIdx.x / H, hd = blockIdx.x - b * H;
    const int i0 = blockIdx.y * QT;
    const int nq = min(QT, Tq - i0);
    const size_t qo = (size_t)b * qsb + (size_t)hd * dh * qsc, ko = (size_t)b * ksb + (size_t)hd * dh * ksc;
    const uint8_t* mk = MASKED ? kmask + (size_t)b * msb : nullptr;          // this item's mask row
    for (int e = tid; e < dh * QT; e += ATT_SEQ_THREADS) {
        const int d = e / QT, i = e - d * QT;
        Qs[e] = i < nq ? Q[qo + (size_t)d * qsc + i0 + i] : 0.0f;
    }
    const float rs = __builtin_sqrtf((float)dh);
    // ---- scores: P[i][j] = chain_d(Q[d][i] K[d][j]) / sqrt(dh) -----------------------------------------------------
    for (int j0 = 0; j0 < Tk; j0 += KT) {
        const int kt = min(KT, Tk - j0);
        __syncthreads();                                                     // previous tile consumed (and Qs written)
        for (int e = tid; e < dh * kt; e += ATT_SEQ_THREADS) {
            const int d = e / kt, jj = e - d * kt;
            T[d * KT + jj] = (!MASKED || mk[j0 + jj] != 0) ? K[ko + (size_t)d * ksc + j0 + jj] : 0.0f;
        }
        __syncthreads();
        for (int p = tid; p < nq * kt; p += ATT_SEQ_THREADS) {
            const int i = p / kt, jj = p - i * kt;
            float a = 0.0f;
            int d = 0;
            for (; d + 8 <= dh; d += 8) {
                float qv[8], kv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { qv[u] = Qs[(d + u) * QT + i]; kv[u] = T[(d + u) * KT + jj]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) a = dfma(qv[u], kv[u], a);
            }
            for (; d < dh; ++d) a = dfma(Qs[d * QT + i], T[d * KT + jj], a);
            P[(size_t)i * TkP + j0 + jj] = a / rs;
        }
    }
    __syncthreads();
    // ---- softmax rows: max (order-free) per wave, exp in parallel, l as ONE chain in j order, divide in parallel --------
    const int wave = tid >> 6, lane = tid & 63;
    if (Tk > 0) {
        for (int i = wave; i < nq; i += ATT_SEQ_THREADS / 64) {
            float* pr = P + (size_t)i * TkP;
            float m = -__builtin_inff();
            for (int j = lane; j < Tk; j += 64) if (!MASKED || mk[j] != 0) m = __builtin_fmaxf(m, pr[j]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o));
            for (int j = lane; j < Tk; j += 64) pr[j] = (!MASKED || mk[j] != 0) ? det_exp(pr[j] - m) : 0.0f;
        }
        __syncthreads();
        if (tid < nq) {
            const float* pr = P + (size_t)tid * TkP;
            float l = 0.0f;
            int j = 0;
            for (; j + 4 <= Tk; j += 4) {
                const float4 v = *reinterpret_cast<const float4*>(pr + j);
                l = l + v.x; l = l + v.y; l = l + v.z; l = l + v.w;
            }
            for (; j < Tk; ++j) l = l + pr[j];
            Ls[tid] = l;
        }
        __syncthreads();
        for (int e = tid; e < nq * Tk; e += ATT_SEQ_THREADS) {
            const int i = e / Tk, j = e - i * Tk;
            if (!MASKED || mk[j] != 0) P[(size_t)i * TkP + j] = P[(size_t)i * TkP + j] / Ls[i];
        }
    }
    // ---- values: ctx[d][i] = chain_j(P[i][j] V[d][j]), NPT outputs per thread held across the V tiles -----------------
    float acc[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) acc[u] = 0.0f;
    for (int j0 = 0; j0 < Tk; j0 += KT) {
        const int kt = min(KT, Tk - j0);
        __syncthreads();                                                     // P final / previous V tile consumed
        for (int e = tid; e < dh * kt; e += ATT_SEQ_THREADS) {
            const int d = e / kt, jj = e - d * kt;
            T[d * KT + jj] = (!MASKED || mk[j0 + jj] != 0) ? V[ko + (size_t)d * ksc + j0 + jj] : 0.0f;
        }
        __syncthreads();
        unsigned long long tm = ~0ull;                                       // present keys of this tile (kt <= 64: one ballot)
        if (MASKED) tm = __ballot(lane < kt && mk[j0 + lane] != 0);
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
            const int o = tid + u * ATT_SEQ_THREADS;
            const int d = o / QT, i = o - d * QT;
            if (d < dh && i < nq) {
                const float* pr = P + (size_t)i * TkP + j0;
                const float* vr = T + d * KT;
                float a = acc[u];
                if (MASKED) {
                    for (int jj = 0; jj < kt; ++jj) if ((tm >> jj) & 1ull) a = dfma(pr[jj], vr[jj], a);
                } else {
                    for (int jj = 0; jj < kt; ++jj) a = dfma(pr[jj], vr[jj], a);
                }
                acc[u] = a;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
        const int o = tid + u * ATT_SEQ_THREADS;
        const int d = o / QT, i = o - d * QT;
        if (d < dh && i < nq) ctx[qo + (size_t)d * qsc + i0 + i] = acc[u];
    }
}

// kmask == NULL: the plain kernels; otherwise the masked instantiations (same grid, same plan)
static hipError_t launch_attention_seq_any(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                           int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                           size_t msb, hipStream_t s)
{
    if (B * H == 0 || Tq == 0) return hipSuccess;
    int qt = 0, kt = 0;
    size_t nf = 0;
    if (!attn_seq_plan(dh, Tk, &qt, &kt, &nf)) return hipErrorInvalidValue;
    const int npt = (dh * qt + ATT_SEQ_THREADS - 1) / ATT_SEQ_THREADS;
    hipError_t e;
    if (!kmask) {
        static BigLdsOptIn o1, o2, o4, o8;
        e = o1.ensure(reinterpret_cast<const void*>(attention_seq_kernel<1, false>));
        if (e == hipSuccess) e = o2.ensure(reinterpret_cast<const void*>(attention_seq_kernel<2, false>));
        if (e == hipSuccess) e = o4.ensure(reinterpret_cast<const void*>(attention_seq_kernel<4, false>));
        if (e == hipSuccess) e = o8.ensure(reinterpret_cast<const void*>(attention_seq_kernel<8, false>));
    } else {
        static BigLdsOptIn m1, m2, m4, m8;
        e = m1.ensure(reinterpret_cast<const void*>(attention_seq_kernel<1, true>));
        if (e == hipSuccess) e = m2.ensure(reinterpret_cast<const void*>(attention_seq_kernel<2, true>));
        if (e == hipSuccess) e = m4.ensure(reinterpret_cast<const void*>(attention_seq_kernel<4, true>));
        if (e == hipSuccess) e = m8.ensure(reinterpret_cast<const void*>(attention_seq_kernel<8, true>));
    }
    if (e != hipSuccess) return e;
    const dim3 grid(B * H, (Tq + qt - 1) / qt);
    const size_t lds = nf * sizeof(float);
    const int tkp = attn_seq_pitch(Tk);
    const int pi = prof_enabled() ? prof_begin(kmask ? "attention_seq_masked_kernel" : "attention_seq_kernel",
                                               4.0 * B * H * (double)Tq * Tk * dh, s) : -1;
#define MVQ_ATT_SEQ(N, M) hipLaunchKernelGGL((attention_seq_kernel<N, M>), grid, dim3(ATT_SEQ_THREADS), lds, s, q, k, v, ctx, H, dh, Tq, \
                                             Tk, qt, kt, tkp, qsb, qsc, ksb, ksc, kmask, msb)
    if (!kmask) {
        if (npt <= 1) MVQ_ATT_SEQ(1, false);
        else if (npt <= 2) MVQ_ATT_SEQ(2, false);
        else if (npt <= 4) MVQ_ATT_SEQ(4, false);
        else MVQ_ATT_SEQ(8, false);
    } else {
        if (npt <= 1) MVQ_ATT_SEQ(1, true);
        else if (npt <= 2) MVQ_ATT_SEQ(2, true);
        else if (npt <= 4) MVQ_ATT_SEQ(4, true);
        else MVQ_ATT_SEQ(8, true);
    }
#undef MVQ_ATT_SEQ
    e = hipGetLastError();
    prof_end(pi, s);
    return e;
}

hipError_t launch_attention_seq(const float* q, const float* k, const float* v, float* ctx,
                                int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                hipStream_t s)
{
    return launch_attention_seq_any(q, k, v, nullptr, ctx, B, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, 0, s);
}

hipError_t launch_attention_seq_masked(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                       int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                       size_t msb, hipStream_t s)
{
    return launch_attention_seq_any(q, k, v, kmask, ctx, B, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, msb, s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int ASB_T = 16;      // 16 x 16 (i, j) pairs per block of the score pass

// MASKED (mvq_attention_seq_masked_bwd_f32): key j of item b is present when kmask[b*msb + j] != 0.  The scratch keeps its
// [B*H][Tq][Tk] layout.  Absent columns are never loaded: the score pass writes S = dP = +0 there, the softmax pass skips
// them in max, l, dot and the final row (so P = dS = +0 stay), the gQ chain is predicated on presence (never multiplied:
// NaN in an absent column cannot leak) and the gK / gV pass stores +0 without running the chains.  Every chain then takes
// the present columns in ascending order: the plain launch on the compacted K / V, bit for bit.
template <bool MASKED>
__global__ __launch_bounds__(256) void attention_seq_bwd_scores_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, const float* __restrict__ G,
    float* __restrict__ S, float* __restrict__ dP, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
    const uint8_t* __restrict__ kmask, size_t msb)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qs = sm;                    // [dh][16]
    float* Gs = Qs + dh * ASB_T;       // [dh][16]
    float* Ks = Gs + dh * ASB_T;       // [dh][16]
    float* Vs = Ks + dh * ASB_T;       // [dh][16]
    const int tid = threadIdx.x;
    const int bh = blockIdx.x, b = bh / H, hd = bh - b * H;
    const int i0 = blockIdx.y * ASB_T, j0 = blockIdx.z * ASB_T;
    const int nq = min(ASB_T, Tq - i0), nk = min(ASB_T, Tk - j0);
    const size_t qo = (size_t)b * qsb + (size_t)hd * dh * qsc, ko = (size_t)b * ksb + (size_t)hd * dh * ksc;
    for (int e = tid; e < dh * ASB_T; e += 256) {
        const int d = e / ASB_T, x = e - d * ASB_T;
        const bool iq = x < nq, ik = x < nk && (!MASKED || kmask[(size_t)b * msb + j0 + x] != 0);
        Qs[e] = iq ? Q[qo + (size_t)d * qsc + i0 + x] : 0.0f;
        Gs[e] = iq ? G[qo + (size_t)d * qsc + i0 + x] : 0.0f;
        Ks[e] = ik ? K[ko + (size_t)d * ksc + j0 + x] : 0.0f;
        Vs[e] = ik ? V[ko + (size_t)d * ksc + j0 + x] : 0.0f;
    }
    __syncthreads();
    const int i = tid / ASB_T, j = tid - i * ASB_T;
    if (i >= nq || j >= nk) return;
    const float rs = __builtin_sqrtf((float)dh);
    float a = 0.0f, dp = 0.0f;
    for (int d = 0; d < dh; ++d) {
        a = dfma(Qs[d * ASB_T + i], Ks[d * ASB_T + j], a);
        dp = dfma(Gs[d * ASB_T + i], Vs[d * ASB_T + j], dp);
    }
    const size_t r = ((size_t)bh * Tq + i0 + i) * Tk + j0 + j;
    if (MASKED && kmask[(size_t)b * msb + j0 + j] == 0) { S[r] = 0.0f; dP[r] = 0.0f; return; }
    S[r] = a / rs;
    dP[r] = dp;
}

// rows_per_item = H * Tq: row r belongs to item r / rows_per_item (MASKED only)
template <bool MASKED>
__global__ void attention_seq_bwd_softmax_kernel(float* __restrict__ S, float* __restrict__ dP, int rows, int Tk, float rs,
                                                 const uint8_t* __restrict__ kmask, size_t msb, int rows_per_item)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float* pr = S + (size_t)r * Tk;
    float* dr = dP + (size_t)r * Tk;
    if (MASKED) {
        const uint8_t* mk = kmask + (size_t)(r / rows_per_item) * msb;
        float m = -__builtin_inff();
        for (int j = 0; j < Tk; ++j) if (mk[j] != 0) m = __builtin_fmaxf(m, pr[j]);
        float l = 0.0f;
        for (int j = 0; j < Tk; ++j) if (mk[j] != 0) { const float e = det_exp(pr[j] - m); pr[j] = e; l += e; }
        float dot = 0.0f;
        for (int j = 0; j < Tk; ++j) if (mk[j] != 0) { pr[j] = pr[j] / l; dot = dfma(dr[j], pr[j], dot); }
        for (int j = 0; j < Tk; ++j) if (mk[j] != 0) dr[j] = pr[j] * (dr[j] - dot) / rs;
        return;
    }
    float m = -__builtin_inff();
    for (int j = 0; j < Tk; ++j) m = __builtin_fmaxf(m, pr[j]);
    float l = 0.0f;
    for (int j = 0; j < Tk; ++j) { const float e = det_exp(pr[j] - m); pr[j] = e; l += e; }
    float dot = 0.0f;
    for (int j = 0; j < Tk; ++j) { pr[j] = pr[j] / l; dot = dfma(dr[j], pr[j], dot); }
    for (int j = 0; j < Tk; ++j) dr[j] = pr[j] * (dr[j] - dot) / rs;      // dL/d(QK^T), with the 1/sqrt(dh)
}

// gQ[d][i] = sum_j dS[i][j] K[d][j]: one thread per (bh, d, i), i fastest
template <bool MASKED>
__global__ void attention_seq_bwd_gq_kernel(const float* __restrict__ K, const float* __restrict__ dS, float* __restrict__ gQ,
                                            int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                            const uint8_t* __restrict__ kmask, size_t msb)
{
    const size_t n = (size_t)B * H * dh * Tq;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e % Tq);
        const size_t r = e / Tq;
        const int d = (int)(r % dh);
        const int bh = (int)(r / dh), b = bh / H, hd = bh - b * H;
        const float* kr = K + (size_t)b * ksb + ((size_t)hd * dh + d) * ksc;
        const float* sr = dS + ((size_t)bh * Tq + i) * Tk;
        float a = 0.0f;
        if (MASKED) {
            const uint8_t* mk = kmask + (size_t)b * msb;
            for (int j = 0; j < Tk; ++j) if (mk[j] != 0) a = dfma(sr[j], kr[j], a);
        } else {
            for (int j = 0; j < Tk; ++j) a = dfma(sr[j], kr[j], a);
        }
        gQ[(size_t)b * qsb + ((size_t)hd * dh + d) * qsc + i] = a;
    }
}

// gK[d][j] = sum_i dS[i][j] Q[d][i],  gV[d][j] = sum_i P[i][j] G[d][i]: one thread per (bh, d, j), j fastest
template <bool MASKED>
__global__ void attention_seq_bwd_gkv_kernel(const float* __restrict__ Q, const float* __restrict__ G, const float* __restrict__ P,
                                             const float* __restrict__ dS, float* __restrict__ gK, float* __restrict__ gV,
                                             int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                             const uint8_t* __restrict__ kmask, size_t msb)
{
    const size_t n = (size_t)B * H * dh * Tk;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % Tk);
        const size_t r = e / Tk;
        const int d = (int)(r % dh);
        const int bh = (int)(r / dh), b = bh / H, hd = bh - b * H;
        const size_t qr = (size_t)b * qsb + ((size_t)hd * dh + d) * qsc;
        const float* pc = P + (size_t)bh * Tq * Tk + j;
        const float* sc = dS + (size_t)bh * Tq * Tk + j;
        float a = 0.0f, c = 0.0f;
        if (!MASKED || kmask[(size_t)b * msb + j] != 0) {
            for (int i = 0; i < Tq; ++i) {
                a = dfma(sc[(size_t)i * Tk], Q[qr + i], a);
                c = dfma(pc[(size_t)i * Tk], G[qr + i], c);
            }
        }
        const size_t o = (size_t)b * ksb + ((size_t)hd * dh + d) * ksc + j;
        gK[o] = a;
        gV[o] = c;
    }
}

static inline unsigned grid_for(size_t n)
{
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

// kmask == NULL: the plain kernels; otherwise the masked instantiations (same grids, same scratch)
static hipError_t launch_attention_seq_bwd_any(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                               float* gq, float* gk, float* gv, float* scratch, int B, int H, int dh, int Tq, int Tk,
                                               size_t qsb, size_t qsc, size_t ksb, size_t ksc, size_t msb, hipStream_t s)
{
    if (B * H == 0 || Tq == 0) return hipSuccess;
    if (Tk == 0) {                                           // ctx = 0 whatever Q is: gQ = 0 (no keys: no gK / gV)
        hipLaunchKernelGGL(attention_seq_bwd_gq_kernel<false>, dim3(grid_for((size_t)B * H * dh * Tq)), dim3(256), 0, s,
                           k, scratch, gq, B, H, dh, Tq, 0, qsb, qsc, ksb, ksc, (const uint8_t*)nullptr, (size_t)0);
        return hipGetLastError();
    }
    const size_t lds = (size_t)4 * dh * ASB_T * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    float* S = scratch;
    float* dS = scratch + (size_t)B * H * Tq * Tk;
    const int pi = prof_enabled() ? prof_begin(kmask ? "attention_seq_masked_bwd (4 kernels)" : "attention_seq_bwd (4 kernels)",
                                               8.0 * B * H * (double)Tq * Tk * dh, s) : -1;
    const dim3 sgrid(B * H, (Tq + ASB_T - 1) / ASB_T, (Tk + ASB_T - 1) / ASB_T);
    const int rows = B * H * Tq;
    const float rs = __builtin_sqrtf((float)dh);
#define MVQ_ATT_SEQ_BWD(M)                                                                                                            \
    do {                                                                                                                              \
        hipLaunchKernelGGL(attention_seq_bwd_scores_kernel<M>, sgrid, dim3(256), lds, s,                                              \
                           q, k, v, g, S, dS, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, kmask, msb);                                         \
        hipLaunchKernelGGL(attention_seq_bwd_softmax_kernel<M>, dim3((rows + 63) / 64), dim3(64), 0, s, S, dS, rows, Tk, rs,          \
                           kmask, msb, H * Tq);                                                                                       \
        hipLaunchKernelGGL(attention_seq_bwd_gq_kernel<M>, dim3(grid_for((size_t)B * H * dh * Tq)), dim3(256), 0, s,                  \
                           k, dS, gq, B, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, kmask, msb);                                              \
        hipLaunchKernelGGL(attention_seq_bwd_gkv_kernel<M>, dim3(grid_for((size_t)B * H * dh * Tk)), dim3(256), 0, s,                 \
                           q, g, S, dS, gk, gv, B, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, kmask, msb);                                    \
    } while (0)
    if (kmask) MVQ_ATT_SEQ_BWD(true);
    else MVQ_ATT_SEQ_BWD(false);
#undef MVQ_ATT_SEQ_BWD
    const hipError_t e = hipGetLastError();
    prof_end(pi, s);
    return e;
}

hipError_t launch_attention_seq_bwd(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                                    float* scratch, int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb,
                                    size_t ksc, hipStream_t s)
{
    return launch_attention_seq_bwd_any(q, k, v, nullptr, g, gq, gk, gv, scratch, B, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, 0, s);
}

// kmask != NULL, Tk > 0 (the entry point sends the other cases to launch_attention_seq_bwd)
hipError_t launch_attention_seq_masked_bwd(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                           float* gq, float* gk, float* gv, float* scratch, int B, int H, int dh, int Tq, int Tk,
                                           size_t qsb, size_t qsc, size_t ksb, size_t ksc, size_t msb, hipStream_t s)
{
    return launch_attention_seq_bwd_any(q, k, v, kmask, g, gq, gk, gv, scratch, B, H, dh, Tq, Tk, qsb, qsc, ksb, ksc, msb, s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// masked fill
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void plc_mask_fill_kernel(const float* __restrict__ zt, const float* __restrict__ zp, const uint8_t* __restrict__ mask,
                                     float* __restrict__ zt_in, float* __restrict__ zf, int C, int T, size_t n, size_t sb, size_t sc)
{
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(e % T);
        const size_t r = e / T;
        const int c = (int)(r % C), b = (int)(r / C);
        const size_t o = (size_t)b * sb + (size_t)c * sc + t;
        const bool m = mask[(size_t)b * T + t] != 0;
        const float x = zt[o] * (m ? 0.0f : 1.0f);            // zt * (~mask): a multiply, as torch's bool promotion
        if (zt_in) zt_in[o] = x;
        if (zf) zf[o] = m ? zp[o] : x;
    }
}

__global__ void plc_mask_fill_bwd_kernel(const float* __restrict__ g, const uint8_t* __restrict__ mask, float* __restrict__ gzp,
                                         int C, int T, size_t n, size_t sb, size_t sc)
{
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(e % T);
        const size_t r = e / T;
        const int c = (int)(r % C), b = (int)(r / C);
        const size_t o = (size_t)b * sb + (size_t)c * sc + t;
        gzp[o] = mask[(size_t)b * T + t] ? g[o] : 0.0f;
    }
}

hipError_t launch_plc_mask_fill(const float* zt, const float* zp, const uint8_t* mask, float* zt_in, float* zf,
                                int B, int C, int T, size_t sb, size_t sc, hipStream_t s)
{
    const size_t n = (size_t)B * C * T;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(plc_mask_fill_kernel, dim3(grid_for(n)), dim3(256), 0, s, zt, zp, mask, zt_in, zf, C, T, n, sb, sc);
    return hipGetLastError();
}

hipError_t launch_plc_mask_fill_bwd(const float* g, const uint8_t* mask, float* gzp, int B, int C, int T, size_t sb, size_t sc,
                                    hipStream_t s)
{
    const size_t n = (size_t)B * C * T;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(plc_mask_fill_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, g, mask, gzp, C, T, n, sb, sc);
    return hipGetLastError();
}

}  // namespace mvq
