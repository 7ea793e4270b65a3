// rvq_beam.hip -- beam search over the books of ResidualVQEMA at the sender (include/mvq.h: mvq_rvq_beam_f32).
//
// The greedy search (kernels_vq.hip) keeps one residual per token; this one keeps up to `beam` (M <= 8) slots per token, each a
// (path, residual, J = E(residual)), and returns the path whose FINAL residual is smallest.  Slot 0 is always the greedy lineage, so
// M = 1 is the greedy search index for index and the winner is never worse than it; the indices cost nothing on the wire.
//
// One block owns `toks` tokens (1 while that leaves CUs without a block, at most 8, as many as fit the LDS beside the codebook
// image) for ALL books; with few tokens the four waves split the resident codes of a token, with many each wave takes a token.
// Per book and 256-code slice the codebook sits in LDS in rvq_ema_forward_kernel's transposed odd-pitch image; every (token, slot)
// is a column scored exactly as that kernel scores a token (lane = code, the d-ascending dfma chain from +0, then dot - 0.5|e|^2),
// four slots per pass.  Selection: every lane keeps the CAP best (key, slot*K + code) of ITS candidates in a sorted register list
// (static, unrolled compare-exchange: no private array, no scratch), and M rounds of a wave arg-min over the list heads give the M
// best of the wave, in order; one wave then merges the waves' lists with the running selection of the slices before in the same
// way, which is how the selection merges across the two slices of K = 512.  The order is total -- a number before a NaN, then the
// key, then the slot, then the code -- so the result does not depend on which lane met which candidate.  The M best of ALL
// pairs, less (0, k*) when it is among them, are the M - 1 best of the others.  Per book a token keeps 8 links (parent slot, code) in LDS; the winner's
// path is read back through them.  The residual update gathers the code rows from global memory (`res - q`, as the search does);
// J' is the rate kernel's energy chain (multiply and add rounded separately: this file is compiled with -ffp-contract=off).
// No atomics; every element of every output is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvq.h"
#include "det_math.hpp"
#include "kernels_small.hpp"

namespace mvq {
void set_last_error(const char* msg);

namespace {

constexpr int BEAM_THR = 256;
constexpr int BEAM_KH = 256;                         // codes resident in LDS at a time (RVQ_KH of the greedy kernel)
constexpr int BEAM_MAX = 8;                          // slots per token
constexpr int BEAM_TOKS_MAX = 8;                     // tokens per block
constexpr int BEAM_COLS = 4;                         // slots scored per pass over the resident codes: 4 chains per LDS read of a code element
constexpr int BEAM_NB_MAX = 32;
constexpr size_t BEAM_LDS_MAX = 160 * 1024;
constexpr int BEAM_NONE = 0x7fffffff;                // id of an empty list entry: behind every candidate

struct BeamArgs {
    const float* z; size_t z_sb, z_sd;
    const float* books;
    int32_t* idx; size_t i_sbook, i_sitem;
    uint8_t* slot;
    float* energy;
    int B, D, T, nb, K, M, toks, ws;                 // ws: the waves that share a token's codes, 4 (few tokens) or 1
};

// the order of the selection: a number before a NaN, the smaller key, then the smaller id = slot*K + code
__device__ __forceinline__ bool beam_before(float ak, int ai, float bk, int bi)
{
    const bool an = ak != ak, bn = bk != bk;
    if (an != bn) return bn;
    if (!an && ak != bk) return ak < bk;
    return ai < bi;
}

template <int CAP>
struct BeamList {
    float k[CAP]; int i[CAP];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int u = 0; u < CAP; ++u) { k[u] = __builtin_nanf(""); i[u] = BEAM_NONE; }
    }
    __device__ __forceinline__ void insert(float ck, int ci)
    {
        if (!beam_before(ck, ci, k[CAP - 1], i[CAP - 1])) return;
#pragma unroll
        for (int u = 0; u < CAP; ++u) {
            const bool b = beam_before(ck, ci, k[u], i[u]);
            const float tk = b ? k[u] : ck; const int ti = b ? i[u] : ci;
            k[u] = b ? ck : k[u]; i[u] = b ? ci : i[u];
            ck = tk; ci = ti;
        }
    }
    __device__ __forceinline__ void pop()
    {
#pragma unroll
        for (int u = 0; u + 1 < CAP; ++u) { k[u] = k[u + 1]; i[u] = i[u + 1]; }
        k[CAP - 1] = __builtin_nanf(""); i[CAP - 1] = BEAM_NONE;
    }
};

__device__ __forceinline__ void beam_amax_combine(float& s, int& i, float os, int oi)
{
    if (os > s || (os == s && oi < i)) { s = os; i = oi; }
}

// the staging order of rvq_ema_forward_kernel (kernels_vq.hip: rvq_stage_map)
__device__ __forceinline__ void beam_stage_map(int i, int dv, bool patch, int& k, int& m)
{
    if (patch) {
        const int p = i >> 5, w = i & 31, nb8 = dv >> 3;
        const int kq = p / nb8, cb = p - kq * nb8;
        k = kq * 4 + (w >> 3);
        m = cb * 8 + (w & 7);
    } else {
        k = i / dv;
        m = i - k * dv;
    }
}

// LDS: Et[D][KH+1] | hn[KH] | R[2][toks][8][D+4] | J[toks][8] | best_s[toks] | best_i[toks] | sel_k[toks][8] | sel_i[toks][8] |
//      wbest_s[toks][4] | wbest_i[toks][4] | wsel_k[toks][4][8] | wsel_i[toks][4][8] | link[toks][nb][8]
template <int CAP>
__global__ __launch_bounds__(BEAM_THR) void rvq_beam_kernel(const BeamArgs a)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float beam_sm[];
    const int D = a.D, K = a.K, M = a.M, nb = a.nb, toks = a.toks, ws = a.ws;
    const int KHP = BEAM_KH + 1, DP = D + 4;
    float* const Et = beam_sm;
    float* const hn = Et + (((size_t)D * KHP + 3) & ~(size_t)3);
    float* const R = hn + BEAM_KH;                                         // 16-byte aligned: rows are read 4 floats at a time
    float* const J = R + (size_t)2 * toks * BEAM_MAX * DP;
    float* const best_s = J + toks * BEAM_MAX;
    int* const best_i = reinterpret_cast<int*>(best_s + toks);
    float* const sel_k = reinterpret_cast<float*>(best_i + toks);
    int* const sel_i = reinterpret_cast<int*>(sel_k + toks * BEAM_MAX);
    float* const wbest_s = reinterpret_cast<float*>(sel_i + toks * BEAM_MAX);       // per wave: its arg-max and its selection
    int* const wbest_i = reinterpret_cast<int*>(wbest_s + toks * 4);
    float* const wsel_k = reinterpret_cast<float*>(wbest_i + toks * 4);
    int* const wsel_i = reinterpret_cast<int*>(wsel_k + toks * 4 * BEAM_MAX);
    uint32_t* const link = reinterpret_cast<uint32_t*>(wsel_i + toks * 4 * BEAM_MAX);     // (code << 3) | parent slot

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long N = (long long)a.B * a.T;
    const long long n0 = (long long)blockIdx.x * toks;
    const int live = (int)(N - n0 < toks ? N - n0 : toks);                 // tokens of this block (>= 1)
    const size_t rbuf = (size_t)toks * BEAM_MAX * DP;

    // slot 0 of every token: r = z(b, :, t)
    for (int e = tid; e < live * D; e += BEAM_THR) {
        const int tok = e % live, d = e / live;
        const long long n = n0 + tok;
        const int b = (int)(n / a.T), t = (int)(n - (long long)b * a.T);
        R[((size_t)tok * BEAM_MAX) * DP + d] = a.z[(size_t)b * a.z_sb + (size_t)d * a.z_sd + (size_t)t];
    }
    __syncthreads();
    if (tid < live) {
        const float* r = R + ((size_t)tid * BEAM_MAX) * DP;
        float E = 0.0f;
        for (int d = 0; d < D; ++d) E = E + r[d] * r[d];
        J[tid * BEAM_MAX] = E;
    }

    int L = 1, cur = 0;
    for (int bk = 0; bk < nb; ++bk) {
        const float* emb = a.books + (size_t)bk * K * D;
        const long long lk = (long long)L * K;
        const int Ln = lk < M ? (int)lk : M;                               // slots after this book
        const float* Rc = R + (size_t)cur * rbuf;
        float* Rn = R + (size_t)(cur ^ 1) * rbuf;
        for (int k0 = 0; k0 < K; k0 += BEAM_KH) {
            const int kh = K - k0 < BEAM_KH ? K - k0 : BEAM_KH;
            __syncthreads();
            {   // stage the transposed slice: global row-major (coalesced) -> Et[d][k] (odd pitch: conflict-free)
                const int dv = D >> 2;
                const int nvec = kh * dv;
                const bool patch = (dv & 7) == 0 && (kh & 3) == 0;
                const float* src = emb + (size_t)k0 * D;
                for (int base = 0; base < nvec; base += BEAM_THR * 8) {
                    v4 r[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = base + u * BEAM_THR + tid;
                        int k, m;
                        beam_stage_map(i < nvec ? i : nvec - 1, dv, patch, k, m);
                        r[u] = *reinterpret_cast<const v4*>(src + 4 * ((size_t)k * dv + m));
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = base + u * BEAM_THR + tid;
                        if (i < nvec) {
                            int k, m;
                            beam_stage_map(i, dv, patch, k, m);
                            const int d4 = m * 4;
                            Et[(d4 + 0) * KHP + k] = r[u].x; Et[(d4 + 1) * KHP + k] = r[u].y;
                            Et[(d4 + 2) * KHP + k] = r[u].z; Et[(d4 + 3) * KHP + k] = r[u].w;
                        }
                    }
                }
            }
            __syncthreads();
            for (int k = tid; k < kh; k += BEAM_THR) {
                float s = 0.0f;
                for (int d = 0; d < D; ++d) { const float e = Et[d * KHP + k]; s = dfma(e, e, s); }
                hn[k] = 0.5f * s;
            }
            __syncthreads();
            // ws waves share a token and split the resident codes between them (lane = code): all its slots, four per pass
            for (int t0 = 0; t0 < live; t0 += 4 / ws) {
                const int tok = t0 + wave / ws, wsub = wave % ws;
                if (tok >= live) continue;                                // wave-uniform
                BeamList<CAP> lst;
                lst.clear();
                float bs = -__builtin_inff(); int bi = BEAM_NONE;
                const float* Rt = Rc + ((size_t)tok * BEAM_MAX) * DP;
                for (int kk = wsub * 64 + lane; kk < kh; kk += 64 * ws) {
                    const float h = hn[kk];
                    const int code = k0 + kk;
                    for (int j0 = 0; j0 < L; j0 += BEAM_COLS) {           // a pass past L - 1 repeats the last slot and drops the result
                        const float* rp[BEAM_COLS]; float Jc[BEAM_COLS];
#pragma unroll
                        for (int c = 0; c < BEAM_COLS; ++c) {
                            const int j = j0 + c < L ? j0 + c : L - 1;
                            rp[c] = Rt + (size_t)j * DP;
                            Jc[c] = J[tok * BEAM_MAX + j];
                        }
                        float dot[BEAM_COLS];
#pragma unroll
                        for (int c = 0; c < BEAM_COLS; ++c) dot[c] = 0.0f;
#pragma unroll 2
                        for (int d = 0; d < D; d += 4) {                  // D % 4 == 0; operands first, then the chains
                            float e[4]; v4 r[BEAM_COLS];
#pragma unroll
                            for (int u = 0; u < 4; ++u) e[u] = Et[(d + u) * KHP + kk];
#pragma unroll
                            for (int c = 0; c < BEAM_COLS; ++c) r[c] = *reinterpret_cast<const v4*>(rp[c] + d);     // one address per wave: a broadcast
#pragma unroll
                            for (int c = 0; c < BEAM_COLS; ++c) {
                                dot[c] = dfma(r[c].x, e[0], dot[c]); dot[c] = dfma(r[c].y, e[1], dot[c]);
                                dot[c] = dfma(r[c].z, e[2], dot[c]); dot[c] = dfma(r[c].w, e[3], dot[c]);
                            }
                        }
#pragma unroll
                        for (int c = 0; c < BEAM_COLS; ++c) {
                            const float sc = dot[c] - h;
                            if (c == 0 && j0 == 0 && sc > bs) { bs = sc; bi = code; }       // the greedy lineage: strict '>' in ascending code order
                            if (M > 1 && j0 + c < L) lst.insert(Jc[c] - 2.0f * sc, (j0 + c) * K + code);
                        }
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {                 // lowest index on ties, as the greedy kernel's reduction
                    const float os = __shfl_xor(bs, off);
                    const int oi = __shfl_xor(bi, off);
                    beam_amax_combine(bs, bi, os, oi);
                }
                if (lane == 0) { wbest_s[tok * 4 + wsub] = bs; wbest_i[tok * 4 + wsub] = bi; }
                // the M best of the wave, in order: M rounds of an arg-min over the list heads
                for (int r = 0; r < M; ++r) {
                    float wk = lst.k[0]; int wi = lst.i[0];
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const float ok = __shfl_xor(wk, off);
                        const int oi = __shfl_xor(wi, off);
                        if (beam_before(ok, oi, wk, wi)) { wk = ok; wi = oi; }
                    }
                    if (wi != BEAM_NONE && lst.i[0] == wi) lst.pop();          // ids are unique: one lane gives its head up
                    if (lane == 0) { wsel_k[(tok * 4 + wsub) * BEAM_MAX + r] = wk; wsel_i[(tok * 4 + wsub) * BEAM_MAX + r] = wi; }
                }
            }
            __syncthreads();
            // per token one wave merges the ws waves' selections and the running one of the slices before (ids stay unique)
            for (int tok = wave; tok < live; tok += BEAM_THR / 64) {
                BeamList<CAP> lst;
                lst.clear();
                if (lane < 8 * ws) {
                    if ((lane & 7) < M) lst.insert(wsel_k[tok * 4 * BEAM_MAX + lane], wsel_i[tok * 4 * BEAM_MAX + lane]);
                } else if (k0 > 0 && lane >= 32 && lane - 32 < M)      // lanes 32 .. 32 + M - 1: the running selection
                    lst.insert(sel_k[tok * BEAM_MAX + lane - 32], sel_i[tok * BEAM_MAX + lane - 32]);
                for (int r = 0; r < M; ++r) {
                    float wk = lst.k[0]; int wi = lst.i[0];
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const float ok = __shfl_xor(wk, off);
                        const int oi = __shfl_xor(wi, off);
                        if (beam_before(ok, oi, wk, wi)) { wk = ok; wi = oi; }
                    }
                    if (wi != BEAM_NONE && lst.i[0] == wi) lst.pop();
                    if (lane == 0) { sel_k[tok * BEAM_MAX + r] = wk; sel_i[tok * BEAM_MAX + r] = wi; }
                }
                if (lane == 0) {
                    float cs = k0 == 0 ? -__builtin_inff() : best_s[tok]; int ci = k0 == 0 ? BEAM_NONE : best_i[tok];
                    for (int w = 0; w < ws; ++w) beam_amax_combine(cs, ci, wbest_s[tok * 4 + w], wbest_i[tok * 4 + w]);
                    best_s[tok] = cs; best_i[tok] = ci;
                }
            }
        }
        __syncthreads();
        // the new slots: 0 = the greedy lineage, then the selection in order without (0, k*)
        if (tid < live) {
            int ks = best_i[tid];
            if (ks < 0 || ks >= K) ks = 0;                                   // all-NaN scores: defined, in range
            uint32_t* lk8 = link + ((size_t)tid * nb + bk) * BEAM_MAX;
            lk8[0] = (uint32_t)ks << 3;
            int s = 1;
            for (int r = 0; r < M && s < Ln; ++r) {
                const int id = sel_i[tid * BEAM_MAX + r];
                if (id < 0 || (long long)id >= (long long)L * K || id == ks) continue;      // empty entries; id of (0, k*) is 0*K + k*
                const int j = id / K, k = id - j * K;
                lk8[s++] = ((uint32_t)k << 3) | (uint32_t)j;
            }
            for (; s < BEAM_MAX; ++s) lk8[s] = lk8[0];                       // never read: s >= Ln
        }
        __syncthreads();
        // r' = r_parent - e_m[k] (the search's res - q; the code rows come from global memory, d across the lanes)
        for (int e = tid; e < live * Ln * D; e += BEAM_THR) {
            const int d = e % D, ts = e / D;
            const int tok = ts / Ln, s = ts - tok * Ln;
            const uint32_t lk1 = link[((size_t)tok * nb + bk) * BEAM_MAX + s];
            const int j = (int)(lk1 & 7u), k = (int)(lk1 >> 3);
            Rn[((size_t)tok * BEAM_MAX + s) * DP + d] = Rc[((size_t)tok * BEAM_MAX + j) * DP + d] - emb[(size_t)k * D + d];
        }
        __syncthreads();
        if (tid < live * Ln) {
            const int tok = tid / Ln, s = tid - tok * Ln;
            const float* r = Rn + ((size_t)tok * BEAM_MAX + s) * DP;
            float E = 0.0f;
            for (int d = 0; d < D; ++d) E = E + r[d] * r[d];
            J[tok * BEAM_MAX + s] = E;
        }
        L = Ln;
        cur ^= 1;
    }
    __syncthreads();
    // the winner: the smallest J by strict '<' in ascending slot order (ties and NaN stay with slot 0), its path back through the links
    if (tid < live) {
        int w = 0; float Jw = J[tid * BEAM_MAX];
        for (int s = 1; s < L; ++s) { const float v = J[tid * BEAM_MAX + s]; if (v < Jw) { Jw = v; w = s; } }
        const long long n = n0 + tid;
        const int b = (int)(n / a.T), t = (int)(n - (long long)b * a.T);
        if (a.slot) a.slot[n] = (uint8_t)w;
        if (a.energy) a.energy[n] = Jw;
        int s = w;
        for (int bk = nb - 1; bk >= 0; --bk) {
            const uint32_t lk1 = link[((size_t)tid * nb + bk) * BEAM_MAX + s];
            a.idx[(size_t)bk * a.i_sbook + (size_t)b * a.i_sitem + (size_t)t] = (int32_t)(lk1 >> 3);
            s = (int)(lk1 & 7u);
        }
    }
}

size_t beam_lds_bytes(int D, int nb, int toks)
{
    const size_t et = ((size_t)D * (BEAM_KH + 1) + 3) & ~(size_t)3;
    const size_t per_tok = (size_t)2 * BEAM_MAX * (D + 4) + BEAM_MAX + 2 + 2 * BEAM_MAX + 8 + 8 * BEAM_MAX + (size_t)(nb > 0 ? nb : 1) * BEAM_MAX;
    return (et + BEAM_KH + per_tok * toks) * sizeof(float);
}

}  // namespace

// The argument rules of the beam search, shared by mvq_rvq_beam_f32 and mvq_ar_latents_staged_rate_beam_f32.  Nothing is launched.
int rvq_beam_check(int dim, int nb_use, int k, int beam, const char* who)
{
    static thread_local char msg[200];
    auto fail = [&](const char* why) {
        snprintf(msg, sizeof(msg), "%s: %s (D=%d nb=%d K=%d beam=%d)", who, why, dim, nb_use, k, beam);
        set_last_error(msg);
        return MVQ_EINVAL;
    };
    if (beam < 1 || beam > BEAM_MAX) return fail("beam outside 1..8");
    if (dim <= 0 || dim % 4 != 0 || dim > 128) return fail("D % 4 == 0 and D <= 128");
    if (k <= 0 || k > (1 << 24)) return fail("K outside 1..2^24");
    if (nb_use < 0 || nb_use > BEAM_NB_MAX) return fail("nb_use outside 0..32");
    return MVQ_OK;
}

hipError_t launch_rvq_beam(const float* z, size_t z_sb, size_t z_sd, const float* books, int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                           uint8_t* slot, float* energy, int B, int D, int T, int nb, int K, int beam, hipStream_t s)
{
    if (B <= 0 || T <= 0) return hipSuccess;
    const long long N = (long long)B * T;
    int toks = 1;                                                                      // every CU a block before a block gets more tokens
    while (toks < BEAM_TOKS_MAX && N / (2 * toks) >= 256) toks <<= 1;
    while (toks > 1 && beam_lds_bytes(D, nb, toks) > BEAM_LDS_MAX) toks >>= 1;         // D = 128: 2 tokens beside the 129 KiB image
    const size_t lds = beam_lds_bytes(D, nb, toks);
    if (lds > BEAM_LDS_MAX) return hipErrorInvalidValue;
    const long long blocks = (N + toks - 1) / toks;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    BeamArgs a{z, z_sb, z_sd, books, idx, idx_sbook, idx_sitem, slot, energy, B, D, T, nb, K, beam, toks, N / 2 >= 256 ? 1 : 4};
    auto kern = beam <= 2 ? rvq_beam_kernel<2> : beam <= 4 ? rvq_beam_kernel<4> : rvq_beam_kernel<8>;
    static BigLdsOptIn opt[3];                                           // per kernel and device: more than 64 KiB of dynamic LDS
    if (hipError_t e = opt[beam <= 2 ? 0 : beam <= 4 ? 1 : 2].ensure(reinterpret_cast<const void*>(kern)); e != hipSuccess) return e;
    const int pi = prof_enabled() ? prof_begin("rvq_beam_kernel", 2.0 * (double)N * D * K * nb * beam, s) : -1;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(BEAM_THR), lds, s, a);
    prof_end(pi, s);
    return hipGetLastError();
}

}  // namespace mvq

extern "C" int mvq_rvq_beam_f32(const float* z, size_t z_sb, size_t z_sd, const float* books, int32_t* idx, size_t idx_sbook,
                                size_t idx_sitem, uint8_t* slot, float* energy, int batch, int dim, int t, int nb_use, int k, int beam,
                                void* stream)
{
    using namespace mvq;
    auto fail = [](int code, const char* msg) { set_last_error(msg); return code; };
    if (batch < 0 || t < 0) return fail(MVQ_EINVAL, "rvq_beam: bad shape (negative batch or t)");
    if (const int rc = rvq_beam_check(dim, nb_use, k, beam, "rvq_beam"); rc != MVQ_OK) return rc;
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!z || (nb_use > 0 && (!idx || !books))) return fail(MVQ_EINVAL, "rvq_beam: null tensor");
    if (reinterpret_cast<uintptr_t>(books) & 15) return fail(MVQ_EINVAL, "rvq_beam: books must be 16-byte aligned");
    if (z_sb == 0 && z_sd == 0) { z_sb = (size_t)dim * t; z_sd = (size_t)t; }
    if (idx_sbook == 0 && idx_sitem == 0) { idx_sbook = (size_t)batch * t; idx_sitem = (size_t)t; }
    const hipError_t e = launch_rvq_beam(z, z_sb, z_sd, books, idx, idx_sbook, idx_sitem, slot, energy, batch, dim, t, nb_use, k, beam,
                                         reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "rvq_beam: %s", hipGetErrorString(e));
        return fail(MVQ_EHIP, msg);
    }
    return MVQ_OK;
}
