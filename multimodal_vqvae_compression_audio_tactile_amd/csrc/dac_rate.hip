// dac_rate.hip -- closed-loop AUDIO rate control (include/mvq.h: mvq_dac_rvq_rate_f32): after the DAC residual VQ has produced the
// codes of a run of tokens, decide ON THE DEVICE how many stages each audio packet carries and form, from exactly those stages, the
// latent the RECEIVER will form (mvq_dac_rvq_from_codes_layers_f32's arithmetic), so that both ends feed the predictor the same bits.
//
// out_w is 1 MB at 32 stages x 1024 channels x 8, so the work of a group is spread over the channel axis; three launches:
//   1. dac_rvq_rate_energy_kernel, gridded like dac_rvq_from_codes_kernel (16 tokens x 64 channels per block): lane (token, channel
//      group) runs from_codes's own chain S_{m+1}(c) = S_m(c) + zq_m(c) for its four channels and, before each stage and after the
//      last, squares d_m(c) = z(c) - S_m(c); the block leaves ONE partial energy per (slab, m, token) in the workspace;
//   2. dac_rvq_rate_decide_kernel, one block per (item, 16-token group): E_m = the partials of the C / 64 slabs added in slab
//      order, then, by its first wave, the rule of rate_decide.hpp (the one csrc/rate.hip runs), lane p = packet p;
//   3. dac_rvq_from_codes_kernel<true> (kernels_vq.hip) on the counts: qa_out.
// The order of the energy sum (include/mvq.h states it) is a function of the channel alone: it does not depend on B, T, the grid or
// the position of the group.  The multiply and the adds are separate fp32 operations (-ffp-contract=off; the stage chain itself is
// from_codes's explicit fma).  No atomics; every element of every output is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvq.h"
#include "dac_stage.hpp"
#include "kernels_small.hpp"
#include "rate_decide.hpp"

namespace mvq {
void set_last_error(const char* msg);

namespace {

constexpr int DR_TOK = 16, DR_CH = 64, DR_DC = 8, DR_MAX_NQ = RATE_NB_MAX;
static_assert(DR_TOK == RATE_GROUP_MAX, "a token tile of the energy kernel is a group of the decision");

__device__ __forceinline__ int clamp_code64(int64_t v, int K) { return v < 0 ? 0 : (v >= K ? K - 1 : (int)v); }

// partial[(slab*(nq+1) + m)*N + n] = sum over cg = 0..15 ascending, from +0, of
//   t(cg) = (((+0 + p(c)) + p(c+16)) + p(c+32)) + p(c+48),  c = 64*slab + cg,  p(c) = fl(d_m(c) * d_m(c)).
__global__ __launch_bounds__(256) void dac_rvq_rate_energy_kernel(
    const float* __restrict__ z, const int64_t* __restrict__ codes, size_t codes_sb, const float* __restrict__ cb,
    const float* __restrict__ out_w, const float* __restrict__ out_b, float* __restrict__ partial, int B, int C, int T, int nq, int K)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float p_s[DR_MAX_NQ][DR_TOK][DR_DC];          // 16 KiB: the raw rows of the tile's tokens
    __shared__ float red[DR_MAX_NQ + 1][DR_CH / 4][DR_TOK];                               // 33 KiB: t(cg) of every (m, token)
    const int tid = threadIdx.x;
    const size_t N = (size_t)B * T;
    const size_t n0 = (size_t)blockIdx.x * DR_TOK;
    for (int e = tid; e < nq * DR_TOK * 2; e += 256) {                                     // (stage, token, half row)
        const int h = e & 1, tk = (e >> 1) % DR_TOK, st = e / (2 * DR_TOK);
        const size_t n = n0 + tk;
        v4 r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (n < N) {
            const int b = (int)(n / T), t = (int)(n % T);
            const int id = clamp_code64(codes[(size_t)b * codes_sb + (size_t)st * T + t], K);
            r = *reinterpret_cast<const v4*>(cb + ((size_t)st * K + id) * DR_DC + 4 * h);
        }
        *reinterpret_cast<v4*>(&p_s[st][tk][4 * h]) = r;
    }
    __syncthreads();
    const int tk = tid % DR_TOK, cg = tid / DR_TOK;                                        // 16 channel groups of 4 channels (stride 16)
    const size_t n = n0 + tk;
    const int c0 = blockIdx.y * DR_CH + cg;
    float zc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n < N) {
        const int b = (int)(n / T), t = (int)(n % T);
#pragma unroll
        for (int u = 0; u < 4; ++u) zc[u] = z[((size_t)b * C + c0 + 16 * u) * T + t];
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int m = 0; m <= nq; ++m) {
        float ts = 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float d = zc[u] - acc[u];
            const float p = d * d;
            ts = ts + p;
        }
        red[m][cg][tk] = ts;
        if (m == nq) break;
        const v4 pa = *reinterpret_cast<const v4*>(&p_s[m][tk][0]);
        const v4 pb = *reinterpret_cast<const v4*>(&p_s[m][tk][4]);
        dac_stage_accumulate(acc, pa, pb, out_w, out_b, m, C, c0);                         // dac_rvq_from_codes_kernel's own stage
    }
    __syncthreads();
    for (int e = tid; e < (nq + 1) * DR_TOK; e += 256) {
        const int m = e / DR_TOK, tk2 = e - m * DR_TOK;
        const size_t n2 = n0 + tk2;
        if (n2 >= N) continue;
        float P = 0.0f;
#pragma unroll
        for (int g = 0; g < DR_CH / 4; ++g) P = P + red[m][g][tk2];
        partial[((size_t)blockIdx.y * (nq + 1) + m) * N + n2] = P;
    }
}

struct DecideArgs {
    const float* partial;
    uint8_t* na_valid;
    uint8_t* na_sent;
    float* energy;
    int B, T, nq, slabs, ptok, min_books, mode, budget;
    float tol2;
};

// One block per (item, group of 16 tokens starting at token 0 of the item): all four waves add the slabs (the loads of one sum are
// issued together, the additions stay in slab order), the first wave decides.
constexpr int DR_DECIDE_THR = 256;
__global__ __launch_bounds__(DR_DECIDE_THR) void dac_rvq_rate_decide_kernel(const DecideArgs a)
{
    __shared__ float Es[(DR_MAX_NQ + 1) * RATE_GROUP_MAX];
    __shared__ int cnt[RATE_GROUP_MAX];
    const int tid = threadIdx.x, nq = a.nq;
    const int groups = (a.T + RATE_GROUP_MAX - 1) / RATE_GROUP_MAX;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
    const int t0 = g * RATE_GROUP_MAX;
    const int ntok = min(RATE_GROUP_MAX, a.T - t0);
    const int npk = (ntok + a.ptok - 1) / a.ptok;
    const int pc = RATE_GROUP_MAX / a.ptok;                                                // packets of a full group
    const int P = (a.T + a.ptok - 1) / a.ptok;
    const size_t N = (size_t)a.B * a.T;
    for (int e = tid; e < (nq + 1) * ntok; e += DR_DECIDE_THR) {
        const int m = e / ntok, i = e - m * ntok;
        const size_t n = (size_t)b * a.T + (size_t)(t0 + i);
        float E = 0.0f;
        for (int s0 = 0; s0 < a.slabs; s0 += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = s0 + u < a.slabs ? a.partial[((size_t)(s0 + u) * (nq + 1) + m) * N + n] : 0.0f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (s0 + u < a.slabs) E = E + v[u];
        }
        Es[m * RATE_GROUP_MAX + i] = E;
        if (a.energy) a.energy[(size_t)m * N + n] = E;
    }
    __syncthreads();
    if (tid < 64) {                                                                        // the first wave, whole: lane = tid
        const int lane = tid;
        const int m = rate_decide(Es, lane, nq, ntok, npk, pc, a.ptok, a.min_books, a.mode, a.tol2, a.budget);
        if (lane < npk) {
            cnt[lane] = m;
            a.na_sent[(size_t)b * P + (size_t)(g * pc + lane)] = (uint8_t)m;
        }
    }
    __syncthreads();
    if (tid < ntok) a.na_valid[(size_t)b * a.T + (size_t)(t0 + tid)] = (uint8_t)cnt[tid / a.ptok];
}

}  // namespace

hipError_t launch_dac_rvq_rate(const float* z, const int64_t* codes, size_t codes_sb, const float* cb, const float* out_w,
                               const float* out_b, float* qa_out, uint8_t* na_valid, uint8_t* na_sent, float* energy, float* partial,
                               int B, int C, int T, int nq, int K, int Dc, int ptok, int min_books, int mode, float tol2, int budget,
                               hipStream_t s)
{
    const size_t N = (size_t)B * T;
    if (N == 0) return hipSuccess;
    if (Dc != DR_DC || C % DR_CH || nq <= 0 || nq > DR_MAX_NQ || ptok < 1 || RATE_GROUP_MAX % ptok) return hipErrorInvalidValue;
    const size_t tiles = (N + DR_TOK - 1) / DR_TOK;
    const long long blocks = (long long)B * ((T + RATE_GROUP_MAX - 1) / RATE_GROUP_MAX);
    if (tiles > 0x7fffffffULL || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    int pi = prof_enabled() ? prof_begin("dac_rvq_rate_energy_kernel", (double)N * C * (nq * 18.0 + (nq + 1) * 3.0), s) : -1;
    hipLaunchKernelGGL(dac_rvq_rate_energy_kernel, dim3((unsigned)tiles, (unsigned)(C / DR_CH)), dim3(256), 0, s, z, codes, codes_sb, cb,
                       out_w, out_b, partial, B, C, T, nq, K);
    prof_end(pi, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const DecideArgs a{partial, na_valid, na_sent, energy, B, T, nq, C / DR_CH, ptok, min_books, mode, budget, tol2};
    pi = prof_enabled() ? prof_begin("dac_rvq_rate_decide_kernel", (double)N * (nq + 1) * (C / DR_CH), s) : -1;
    hipLaunchKernelGGL(dac_rvq_rate_decide_kernel, dim3((unsigned)blocks), dim3(DR_DECIDE_THR), 0, s, a);
    prof_end(pi, s);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_dac_rvq_from_codes_layers(codes, codes_sb, cb, out_w, out_b, na_valid, qa_out, nullptr, B, C, T, nq, K, Dc, s);
}

}  // namespace mvq

extern "C" size_t mvq_dac_rvq_rate_workspace_bytes(int batch, int c, int t, int na_use)
{
    if (batch <= 0 || c <= 0 || t <= 0 || na_use < 0 || c % 64) return 0;
    return (size_t)(c / 64) * (size_t)(na_use + 1) * (size_t)batch * (size_t)t * sizeof(float);
}

extern "C" int mvq_dac_rvq_rate_f32(const float* z, const int64_t* codes, size_t codes_sb, const float* codebook, const float* out_w,
                                    const float* out_b, float* qa_out, uint8_t* na_valid, uint8_t* na_sent, float* energy,
                                    float* workspace, size_t workspace_bytes, int batch, int c, int t, int na_use, int k, int dc,
                                    int packet_tok, int min_books, int mode, float tol2, int budget, void* stream)
{
    using namespace mvq;
    static thread_local char msg[256];
    auto fail = [&](int code, const char* why) {
        snprintf(msg, sizeof(msg), "dac_rvq_rate: %s (B=%d C=%d T=%d na_use=%d K=%d Dc=%d packet_tok=%d)", why, batch, c, t, na_use, k, dc,
                 packet_tok);
        set_last_error(msg);
        return code;
    };
    if (batch < 0 || t < 0 || c <= 0 || k <= 0 || na_use < 1) return fail(MVQ_EINVAL, "bad shape");
    if (c % 64 != 0 || dc != 8 || na_use > 32) return fail(MVQ_EUNSUPPORTED, "C % 64 == 0, Dc = 8, na_use <= 32");
    if (const int rc = rvq_rate_check(dc, na_use, k, packet_tok, RATE_GROUP_MAX, min_books, mode, tol2, budget, "dac_rvq_rate"); rc != MVQ_OK) return rc;
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!z || !codes || !codebook || !out_w || !out_b || !qa_out || !na_valid || !na_sent || !workspace)
        return fail(MVQ_EINVAL, "null tensor");
    if ((reinterpret_cast<uintptr_t>(codebook) | reinterpret_cast<uintptr_t>(out_w)) & 15)
        return fail(MVQ_EINVAL, "codebook and out_w must be 16-byte aligned");
    if (codes_sb == 0) codes_sb = (size_t)na_use * t;
    if (codes_sb < (size_t)na_use * t) return fail(MVQ_EINVAL, "codes_sb is smaller than na_use * T");
    if (workspace_bytes < mvq_dac_rvq_rate_workspace_bytes(batch, c, t, na_use)) return fail(MVQ_EINVAL, "workspace too small");
    const hipError_t e = launch_dac_rvq_rate(z, codes, codes_sb, codebook, out_w, out_b, qa_out, na_valid, na_sent, energy, workspace,
                                             batch, c, t, na_use, k, dc, packet_tok, min_books, mode, tol2, budget,
                                             reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        snprintf(msg, sizeof(msg), "dac_rvq_rate: %s", hipGetErrorString(e));
        set_last_error(msg);
        return MVQ_EHIP;
    }
    return MVQ_OK;
}
