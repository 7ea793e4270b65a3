// rate.hip -- closed-loop sender rate control (include/mvq.h: mvq_rvq_rate_f32): after the codebook search of a chunk, decide ON THE
// DEVICE how many books each packet carries and form the sum of code vectors the RECEIVER will form from exactly those books, in the
// receiver's arithmetic (rvq_dequant_layers_kernel, packets.hip), so that the sender's AR history equals the receiver's bit for bit.
//
// Per token of a group (one AR chunk: at most 16 tokens of one item), r_0 = z and r_{k+1} = r_k - e_k[idx_k] (the search's own
// `res = res - q`), E_m = (...((+0 + r_m[0]*r_m[0]) + r_m[1]*r_m[1]) + ...), d ascending, the multiply and the add rounded
// separately (this file is compiled with -ffp-contract=off; no fma here: numpy float32 restates it exactly).
//
// One block per (item, group), three phases:
//   1. residuals: thread (token, 4-dim piece) walks the books once, 16-byte loads of the code rows, and leaves r_0 .. r_nb in LDS
//      (tokens in passes of as many as fit 64 KiB); then thread (token, m) runs the energy chain of r_m over d -- the nb+1 chains of
//      a token are independent threads;
//   2. the decision, by the first wave: the max over a packet of the per-token need (constant quality), or the greedy loop that
//      gives the next book to the packet that gains most (constant rate), lane p = packet p, the scan over candidates in ascending
//      packet order exactly as the rule states it (a later candidate displaces only on a strictly greater gain);
//   3. thread (token, 4-dim piece) forms ((+0 + e_0[idx_0]) + e_1[idx_1]) + ... over the packet's count.
// No atomics; every element of every output is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvq.h"
#include "kernels_small.hpp"
#include "rate_decide.hpp"

namespace mvq {
void set_last_error(const char* msg);

namespace {

constexpr int RATE_THR = 256;
constexpr size_t RATE_LDS_BUDGET = 64 * 1024;

struct RateArgs {
    const float* z; size_t z_sb, z_sd;
    const int32_t* idx; size_t i_sbook, i_sitem;
    const float* books;
    float* q; size_t q_sb, q_sd;
    uint8_t* nb_valid; size_t v_sb;
    uint8_t* nb_sent; size_t s_sb;
    float* energy;
    int B, D, T, nb, K, ptok, gtok, min_books, mode, budget, tg;
    float tol2;
};

__device__ __forceinline__ int clamp_idx(int v, int K) { return v < 0 ? 0 : (v >= K ? K - 1 : v); }

__global__ __launch_bounds__(RATE_THR) void rvq_rate_kernel(const RateArgs a)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float rate_sm[];
    const int D = a.D, nb = a.nb, K = a.K, DV = D >> 2, PITCH = D + 4;
    float* const R = rate_sm;                                              // [tg][nb + 1][PITCH]
    float* const Es = R + (size_t)a.tg * (nb + 1) * PITCH;                 // [nb + 1][16]
    int* const ids = reinterpret_cast<int*>(Es + (nb + 1) * RATE_GROUP_MAX);   // [nb][16], clamped
    int* const cnt = ids + nb * RATE_GROUP_MAX;                            // [16] books of each packet of the group
    const int tid = threadIdx.x;
    const int groups = (a.T + a.gtok - 1) / a.gtok;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
    const int t0 = g * a.gtok;
    const int ntok = min(a.gtok, a.T - t0);
    const int npk = (ntok + a.ptok - 1) / a.ptok;
    const int pc = a.gtok / a.ptok;                                        // packets of a full group
    const size_t N = (size_t)a.B * a.T;

    for (int e = tid; e < nb * ntok; e += RATE_THR) {
        const int bk = e / ntok, i = e - bk * ntok;
        ids[bk * RATE_GROUP_MAX + i] = clamp_idx(a.idx[(size_t)bk * a.i_sbook + (size_t)b * a.i_sitem + (size_t)(t0 + i)], K);
    }
    __syncthreads();

    // ---- phase 1: residuals of a pass of tokens into LDS, then their energy chains
    for (int p0 = 0; p0 < ntok; p0 += a.tg) {
        const int pn = min(a.tg, ntok - p0);
        for (int e = tid; e < pn * DV; e += RATE_THR) {
            const int j = e / pn, il = e - j * pn, i = p0 + il;            // tokens fastest across the lanes: coalesced reads of z
            const float* zp = a.z + (size_t)b * a.z_sb + (size_t)(4 * j) * a.z_sd + (size_t)(t0 + i);
            v4 r = {zp[0], zp[a.z_sd], zp[2 * a.z_sd], zp[3 * a.z_sd]};
            float* row = R + (size_t)il * (nb + 1) * PITCH + 4 * j;
            *reinterpret_cast<v4*>(row) = r;
#pragma unroll 4
            for (int bk = 0; bk < nb; ++bk) {
                const int id = ids[bk * RATE_GROUP_MAX + i];
                const v4 c = *reinterpret_cast<const v4*>(a.books + ((size_t)bk * K + id) * D + 4 * j);
                r = r - c;
                *reinterpret_cast<v4*>(row + (size_t)(bk + 1) * PITCH) = r;
            }
        }
        __syncthreads();
        for (int e = tid; e < pn * (nb + 1); e += RATE_THR) {
            const int il = e / (nb + 1), m = e - il * (nb + 1), i = p0 + il;   // row e of R: a lane stride of PITCH floats
            const float* row = R + (size_t)e * PITCH;
            float E = 0.0f;
            for (int j = 0; j < DV; ++j) {
                const v4 r = *reinterpret_cast<const v4*>(row + 4 * j);
                E = E + r.x * r.x; E = E + r.y * r.y; E = E + r.z * r.z; E = E + r.w * r.w;
            }
            Es[m * RATE_GROUP_MAX + i] = E;
            if (a.energy) a.energy[(size_t)m * N + (size_t)b * a.T + (size_t)(t0 + i)] = E;
        }
        __syncthreads();
    }

    // ---- phase 2: the decision (first wave; lane p = packet p of the group; the rule itself: rate_decide.hpp)
    if (tid < 64) {
        const int lane = tid;
        const int m = rate_decide(Es, lane, nb, ntok, npk, pc, a.ptok, a.min_books, a.mode, a.tol2, a.budget);
        if (lane < npk) {
            cnt[lane] = m;
            a.nb_sent[(size_t)b * a.s_sb + (size_t)(g * pc + lane)] = (uint8_t)m;
        }
    }
    __syncthreads();

    // ---- phase 3: the receiver's sum over each token's count
    if (tid < ntok) a.nb_valid[(size_t)b * a.v_sb + (size_t)(t0 + tid)] = (uint8_t)cnt[tid / a.ptok];
    for (int e = tid; e < ntok * DV; e += RATE_THR) {
        const int j = e / ntok, i = e - j * ntok;
        const int c = cnt[i / a.ptok];
        v4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int bk = 0; bk < c; ++bk) {
            const int id = ids[bk * RATE_GROUP_MAX + i];
            const v4 ev = *reinterpret_cast<const v4*>(a.books + ((size_t)bk * K + id) * D + 4 * j);
            acc = acc + ev;
        }
        float* o = a.q + (size_t)b * a.q_sb + (size_t)(4 * j) * a.q_sd + (size_t)(t0 + i);
        o[0] = acc.x;
        o[a.q_sd] = acc.y;
        o[2 * a.q_sd] = acc.z;
        o[3 * a.q_sd] = acc.w;
    }
}

}  // namespace

// The argument rules of the rate decision, shared by mvq_rvq_rate_f32 and mvq_ar_latents_staged_rate_f32; MVQ_OK or the code, the
// text through set_last_error.  Nothing is launched.
int rvq_rate_check(int dim, int nb_use, int k, int packet_tok, int group_tok, int min_books, int mode, float tol2, int budget, const char* who)
{
    static thread_local char msg[256];
    auto fail = [&](int code, const char* why) {
        snprintf(msg, sizeof(msg), "%s: %s (D=%d nb=%d K=%d packet_tok=%d group_tok=%d min_books=%d mode=%d tol2=%g budget=%d)", who, why, dim,
                 nb_use, k, packet_tok, group_tok, min_books, mode, (double)tol2, budget);
        set_last_error(msg);
        return code;
    };
    if (dim <= 0 || nb_use < 0 || k <= 0 || packet_tok < 1 || group_tok < 1) return fail(MVQ_EINVAL, "bad shape");
    if (dim % 4 != 0 || dim > 128) return fail(MVQ_EUNSUPPORTED, "D % 4 == 0 and D <= 128");
    if (nb_use > RATE_NB_MAX) return fail(MVQ_EUNSUPPORTED, "nb_use <= 32");
    if (group_tok > RATE_GROUP_MAX) return fail(MVQ_EUNSUPPORTED, "group_tok <= 16");
    if (group_tok % packet_tok != 0) return fail(MVQ_EINVAL, "packet_tok must divide group_tok");
    if (mode != MVQ_RATE_FULL && mode != MVQ_RATE_TOL2 && mode != MVQ_RATE_BUDGET) return fail(MVQ_EINVAL, "unknown mode");
    if (nb_use > 0 && (min_books < 1 || min_books > nb_use)) return fail(MVQ_EINVAL, "1 <= min_books <= nb_use");
    if (mode == MVQ_RATE_TOL2 && !(tol2 > 0.0f && tol2 <= 3.4028234e38f)) return fail(MVQ_EINVAL, "tol2 must be a finite positive fp32");
    if (mode == MVQ_RATE_BUDGET && nb_use > 0) {
        const int pc = group_tok / packet_tok;
        if (budget < pc * min_books || budget > pc * nb_use) return fail(MVQ_EINVAL, "P_c*min_books <= budget <= P_c*nb_use");
    }
    return MVQ_OK;
}

hipError_t launch_rvq_rate(const float* z, size_t z_sb, size_t z_sd, const int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                           const float* books, float* q_out, size_t out_sb, size_t out_sd, uint8_t* nb_valid, size_t nbv_sb,
                           uint8_t* nb_sent, size_t nbs_sb, float* energy, int B, int D, int T, int nb, int K, int ptok, int gtok,
                           int min_books, int mode, float tol2, int budget, hipStream_t s)
{
    if (B <= 0 || T <= 0) return hipSuccess;
    RateArgs a{z, z_sb, z_sd, idx, idx_sbook, idx_sitem, books, q_out, out_sb, out_sd, nb_valid, nbv_sb, nb_sent, nbs_sb, energy,
               B, D, T, nb, K, ptok, gtok, min_books, mode, budget, 0, tol2};
    const size_t fixed = ((size_t)(nb + 1) * RATE_GROUP_MAX + (size_t)nb * RATE_GROUP_MAX + RATE_GROUP_MAX) * sizeof(float);
    const size_t per_tok = (size_t)(nb + 1) * (D + 4) * sizeof(float);
    size_t tg = (RATE_LDS_BUDGET - fixed) / per_tok;                       // 16 at 8 books x D = 96, 4 at 32 x 96, 3 at the largest shape covered (32 x 128)
    if (tg > (size_t)gtok) tg = (size_t)gtok;
    if (tg < 1) return hipErrorInvalidValue;
    a.tg = (int)tg;
    const size_t lds = tg * per_tok + fixed;
    const int groups = (T + gtok - 1) / gtok;
    const long long blocks = (long long)B * groups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const int pi = prof_enabled() ? prof_begin("rvq_rate_kernel", (double)B * T * D * (3.0 * nb + 2.0 * (nb + 1)), s) : -1;
    hipLaunchKernelGGL(rvq_rate_kernel, dim3((unsigned)blocks), dim3(RATE_THR), lds, s, a);
    prof_end(pi, s);
    return hipGetLastError();
}

}  // namespace mvq

extern "C" int mvq_rvq_rate_f32(const float* z, size_t z_sb, size_t z_sd, const int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                                const float* books, float* q_out, size_t out_sb, size_t out_sd, uint8_t* nb_valid, size_t nbv_sb,
                                uint8_t* nb_sent, size_t nbs_sb, float* energy, int batch, int dim, int t, int nb_use, int k,
                                int packet_tok, int group_tok, int min_books, int mode, float tol2, int budget, void* stream)
{
    using namespace mvq;
    auto fail = [](int code, const char* msg) { set_last_error(msg); return code; };
    if (batch < 0 || t < 0) return fail(MVQ_EINVAL, "rvq_rate: bad shape (negative batch or t)");
    if (const int rc = rvq_rate_check(dim, nb_use, k, packet_tok, group_tok, min_books, mode, tol2, budget); rc != MVQ_OK) return rc;
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!z || !q_out || !nb_valid || !nb_sent || (nb_use > 0 && (!idx || !books))) return fail(MVQ_EINVAL, "rvq_rate: null tensor");
    if (reinterpret_cast<uintptr_t>(books) & 15) return fail(MVQ_EINVAL, "rvq_rate: books must be 16-byte aligned");
    if (z_sb == 0 && z_sd == 0) { z_sb = (size_t)dim * t; z_sd = (size_t)t; }
    if (out_sb == 0 && out_sd == 0) { out_sb = (size_t)dim * t; out_sd = (size_t)t; }
    if (idx_sbook == 0 && idx_sitem == 0) { idx_sbook = (size_t)batch * t; idx_sitem = (size_t)t; }
    if (nbv_sb == 0) nbv_sb = (size_t)t;
    if (nbs_sb == 0) nbs_sb = (size_t)((t + packet_tok - 1) / packet_tok);
    const hipError_t e = launch_rvq_rate(z, z_sb, z_sd, idx, idx_sbook, idx_sitem, books, q_out, out_sb, out_sd, nb_valid, nbv_sb, nb_sent,
                                         nbs_sb, energy, batch, dim, t, nb_use, k, packet_tok, group_tok, min_books, mode, tol2, budget,
                                         reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "rvq_rate: %s", hipGetErrorString(e));
        return fail(MVQ_EHIP, msg);
    }
    return MVQ_OK;
}
