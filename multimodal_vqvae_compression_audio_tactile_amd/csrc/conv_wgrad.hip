// conv_wgrad.hip -- parameter gradients of the DAC decoder's layers (fine-tuning T_DEC):
//   mvq_conv1d_wgrad_f32      conv / transposed-conv weight gradient, an implicit GEMM over the TOKEN axis on the fp32 MFMA
//   mvq_snake_bwd_f32         Snake1d backward: gx (the dgrad epilogue's arithmetic, det_dsnake) and d/d alpha
//   mvq_bias_grad_f32         db[c] = sum over items and tokens
//   mvq_weight_norm_bwd_f32   (dW, v, g) -> (dg, dv) of w = g * v / ||v||
// fp32 throughout, no atomics: every sum that is split over blocks goes through a caller-provided workspace and is added in
// ascending split order by a second kernel, so the same inputs give the same bits on every run.
//
// The weight gradient in one form for both conv kinds.  With P the operand that is read unshifted and Q the tapped one,
//     dW[m][n][k] = sum_b sum_t P[b][m][t] * Q[b][n][t*sq + k*dil - pad]          (terms outside a row of Q are 0)
//   Conv1d (stride 1):           P = gy [B,cout,tout], Q = a  [B,cin,tin],   sq = 1       -> dW[co][ci][k]
//   ConvTranspose1d (ks = 2 s):  P = a  [B,cin,tin],   Q = gy [B,cout,tout], sq = s, dil 1 -> dW[ci][co][k]
// which are the torch layouts of weight_v.  GEMM view: M = rows of P, N = rows of Q (x taps), K = tokens.  Both operands are
// token-contiguous in memory, which is the K-contiguous layout v_mfma_f32_32x32x2_f32 takes (lane l: A[l&31][k = l>>5],
// B[k = l>>5][l&31]): a tile of TK tokens of 64 rows of P and the matching window of 64 rows of Q are staged in LDS (Snake
// applied while staging when the forward input was a Snake output), and a tap is an LDS address offset of k*dil.
// A block of 4 waves owns a 64 x 64 tile of (m, n) for TG taps (7 taps of a k7 conv: 7 accumulator tiles per wave) and one
// contiguous range of the (item, token-chunk) list: split-K.  Partials [split][M][N][ks] go to the workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mvq.h"
#include "det_math.hpp"
#include "kernels_small.hpp"

namespace mvq {
void set_last_error(const char* msg);

namespace {
typedef float wg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_BM = 64, WG_BN = 64;          // block tile: 2 x 2 waves of 32 x 32
constexpr int WG_ROWS_TK = 1024;               // token chunk of the reduction form (M <= WG_ROWS_MAX_M)
constexpr int WG_ROWS_MAX_M = 4;
constexpr int WG_TARGET_BLOCKS = 1024;         // split-K until the grid has about this many blocks (a constant: the split, and
                                               // with it the summation order, depends on the shape alone, never on the device)
constexpr int WG_MAX_SPLIT = 4096;

struct WgradArgs {
    const float* p; const float* q;            // P [B][M][Tp], Q [B][N][Tq]
    const float* alpha;                        // Snake in front of the forward layer (nullptr: none), indexed by the rows of `a`
    float* out;                                // [nsplit][M][N][ks]
    int B, M, N, Tp, Tq, ks, sq, dil, pad;
    int snake_on_p;                            // the forward input `a` is P (transposed conv) or Q (conv)
    int TK, tk_shift, PQ, cpb, nsplit, ntg;    // tokens per chunk (power of two), LDS pitch of Q, chunks per item, splits, tap groups
};

// chunk range [c0, c1) of split `s`: the list of (item, token chunk) pairs in (item, chunk) order, cut into nsplit contiguous ranges
__device__ __forceinline__ void wg_range(const WgradArgs& a, int s, long long& c0, long long& c1)
{
    const long long n = (long long)a.B * a.cpb;
    c0 = n * s / a.nsplit;
    c1 = n * (s + 1) / a.nsplit;
}

template <int TG>
__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(const WgradArgs a)
{
    extern __shared__ float wg_lds[];
    const int TK = a.TK, PP = TK + 2, PQ = a.PQ;      // pitches = 2 (mod 4): the 64 lanes of an operand read (32 rows x 2 tokens) hit 64 banks
    float* const Ps = wg_lds;                         // [64][PP]
    float* const Qs = wg_lds + WG_BM * PP;            // [64][PQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * WG_BN, m0 = blockIdx.y * WG_BM;
    const int split = blockIdx.z / a.ntg, kg = blockIdx.z - split * a.ntg;
    const int k0 = kg * TG;
    const int WQ = (TK - 1) * a.sq + (TG - 1) * a.dil + 1;        // window of Q one chunk of this tap group touches (<= PQ)
    const bool active = m0 + wm * 32 < a.M && n0 + wn * 32 < a.N;

    wg_f32x16 acc[TG];
#pragma unroll
    for (int k = 0; k < TG; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[k][i] = 0.0f;

    long long c0, c1;
    wg_range(a, split, c0, c1);
    const float* const pa = Ps + (wm * 32 + (lane & 31)) * PP + (lane >> 5);
    const float* const qb = Qs + (wn * 32 + (lane & 31)) * PQ + (lane >> 5) * a.sq;

    for (long long c = c0; c < c1; ++c) {
        const int b = (int)(c / a.cpb);
        const int t0 = (int)(c - (long long)b * a.cpb) << a.tk_shift;
        const int q0 = t0 * a.sq + k0 * a.dil - a.pad;            // position in Q of column 0 of the staged window
        // ---- stage: one row per wave at a time, lanes along the tokens (coalesced); rows / tokens outside the tensors are zeros
        for (int r = wave; r < WG_BM; r += 4) {
            const int m = m0 + r;
            const bool row_ok = m < a.M;
            const float* const src = a.p + ((size_t)b * a.M + (row_ok ? m : 0)) * a.Tp;
            const bool sn = a.alpha != nullptr && a.snake_on_p;
            const float al = sn && row_ok ? a.alpha[m] : 1.0f;
            const float inv = 1.0f / (al + 1e-9f);
            for (int j = lane; j < TK; j += 64) {
                const int t = t0 + j;
                float v = 0.0f;
                if (row_ok && t < a.Tp) { v = src[t]; if (sn) v = det_snake(v, al, inv); }
                Ps[r * PP + j] = v;
            }
        }
        for (int r = wave; r < WG_BN; r += 4) {
            const int n = n0 + r;
            const bool row_ok = n < a.N;
            const float* const src = a.q + ((size_t)b * a.N + (row_ok ? n : 0)) * a.Tq;
            const bool sn = a.alpha != nullptr && !a.snake_on_p;
            const float al = sn && row_ok ? a.alpha[n] : 1.0f;
            const float inv = 1.0f / (al + 1e-9f);
            for (int j = lane; j < WQ; j += 64) {
                const int pos = q0 + j;
                float v = 0.0f;
                if (row_ok && pos >= 0 && pos < a.Tq) { v = src[pos]; if (sn) v = det_snake(v, al, inv); }
                Qs[r * PQ + j] = v;
            }
        }
        __syncthreads();
        if (active) {
            const int left = a.Tp - t0;                           // >= 1
            const int steps = ((left < TK ? left : TK) + 1) >> 1; // an odd last token pairs with a staged zero (TK is even)
            for (int s = 0; s < steps; ++s) {
                const float av = pa[2 * s];
                const float* const qs = qb + 2 * s * a.sq;
#pragma unroll
                for (int k = 0; k < TG; ++k)
                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, qs[k * a.dil], acc[k], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    if (active) {
        float* const dst = a.out + (size_t)split * a.M * a.N * a.ks;
        const int n = n0 + wn * 32 + (lane & 31);
#pragma unroll
        for (int k = 0; k < TG; ++k)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                if (m < a.M && n < a.N) dst[((size_t)m * a.N + n) * a.ks + k0 + k] = acc[k][i];
            }
    }
}

// Reduction form for a layer with very few rows on one side (the decoder's final conv: cout = 1, dW[1][96][7]): one block per
// (n, k, m, split); 256 threads walk the tokens of the split's chunks with a stride of 256, then a fixed tree adds them.
__global__ __launch_bounds__(256) void conv1d_wgrad_rows_kernel(const WgradArgs a)
{
    __shared__ float red[256];
    const int n = blockIdx.x / a.ks, k = blockIdx.x - n * a.ks, m = blockIdx.y, split = blockIdx.z;
    const int tid = threadIdx.x;
    const float alp = a.alpha && a.snake_on_p ? a.alpha[m] : 1.0f, alq = a.alpha && !a.snake_on_p ? a.alpha[n] : 1.0f;
    const float invp = 1.0f / (alp + 1e-9f), invq = 1.0f / (alq + 1e-9f);
    long long c0, c1;
    wg_range(a, split, c0, c1);
    float acc = 0.0f;
    for (long long c = c0; c < c1; ++c) {
        const int b = (int)(c / a.cpb);
        const int t0 = (int)(c - (long long)b * a.cpb) << a.tk_shift;
        const float* const pr = a.p + ((size_t)b * a.M + m) * a.Tp;
        const float* const qr = a.q + ((size_t)b * a.N + n) * a.Tq;
        for (int j = tid; j < a.TK; j += 256) {
            const int t = t0 + j;
            const int pos = t * a.sq + k * a.dil - a.pad;
            if (t < a.Tp && pos >= 0 && pos < a.Tq) {
                float pv = pr[t], qv = qr[pos];
                if (a.alpha) { if (a.snake_on_p) pv = det_snake(pv, alp, invp); else qv = det_snake(qv, alq, invq); }
                acc = dfma(pv, qv, acc);
            }
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) a.out[(size_t)split * a.M * a.N * a.ks + ((size_t)m * a.N + n) * a.ks + k] = red[0];
}

// out[i] = ((part[0][i] + part[1][i]) + part[2][i]) + ...   (ascending split order)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, size_t count, int nsplit)
{
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        float v = part[i];
        for (int s = 1; s < nsplit; ++s) v += part[(size_t)s * count + i];
        out[i] = v;
    }
}

struct WgradPlan { bool rows; int tg; size_t lds; size_t count; const char* name; };

// Geometry checks and the launch plan, from the shape alone.  Returns nullptr or the refusal text.
const char* wgrad_plan(int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil, int pad, int transposed,
                       WgradArgs& a, WgradPlan& pl)
{
    if (batch < 0 || cin < 1 || cout < 1 || tin < 0 || tout < 0 || ks < 1 || stride < 1 || dil < 1 || pad < 0)
        return "conv1d_wgrad: bad shape";
    if (tin > (1 << 28) || tout > (1 << 28) || ks > 64 || dil > 4096 || pad > (1 << 20)) return "conv1d_wgrad: shape out of range";
    if (!transposed) {
        if (stride != 1) return "conv1d_wgrad: the Conv1d form is stride 1";
        const long long want = (long long)tin + 2LL * pad - (long long)dil * (ks - 1);
        if (want != tout || tout < 0) return "conv1d_wgrad: tout does not match tin, ks, dil, pad";
        a.M = cout; a.N = cin; a.Tp = tout; a.Tq = tin; a.sq = 1; a.dil = dil; a.snake_on_p = 0;
    } else {
        if (ks != 2 * stride) return "conv1d_wgrad: the ConvTranspose1d form covers ks == 2*stride";
        if (dil != 1) return "conv1d_wgrad: the ConvTranspose1d form has no dilation";
        const long long base = tin > 0 ? (long long)(tin - 1) * stride - 2LL * pad + ks : 0;
        if (tin > 0 && (tout < base || tout >= base + stride || base < 0)) return "conv1d_wgrad: tout does not match tin, stride, pad (output_padding < stride)";
        if (tin == 0 && tout != 0) return "conv1d_wgrad: tout does not match tin";
        a.M = cin; a.N = cout; a.Tp = tin; a.Tq = tout; a.sq = stride; a.dil = 1; a.snake_on_p = 1;
    }
    a.B = batch; a.ks = ks; a.pad = pad;
    pl.count = (size_t)a.M * a.N * ks;
    pl.rows = a.M <= WG_ROWS_MAX_M;
    long long tiles;
    if (pl.rows) {
        a.TK = WG_ROWS_TK; a.ntg = 1; a.PQ = 0; pl.tg = 0; pl.lds = 0; pl.name = "conv1d_wgrad_rows_kernel";
        tiles = (long long)a.N * ks * a.M;
        if ((long long)a.N * ks > 0x7fffffffLL) return "conv1d_wgrad: shape out of range";
    } else {
        // taps held in registers per block: every tap of a 1-, 3-, 7-tap conv; 4-, 5- or 8-tap groups of a transposed conv's 2*stride
        static const int groups[] = {8, 7, 5, 4, 3, 2, 1};
        int tg = 1;
        for (int g : groups) if (ks % g == 0) { tg = g; break; }
        if (ks / tg > 16) return "conv1d_wgrad: kernel size outside the path";
        // token chunk: the staged window of Q, (TK-1)*sq + (tg-1)*dil + 1 columns, stays near 128 columns
        a.TK = a.sq == 1 ? 64 : a.sq == 2 ? 64 : a.sq <= 5 ? 32 : 16;
        if (a.sq > 16) return "conv1d_wgrad: stride outside the path";
        a.ntg = ks / tg; pl.tg = tg;
        const int wq = (a.TK - 1) * a.sq + (tg - 1) * a.dil + 1;
        a.PQ = wq + ((6 - (wq & 3)) & 3);                          // next value = 2 (mod 4)
        pl.lds = ((size_t)WG_BM * (a.TK + 2) + (size_t)WG_BN * a.PQ) * sizeof(float);
        if (pl.lds > 64 * 1024) return "conv1d_wgrad: dilation outside the path (the staged window is kept within 64 KiB of LDS)";
        pl.name = tg == 8 ? "conv1d_wgrad_kernel<8>" : tg == 7 ? "conv1d_wgrad_kernel<7>" : tg == 5 ? "conv1d_wgrad_kernel<5>" :
                  tg == 4 ? "conv1d_wgrad_kernel<4>" : tg == 3 ? "conv1d_wgrad_kernel<3>" : tg == 2 ? "conv1d_wgrad_kernel<2>" : "conv1d_wgrad_kernel<1>";
        tiles = (long long)((a.M + WG_BM - 1) / WG_BM) * ((a.N + WG_BN - 1) / WG_BN) * a.ntg;
    }
    a.tk_shift = 0;
    while ((1 << a.tk_shift) < a.TK) ++a.tk_shift;
    a.cpb = (a.Tp + a.TK - 1) / a.TK;
    const long long nchunks = (long long)batch * a.cpb;
    long long ns = (WG_TARGET_BLOCKS + tiles - 1) / tiles;
    if (ns > nchunks) ns = nchunks;
    if (ns > WG_MAX_SPLIT) ns = WG_MAX_SPLIT;
    if (ns < 1) ns = 1;
    if (ns * a.ntg > 65535) ns = 65535 / a.ntg;
    a.nsplit = (int)ns;
    return nullptr;
}

template <int TG>
void wgrad_launch(const WgradArgs& a, const WgradPlan& pl, hipStream_t s)
{
    const dim3 grid((a.N + WG_BN - 1) / WG_BN, (a.M + WG_BM - 1) / WG_BM, a.nsplit * a.ntg);
    hipLaunchKernelGGL(conv1d_wgrad_kernel<TG>, grid, dim3(256), pl.lds, s, a);
}

// ---- per-channel sums over [B][C][T] (bias gradient, d/d alpha): slabs of CR_TS tokens of one item, cut into G contiguous ranges
constexpr int CR_TS = 2048;
constexpr int CR_TARGET_BLOCKS = 2048;
int cr_groups(int batch, int c, int t)
{
    const long long nslab = (long long)batch * ((t + CR_TS - 1) / CR_TS);
    long long g = CR_TARGET_BLOCKS / (c > 0 ? c : 1);
    if (g < 1) g = 1;
    if (g > nslab) g = nslab;
    if (g < 1) g = 1;
    return (int)g;
}

template <bool SNAKE>
__global__ __launch_bounds__(256) void chan_bwd_kernel(const float* __restrict__ gs, const float* __restrict__ x, const float* __restrict__ alpha,
                                                       const float* __restrict__ residual, float* __restrict__ gx, float* __restrict__ partial,
                                                       int B, int C, int T, int G)
{
    __shared__ float red[256];
    const int c = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
    const int spb = (T + CR_TS - 1) / CR_TS;
    const long long nslab = (long long)B * spb;
    const long long s0 = nslab * g / G, s1 = nslab * (g + 1) / G;
    const float al = SNAKE ? alpha[c] : 1.0f;
    const float inv = 1.0f / (al + 1e-9f);
    float acc = 0.0f;
    for (long long sl = s0; sl < s1; ++sl) {
        const int b = (int)(sl / spb);
        const int t0 = (int)(sl - (long long)b * spb) * CR_TS;
        const int t1 = t0 + CR_TS < T ? t0 + CR_TS : T;
        const size_t off = ((size_t)b * C + c) * T;
        for (int t = t0 + tid; t < t1; t += 256) {
            const float gv = gs[off + t];
            if (SNAKE) {
                const float xv = x[off + t];
                float v = gv * det_dsnake(xv, al, inv);                   // the input-gradient epilogue of mvq_conv1d_dgrad_f32, same function
                if (residual) v = v + residual[off + t];
                gx[off + t] = v;
                if (partial) acc = dfma(gv, det_dsnake_dalpha(xv, al, inv), acc);
            } else {
                acc += gv;
            }
        }
    }
    if (!partial) return;
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) partial[(size_t)c * G + g] = red[0];
}

__global__ __launch_bounds__(256) void chan_final_kernel(const float* __restrict__ partial, float* __restrict__ out, int C, int G)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float v = partial[(size_t)c * G];
    for (int g = 1; g < G; ++g) v += partial[(size_t)c * G + g];
    out[c] = v;
}

// one block per row r of v[rows][cols]: n = ||v_r||, s = <dW_r, v_r>;  dg_r = s/n;  dv_r = (g_r/n) * (dW_r - (s/n^2) v_r)
__global__ __launch_bounds__(256) void weight_norm_bwd_kernel(const float* __restrict__ dw, const float* __restrict__ v, const float* __restrict__ g,
                                                              float* __restrict__ dg, float* __restrict__ dv, int cols)
{
    __shared__ float red[2][256];
    const int tid = threadIdx.x;
    const size_t off = (size_t)blockIdx.x * cols;
    float ss = 0.0f, sd = 0.0f;
    for (int i = tid; i < cols; i += 256) { const float vi = v[off + i]; ss = dfma(vi, vi, ss); sd = dfma(dw[off + i], vi, sd); }
    red[0][tid] = ss; red[1][tid] = sd;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    const float n2 = red[0][0], s = red[1][0];
    const float n = __builtin_sqrtf(n2);
    if (dg && tid == 0) dg[blockIdx.x] = s / n;
    if (dv) {
        const float coef = g[blockIdx.x] / n, k = s / n2;
        for (int i = tid; i < cols; i += 256) dv[off + i] = coef * dfma(-k, v[off + i], dw[off + i]);
    }
}

int wfail(int code, const char* msg) { set_last_error(msg); return code; }
int wdone(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MVQ_OK;
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", what, hipGetErrorString(e));
    return wfail(MVQ_EHIP, msg);
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
}  // namespace
}  // namespace mvq

using namespace mvq;

extern "C" size_t mvq_conv1d_wgrad_workspace_bytes(int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil, int pad,
                                                   int transposed)
{
    WgradArgs a{}; WgradPlan pl{};
    if (wgrad_plan(batch, cin, tin, cout, tout, ks, stride, dil, pad, transposed, a, pl)) return 0;
    return a.nsplit > 1 ? (size_t)a.nsplit * pl.count * sizeof(float) : 0;
}

extern "C" int mvq_conv1d_wgrad_f32(const float* gy, const float* a_in, const float* snake_alpha, float* dw, void* workspace,
                                    size_t workspace_bytes, int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil,
                                    int pad, int transposed, void* stream)
{
    WgradArgs a{}; WgradPlan pl{};
    if (const char* why = wgrad_plan(batch, cin, tin, cout, tout, ks, stride, dil, pad, transposed, a, pl)) return wfail(MVQ_EINVAL, why);
    if (!dw) return wfail(MVQ_EINVAL, "conv1d_wgrad: null output");
    const bool empty = batch == 0 || a.Tp == 0;
    if (!empty && (!gy || !a_in)) return wfail(MVQ_EINVAL, "conv1d_wgrad: null tensor");
    const size_t need = a.nsplit > 1 ? (size_t)a.nsplit * pl.count * sizeof(float) : 0;
    if (need && (!workspace || workspace_bytes < need)) return wfail(MVQ_EINVAL, "conv1d_wgrad: workspace smaller than mvq_conv1d_wgrad_workspace_bytes()");
    if (need && (reinterpret_cast<uintptr_t>(workspace) & 3)) return wfail(MVQ_EINVAL, "conv1d_wgrad: workspace is not 4-byte aligned");
    hipStream_t s = S(stream);
    if (empty) {                                                    // no token: every sum is empty
        if (hipMemsetAsync(dw, 0, pl.count * sizeof(float), s) != hipSuccess) return wdone("conv1d_wgrad");
        return MVQ_OK;
    }
    a.p = transposed ? a_in : gy;
    a.q = transposed ? gy : a_in;
    a.alpha = snake_alpha;
    a.out = a.nsplit > 1 ? static_cast<float*>(workspace) : dw;
    const int pi = prof_enabled() ? prof_begin(pl.name, 2.0 * cin * (double)cout * ks * (double)a.Tp * batch, s) : -1;
    if (pl.rows) {
        hipLaunchKernelGGL(conv1d_wgrad_rows_kernel, dim3(a.N * a.ks, a.M, a.nsplit), dim3(256), 0, s, a);
    } else {
        switch (pl.tg) {
            case 8: wgrad_launch<8>(a, pl, s); break;
            case 7: wgrad_launch<7>(a, pl, s); break;
            case 5: wgrad_launch<5>(a, pl, s); break;
            case 4: wgrad_launch<4>(a, pl, s); break;
            case 3: wgrad_launch<3>(a, pl, s); break;
            case 2: wgrad_launch<2>(a, pl, s); break;
            default: wgrad_launch<1>(a, pl, s); break;
        }
    }
    if (a.nsplit > 1) {
        size_t blocks = (pl.count + 255) / 256; if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<const float*>(workspace), dw, pl.count, a.nsplit);
    }
    prof_end(pi, s);
    return wdone("conv1d_wgrad");
}

extern "C" size_t mvq_channel_reduce_workspace_bytes(int batch, int c, int t)
{
    if (batch < 1 || c < 1 || t < 1) return 0;
    return (size_t)c * cr_groups(batch, c, t) * sizeof(float);
}

static int chan_check(const char* who, int batch, int c, int t, const void* out, const void* workspace, size_t workspace_bytes)
{
    char msg[160];
    if (batch < 0 || c < 1 || t < 0 || t > (1 << 28)) { snprintf(msg, sizeof(msg), "%s: bad shape", who); return wfail(MVQ_EINVAL, msg); }
    if (out && batch > 0 && t > 0) {
        const size_t need = mvq_channel_reduce_workspace_bytes(batch, c, t);
        if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3)) {
            snprintf(msg, sizeof(msg), "%s: workspace smaller than mvq_channel_reduce_workspace_bytes()", who);
            return wfail(MVQ_EINVAL, msg);
        }
    }
    return MVQ_OK;
}

extern "C" int mvq_snake_bwd_f32(const float* gs, const float* x, const float* alpha, const float* residual, float* gx, float* dalpha,
                                 void* workspace, size_t workspace_bytes, int batch, int c, int t, void* stream)
{
    if (const int rc = chan_check("snake_bwd", batch, c, t, dalpha, workspace, workspace_bytes)) return rc;
    if (!alpha || !gx) return wfail(MVQ_EINVAL, "snake_bwd: null tensor");
    hipStream_t s = S(stream);
    if (batch == 0 || t == 0) {
        if (dalpha && hipMemsetAsync(dalpha, 0, (size_t)c * sizeof(float), s) != hipSuccess) return wdone("snake_bwd");
        return MVQ_OK;
    }
    if (!gs || !x) return wfail(MVQ_EINVAL, "snake_bwd: null tensor");
    const int G = cr_groups(batch, c, t);
    const int pi = prof_enabled() ? prof_begin("snake_bwd_kernel", 0.0, s) : -1;
    hipLaunchKernelGGL(chan_bwd_kernel<true>, dim3(c, G), dim3(256), 0, s, gs, x, alpha, residual, gx, dalpha ? static_cast<float*>(workspace) : nullptr,
                       batch, c, t, G);
    if (dalpha) hipLaunchKernelGGL(chan_final_kernel, dim3((c + 255) / 256), dim3(256), 0, s, static_cast<const float*>(workspace), dalpha, c, G);
    prof_end(pi, s);
    return wdone("snake_bwd");
}

extern "C" int mvq_bias_grad_f32(const float* gy, float* db, void* workspace, size_t workspace_bytes, int batch, int c, int t, void* stream)
{
    if (!db) return wfail(MVQ_EINVAL, "bias_grad: null output");
    if (const int rc = chan_check("bias_grad", batch, c, t, db, workspace, workspace_bytes)) return rc;
    hipStream_t s = S(stream);
    if (batch == 0 || t == 0) {
        if (hipMemsetAsync(db, 0, (size_t)c * sizeof(float), s) != hipSuccess) return wdone("bias_grad");
        return MVQ_OK;
    }
    if (!gy) return wfail(MVQ_EINVAL, "bias_grad: null tensor");
    const int G = cr_groups(batch, c, t);
    const int pi = prof_enabled() ? prof_begin("bias_grad_kernel", 0.0, s) : -1;
    hipLaunchKernelGGL(chan_bwd_kernel<false>, dim3(c, G), dim3(256), 0, s, gy, nullptr, nullptr, nullptr, nullptr, static_cast<float*>(workspace),
                       batch, c, t, G);
    hipLaunchKernelGGL(chan_final_kernel, dim3((c + 255) / 256), dim3(256), 0, s, static_cast<const float*>(workspace), db, c, G);
    prof_end(pi, s);
    return wdone("bias_grad");
}

extern "C" int mvq_weight_norm_bwd_f32(const float* dw, const float* v, const float* g, float* dg, float* dv, int rows, int cols, void* stream)
{
    if (rows < 0 || cols < 1) return wfail(MVQ_EINVAL, "weight_norm_bwd: bad shape");
    if (rows == 0) return MVQ_OK;
    if (!dw || !v || (dv && !g) || (!dg && !dv)) return wfail(MVQ_EINVAL, "weight_norm_bwd: null tensor");
    hipLaunchKernelGGL(weight_norm_bwd_kernel, dim3(rows), dim3(256), 0, S(stream), dw, v, g, dg, dv, cols);
    return wdone("weight_norm_bwd");
}
