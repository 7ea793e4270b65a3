// kernels_small.hip -- everything on the path that is not a dense conv GEMM:
//   weight preparation (weight-norm fold, K-major packing), direct convs for the degenerate ends of the
//   stacks (Cin = 1, Cout = 1, odd shapes), LayerNorm / attention / GELU of the CrossPredictor and row
//   glue.  All follow the arithmetic contract of include/mvq.h (sequential fp32 fma chains).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "det_math.hpp"
#include "kernels_small.hpp"
#include "ln_lat.hpp"

namespace mvq {

// ------------------------------------------------------------------------------------------------
// weight_norm fold: one thread per dim-0 row, chain over the row (one-off at model load)
// ------------------------------------------------------------------------------------------------
__global__ void weight_norm_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                   float* __restrict__ w, int rows, int inner)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* vr = v + (size_t)r * inner;
    float ss = 0.0f;
    for (int i = 0; i < inner; ++i) ss = dfma(vr[i], vr[i], ss);
    const float scale = g[r] / __builtin_sqrtf(ss);
    for (int i = 0; i < inner; ++i) w[(size_t)r * inner + i] = vr[i] * scale;
}

hipError_t launch_weight_norm(const float* v, const float* g, float* w, int rows, int inner, hipStream_t s)
{
    hipLaunchKernelGGL(weight_norm_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, v, g, w, rows, inner);
    return hipGetLastError();
}

// wp[(ci*ks + kk) * Mpad + co] = w[co, ci, kk]   (zero for co >= Cout)
__global__ void pack_conv1d_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                   int cin, int cout, int ks, int mpad)
{
    const size_t total = (size_t)cin * ks * mpad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i % mpad);
        const size_t row = i / mpad;
        const int kk = (int)(row % ks);
        const int ci = (int)(row / ks);
        wp[i] = m < cout ? w[((size_t)m * cin + ci) * ks + kk] : 0.0f;
    }
}

hipError_t launch_pack_conv1d(const float* w, float* wp, int cin, int cout, int ks, int mpad, hipStream_t s)
{
    const size_t total = (size_t)cin * ks * mpad;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv1d_kernel, dim3(blocks), dim3(256), 0, s, w, wp, cin, cout, ks, mpad);
    return hipGetLastError();
}

// polyphase image of ConvTranspose1d weights w[Cin, Cout, 2S]:
//   wp[(ci*2 + j) * Mpad + (co*S + r)] = j == 0 ? w[ci, co, r + S] (pairs with x[q-1]) : w[ci, co, r] (x[q])
__global__ void pack_convtr_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                   int cin, int cout, int S, int mpad)
{
    const size_t total = (size_t)cin * 2 * mpad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i % mpad);
        const size_t row = i / mpad;
        const int j = (int)(row & 1);
        const int ci = (int)(row >> 1);
        float val = 0.0f;
        if (m < cout * S) {
            const int co = m / S, r = m - co * S;
            val = w[((size_t)ci * cout + co) * (2 * S) + (j == 0 ? r + S : r)];
        }
        wp[i] = val;
    }
}

hipError_t launch_pack_convtr(const float* w, float* wp, int cin, int cout, int S, int mpad, hipStream_t s)
{
    const size_t total = (size_t)cin * 2 * mpad;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_convtr_kernel, dim3(blocks), dim3(256), 0, s, w, wp, cin, cout, S, mpad);
    return hipGetLastError();
}

// dgrad weight images (the input-gradient of a conv is a conv with transformed weights):
//   Conv1d w[Cout,Cin,ks] (stride 1, symmetric padding):  dX = conv1d(dY, w'),  w'[ci,co,k] = w[co,ci,ks-1-k]
//      packed  wp[(co*ks + k) * Mpad + ci] = w[co, ci, ks-1-k]          (K index = (co, k), rows = ci)
//   ConvTranspose1d w[Cin,Cout,ks] (stride s, padding p): dX = conv1d(dY, w, stride s, pad p) with out = Cin, in = Cout
//      packed  wp[(co*ks + k) * Mpad + ci] = w[ci, co, k]
__global__ void pack_conv1d_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                         int cin, int cout, int ks, int mpad, int transposed)
{
    const size_t total = (size_t)cout * ks * mpad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % mpad);
        const size_t row = i / mpad;
        const int k = (int)(row % ks);
        const int co = (int)(row / ks);
        float v = 0.0f;
        if (ci < cin) v = transposed ? w[((size_t)ci * cout + co) * ks + k] : w[((size_t)co * cin + ci) * ks + (ks - 1 - k)];
        wp[i] = v;
    }
}

hipError_t launch_pack_conv1d_dgrad(const float* w, float* wp, int cin, int cout, int ks, int mpad, hipStream_t s)
{
    const size_t total = (size_t)cout * ks * mpad;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv1d_dgrad_kernel, dim3(blocks), dim3(256), 0, s, w, wp, cin, cout, ks, mpad, 0);
    return hipGetLastError();
}

hipError_t launch_pack_convtr_dgrad(const float* w, float* wp, int cin, int cout, int ks, int mpad, hipStream_t s)
{
    const size_t total = (size_t)cout * ks * mpad;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv1d_dgrad_kernel, dim3(blocks), dim3(256), 0, s, w, wp, cin, cout, ks, mpad, 1);
    return hipGetLastError();
}

__global__ void mul_dtanh_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ out, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = g[i] * dfma(-y[i], y[i], 1.0f);
}

hipError_t launch_mul_dtanh(const float* g, const float* y, float* out, size_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(mul_dtanh_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, y, out, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// direct conv1d: one thread per output sample, chain over (ci, kk).  Reads the PACKED weight image so
// that callers hold one weight format.  Used where the GEMM view has no dense tile: Cin = 1 (encoder
// input conv), Cout = 1 (decoder output conv + tanh), Cout = 8 and any shape the MFMA units lack.
// ------------------------------------------------------------------------------------------------
__global__ void conv1d_direct_kernel(DirectConvArgs a)
{
    const size_t total = (size_t)a.B * a.Cout * a.Tout;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % a.Tout);
        const size_t bc = i / a.Tout;
        const int co = (int)(bc % a.Cout);
        const int b = (int)(bc / a.Cout);
        const float* xb = a.x + (size_t)b * a.Cin * a.Tin;
        const int g0 = t * a.stride - a.pad;
        float acc = 0.0f;
        for (int ci = 0; ci < a.Cin; ++ci) {
            float al = 0.0f, inv = 0.0f;
            if (a.alpha_in) { al = a.alpha_in[ci]; inv = 1.0f / (al + 1e-9f); }
            const float* xr = xb + (size_t)ci * a.Tin;
            const float* wr = a.wp + (size_t)ci * a.ks * a.Mpad + co;
            for (int kk = 0; kk < a.ks; ++kk) {
                const int g = g0 + kk * a.dil;
                float xv = 0.0f;
                if (g >= 0 && g < a.Tin) { xv = xr[g]; if (a.alpha_in) xv = det_snake(xv, al, inv); }
                acc = dfma(wr[(size_t)kk * a.Mpad], xv, acc);
            }
        }
        float v = acc + (a.bias ? a.bias[co] : 0.0f);
        if (a.dsn_src) { const float ad = a.dsn_alpha[co]; v = v * det_dsnake(a.dsn_src[i], ad, 1.0f / (ad + 1e-9f)); }
        if (a.residual) v = v + a.residual[i];
        if (a.y2) { const float a2 = a.alpha2[co]; a.y2[i] = det_snake(v, a2, 1.0f / (a2 + 1e-9f)); }
        if (a.alpha_out) { const float al = a.alpha_out[co]; v = det_snake(v, al, 1.0f / (al + 1e-9f)); }
        if (a.act == 1) v = det_tanh(v);
        a.y[i] = v;
    }
}

// Cin == 1, stride 1, dil 1 (encoder input conv; the input-gradient of the decoder output conv): a pure streaming WRITE
// (Cout rows out for one row in).  Each thread owns 4 consecutive output samples and walks CG output channels with the
// KS + 3 input samples of its window held in registers (fetched once, as three aligned 16-byte loads when the row allows),
// so the only memory instruction per 16 bytes written is the store itself; the taps / bias / alphas of a channel are
// block-uniform (scalar loads).  Chain per output: taps ascending from +0.0f, then + bias (the contract).
constexpr int CIN1_CG = 16;

template <int KS>
__global__ __launch_bounds__(256) void conv1d_cin1_kernel(DirectConvArgs a)
{
    const int co0 = blockIdx.y * CIN1_CG, b = blockIdx.z;
    const int t0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= a.Tout) return;
    const float* xr = a.x + (size_t)b * a.Tin;
    float xv[KS + 3];
    const bool vin = KS == 7 && a.pad == 3 && (a.Tin & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.x) & 15) == 0) && t0 + 3 < a.Tin;
    if (vin) {                                           // window t0-3 .. t0+6 inside the aligned quads t0-4, t0, t0+4
        typedef float v4 __attribute__((ext_vector_type(4)));
        const v4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
        const v4 q0 = t0 >= 4 ? *reinterpret_cast<const v4*>(xr + t0 - 4) : z4;
        const v4 q1 = *reinterpret_cast<const v4*>(xr + t0);
        const v4 q2 = t0 + 4 < a.Tin ? *reinterpret_cast<const v4*>(xr + t0 + 4) : z4;
        xv[0] = q0.y; xv[1] = q0.z; xv[2] = q0.w; xv[3] = q1.x; xv[4] = q1.y; xv[5] = q1.z; xv[6] = q1.w;
        xv[7] = q2.x; xv[8] = q2.y; xv[9] = q2.z;
    } else {
#pragma unroll
        for (int i = 0; i < KS + 3; ++i) {
            const int g = t0 - a.pad + i;
            xv[i] = (g >= 0 && g < a.Tin) ? xr[g] : 0.0f;
        }
    }
    const int nco = a.Cout - co0 < CIN1_CG ? a.Cout - co0 : CIN1_CG;
    for (int c = 0; c < nco; ++c) {
        const int co = co0 + c;
        float w[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) w[k] = a.wp[(size_t)k * a.Mpad + co];
        const float bv = a.bias ? a.bias[co] : 0.0f;
        float al = 0.0f, inv = 0.0f, a2 = 0.0f, i2 = 0.0f, ad = 0.0f, idv = 0.0f;
        if (a.dsn_src) { ad = a.dsn_alpha[co]; idv = 1.0f / (ad + 1e-9f); }
        if (a.alpha_out) { al = a.alpha_out[co]; inv = 1.0f / (al + 1e-9f); }
        if (a.y2) { a2 = a.alpha2[co]; i2 = 1.0f / (a2 + 1e-9f); }
        const size_t off = ((size_t)b * a.Cout + co) * a.Tout + t0;
        const bool vec = (t0 + 3 < a.Tout) && ((off & 3) == 0);
        float ds[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.dsn_src) {
            if (vec) { const float4 d4 = *reinterpret_cast<const float4*>(a.dsn_src + off); ds[0] = d4.x; ds[1] = d4.y; ds[2] = d4.z; ds[3] = d4.w; }
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (t0 + j < a.Tout) ds[j] = a.dsn_src[off + j];
            }
        }
        float o[4], o2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < KS; ++k) acc = dfma(w[k], xv[j + k], acc);
            float v = acc + bv;
            if (a.dsn_src) v = v * det_dsnake(ds[j], ad, idv);
            o2[j] = a.y2 ? det_snake(v, a2, i2) : 0.0f;
            if (a.alpha_out) v = det_snake(v, al, inv);
            if (a.act == 1) v = det_tanh(v);
            o[j] = v;
        }
        if (vec) {
            *reinterpret_cast<float4*>(a.y + off) = make_float4(o[0], o[1], o[2], o[3]);
            if (a.y2) *reinterpret_cast<float4*>(a.y2 + off) = make_float4(o2[0], o2[1], o2[2], o2[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + j < a.Tout) { a.y[off + j] = o[j]; if (a.y2) a.y2[off + j] = o2[j]; }
        }
    }
}

// Cout == 1, stride 1, dil 1 (decoder output conv + tanh): 4 outputs per thread share a sliding window of KS+3
// inputs per channel; weights staged in LDS.  Chain order per output: ci ascending, tap ascending (the contract).
template <int KS>
__global__ __launch_bounds__(256) void conv1d_cout1_kernel(DirectConvArgs a)
{
    extern __shared__ float wl[];                        // [Cin*KS]
    for (int i = threadIdx.x; i < a.Cin * KS; i += 256) wl[i] = a.wp[(size_t)i * a.Mpad];
    __syncthreads();
    const int b = blockIdx.y;
    const int t0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= a.Tout) return;
    const float* xb = a.x + (size_t)b * a.Cin * a.Tin;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool vec = KS == 7 && a.pad == 3 && (a.Tin & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.x) & 15) == 0) && t0 + 3 < a.Tin;
    for (int ci = 0; ci < a.Cin; ++ci) {
        const float* xr = xb + (size_t)ci * a.Tin;
        float xv[KS + 3];
        if (vec) {                                       // pad == 3, rows 16-byte aligned: the window t0-3 .. t0+6 sits inside
            typedef float v4 __attribute__((ext_vector_type(4)));          // the three aligned quads t0-4, t0, t0+4
            const v4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
            const v4 q0 = t0 >= 4 ? *reinterpret_cast<const v4*>(xr + t0 - 4) : z4;
            const v4 q1 = *reinterpret_cast<const v4*>(xr + t0);
            const v4 q2 = t0 + 4 < a.Tin ? *reinterpret_cast<const v4*>(xr + t0 + 4) : z4;
            xv[0] = q0.y; xv[1] = q0.z; xv[2] = q0.w; xv[3] = q1.x; xv[4] = q1.y; xv[5] = q1.z; xv[6] = q1.w;
            xv[7] = q2.x; xv[8] = q2.y; xv[9] = q2.z;
        } else {
#pragma unroll
            for (int i = 0; i < KS + 3; ++i) {
                const int g = t0 - a.pad + i;
                xv[i] = (g >= 0 && g < a.Tin) ? xr[g] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const float w = wl[ci * KS + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = dfma(w, xv[j + k], acc[j]);
        }
    }
    const float bv = a.bias ? a.bias[0] : 0.0f;
    const size_t off = (size_t)b * a.Tout + t0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (t0 + j < a.Tout) {
            float v = acc[j] + bv;
            if (a.residual) v = v + a.residual[off + j];
            if (a.alpha_out) { const float al = a.alpha_out[0]; v = det_snake(v, al, 1.0f / (al + 1e-9f)); }
            if (a.act == 1) v = det_tanh(v);
            a.y[off + j] = v;
        }
    }
}

hipError_t launch_conv1d_direct(const DirectConvArgs& a, hipStream_t s)
{
    if (a.Cin == 1 && a.ks == 7 && a.stride == 1 && a.dil == 1 && !a.alpha_in && !a.residual) {
        dim3 grid((unsigned)((a.Tout + 1023) / 1024), (unsigned)((a.Cout + CIN1_CG - 1) / CIN1_CG), (unsigned)a.B);
        const int pi = prof_enabled() ? prof_begin("conv1d_cin1_kernel<7>", 2.0 * 7 * a.Cout * (double)a.Tout * a.B, s) : -1;
        hipLaunchKernelGGL(conv1d_cin1_kernel<7>, grid, dim3(256), 0, s, a);
        prof_end(pi, s);
        return hipGetLastError();
    }
    if (a.Cout == 1 && a.ks == 7 && a.stride == 1 && a.dil == 1 && !a.alpha_in && !a.y2 && !a.dsn_src && a.Cin * 7 * 4 <= 48 * 1024) {
        dim3 grid((unsigned)((a.Tout + 1023) / 1024), (unsigned)a.B);
        const int pi = prof_enabled() ? prof_begin("conv1d_cout1_kernel<7>", 2.0 * 7 * a.Cin * (double)a.Tout * a.B, s) : -1;
        hipLaunchKernelGGL(conv1d_cout1_kernel<7>, grid, dim3(256), (size_t)a.Cin * 7 * sizeof(float), s, a);
        prof_end(pi, s);
        return hipGetLastError();
    }
    const size_t total = (size_t)a.B * a.Cout * a.Tout;
    size_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(conv1d_direct_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// direct conv_transpose1d on the polyphase image (one thread per output sample)
__global__ void convtr_direct_kernel(DirectConvArgs a)   // a.stride = S, a.pad = P, a.ks unused
{
    const size_t total = (size_t)a.B * a.Cout * a.Tout;
    const int S = a.stride;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % a.Tout);
        const size_t bc = i / a.Tout;
        const int co = (int)(bc % a.Cout);
        const int b = (int)(bc / a.Cout);
        const int num = t + a.pad;
        const int q = num / S, r = num - q * S;
        const float* xb = a.x + (size_t)b * a.Cin * a.Tin;
        const int m = co * S + r;
        float acc = 0.0f;
        for (int ci = 0; ci < a.Cin; ++ci) {
            float al = 0.0f, inv = 0.0f;
            if (a.alpha_in) { al = a.alpha_in[ci]; inv = 1.0f / (al + 1e-9f); }
            const float* xr = xb + (size_t)ci * a.Tin;
            float x0 = 0.0f, x1 = 0.0f;
            if (q - 1 >= 0 && q - 1 < a.Tin) { x0 = xr[q - 1]; if (a.alpha_in) x0 = det_snake(x0, al, inv); }
            if (q < a.Tin) { x1 = xr[q]; if (a.alpha_in) x1 = det_snake(x1, al, inv); }
            acc = dfma(a.wp[((size_t)ci * 2 + 0) * a.Mpad + m], x0, acc);
            acc = dfma(a.wp[((size_t)ci * 2 + 1) * a.Mpad + m], x1, acc);
        }
        float v = acc + (a.bias ? a.bias[co] : 0.0f);
        if (a.y2) { const float a2 = a.alpha2[co]; a.y2[i] = det_snake(v, a2, 1.0f / (a2 + 1e-9f)); }
        if (a.alpha_out) { const float al = a.alpha_out[co]; v = det_snake(v, al, 1.0f / (al + 1e-9f)); }
        a.y[i] = v;
    }
}

hipError_t launch_convtr_direct(const DirectConvArgs& a, hipStream_t s)
{
    const size_t total = (size_t)a.B * a.Cout * a.Tout;
    size_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(convtr_direct_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// LayerNorm over C of channel-major x (+ optional positional-encoding add, tanh, scale); element (b,c,t) at
// b*sb + c*sc + t.  The contract fixes the reduction order (channel ascending, sequential), so a block stages a
// [C][LN_TOK-token] tile in LDS with coalesced loads, LN_TOK threads walk their token's channel column out of LDS
// (conflict-free: lane = token), and all 256 threads normalise and store coalesced.
// Fallback (C too large for LDS): one thread per token straight from global memory.
// ------------------------------------------------------------------------------------------------
// LN_TOK tokens per block: 8 for throughput; 4 when there are only a few tokens (one AR chunk of one segment): the block's
// staging and normalise passes shrink and more blocks share the work -- the ordered per-token chain is unchanged.

template <int LN_TOK>
__global__ __launch_bounds__(256) void layernorm_c_tile_kernel(
    const float* __restrict__ x, const float* __restrict__ pe, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ y, int B, int C, int T, size_t sb, size_t sc,
    float eps, int do_tanh, float post_scale, const float* __restrict__ sub)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [C][LN_TOK] | mean[LN_TOK] | rstd[LN_TOK]
    float* mean_s = tile + (size_t)C * LN_TOK;
    float* rstd_s = mean_s + LN_TOK;
    const int tid = threadIdx.x;
    const int tok = tid & (LN_TOK - 1);
    const int cg = tid / LN_TOK;                                       // 0..7
    const int n = blockIdx.x * LN_TOK + tok;
    const bool live = n < B * T;
    const int b = live ? n / T : 0, t = live ? n - b * T : 0;
    const float* xb = x + (size_t)b * sb + t;
    const float* sbp = sub ? sub + (size_t)b * sb + t : nullptr;       // x - sub (the AR residual r = zt - z_pred), same layout
    const float* per = pe ? pe + (size_t)t * C : nullptr;
    constexpr int CG = 256 / LN_TOK;                                   // channel groups (8)
    for (int c0 = cg; c0 < C; c0 += CG * 8) {                          // 8 loads in flight per thread
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = c0 + u * CG;
            v[u] = (live && c < C) ? xb[(size_t)c * sc] : 0.0f;
        }
        if (sbp) {
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int c = c0 + u * CG; if (live && c < C) v[u] = v[u] - sbp[(size_t)c * sc]; }
        }
        if (per) {
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int c = c0 + u * CG; if (live && c < C) v[u] = v[u] + per[c]; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int c = c0 + u * CG; if (c < C) tile[c * LN_TOK + tok] = v[u]; }
    }
    __syncthreads();
    if (tid < LN_TOK) {
        // The two ordered chains (sum, then squared deviations: 2 C dependent operations) are what a small call waits for.  Their
        // LDS operands are fetched one batch AHEAD of the chain (round 5: each batch of 16 reads used to be issued only after the
        // previous batch's additions -- 128 exposed LDS latencies per token at C = 1024, about half of the call).
        const float* col = tile + tid;
        float s = 0.0f;
        int c = 0;
        float v[16], w[16];
        if (C >= 16) {
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = col[u * LN_TOK];
        }
        for (; c + 32 <= C; c += 32) {
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = col[(c + 16 + u) * LN_TOK];
#pragma unroll
            for (int u = 0; u < 16; ++u) s = s + v[u];
            if (c + 48 <= C) {
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = col[(c + 32 + u) * LN_TOK];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) s = s + w[u];
        }
        if (c + 16 <= C) {                                        // an odd number of 16-channel batches: v holds the last one
#pragma unroll
            for (int u = 0; u < 16; ++u) s = s + v[u];
            c += 16;
        }
        for (; c < C; ++c) s = s + col[c * LN_TOK];
        const float mean = s / (float)C;
        float var = 0.0f;
        c = 0;
        if (C >= 16) {
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = col[u * LN_TOK];
        }
        for (; c + 32 <= C; c += 32) {
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = col[(c + 16 + u) * LN_TOK];
#pragma unroll
            for (int u = 0; u < 16; ++u) { const float d = v[u] - mean; var = dfma(d, d, var); }
            if (c + 48 <= C) {
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = col[(c + 32 + u) * LN_TOK];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) { const float d = w[u] - mean; var = dfma(d, d, var); }
        }
        if (c + 16 <= C) {
#pragma unroll
            for (int u = 0; u < 16; ++u) { const float d = v[u] - mean; var = dfma(d, d, var); }
            c += 16;
        }
        for (; c < C; ++c) { const float d = col[c * LN_TOK] - mean; var = dfma(d, d, var); }
        mean_s[tid] = mean;
        rstd_s[tid] = 1.0f / __builtin_sqrtf(var / (float)C + eps);
    }
    __syncthreads();
    if (!live) return;
    const float mean = mean_s[tok], rstd = rstd_s[tok];
    float* yb = y + (size_t)b * sb + t;
    for (int c = cg; c < C; c += 256 / LN_TOK) {
        float o = dfma((tile[c * LN_TOK + tok] - mean) * rstd, gamma[c], beta[c]);
        if (do_tanh) o = det_tanh(o);
        if (do_tanh || post_scale != 1.0f) o = post_scale * o;
        yb[(size_t)c * sc] = o;
    }
}

// The latency form (ln_lat.hpp): 4 tokens per block, every operand requested up front, b128-fed chains.  Few tokens -- one AR chunk,
// the keys / values of a handful of segments -- are what it is for; beyond a block per CU the 8-token tiles above take over.
__global__ __launch_bounds__(256) void layernorm_c_lat_kernel(const LnIo io, int B, int C, int T)
{
    extern __shared__ __attribute__((aligned(16))) float ln_lat_smem[];
    ln_lat_task(io, blockIdx.x, B, T, C, ln_lat_smem, threadIdx.x, [](const float* p) { return *p; });
}

hipError_t launch_layernorm_lat_io(const LnIo& io, int B, int C, int n, hipStream_t s)      // the general form (two outputs, shifted input): ar_fused.hip
{
    if (B * n == 0) return hipSuccess;
    if (C % 64 != 0 || ln_lat_lds_floats(C) * sizeof(float) > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(layernorm_c_lat_kernel, dim3((B * n + LN_LAT_TOK - 1) / LN_LAT_TOK), dim3(256), ln_lat_lds_floats(C) * sizeof(float), s, io, B, C, n);
    return hipGetLastError();
}

__global__ void layernorm_c_kernel(const float* __restrict__ x, const float* __restrict__ pe,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ y, int B, int C, int T, size_t sb, size_t sc,
                                   float eps, int do_tanh, float post_scale, const float* __restrict__ sub)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= B * T) return;
    const int b = n / T, t = n - b * T;
    const float* xb = x + (size_t)b * sb + t;
    const float* sbp = sub ? sub + (size_t)b * sb + t : nullptr;
    const float* per = pe ? pe + (size_t)t * C : nullptr;
    float s = 0.0f;
    for (int c = 0; c < C; ++c) {
        float v = xb[(size_t)c * sc];
        if (sbp) v = v - sbp[(size_t)c * sc];
        if (per) v = v + per[c];
        s = s + v;
    }
    const float mean = s / (float)C;
    float var = 0.0f;
    for (int c = 0; c < C; ++c) {
        float v = xb[(size_t)c * sc];
        if (sbp) v = v - sbp[(size_t)c * sc];
        if (per) v = v + per[c];
        const float d = v - mean;
        var = dfma(d, d, var);
    }
    const float rstd = 1.0f / __builtin_sqrtf(var / (float)C + eps);
    float* yb = y + (size_t)b * sb + t;
    for (int c = 0; c < C; ++c) {
        float v = xb[(size_t)c * sc];
        if (sbp) v = v - sbp[(size_t)c * sc];
        if (per) v = v + per[c];
        float o = dfma((v - mean) * rstd, gamma[c], beta[c]);
        if (do_tanh) o = det_tanh(o);
        if (do_tanh || post_scale != 1.0f) o = post_scale * o;
        yb[(size_t)c * sc] = o;
    }
}

// The tile kernels and the latency form serve C <= LN_TILE_MAX_C: the width whose [C][32-token] tile (+ 64 floats) filled the CU's
// 160 KiB when 32-token tiles were the throughput form.  The bound outlived that tile: wider inputs take the one-thread-per-token
// kernel, and every decision below depends on it.
constexpr int LN_TILE_MAX_C = 1278;
static_assert(((size_t)LN_TILE_MAX_C * 8 + 16) * sizeof(float) <= 64 * 1024, "the 8-token tile fits the default dynamic LDS limit");

LnForm layernorm_form(int n, int C)
{
    if (C > LN_TILE_MAX_C) return LnForm::Scalar;
    // The per-token chain (2 x C dependent operations) is latency, not bandwidth: what shortens a call is MORE BLOCKS walking
    // chains side by side.  8-token tiles (32 KB of LDS at C = 1024: five blocks per CU) put 2 400 blocks on the 19 200 tokens
    // of a 256-segment batch where a 32-token tile (128 KB, one block per CU) put 600 -- round 4: 2.3 -> see DESIGN 6c ms per step.
    if (n <= 1024 && C % 64 == 0 && ln_lat_lds_floats(C) * sizeof(float) <= 64 * 1024) return LnForm::Lat;
    return n > 64 ? LnForm::Tile8 : LnForm::Tile4;
}

const char* layernorm_form_name(LnForm f)
{
    switch (f) {
        case LnForm::Lat:   return "layernorm_c_lat_kernel";
        case LnForm::Tile8: return "layernorm_c_tile_kernel<8>";
        case LnForm::Tile4: return "layernorm_c_tile_kernel<4>";
        default:            return "layernorm_c_kernel";
    }
}

hipError_t launch_layernorm_c(const float* x, const float* pe, const float* gamma, const float* beta, float* y,
                              int B, int C, int T, size_t sb, size_t sc, float eps, int do_tanh, float post_scale,
                              const float* sub, hipStream_t s)
{
    const int n = B * T;
    if (n == 0) return hipSuccess;
    const LnForm form = layernorm_form(n, C);
    if (form != LnForm::Scalar) {
        static BigLdsOptIn opt8, opt4;
        hipError_t e = opt8.ensure(reinterpret_cast<const void*>(layernorm_c_tile_kernel<8>));
        if (e == hipSuccess) e = opt4.ensure(reinterpret_cast<const void*>(layernorm_c_tile_kernel<4>));
        if (e != hipSuccess) return e;
    }
    switch (form) {
        case LnForm::Lat: {
            LnIo io{};
            io.x = x; io.x_sb = sb; io.x_sc = sc;
            io.sub = sub; io.sub_sb = sb; io.sub_sc = sc;
            io.pe = pe; io.gamma = gamma; io.beta = beta;
            io.y0 = y; io.y0_sb = sb; io.y0_sc = sc;
            io.eps = eps; io.post_scale = post_scale; io.do_tanh = do_tanh;
            hipLaunchKernelGGL(layernorm_c_lat_kernel, dim3((n + LN_LAT_TOK - 1) / LN_LAT_TOK), dim3(256), ln_lat_lds_floats(C) * sizeof(float), s, io, B, C, T);
            break;
        }
        case LnForm::Tile8:
            hipLaunchKernelGGL(layernorm_c_tile_kernel<8>, dim3((n + 7) / 8), dim3(256), ((size_t)C * 8 + 16) * sizeof(float), s,
                               x, pe, gamma, beta, y, B, C, T, sb, sc, eps, do_tanh, post_scale, sub);
            break;
        case LnForm::Tile4:
            hipLaunchKernelGGL(layernorm_c_tile_kernel<4>, dim3((n + 3) / 4), dim3(256), ((size_t)C * 4 + 8) * sizeof(float), s,
                               x, pe, gamma, beta, y, B, C, T, sb, sc, eps, do_tanh, post_scale, sub);
            break;
        case LnForm::Scalar:
            hipLaunchKernelGGL(layernorm_c_kernel, dim3((n + 63) / 64), dim3(64), 0, s, x, pe, gamma, beta, y, B, C, T, sb, sc,
                               eps, do_tanh, post_scale, sub);
            break;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// attention core: one block per (batch element, head).  Q, K, V head slices are staged in LDS; one thread per
// (query, key) pair walks the dh-long score chain, Tq threads do the (ordered) softmax rows, then one thread per
// (channel, query) output walks the Tk-long value chain.  Tq, Tk <= 64.
// MASKED (mvq_attention_masked_f32): item b's key j is present when kmask[b*msb + j] != 0.  Tk <= 64 is one wave, so every
// wave takes ONE ballot of the item's mask row; a present key's slot among the staged columns is the popcount of the
// present keys below it, and absent columns are never loaded.  From there on the kernel is the plain one at Tk = the
// number of present keys: the result is that of the plain launch on the compacted K / V, bit for bit, and 0 keys give +0.
// ------------------------------------------------------------------------------------------------
template <bool MASKED>
__global__ __launch_bounds__(256) void attention_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, float* __restrict__ ctx,
    int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
    const uint8_t* __restrict__ kmask, size_t msb)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / H, hd = blockIdx.x - b * H;
    const float* q = Q + (size_t)b * qsb + (size_t)hd * dh * qsc;
    const float* kb = K + (size_t)b * ksb + (size_t)hd * dh * ksc;
    const float* vb = V + (size_t)b * ksb + (size_t)hd * dh * ksc;
    unsigned long long present = 0;
    const int TkAll = Tk;                 // columns in memory
    if (MASKED) {
        const int lane = tid & 63;
        present = __ballot(lane < TkAll && kmask[(size_t)b * msb + lane] != 0);
        Tk = __popcll(present);           // the same in every wave
    }
    float* Qs = sm;                       // [dh][Tq]
    float* Ks = Qs + dh * Tq;             // [dh][Tk]
    float* Vs = Ks + dh * Tk;             // [dh][Tk]
    float* P = Vs + dh * Tk;              // [Tq][Tk]
    for (int e = tid; e < dh * Tq; e += 256) { const int d = e / Tq, i = e - d * Tq; Qs[e] = q[(size_t)d * qsc + i]; }
    if (MASKED) {
        for (int e = tid; e < dh * TkAll; e += 256) {
            const int d = e / TkAll, j = e - d * TkAll;
            if ((present >> j) & 1ull) {
                const int slot = __popcll(present & ((1ull << j) - 1ull));
                Ks[d * Tk + slot] = kb[(size_t)d * ksc + j];
                Vs[d * Tk + slot] = vb[(size_t)d * ksc + j];
            }
        }
    } else {
        for (int e = tid; e < dh * Tk; e += 256) {
            const int d = e / Tk, j = e - d * Tk;
            Ks[e] = kb[(size_t)d * ksc + j];
            Vs[e] = vb[(size_t)d * ksc + j];
        }
    }
    __syncthreads();
    const float rs = __builtin_sqrtf((float)dh);
    for (int p = tid; p < Tq * Tk; p += 256) {
        const int i = p / Tk, j = p - i * Tk;
        float a = 0.0f;
        int d = 0;
        for (; d + 8 <= dh; d += 8) {
            float qv[8], kv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { qv[u] = Qs[(d + u) * Tq + i]; kv[u] = Ks[(d + u) * Tk + j]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) a = dfma(qv[u], kv[u], a);
        }
        for (; d < dh; ++d) a = dfma(Qs[d * Tq + i], Ks[d * Tk + j], a);
        P[p] = a / rs;
    }
    __syncthreads();
    if (tid < Tq) {
        float* pr = P + tid * Tk;
        float m = -__builtin_inff();
        for (int j = 0; j < Tk; ++j) m = __builtin_fmaxf(m, pr[j]);
        float l = 0.0f;
        for (int j = 0; j < Tk; ++j) { const float e = det_exp(pr[j] - m); pr[j] = e; l = l + e; }
        for (int j = 0; j < Tk; ++j) pr[j] = pr[j] / l;
    }
    __syncthreads();
    float* out = ctx + (size_t)b * qsb + (size_t)hd * dh * qsc;
    for (int e = tid; e < dh * Tq; e += 256) {
        const int d = e / Tq, i = e - d * Tq;
        float a = 0.0f;
        for (int j = 0; j < Tk; ++j) a = dfma(P[i * Tk + j], Vs[d * Tk + j], a);
        out[(size_t)d * qsc + i] = a;
    }
}

hipError_t launch_attention(const float* q, const float* k, const float* v, float* ctx,
                            int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                            hipStream_t s)
{
    if (B * H * Tq == 0) return hipSuccess;
    const size_t lds = ((size_t)dh * (Tq + 2 * Tk) + (size_t)Tq * Tk) * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_kernel<false>, dim3(B * H), dim3(256), lds, s, q, k, v, ctx, B, H, dh, Tq, Tk,
                       qsb, qsc, ksb, ksc, (const uint8_t*)nullptr, (size_t)0);
    return hipGetLastError();
}

// kmask != NULL, Tk > 0 (the entry point sends the other cases to launch_attention)
hipError_t launch_attention_masked(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                   int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                   size_t msb, hipStream_t s)
{
    if (B * H * Tq == 0) return hipSuccess;
    const size_t lds = ((size_t)dh * (Tq + 2 * Tk) + (size_t)Tq * Tk) * sizeof(float);
    if (lds > 64 * 1024 || Tk > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_kernel<true>, dim3(B * H), dim3(256), lds, s, q, k, v, ctx, B, H, dh, Tq, Tk,
                       qsb, qsc, ksb, ksc, kmask, msb);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// hold fill (mvq_hold_fill_f32): y[b,c,t] = x[b,c,s(b,t)], s(b,t) = the largest t' <= t with valid[b,t'] != 0, else carry[b,c]
// (+0 without carry); in place on x[B,C,T]; afterwards carry[b,c] = y[b,c,T-1].  Pure copies.
// One block per (item, slab of HOLD_CH channels); its four waves take HOLD_CH / 4 channels each and walk the time axis in tiles
// of 64 tokens, one lane per token.  Per tile a wave takes one ballot of valid[b, t0..t0+63]; lane t's source is the highest set
// bit at or below it, or the last valid token of the tiles before (a wave-uniform index), so s(b, .) costs one ballot per tile
// and every access runs along t.  Only tokens with valid == 0 are written, so a source column -- always a valid one -- is never
// written by anybody: the in-place update has no hazard.  carry[b,c] is touched by the one wave that owns channel c, which
// reads it before the single lane holding t = T-1 writes it.
// ------------------------------------------------------------------------------------------------
constexpr int HOLD_CH = 16;

// Where item b's carry row lies: the dense call's carry[b] (NULL carry: none), or row slots[b] of a pool of n_slots rows
// (mvq_hold_fill_slots_f32: the sessions of a group).  A slot outside [0, n_slots) has no row, as in the
// other slot kernels (stream.hip): +0 is read as the carry and none is stored.  ``open(b)`` is what a thread keeps of item b:
// has(carry) -- whether there is a row; at(b, C, c) -- the index of its channel c in the carry buffer.
struct HoldDense {
    struct Row {
        __device__ bool has(const float* carry) const { return carry != nullptr; }
        __device__ size_t at(int b, int C, int c) const { return (size_t)b * C + c; }
    };
    __device__ Row open(int) const { return Row{}; }
};
struct HoldSlots {
    const int32_t* slots;
    int n_slots;
    struct Row {
        int slot;
        bool ok;
        __device__ bool has(const float*) const { return ok; }
        __device__ size_t at(int, int C, int c) const { return (size_t)slot * C + c; }
    };
    __device__ Row open(int b) const
    {
        const int slot = slots[b];
        return Row{slot, slot >= 0 && slot < n_slots};
    }
};

// ONE body: ROWS is the addressing, SLOT_ARGS what it is built from -- none for the dense call, whose kernel so keeps its five
// arguments and its device code, or (slots, n_slots).
template <class ROWS, class... SLOT_ARGS>
__global__ __launch_bounds__(256) void hold_fill_kernel(float* __restrict__ x, const uint8_t* __restrict__ valid,
                                                        float* __restrict__ carry, int C, int T, SLOT_ARGS... slot_args)
{
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.y * HOLD_CH + wave * (HOLD_CH / 4);
    const uint8_t* vr = valid + (size_t)b * T;
    const auto cr = ROWS{slot_args...}.open(b);              // item b's carry row, or none
    int prev = -1;                                           // last valid token before this tile (wave-uniform)
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool ok = t < T && vr[t] != 0;
        const unsigned long long m = __ballot(ok);
        const unsigned long long below = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int src = below ? t0 + 63 - __clzll((long long)below) : prev;
        if (t < T) {
#pragma unroll
            for (int u = 0; u < HOLD_CH / 4; ++u) {
                const int c = c0 + u;
                if (c >= C) break;
                float* row = x + ((size_t)b * C + c) * T;
                const float val = src >= 0 ? row[src] : (cr.has(carry) ? carry[cr.at(b, C, c)] : 0.0f);
                if (!ok) row[t] = val;
                if (cr.has(carry) && t == T - 1) carry[cr.at(b, C, c)] = val;
            }
        }
        if (m) prev = t0 + 63 - __clzll((long long)m);
    }
}

hipError_t launch_hold_fill(float* x, const uint8_t* valid, float* carry, int B, int C, int T, hipStream_t s)
{
    if ((size_t)B * C * T == 0) return hipSuccess;
    hipLaunchKernelGGL(hold_fill_kernel<HoldDense>, dim3(B, (C + HOLD_CH - 1) / HOLD_CH), dim3(256), 0, s, x, valid, carry, C, T);
    return hipGetLastError();
}

// item g of x[G, C, T] / valid[G, T] on carry row slots[g] of carry_pool[n_slots, C]
hipError_t launch_hold_fill_slots(float* x, const uint8_t* valid, float* carry_pool, const int32_t* slots, int G, int n_slots, int C,
                                  int T, hipStream_t s)
{
    if ((size_t)G * C * T == 0) return hipSuccess;
    hipLaunchKernelGGL((hold_fill_kernel<HoldSlots, const int32_t*, int>), dim3(G, (C + HOLD_CH - 1) / HOLD_CH), dim3(256), 0, s, x, valid,
                       carry_pool, C, T, slots, n_slots);
    return hipGetLastError();
}

__global__ void gelu_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = det_gelu(x[i]);
}

hipError_t launch_gelu(const float* x, float* y, size_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, n);
    return hipGetLastError();
}

// y(b,c,t) = a(b,c,t) [- b2(b,c,t)] on [B,C,n] views with per-tensor (batch, channel) strides, time stride 1:
// slicing chunks out of [B,C,T] tensors and converting to/from the token-folded [C, B*n] layout of the AR loop.
__global__ void strided3d_kernel(const float* __restrict__ a, size_t asb, size_t asc,
                                 const float* __restrict__ b2, size_t bsb, size_t bsc,
                                 float* __restrict__ y, size_t ysb, size_t ysc, int B, int C, int n)
{
    const size_t total = (size_t)B * C * n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % n);
        const size_t bc = i / n;
        const int c = (int)(bc % C);
        const int b = (int)(bc / C);
        float v = a[(size_t)b * asb + (size_t)c * asc + t];
        if (b2) v = v - b2[(size_t)b * bsb + (size_t)c * bsc + t];
        y[(size_t)b * ysb + (size_t)c * ysc + t] = v;
    }
}

hipError_t launch_strided3d(const float* a, size_t asb, size_t asc, const float* b2, size_t bsb, size_t bsc,
                            float* y, size_t ysb, size_t ysc, int B, int C, int n, hipStream_t s)
{
    const size_t total = (size_t)B * C * n;
    if (total == 0) return hipSuccess;
    size_t blocks = (total + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(strided3d_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, asb, asc, b2, bsb, bsc, y, ysb, ysc, B, C, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// align_by_xcorr: one thread per integer shift walks its correlation chain (sample order, the contract); a second
// single-wave kernel takes the first maximum.  Replaces 401 separate torch reductions + host comparisons per file.
// ------------------------------------------------------------------------------------------------
__global__ void xcorr_kernel(const float* __restrict__ r, const float* __restrict__ e, int T, int max_shift,
                             float* __restrict__ corr, int* __restrict__ valid)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > 2 * max_shift) return;
    const int s = k - max_shift;
    const int n = T - (s < 0 ? -s : s);
    const float* rp = s < 0 ? r - s : r;
    const float* ep = s > 0 ? e + s : e;
    float c = 0.0f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { a[u] = rp[i + u]; b[u] = ep[i + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) c = dfma(a[u], b[u], c);
    }
    for (; i < n; ++i) c = dfma(rp[i], ep[i], c);
    corr[k] = n > 0 ? c : 0.0f;
    valid[k] = n > 0;
}

__global__ void xcorr_pick_kernel(const float* __restrict__ corr, const int* __restrict__ valid, int max_shift,
                                  int* __restrict__ best_shift)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int best_s = 0; float best = -1e18f;
    for (int k = 0; k <= 2 * max_shift; ++k)
        if (valid[k] && corr[k] > best) { best = corr[k]; best_s = k - max_shift; }
    *best_shift = best_s;
}

// batched form: grid.y = item (rows of pitch T); the per-shift chain is the same, so every item's result equals the
// single-item launch bit for bit
__global__ void xcorr_batch_kernel(const float* __restrict__ r, const float* __restrict__ e, int T, int max_shift,
                                   float* __restrict__ corr, int* __restrict__ valid)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > 2 * max_shift) return;
    const int b = blockIdx.y, n1 = 2 * max_shift + 1;
    const float* rb = r + (size_t)b * T;
    const float* eb = e + (size_t)b * T;
    const int s = k - max_shift;
    const int n = T - (s < 0 ? -s : s);
    const float* rp = s < 0 ? rb - s : rb;
    const float* ep = s > 0 ? eb + s : eb;
    float c = 0.0f;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float a[8], q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { a[u] = rp[i + u]; q[u] = ep[i + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) c = dfma(a[u], q[u], c);
    }
    for (; i < n; ++i) c = dfma(rp[i], ep[i], c);
    corr[(size_t)b * n1 + k] = n > 0 ? c : 0.0f;
    valid[(size_t)b * n1 + k] = n > 0;
}

__global__ void xcorr_pick_batch_kernel(const float* __restrict__ corr, const int* __restrict__ valid, int max_shift,
                                        int* __restrict__ best_shift, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n1 = 2 * max_shift + 1;
    int best_s = 0; float best = -1e18f;
    for (int k = 0; k < n1; ++k)
        if (valid[(size_t)b * n1 + k] && corr[(size_t)b * n1 + k] > best) { best = corr[(size_t)b * n1 + k]; best_s = k - max_shift; }
    best_shift[b] = best_s;
}

hipError_t launch_align_xcorr_batch(const float* r, const float* e, int B, int T, int max_shift, float* corr, int* scratch_valid,
                                    int* best_shift, hipStream_t s)
{
    const int n = 2 * max_shift + 1;
    hipLaunchKernelGGL(xcorr_batch_kernel, dim3((n + 63) / 64, B), dim3(64), 0, s, r, e, T, max_shift, corr, scratch_valid);
    hipLaunchKernelGGL(xcorr_pick_batch_kernel, dim3((B + 63) / 64), dim3(64), 0, s, corr, scratch_valid, max_shift, best_shift, B);
    return hipGetLastError();
}

hipError_t launch_align_xcorr(const float* r, const float* e, int T, int max_shift, float* corr, int* scratch_valid,
                              int* best_shift, hipStream_t s)
{
    const int n = 2 * max_shift + 1;
    hipLaunchKernelGGL(xcorr_kernel, dim3((n + 63) / 64), dim3(64), 0, s, r, e, T, max_shift, corr, scratch_valid);
    hipLaunchKernelGGL(xcorr_pick_kernel, dim3(1), dim3(64), 0, s, corr, scratch_valid, max_shift, best_shift);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// polyphase sinc resampler (torchaudio.transforms.Resample as the reference uses it, Training/compare_dacvsproposal_5.py:
// 110-113): y[b][n*newf + p] = sum_k kern[p][k] * xpad[b][n*orig + k], xpad = x zero-padded by `width` on the left.
// HBM-bound (L in, Lout out); the [newf][ks] filter bank sits in LDS when it fits.  One fma chain per output, k ascending.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, const float* __restrict__ kern,
                                                       float* __restrict__ y, int L, int Lout, int orig, int newf,
                                                       int width, int ks, int kern_in_lds)
{
    extern __shared__ __attribute__((aligned(16))) float ksm[];
    if (kern_in_lds) {
        for (int e = threadIdx.x; e < newf * ks; e += 256) ksm[e] = kern[e];
        __syncthreads();
    }
    const float* kt = kern_in_lds ? ksm : kern;
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= Lout) return;
    const int b = blockIdx.y;
    const int n = m / newf, p = m - n * newf;
    const float* xb = x + (size_t)b * L;
    const float* kp = kt + (size_t)p * ks;
    const int j0 = n * orig - width;
    int k_lo = j0 < 0 ? -j0 : 0;
    int k_hi = ks; if (j0 + k_hi > L) k_hi = L - j0;
    float acc = 0.0f;
    for (int k = k_lo; k < k_hi; ++k) acc = dfma(kp[k], xb[j0 + k], acc);
    y[(size_t)b * Lout + m] = acc;
}

// ragged form for the aligned-PSNR metric (Evaluation/compare_dacvsproposal_5_eval.py:212-223): item b resamples the slice
// x[b][off[b] : off[b] + len[b]] (off / len on the DEVICE: they come from the alignment shifts, no host round trip);
// y rows have pitch lout_pitch, entries past ceil(newf * len[b] / orig) are written as zeros; lout[b] receives that length.
__global__ __launch_bounds__(256) void resample_ragged_kernel(const float* __restrict__ x, const float* __restrict__ kern,
                                                              float* __restrict__ y, const int* __restrict__ off,
                                                              const int* __restrict__ len, int* __restrict__ lout,
                                                              int pitch, int lout_pitch, int orig, int newf, int width, int ks,
                                                              int kern_in_lds)
{
    extern __shared__ __attribute__((aligned(16))) float ksm[];
    if (kern_in_lds) {
        for (int e = threadIdx.x; e < newf * ks; e += 256) ksm[e] = kern[e];
        __syncthreads();
    }
    const float* kt = kern_in_lds ? ksm : kern;
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    // the slice is clamped to its row: a wrong offset / length on the device must not read outside x
    int o = off[b];
    o = o < 0 ? 0 : (o > pitch ? pitch : o);
    int L = len[b];
    L = L < 0 ? 0 : (L > pitch - o ? pitch - o : L);
    int Lo = (int)(((long long)newf * L + orig - 1) / orig);
    if (Lo > lout_pitch) Lo = lout_pitch;
    if (m == 0 && lout) lout[b] = Lo;
    if (m >= lout_pitch) return;
    float acc = 0.0f;
    if (m < Lo) {
        const int n = m / newf, p = m - n * newf;
        const float* xb = x + (size_t)b * pitch + o;
        const float* kp = kt + (size_t)p * ks;
        const int j0 = n * orig - width;
        int k_lo = j0 < 0 ? -j0 : 0;
        int k_hi = ks; if (j0 + k_hi > L) k_hi = L - j0;
        for (int k = k_lo; k < k_hi; ++k) acc = dfma(kp[k], xb[j0 + k], acc);
    }
    y[(size_t)b * lout_pitch + m] = acc;
}

hipError_t launch_resample_ragged(const float* x, const float* kern, float* y, const int* off, const int* len, int* lout, int B,
                                  int pitch, int lout_pitch, int orig, int newf, int width, int ks, hipStream_t s)
{
    if (B == 0 || lout_pitch == 0) return hipSuccess;
    const size_t kbytes = (size_t)newf * ks * sizeof(float);
    const int in_lds = kbytes <= 48 * 1024;
    hipLaunchKernelGGL(resample_ragged_kernel, dim3((lout_pitch + 255) / 256, B), dim3(256), in_lds ? kbytes : 0, s,
                       x, kern, y, off, len, lout, pitch, lout_pitch, orig, newf, width, ks, in_lds);
    return hipGetLastError();
}

hipError_t launch_resample(const float* x, const float* kern, float* y, int B, int L, int Lout, int orig, int newf,
                           int width, int ks, hipStream_t s)
{
    if (B == 0 || Lout == 0) return hipSuccess;
    const size_t lds = (size_t)newf * ks * sizeof(float);
    const int in_lds = lds <= 64 * 1024;
    hipLaunchKernelGGL(resample_kernel, dim3((Lout + 255) / 256, B), dim3(256), in_lds ? lds : 0, s, x, kern, y, L, Lout,
                       orig, newf, width, ks, in_lds);
    return hipGetLastError();
}

}  // namespace mvq
