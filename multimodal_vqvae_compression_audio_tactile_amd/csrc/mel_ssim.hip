// mel_ssim.hip -- the evaluation side of the packet-loss-concealment model (PLC/PLC1_eval.py:200-333,585-663 and
// PLC/PLC1_low_mid_high_eval.py:264-288): masked mel ST-SIM and the masked waveform statistics, without host round trips.
//
// Frame subsets (compute_stsim_mel_with_mask, steps 2-3 of DESIGN.md section 11): one block of 1024 threads.
//   spt = double(T_wave) / double(T_lat);  token(f) = clip(floor(double(f * hop) / spt), 0, T_lat - 1)   (numpy float64)
//   frame_mask[f] = latent_mask[token(f)];  cols_masked / cols_unmasked = the ascending frame indices of each side.
// Each thread owns a contiguous run of frames; an exclusive block scan of the per-thread counts gives every thread its write
// base, so the lists are in ascending order and the counts (written to counts[0..1]) never leave the device.
//
// Mel SSIM (_stsim_core, step 4): one block per image; an image is a column list into the [64, ld] mel plane pair (x columns
// from xc0, y columns from yc0), normalised on load by a true division M / max(maxv, 1e-8).  Mode SSIM (width >= 7): the
// defaults of skimage.metrics.structural_similarity -- 7x7 uniform window, filtered rows (axis 0) first, then columns, each
// pass a mean of 7 values summed fresh in ascending order (never a running sum), cov_norm = 49/48, C1 = 1e-4, C2 = 9e-4 --
// cropped by 3 on every side.  The crop only needs in-image neighbours, so the 'reflect' border never enters.  The image is
// walked in bands of 250 output columns: thread t owns input column band + t, keeps its last 7 rows in registers and writes
// the vertical means of 8 output rows at a time to LDS; threads t < 250 then form the horizontal means and S and add S to a
// float64 accumulator (rows ascending, bands ascending).  Mode NORM (or SSIM with width 1..6, the reference's fall-through):
// max(0, 1 - |A-B| / (|A| + |B| + 1e-12)), squares summed in float64.  Width 0 gives NaN.  The float64 partials meet in a
// fixed LDS tree, so a value depends only on its own image: bit-identical run to run and whatever else shares the launch.
//
// Subset statistics (masked_metrics + psnr_global_peak_db): one block of 1024 threads; sample n belongs to token
// floor(float(n) / float(spt)) (the float32 rule of token_to_sample_mask); per side the count, sum |r-e|, sum r^2 and
// sum (r-e)^2 (float32 terms, float64 sums over a fixed stride, then a fixed LDS tree).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels_small.hpp"

namespace mvq {

constexpr int FS_THREADS = 1024;
constexpr int SS_THREADS = 1024;
constexpr int SSIM_ROWS = 64, SSIM_PAD = 3, SSIM_WIN = 7;
constexpr int SSIM_THREADS = 256;
constexpr int SSIM_BAND = SSIM_THREADS - 2 * SSIM_PAD;   // output columns per band
constexpr int SSIM_G = 8;                                 // output rows per LDS chunk
constexpr int SSIM_OUT_ROWS = SSIM_ROWS - 2 * SSIM_PAD;   // 58

__device__ __forceinline__ bool frame_lost(const uint8_t* lat, int t_lat, double spt, int hop, int f)
{
    const double tk = floor((double)((long long)f * hop) / spt);
    long long ti = (long long)tk;
    ti = ti < 0 ? 0 : (ti > t_lat - 1 ? t_lat - 1 : ti);
    return lat[ti] != 0;
}

__global__ __launch_bounds__(FS_THREADS) void frame_subsets_kernel(const uint8_t* __restrict__ lat, int t_lat, double spt,
                                                                   int hop, int t_f, uint8_t* __restrict__ fmask,
                                                                   int* __restrict__ cols_m, int* __restrict__ cols_u,
                                                                   int* __restrict__ counts)
{
    __shared__ int scan[FS_THREADS];
    const int t = threadIdx.x;
    const bool any = t_lat > 0 && spt > 0.0;
    const int per = (t_f + FS_THREADS - 1) / FS_THREADS;
    const int f0 = min(t * per, t_f), f1 = min(f0 + per, t_f);
    int nm = 0;
    if (any)
        for (int f = f0; f < f1; ++f) nm += frame_lost(lat, t_lat, spt, hop, f) ? 1 : 0;
    scan[t] = nm;
    __syncthreads();
    for (int o = 1; o < FS_THREADS; o <<= 1) {                  // inclusive Hillis-Steele scan (integers: exact)
        const int v = t >= o ? scan[t - o] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    int bm = scan[t] - nm, bu = f0 - bm;
    for (int f = f0; f < f1; ++f) {
        const bool m = any && frame_lost(lat, t_lat, spt, hop, f);
        fmask[f] = m ? 1 : 0;
        if (!any) continue;
        if (m) cols_m[bm++] = f; else cols_u[bu++] = f;
    }
    if (t == FS_THREADS - 1) {
        counts[0] = any ? scan[t] : 0;
        counts[1] = any ? t_f - scan[t] : 0;
    }
}

template <int N>
__device__ __forceinline__ void block_sum_f64(double (&v)[N], double* red)
{
    // fixed tree over SSIM_THREADS lanes; thread 0 ends with the totals
    for (int q = 0; q < N; ++q) {
        red[threadIdx.x] = v[q];
        __syncthreads();
        for (int o = SSIM_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        v[q] = red[0];
        __syncthreads();
    }
}

// horizontal pass of ng chunk rows: S of output column (band start + t) for each, added to acc in row order
__device__ __forceinline__ double ssim_rows(const float (*V)[5][SSIM_THREADS], int ng, int t, double acc)
{
    const float cov = 49.0f / 48.0f, C1 = 0.0001f, C2 = 0.0009f;
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
        float u[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float s = V[g][q][t];
#pragma unroll
            for (int k = 1; k < SSIM_WIN; ++k) s += V[g][q][t + k];
            u[q] = s / 7.0f;
        }
        const float ux = u[0], uy = u[1], uxx = u[2], uyy = u[3], uxy = u[4];
        const float vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
        const float A1 = 2.0f * ux * uy + C1, A2 = 2.0f * vxy + C2;
        const float B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        acc += (double)((A1 * A2) / (B1 * B2));
    }
    return acc;
}

__global__ __launch_bounds__(SSIM_THREADS) void mel_ssim_kernel(const float* __restrict__ M, size_t ld, const float* __restrict__ maxv,
                                                                int n_maxv, const int* __restrict__ desc,
                                                                const int* __restrict__ cols, size_t n_cols,
                                                                const int* __restrict__ widths, int max_width, int mode,
                                                                double* __restrict__ out)
{
    __shared__ float V[SSIM_G][5][SSIM_THREADS];
    __shared__ double red[SSIM_THREADS];
    const int img = blockIdx.x, t = threadIdx.x;
    const int* d = desc + 5 * img;
    const long long ldl = (long long)ld;
    const long long xc0 = d[0], yc0 = d[1];
    const int ix = min(max(d[2], 0), n_maxv - 1), iy = min(max(d[3], 0), n_maxv - 1);
    const float denx = fmaxf(maxv[ix], 1e-8f), deny = fmaxf(maxv[iy], 1e-8f);
    const long long loff = d[4];
    const int W = min(max(widths[img], 0), max_width);
    if (W == 0) {
        if (t == 0) out[img] = __builtin_nan("");
        return;
    }
    // column j of the image -> plane column offsets (clamped into the plane: a bad list cannot read outside it)
    auto colx = [&](int j, long long& cx, long long& cy) {
        long long c = j;
        if (loff >= 0 && n_cols > 0) {
            long long li = loff + j;
            li = li < (long long)n_cols ? li : (long long)n_cols - 1;
            c = cols[li];
        }
        cx = xc0 + c; cy = yc0 + c;
        cx = cx < 0 ? 0 : (cx >= ldl ? ldl - 1 : cx);
        cy = cy < 0 ? 0 : (cy >= ldl ? ldl - 1 : cy);
    };
    if (mode == 1 && W >= SSIM_WIN) {
        double acc = 0.0;
        for (int c0 = 0; c0 < W - 2 * SSIM_PAD; c0 += SSIM_BAND) {
            const int nout = min(SSIM_BAND, W - 2 * SSIM_PAD - c0);
            const int j = c0 + t;
            const bool live = j < W;
            long long cx = 0, cy = 0;
            if (live) colx(j, cx, cy);
            const float* px = M + cx;
            const float* py = M + cy;
            float rx[SSIM_WIN], ry[SSIM_WIN];
#pragma unroll
            for (int m = 0; m < SSIM_ROWS; ++m) {
                rx[m % SSIM_WIN] = live ? px[(long long)m * ldl] / denx : 0.0f;
                ry[m % SSIM_WIN] = live ? py[(long long)m * ldl] / deny : 0.0f;
                if (m >= SSIM_WIN - 1) {
                    const int r = m - SSIM_PAD;                  // output row (3 .. 60)
                    float sx = 0.0f, sy = 0.0f, sxx = 0.0f, syy = 0.0f, sxy = 0.0f;
#pragma unroll
                    for (int k = 0; k < SSIM_WIN; ++k) {
                        const float x = rx[(m - (SSIM_WIN - 1) + k) % SSIM_WIN], y = ry[(m - (SSIM_WIN - 1) + k) % SSIM_WIN];
                        sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
                    }
                    const int g = (r - SSIM_PAD) % SSIM_G;
                    V[g][0][t] = sx / 7.0f; V[g][1][t] = sy / 7.0f;
                    V[g][2][t] = sxx / 7.0f; V[g][3][t] = syy / 7.0f; V[g][4][t] = sxy / 7.0f;
                    if (g == SSIM_G - 1 || r == SSIM_ROWS - 1 - SSIM_PAD) {
                        __syncthreads();
                        if (t < nout) acc = ssim_rows(V, g + 1, t, acc);
                        __syncthreads();
                    }
                }
            }
        }
        double v[1] = {acc};
        block_sum_f64<1>(v, red);
        if (t == 0) out[img] = v[0] / ((double)SSIM_OUT_ROWS * (double)(W - 2 * SSIM_PAD));
        return;
    }
    // NORM: max(0, 1 - |A-B| / (|A| + |B| + 1e-12)), Frobenius norms
    double v[3] = {0.0, 0.0, 0.0};
    for (int j = t; j < W; j += SSIM_THREADS) {
        long long cx, cy;
        colx(j, cx, cy);
        for (int m = 0; m < SSIM_ROWS; ++m) {
            const float a = M[cx + (long long)m * ldl] / denx, b = M[cy + (long long)m * ldl] / deny;
            const float df = a - b;
            v[0] += (double)(df * df); v[1] += (double)(a * a); v[2] += (double)(b * b);
        }
    }
    block_sum_f64<3>(v, red);
    if (t == 0) {
        const double s = 1.0 - sqrt(v[0]) / (sqrt(v[1]) + sqrt(v[2]) + 1e-12);
        out[img] = s > 0.0 ? s : 0.0;
    }
}

__global__ __launch_bounds__(SS_THREADS) void subset_stats_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                                  int T, const uint8_t* __restrict__ lat, int t_lat, float spt,
                                                                  double* __restrict__ out)
{
    __shared__ double red[SS_THREADS];
    const int t = threadIdx.x;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // per side (lost, kept): count, sum|d|, sum r^2, sum d^2
    for (int n = t; n < T; n += SS_THREADS) {
        int tok = (int)floorf((float)n / spt);
        tok = tok < 0 ? 0 : (tok > t_lat - 1 ? t_lat - 1 : tok);
        const float r = ref[n], e = est[n], df = r - e;
        const double c = 1.0, a = (double)fabsf(df), r2 = (double)(r * r), d2 = (double)(df * df);
        if (t_lat > 0 && lat[tok]) { v[0] += c; v[1] += a; v[2] += r2; v[3] += d2; }
        else          { v[4] += c; v[5] += a; v[6] += r2; v[7] += d2; }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        red[t] = v[q];
        __syncthreads();
        for (int o = SS_THREADS / 2; o > 0; o >>= 1) {
            if (t < o) red[t] += red[t + o];
            __syncthreads();
        }
        if (t == 0) out[q] = red[0];
        __syncthreads();
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
hipError_t launch_frame_subsets(const uint8_t* lat, int t_lat, double spt, int hop, int t_f, uint8_t* fmask, int* cols_m,
                                int* cols_u, int* counts, hipStream_t s)
{
    hipLaunchKernelGGL(frame_subsets_kernel, dim3(1), dim3(FS_THREADS), 0, s, lat, t_lat, spt, hop, t_f, fmask, cols_m, cols_u, counts);
    return hipGetLastError();
}

hipError_t launch_mel_ssim(const float* M, size_t ld, const float* maxv, int n_maxv, const int* desc, const int* cols, size_t n_cols,
                           const int* widths, int n, int max_width, int mode, double* out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mel_ssim_kernel, dim3(n), dim3(SSIM_THREADS), 0, s, M, ld, maxv, n_maxv, desc, cols, n_cols, widths,
                       max_width, mode, out);
    return hipGetLastError();
}

hipError_t launch_subset_stats(const float* ref, const float* est, int T, const uint8_t* lat, int t_lat, float spt, double* out,
                               hipStream_t s)
{
    hipLaunchKernelGGL(subset_stats_kernel, dim3(1), dim3(SS_THREADS), 0, s, ref, est, T, lat, t_lat, spt, out);
    return hipGetLastError();
}

}  // namespace mvq
