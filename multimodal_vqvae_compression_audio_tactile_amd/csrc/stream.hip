// stream.hip -- the state kernels of the streaming sessions (include/mvq.h): the receiver's mvq_stream_window_f32,
// mvq_stream_stage_window_f32 (the stateful decoder's per-stage window) and mvq_resample_stream_f32, the sender's mvq_stream_samples_f32
// and mvq_stream_stage_window_snake_f32 (the stateful encoder's raw + Snake window of a wide block).  Each keeps its session state in a fixed device buffer that
// the kernel itself updates in place, so the steady step of a session is the same launch sequence on the same addresses
// every time (a captured graph replays it).  A POOL of sessions keeps one row block per session slot in
// the same buffers and a launch works on the slots a device list names: the window and the resampler kernel are each ONE body,
// instantiated for the dense addressing and for the slot list (Sessions<SLOTS> below), the sample-state kernel likewise
// (SampleRows<SLOTS>: a pool's sender sessions also bring their own fill / n / drop, section 17), and stream_rows_kernel moves
// the carried tokens; audio_fade_kernel (the receiver's audio output, mvq_audio_fade_f32) is one body over Sessions<SLOTS> too, and so
// are the two kernels of the rational resampler's split form (mvq_resample_stream_rational_split_f32: outputs over many blocks per
// session, the state moved in a launch of its own).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "det_math.hpp"
#include "kernels_small.hpp"

namespace mvq {
namespace {
constexpr int WIN_ROWS = 32;          // (b, c) rows of one block of stream_window_kernel
constexpr int SMP_THREADS = 1024;     // stream_samples_kernel: one block per row
constexpr int SMP_PER = 4;            // elements a thread carries across the barrier: a tile is SMP_THREADS * SMP_PER samples
}  // namespace

// Which session of the state buffer a kernel's session g works on, fixed at compile time.  Dense (a lockstep session object):
// session g itself, always valid -- nothing is loaded and every guard folds away.  Slots (a group of a pool): slots[g], valid
// inside [0, n_slots); the host wrapper refuses a repeated slot, so two sessions of a launch never share state rows.
template <bool SLOTS> struct Sessions;
template <> struct Sessions<false> {
    __device__ bool session(int g, size_t& s) const { s = (size_t)g; return true; }
    __device__ bool row(size_t r, size_t& at) const { at = r; return true; }
};
template <> struct Sessions<true> {
    const int32_t* slots;
    int n_slots;
    int C;                                                               // rows per session (stream_window; rows <= INT_MAX)
    __device__ bool session(int g, size_t& s) const
    {
        const int slot = slots[g];
        s = (size_t)slot;
        return slot >= 0 && slot < n_slots;
    }
    __device__ bool row(size_t r, size_t& at) const                      // row g*C + c of the group -> row slots[g]*C + c of the pool
    {
        const int g = (int)r / C, c = (int)r - g * C;
        size_t s;
        const bool ok = session(g, s);
        at = s * C + c;
        return ok;
    }
};

// win[r][0 .. h_in + n) = [hist[r'][0 .. h_in) | z_new[r][0 .. n)], then hist[r'][0 .. h_out) = the last h_out columns of win[r].
// r = b*C + c; z_new and win are dense, r' = ses.row(r) is the session's row of hist (pitch `cap`): r itself, or the row of the
// slot.  A block owns WIN_ROWS consecutive rows r: phase 1 reads hist and z_new and writes win (a buffer of its own), the barrier
// ends every read of the block's hist rows, phase 2 rewrites those rows from the block's own part of win.  Distinct r are
// distinct r' (distinct slots), so no hist row is touched by two blocks and the in-place update has no cross-block hazard,
// wherever the rows lie in a pool.  A slot outside [0, n_slots) reads zeros and stores nothing.
template <bool SLOTS>
__global__ __launch_bounds__(256) void stream_window_kernel(float* __restrict__ hist, const float* __restrict__ z_new, float* win,
                                                            int h_in, int n, int h_out, int cap, size_t rows, Sessions<SLOTS> ses)
{
    const size_t row0 = (size_t)blockIdx.x * WIN_ROWS;
    const int nrow = (int)(rows - row0 < (size_t)WIN_ROWS ? rows - row0 : (size_t)WIN_ROWS);
    const int W = h_in + n;
    const int total = nrow * W;
    float* wb = win + row0 * (size_t)W;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int r = e / W, j = e - r * W;
        size_t at;
        const bool ok = ses.row(row0 + r, at);
        wb[e] = j < h_in ? (ok ? hist[at * (size_t)cap + j] : 0.0f) : z_new[(row0 + r) * (size_t)n + (j - h_in)];
    }
    __syncthreads();
    const int skip = W - h_out;
    const int total_h = nrow * h_out;
    for (int e = threadIdx.x; e < total_h; e += 256) {
        const int r = e / h_out, j = e - r * h_out;
        size_t at;
        if (ses.row(row0 + r, at)) hist[at * (size_t)cap + j] = wb[r * W + skip + j];
    }
}

// The window of one decoder STAGE of the stateful streaming decoder: stream_window_kernel with the new
// columns taken from a slice of a wider tensor, the crop of the producer's inexact edges folded into the window build.
//   win(g, c)[0 .. win_t) = [tail(g, c)[0 .. h_in) | src(g, c)[src_off .. src_off + n) | zeros],
//   then tail(g, c)[0 .. h_out) = win(g, c)[W - h_out .. W),   W = h_in + n <= win_t.
// Rows of src and win: with seg == 1 the dense row g*C + c of pitch src_t / win_t; with seg > 1 PACKED latent-rate rows
// (include/mvq.h): item g is segment g % seg of row (g / seg)*C + c, the segments src_t / win_t columns apart -- the layout
// mvq_conv1d_packed_rows_f32 reads and writes, so the head of the stack stays packed at throughput batches.  The zero tail of a
// window row (or segment) is the zero padding its consumer reads.  tail(g, c) = tail + session*tail_stride + c*cap: a stage's tail
// is a [C, cap] block at a fixed offset of the session's state row, session = g or slots[g].  Same ownership rule as
// stream_window_kernel: a block owns `rpb` consecutive (g, c), reads them completely, writes their part of win (a buffer of its
// own), and rewrites only its own tail rows after the barrier.  A slot outside [0, n_slots) reads zeros and stores nothing.
// V = float4 when every column count, pitch and offset is a multiple of 4 and every pointer 16-byte aligned (the launcher
// decides; all counts are then in units of V), else float.
struct StageRows {
    int pitch, seg;                                                      // columns of a row (or segment); segments per row
    __device__ size_t at(int g, int c, int C) const
    {
        return ((size_t)(g / seg) * C + c) * ((size_t)seg * pitch) + (size_t)(g % seg) * pitch;
    }
};
// SNAKE (the stateful streaming ENCODER's wide blocks): the launch also writes the window's Snake,
//   win_s(g, c)[j] = det_snake(win(g, c)[j], alpha[c], 1.0f / (alpha[c] + 1e-9f)) for j < W and +0 in the zero tail,
// the function and the reciprocal expression of the conv epilogues' dual output, so win_s is bit for bit what the producer would
// have written beside the raw activation; the tail stays raw.  win_s has win's layout.  SnakeOut<false> is empty: the instantiations
// without it carry no extra argument.
template <bool SNAKE, class V> struct SnakeOut;
template <class V> struct SnakeOut<false, V> {};
template <class V> struct SnakeOut<true, V> { V* win_s; const float* alpha; };
__device__ __forceinline__ float snake_of(float v, float al, float inv) { return det_snake(v, al, inv); }
__device__ __forceinline__ float4 snake_of(float4 v, float al, float inv)
{
    return make_float4(det_snake(v.x, al, inv), det_snake(v.y, al, inv), det_snake(v.z, al, inv), det_snake(v.w, al, inv));
}
template <bool SLOTS, class V, bool SNAKE = false>
__global__ __launch_bounds__(256) void stream_stage_window_kernel(V* tail, const V* __restrict__ src, V* win, int h_in, int n, int h_out,
                                                                  int cap, size_t tail_stride, StageRows sr, int src_off, StageRows wr,
                                                                  int C, int rpb, size_t rows, Sessions<SLOTS> ses, SnakeOut<SNAKE, V> so = {})
{
    const size_t row0 = (size_t)blockIdx.x * rpb;
    const int nrow = (int)(rows - row0 < (size_t)rpb ? rows - row0 : (size_t)rpb);
    const int W = h_in + n, win_t = wr.pitch;
    const int total = nrow * win_t;
    const V zero{};
    for (int e = threadIdx.x; e < total; e += 256) {
        const int r = e / win_t, j = e - r * win_t;
        const int g = (int)((row0 + r) / C), c = (int)((row0 + r) - (size_t)g * C);
        V v = zero;
        if (j < h_in) {
            size_t s;
            if (ses.session(g, s)) v = tail[s * tail_stride + (size_t)c * cap + j];
        } else if (j < W) {
            v = src[sr.at(g, c, C) + src_off + (j - h_in)];
        }
        win[wr.at(g, c, C) + j] = v;
        if constexpr (SNAKE) {
            const float al = so.alpha[c];
            so.win_s[wr.at(g, c, C) + j] = j < W ? snake_of(v, al, 1.0f / (al + 1e-9f)) : zero;
        }
    }
    __syncthreads();
    const int skip = W - h_out;
    const int total_h = nrow * h_out;
    for (int e = threadIdx.x; e < total_h; e += 256) {
        const int r = e / h_out, j = e - r * h_out;
        const int g = (int)((row0 + r) / C), c = (int)((row0 + r) - (size_t)g * C);
        size_t s;
        if (ses.session(g, s)) tail[s * tail_stride + (size_t)c * cap + j] = win[wr.at(g, c, C) + skip + j];
    }
}

// Stateful decimation (newf == 1).  state[s][0 .. S), S = hold*orig + width with hold = ceil(width / orig), holds the last S
// samples of (zeros | x received so far) of session s = ses.session(b): b itself, or slots[b]; x_new and y are dense [B, .].
// With v = [state | x_new] (S + n_new samples), output m of this call reads v[base + m*orig + k], k < ks = 2*width + orig;
// `lead` leading samples of v are left padding and `S + n_new` is where the right padding begins: taps outside [lead, S + n_new)
// are skipped, exactly the taps resample_kernel skips, so the fma chain (k ascending) of an output is the one the whole-signal
// kernel runs.  base / lead / n_out are one launch's: a group of a pool shares a launch class (every member has consumed == 0,
// or every member has consumed >= S).  One block per item: outputs first, then the barrier, then the state moves up by n_new
// samples (each thread carries its elements in registers across a second barrier: a shift by less than S overlaps itself).
// A slot outside [0, n_slots) reads a zero state and stores none.
template <bool SLOTS>
__global__ __launch_bounds__(256) void resample_stream_kernel(const float* __restrict__ x_new, const float* __restrict__ kern,
                                                              float* __restrict__ state, float* __restrict__ y, int n_new, int n_out,
                                                              int orig, int ks, int S, int base, int lead, int kern_in_lds,
                                                              Sessions<SLOTS> ses)
{
    extern __shared__ __attribute__((aligned(16))) float ksm[];
    if (kern_in_lds) {
        for (int e = threadIdx.x; e < ks; e += 256) ksm[e] = kern[e];
        __syncthreads();
    }
    const float* kp = kern_in_lds ? ksm : kern;
    const int b = blockIdx.x;
    size_t at;
    const bool ok = ses.session(b, at);
    float* st = state + (ok ? at : 0) * S;
    const float* xb = x_new + (size_t)b * n_new;
    const int V = S + n_new;
    for (int m = threadIdx.x; m < n_out; m += 256) {
        const int j0 = base + m * orig;
        const int k_lo = j0 < lead ? lead - j0 : 0;
        int k_hi = ks; if (j0 + k_hi > V) k_hi = V - j0;
        float acc = 0.0f;
        for (int k = k_lo; k < k_hi; ++k) {
            const int j = j0 + k;
            acc = dfma(kp[k], j < S ? (ok ? st[j] : 0.0f) : xb[j - S], acc);
        }
        y[(size_t)b * n_out + m] = acc;
    }
    if (!ok) return;                                                     // block-uniform: the whole block leaves before the barriers
    __syncthreads();
    float keep[4];                                                       // S <= 1024 (checked by the entry point)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u;
        const int j = i + n_new;
        keep[u] = i < S ? (j < S ? st[j] : xb[j - S]) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u;
        if (i < S) st[i] = keep[u];
    }
}

// Stateful resampling by any rational ratio orig : newf: resample_stream_kernel with the polyphase bank of
// resample_kernel and a lag the caller chooses.  state[s][0 .. S), S = hold*orig + width, holds the last S samples of
// (zeros | x received so far) of session s, hold >= ceil(width / orig) the lag in filter blocks (a block: orig inputs, newf outputs).
// With v = [state | x_new], output m of this call is phase p = m - q*newf of block q = m / newf and reads v[base + q*orig + k]
// against bank row p, kern[p*ks + k], k < ks; taps outside [lead, S + n_new) are skipped, exactly the taps resample_kernel skips,
// and the chain is one dfma per tap, k ascending: an output's arithmetic is the whole-signal kernel's bit for bit.  n_out counts
// outputs, not blocks: the final call's last block may be partial in its inputs (right padding) and in its outputs.  base / lead /
// n_out are one launch's (a pool group shares a launch class, as above); both are 0 once consumed >= S.  The bank sits in LDS
// when the launcher says so, rows `kp` floats apart: an odd pitch, so that the 64 lanes of a wave, which walk the phases, hit
// distinct banks (ks = 94 of 24 kHz -> 44.1 kHz would pair them up).  One block per session, the state moved as above (keep[4]).
// A slot outside [0, n_slots) reads a zero state and stores none.
template <bool SLOTS>
__global__ __launch_bounds__(256) void resample_stream_rational_kernel(const float* __restrict__ x_new, const float* __restrict__ kern,
                                                                       float* __restrict__ state, float* __restrict__ y, int n_new,
                                                                       int n_out, int orig, int newf, int ks, int kp, int S, int base,
                                                                       int lead, int kern_in_lds, Sessions<SLOTS> ses)
{
    extern __shared__ __attribute__((aligned(16))) float ksm[];
    if (kern_in_lds) {
        for (int e = threadIdx.x; e < newf * ks; e += 256) {
            const int p = e / ks;
            ksm[p * kp + (e - p * ks)] = kern[e];
        }
        __syncthreads();
    }
    const float* kt = kern_in_lds ? ksm : kern;
    const int b = blockIdx.x;
    size_t at;
    const bool ok = ses.session(b, at);
    float* st = state + (ok ? at : 0) * S;
    const float* xb = x_new + (size_t)b * n_new;
    const int V = S + n_new;
    for (int m = threadIdx.x; m < n_out; m += 256) {
        const int q = m / newf, p = m - q * newf;
        const float* kr = kt + (size_t)p * kp;
        const int j0 = base + q * orig;
        const int k_lo = j0 < lead ? lead - j0 : 0;
        int k_hi = ks; if (j0 + k_hi > V) k_hi = V - j0;
        float acc = 0.0f;
        for (int k = k_lo; k < k_hi; ++k) {
            const int j = j0 + k;
            acc = dfma(kr[k], j < S ? (ok ? st[j] : 0.0f) : xb[j - S], acc);
        }
        y[(size_t)b * n_out + m] = acc;
    }
    if (!ok) return;                                                     // block-uniform: the whole block leaves before the barriers
    __syncthreads();
    float keep[4];                                                       // S <= 1024 (checked by the entry point)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u;
        const int j = i + n_new;
        keep[u] = i < S ? (j < S ? st[j] : xb[j - S]) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u;
        if (i < S) st[i] = keep[u];
    }
}

// The SPLIT form of resample_stream_rational_kernel: the same outputs and the same state in two launches, so
// that one session's outputs are spread over many blocks instead of walked by one.
// Outputs launch, grid (parts, sessions): part = qg*n_pg + pg owns the phases [pg*pp, pg*pp + pp) of the filter blocks
// [qg*qq, qg*qq + qq) of the call -- a rectangle of the (q, p) plane, so it needs only its own pp rows of the bank (in LDS at the
// odd pitch `kp` when the launcher says so, else read from memory at pitch ks).  It reads v = [state | x_new] and never writes the
// state; output m = q*newf + p is the one-block kernel's expression token for token (j0, the skipped taps, one dfma per tap, k
// ascending, from +0), so which block computes it changes nothing.  Lanes walk the part's phases first: distinct bank rows, one
// shared v window.  Sessions beyond the grid's y limit are walked by the same blocks.  A slot outside [0, n_slots) reads a zero state.
template <bool SLOTS>
__global__ __launch_bounds__(256) void resample_stream_rational_outputs_kernel(const float* __restrict__ x_new, const float* __restrict__ kern,
                                                                               const float* __restrict__ state, float* __restrict__ y, int B,
                                                                               int n_new, int n_out, int orig, int newf, int ks, int kp, int S,
                                                                               int base, int lead, int kern_in_lds, int pp, int qq, int n_pg,
                                                                               Sessions<SLOTS> ses)
{
    extern __shared__ __attribute__((aligned(16))) float ksm[];
    const int qg = blockIdx.x / n_pg, pg = blockIdx.x - qg * n_pg;
    const int p0 = pg * pp, q0 = qg * qq;
    const int np = newf - p0 < pp ? newf - p0 : pp;                      // phases of this part (the last group may be short)
    const float* kg = kern + (size_t)p0 * ks;                            // the part's rows of the bank
    if (kern_in_lds) {
        for (int e = threadIdx.x; e < np * ks; e += 256) {
            const int r = e / ks;
            ksm[r * kp + (e - r * ks)] = kg[e];
        }
        __syncthreads();
    }
    const float* kt = kern_in_lds ? ksm : kg;
    const int V = S + n_new;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        size_t at;
        const bool ok = ses.session(b, at);
        const float* st = state + (ok ? at : 0) * S;
        const float* xb = x_new + (size_t)b * n_new;
        for (int e = threadIdx.x; e < np * qq; e += 256) {
            const int ql = e / np, pl = e - ql * np;
            const int q = q0 + ql;
            const long long m = (long long)q * newf + (p0 + pl);
            if (m >= n_out) continue;                                    // the call's last filter block may be partial in its outputs
            const float* kr = kt + (size_t)pl * kp;
            const int j0 = base + q * orig;
            const int k_lo = j0 < lead ? lead - j0 : 0;
            int k_hi = ks; if (j0 + k_hi > V) k_hi = V - j0;
            float acc = 0.0f;
            for (int k = k_lo; k < k_hi; ++k) {
                const int j = j0 + k;
                acc = dfma(kr[k], j < S ? (ok ? st[j] : 0.0f) : xb[j - S], acc);
            }
            y[(size_t)b * n_out + (size_t)m] = acc;
        }
    }
}

// State launch of the split form, behind the outputs launch on the same stream (no block of that launch is still reading): one
// block per session moves its state up by n_new samples, st[i] = v[i + n_new], the one-block kernels' register-carried move.  The
// shift overlaps itself, so every thread holds its elements across the barrier; the barrier in front of the loads, which in the
// one-block kernels ends the reads of the outputs, has nothing to wait for here.  A slot outside [0, n_slots) stores nothing.
template <bool SLOTS>
__global__ __launch_bounds__(256) void resample_stream_state_kernel(const float* __restrict__ x_new, float* __restrict__ state, int n_new, int S,
                                                                    Sessions<SLOTS> ses)
{
    const int b = blockIdx.x;
    size_t at;
    if (!ses.session(b, at)) return;                                     // block-uniform: the whole block leaves before the barrier
    float* st = state + at * S;
    const float* xb = x_new + (size_t)b * n_new;
    float keep[4];                                                       // S <= 1024 (checked by the entry point)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u;
        const int j = i + n_new;
        keep[u] = i < S ? (j < S ? st[j] : xb[j - S]) : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = threadIdx.x + 256 * u;
        if (i < S) st[i] = keep[u];
    }
}

// Which row of the sender's sample state block `blk` of stream_samples_kernel works on and with which parameters, fixed at
// compile time.  Dense (a lockstep StreamSender): row blk of buf[rows, cap], x_new[rows, n] and win[rows, w], with the ONE
// (fill, n, drop) of the launch -- nothing is loaded and the check folds away (the entry point has made it).  Slots (a group of G
// sessions of a pool): block m*G + g is modality m of session g, whose descriptor desc[g] = (slot, fill,
// n, drop, x_off) names ITS parameters: row 2*slot + m of buf[n_slots, 2, cap], its n new samples at x_new[x_off + m*n], row
// m*G + g of win[2, G, w].  The kernel checks a descriptor itself as a second line behind the host wrapper: the slot inside
// [0, n_slots), every value what mvq_stream_samples_f32 accepts, the samples inside x_new[0 .. x_total).  All threads of a block
// read the same five words, so the verdict is block-uniform.
struct SampleRow {
    size_t buf_row;                                                      // row of buf
    size_t x_at;                                                         // offset of the row's new samples in x_new
    int fill, n, drop;
};
template <bool SLOTS> struct SampleRows;
template <> struct SampleRows<false> {
    int fill, n, drop;
    __device__ bool row(int blk, int, int, SampleRow& r) const
    {
        r.buf_row = (size_t)blk;
        r.x_at = (size_t)blk * n;
        r.fill = fill, r.n = n, r.drop = drop;
        return true;
    }
};
template <> struct SampleRows<true> {
    const int32_t* desc;                                                 // [G][5]
    int G, n_slots, x_total;
    __device__ bool row(int blk, int w, int cap, SampleRow& r) const
    {
        const int m = blk / G, g = blk - m * G;
        const int32_t* d = desc + (size_t)g * 5;
        const int slot = d[0], fill = d[1], n = d[2], drop = d[3], x_off = d[4];
        r.buf_row = (size_t)(slot < 0 ? 0 : slot) * 2 + m;
        r.x_at = (size_t)(x_off < 0 ? 0 : x_off) + (size_t)m * (n < 0 ? 0 : n);
        r.fill = fill, r.n = n, r.drop = drop;
        const long long have = (long long)fill + n;
        return slot >= 0 && slot < n_slots && fill >= 0 && n >= 0 && drop >= 0 && x_off >= 0 && n <= (1 << 24) && fill <= cap &&
               drop <= have && have - drop <= cap && w <= have && (long long)x_off + 2LL * n <= x_total;
    }
};

// The sender's sample state.  Per row (one block each; rows.row() says which and with what fill, n and drop): v = [buf[0 .. fill)
// | x_new[0 .. n)], win[0 .. w) = v[0 .. w) (a buffer of its own, pitch w), then buf[0 .. fill + n - drop) = v[drop ..): the
// samples the next window still needs move to the front of the row, the new ones behind them.  The move overlaps itself
// (drop < fill + n), so it goes tile by tile in ascending order: a tile's sources lie at or past its own start, every thread holds
// its elements in registers across the barrier, and only then are they stored -- a store of tile k lands below (k+1)*TILE, where
// no later tile reads.  With drop == 0 the old samples stay where they are and only x_new is appended.  No row is touched by two
// blocks (distinct slots are distinct rows), and the trip counts are one row's, so block-uniform, whatever the other blocks of
// the launch hold.  A block whose descriptor fails the check writes zeros to its window row and leaves, before any barrier.
template <bool SLOTS>
__global__ __launch_bounds__(SMP_THREADS) void stream_samples_kernel(float* buf, const float* __restrict__ x_new,
                                                                     float* __restrict__ win, int w, int cap, SampleRows<SLOTS> rows)
{
    float* wr = win + (size_t)blockIdx.x * w;
    SampleRow r;
    if (!rows.row(blockIdx.x, w, cap, r)) {
        for (int i = threadIdx.x; i < w; i += SMP_THREADS) wr[i] = 0.0f;
        return;
    }
    const int fill = r.fill, n = r.n, drop = r.drop;
    float* b = buf + r.buf_row * (size_t)cap;
    const float* x = x_new + r.x_at;
    for (int i = threadIdx.x; i < w; i += SMP_THREADS) wr[i] = i < fill ? b[i] : x[i - fill];
    __syncthreads();                                                     // every read of the window is done before the row moves
    const int keep = fill + n - drop;
    constexpr int TILE = SMP_THREADS * SMP_PER;
    for (int t0 = drop ? 0 : fill; t0 < keep; t0 += TILE) {
        float v[SMP_PER];
#pragma unroll
        for (int u = 0; u < SMP_PER; ++u) {
            const int i = t0 + threadIdx.x + SMP_THREADS * u;
            const int j = i + drop;
            v[u] = i < keep ? (j < fill ? b[j] : x[j - fill]) : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SMP_PER; ++u) {
            const int i = t0 + threadIdx.x + SMP_THREADS * u;
            if (i < keep) b[i] = v[u];
        }
    }
}

// ---- the receiver's audio output: lost tokens fade out and back in ---------------------------------------------
// packets.AudioFade is the definition.  r = the saturated run length of lost tokens ending at a token (0 at an arrived one, at
// most cap = H + F), g = 1 for r <= H, else (cap - r) / F; sample j of token t is scaled by g[t-1] + (g[t] - g[t-1]) * ((j+1)/320),
// every operation rounded on its own, and is +0 where that gain is 0, whatever it held.
// A launch works on the piece y[g][0 .. len) of every session g, which starts `back` tokens in front of the step's n new tokens
// valid[g][0 .. n): piece token p is the step's token q = p - back.  state[session][0 .. AF_STATE) holds r of the AF_STATE tokens in
// front of the new ones, the newest last, so q in [-AF_STATE, 0) is state[AF_STATE + q] and the piece's first sample finds g[t-1]
// there (back <= AF_HALO).  `fresh` (nothing came before the step): the row is not read, every r in front is 0.
// Ownership: ONE block per session.  Its first AF_STATE threads copy the state row to LDS (clamped to [0, cap], so a row that was
// never written cannot index past anything); the barrier ends every read of the row; only then the same threads store r of the
// last AF_STATE tokens of [row | new] to it, from the LDS copy and valid alone.  Distinct sessions are distinct rows (the wrapper
// refuses a repeated slot) and a session's samples are its block's, so neither the row nor y is touched by two blocks.  A slot
// outside [0, n_slots) reads "no loss so far" and stores no row.  The run of a new token is found by walking back over valid, at
// most cap <= 255 bytes; the gains of AF_TILE tokens at a time go through LDS.
namespace {
constexpr int AF_HOP = 320;           // samples per token
constexpr int AF_HALO = 10;           // stream.DEC_HALO_TOK: a step emits samples this many tokens behind the newest one
constexpr int AF_STATE = AF_HALO + 1; // ... and a sample needs g[t-1] too
constexpr int AF_TILE = 64;           // tokens whose gains one pass keeps in LDS
}  // namespace

__device__ __forceinline__ int fade_run(const uint8_t* __restrict__ valid, const int* st, int q, int cap)
{
    if (q < 0) return st[AF_STATE + q];
    for (int d = 0; d < cap; ++d) {
        if (q - d < 0) {                                                // the d new tokens up to q are lost: the run in front goes on
            const int r = st[AF_STATE - 1] + d;
            return r < cap ? r : cap;
        }
        if (valid[q - d]) return d;
    }
    return cap;
}

template <bool SLOTS>
__global__ __launch_bounds__(256) void audio_fade_kernel(float* y, const uint8_t* __restrict__ valid, int32_t* state, int len, int n,
                                                         int back, int fresh, int H, int F, Sessions<SLOTS> ses)
{
    __shared__ int st[AF_STATE];
    __shared__ float gs[AF_TILE + 1];
    const int g = blockIdx.x, tid = threadIdx.x, cap = H + F;
    size_t s;
    const bool ok = ses.session(g, s);
    int32_t* row = state + (ok ? s : 0) * AF_STATE;
    if (tid < AF_STATE) {
        const int v = ok && !fresh ? row[tid] : 0;
        st[tid] = v < 0 ? 0 : (v > cap ? cap : v);
    }
    __syncthreads();                                                     // every read of the state row is done
    const uint8_t* vb = valid + (size_t)g * n;
    if (ok && tid < AF_STATE) row[tid] = fade_run(vb, st, n - AF_STATE + tid, cap);
    float* yb = y + (size_t)g * len;
    const int np = (len + AF_HOP - 1) / AF_HOP;                          // piece tokens with a sample (the last one lacks 8)
    for (int p0 = 0; p0 < np; p0 += AF_TILE) {
        const int cnt = np - p0 < AF_TILE ? np - p0 : AF_TILE;
        if (tid <= cnt) {                                                // gs[i] = g of piece token p0 + i - 1
            const int r = fade_run(vb, st, p0 + tid - 1 - back, cap);
            gs[tid] = r <= H ? 1.0f : (float)(cap - r) / (float)F;
        }
        __syncthreads();
        const int s_hi = (p0 + cnt) * AF_HOP < len ? (p0 + cnt) * AF_HOP : len;
        for (int i = p0 * AF_HOP + tid; i < s_hi; i += 256) {
            const int p = i / AF_HOP, j = i - p * AF_HOP;
            const float g0 = gs[p - p0], g1 = gs[p - p0 + 1];
            const float w = (float)(j + 1) / (float)AF_HOP;
            const float gain = g0 + (g1 - g0) * w;                       // three roundings: the library is built with -ffp-contract=off
            yb[i] = gain == 0.0f ? 0.0f : yb[i] * gain;
        }
        __syncthreads();                                                 // before the next pass rewrites gs
    }
}

// slots == nullptr: the dense instantiation; else the group slots[G] of a pool of n_slots sessions.  The entry points have checked
// every size (np - back <= n, back <= AF_HALO).
hipError_t launch_audio_fade(float* y, const uint8_t* valid, int32_t* state, const int32_t* slots, int G, int n_slots, int len, int n,
                             int back, int fresh, int H, int F, hipStream_t s)
{
    if (G == 0) return hipSuccess;
    if (slots)
        hipLaunchKernelGGL(audio_fade_kernel<true>, dim3(G), dim3(256), 0, s, y, valid, state, len, n, back, fresh, H, F,
                           Sessions<true>{slots, n_slots, 1});
    else
        hipLaunchKernelGGL(audio_fade_kernel<false>, dim3(G), dim3(256), 0, s, y, valid, state, len, n, back, fresh, H, F,
                           Sessions<false>{});
    return hipGetLastError();
}

// ---- the session pool: the carried tokens ----------------------------------------------------------------------------------------
// rows[g][0 .. C) <- pool[slots[g]][0 .. C) (scatter == 0) or the other way (scatter != 0): the carried token of a group, so that
// decode_latents works on a dense [G, C] copy.  One element per thread; a slot outside [0, n_slots) gathers zeros and scatters
// nothing.  (At 256 sessions x 1024 channels this moves 1 MB: the launch, not the traffic, is its cost.)
__global__ __launch_bounds__(256) void stream_rows_kernel(float* __restrict__ pool, const int32_t* __restrict__ slots,
                                                          float* __restrict__ rows, int C, int n_slots, int total, int scatter)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int g = e / C, c = e - g * C;
    const int slot = slots[g];
    const bool ok = slot >= 0 && slot < n_slots;
    if (scatter) {
        if (ok) pool[(size_t)slot * C + c] = rows[e];
    } else {
        rows[e] = ok ? pool[(size_t)slot * C + c] : 0.0f;
    }
}

// slots == nullptr: the dense instantiation; else the group slots[rows / C] (slots[B]) of a pool of n_slots sessions.
hipError_t launch_stream_window(float* hist, const int32_t* slots, const float* z_new, float* win, int h_in, int n, int h_out, int cap,
                                int C, int n_slots, size_t rows, hipStream_t s)
{
    if (rows == 0 || h_in + n == 0) return hipSuccess;
    const dim3 grid((unsigned)((rows + WIN_ROWS - 1) / WIN_ROWS)), block(256);
    if (slots)
        hipLaunchKernelGGL(stream_window_kernel<true>, grid, block, 0, s, hist, z_new, win, h_in, n, h_out, cap, rows,
                           Sessions<true>{slots, n_slots, C});
    else
        hipLaunchKernelGGL(stream_window_kernel<false>, grid, block, 0, s, hist, z_new, win, h_in, n, h_out, cap, rows,
                           Sessions<false>{});
    return hipGetLastError();
}

// slots == nullptr: the dense instantiation; else the group slots[rows / C] of a pool of n_slots sessions.  The entry points have
// checked every size; src_seg / win_seg: 1 = dense rows, else packed rows of that many segments.
hipError_t launch_stream_stage_window(float* tail, size_t tail_stride, const int32_t* slots, const float* src, int src_t, int src_seg,
                                      int src_off, float* win, int win_t, int win_seg, int h_in, int n, int h_out, int cap, int C,
                                      int n_slots, size_t rows, hipStream_t s)
{
    if (rows == 0 || h_in + n == 0) return hipSuccess;
    int rpb = 2048 / win_t;                                             // about 2048 window elements per block
    rpb = rpb < 1 ? 1 : (rpb > WIN_ROWS ? WIN_ROWS : rpb);
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb)), block(256);
    const bool vec = !((h_in | n | h_out | cap | src_t | src_off | win_t) & 3) && !(tail_stride & 3) &&
                     !(((uintptr_t)tail | (uintptr_t)src | (uintptr_t)win) & 15);
    if (vec) {
        float4* t4 = reinterpret_cast<float4*>(tail);
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* w4 = reinterpret_cast<float4*>(win);
        const StageRows sr{src_t / 4, src_seg}, wr{win_t / 4, win_seg};
        if (slots)
            hipLaunchKernelGGL((stream_stage_window_kernel<true, float4>), grid, block, 0, s, t4, s4, w4, h_in / 4, n / 4, h_out / 4, cap / 4,
                               tail_stride / 4, sr, src_off / 4, wr, C, rpb, rows, Sessions<true>{slots, n_slots, C});
        else
            hipLaunchKernelGGL((stream_stage_window_kernel<false, float4>), grid, block, 0, s, t4, s4, w4, h_in / 4, n / 4, h_out / 4, cap / 4,
                               tail_stride / 4, sr, src_off / 4, wr, C, rpb, rows, Sessions<false>{});
    } else {
        const StageRows sr{src_t, src_seg}, wr{win_t, win_seg};
        if (slots)
            hipLaunchKernelGGL((stream_stage_window_kernel<true, float>), grid, block, 0, s, tail, src, win, h_in, n, h_out, cap, tail_stride,
                               sr, src_off, wr, C, rpb, rows, Sessions<true>{slots, n_slots, C});
        else
            hipLaunchKernelGGL((stream_stage_window_kernel<false, float>), grid, block, 0, s, tail, src, win, h_in, n, h_out, cap, tail_stride,
                               sr, src_off, wr, C, rpb, rows, Sessions<false>{});
    }
    return hipGetLastError();
}

// launch_stream_stage_window on dense rows with the Snake copy win_s (layout of win) beside win: the SNAKE instantiations
hipError_t launch_stream_stage_window_snake(float* tail, size_t tail_stride, const int32_t* slots, const float* src, int src_t, int src_off,
                                            float* win, float* win_s, const float* alpha, int win_t, int h_in, int n, int h_out, int cap,
                                            int C, int n_slots, size_t rows, hipStream_t s)
{
    if (rows == 0 || h_in + n == 0) return hipSuccess;
    int rpb = 2048 / win_t;
    rpb = rpb < 1 ? 1 : (rpb > WIN_ROWS ? WIN_ROWS : rpb);
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb)), block(256);
    const bool vec = !((h_in | n | h_out | cap | src_t | src_off | win_t) & 3) && !(tail_stride & 3) &&
                     !(((uintptr_t)tail | (uintptr_t)src | (uintptr_t)win | (uintptr_t)win_s) & 15);
    if (vec) {
        float4* t4 = reinterpret_cast<float4*>(tail);
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* w4 = reinterpret_cast<float4*>(win);
        const SnakeOut<true, float4> so{reinterpret_cast<float4*>(win_s), alpha};
        const StageRows sr{src_t / 4, 1}, wr{win_t / 4, 1};
        if (slots)
            hipLaunchKernelGGL((stream_stage_window_kernel<true, float4, true>), grid, block, 0, s, t4, s4, w4, h_in / 4, n / 4, h_out / 4,
                               cap / 4, tail_stride / 4, sr, src_off / 4, wr, C, rpb, rows, Sessions<true>{slots, n_slots, C}, so);
        else
            hipLaunchKernelGGL((stream_stage_window_kernel<false, float4, true>), grid, block, 0, s, t4, s4, w4, h_in / 4, n / 4, h_out / 4,
                               cap / 4, tail_stride / 4, sr, src_off / 4, wr, C, rpb, rows, Sessions<false>{}, so);
    } else {
        const SnakeOut<true, float> so{win_s, alpha};
        const StageRows sr{src_t, 1}, wr{win_t, 1};
        if (slots)
            hipLaunchKernelGGL((stream_stage_window_kernel<true, float, true>), grid, block, 0, s, tail, src, win, h_in, n, h_out, cap,
                               tail_stride, sr, src_off, wr, C, rpb, rows, Sessions<true>{slots, n_slots, C}, so);
        else
            hipLaunchKernelGGL((stream_stage_window_kernel<false, float, true>), grid, block, 0, s, tail, src, win, h_in, n, h_out, cap,
                               tail_stride, sr, src_off, wr, C, rpb, rows, Sessions<false>{}, so);
    }
    return hipGetLastError();
}

hipError_t launch_resample_stream(const float* x_new, const float* kern, float* state, const int32_t* slots, float* y, int B, int n_new,
                                  int n_out, int orig, int ks, int S, int base, int lead, int n_slots, hipStream_t s)
{
    if (B == 0) return hipSuccess;
    const size_t lds = (size_t)ks * sizeof(float);
    const int in_lds = lds <= 48 * 1024;
    if (slots)
        hipLaunchKernelGGL(resample_stream_kernel<true>, dim3(B), dim3(256), in_lds ? lds : 0, s, x_new, kern, state, y, n_new, n_out,
                           orig, ks, S, base, lead, in_lds, Sessions<true>{slots, n_slots, 1});
    else
        hipLaunchKernelGGL(resample_stream_kernel<false>, dim3(B), dim3(256), in_lds ? lds : 0, s, x_new, kern, state, y, n_new, n_out,
                           orig, ks, S, base, lead, in_lds, Sessions<false>{});
    return hipGetLastError();
}

// The bank [newf][ks] goes to LDS when it fits 64 KB at an odd row pitch (ks, or ks + 1 for an even ks); else it is read from
// memory at pitch ks.
hipError_t launch_resample_stream_rational(const float* x_new, const float* kern, float* state, const int32_t* slots, float* y, int B,
                                           int n_new, int n_out, int orig, int newf, int ks, int S, int base, int lead, int n_slots,
                                           hipStream_t s)
{
    if (B == 0) return hipSuccess;
    const int odd = ks | 1;
    const size_t lds = (size_t)newf * odd * sizeof(float);
    const int in_lds = lds <= 64 * 1024;
    const int kp = in_lds ? odd : ks;
    if (slots)
        hipLaunchKernelGGL(resample_stream_rational_kernel<true>, dim3(B), dim3(256), in_lds ? lds : 0, s, x_new, kern, state, y, n_new,
                           n_out, orig, newf, ks, kp, S, base, lead, in_lds, Sessions<true>{slots, n_slots, 1});
    else
        hipLaunchKernelGGL(resample_stream_rational_kernel<false>, dim3(B), dim3(256), in_lds ? lds : 0, s, x_new, kern, state, y, n_new,
                           n_out, orig, newf, ks, kp, S, base, lead, in_lds, Sessions<false>{});
    return hipGetLastError();
}

// The split form: the outputs launch, then the state launch, on the one stream.  A part is at most 16 phases (newf spread evenly
// over the phase groups: 10 groups of 15 for newf = 147) by as many filter blocks as make about 256 outputs, one per thread; the
// result does not depend on either number.  The bank goes to LDS under the one-block launcher's rule (so both forms read a given
// bank from the same place), but only the part's pp rows of it: 5.6 KB instead of 55 KB for 24 kHz -> 44.1 kHz.  With n_out == 0 or
// n_new == 0 the launch that would do nothing is left out.
hipError_t launch_resample_stream_rational_split(const float* x_new, const float* kern, float* state, const int32_t* slots, float* y, int B,
                                                 int n_new, int n_out, int orig, int newf, int ks, int S, int base, int lead, int n_slots,
                                                 hipStream_t s)
{
    if (B == 0) return hipSuccess;
    if (n_out > 0) {
        const int odd = ks | 1;
        const int in_lds = (size_t)newf * odd * sizeof(float) <= 64 * 1024;
        const int kp = in_lds ? odd : ks;
        const int groups = (newf + 15) / 16;
        const int pp = (newf + groups - 1) / groups, n_pg = (newf + pp - 1) / pp;
        const int qq = 256 / pp > 1 ? 256 / pp : 1;
        const int nq = (int)(((long long)n_out + newf - 1) / newf);
        const long long parts = (long long)n_pg * ((nq + qq - 1) / qq);
        if (parts > 0x7FFFFFFFLL) return hipErrorInvalidConfiguration;
        const size_t lds = in_lds ? (size_t)pp * kp * sizeof(float) : 0;
        const dim3 grid((unsigned)parts, (unsigned)(B < 65535 ? B : 65535)), block(256);
        if (slots)
            hipLaunchKernelGGL(resample_stream_rational_outputs_kernel<true>, grid, block, lds, s, x_new, kern, state, y, B, n_new, n_out, orig,
                               newf, ks, kp, S, base, lead, in_lds, pp, qq, n_pg, Sessions<true>{slots, n_slots, 1});
        else
            hipLaunchKernelGGL(resample_stream_rational_outputs_kernel<false>, grid, block, lds, s, x_new, kern, state, y, B, n_new, n_out, orig,
                               newf, ks, kp, S, base, lead, in_lds, pp, qq, n_pg, Sessions<false>{});
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (n_new > 0) {
        if (slots)
            hipLaunchKernelGGL(resample_stream_state_kernel<true>, dim3(B), dim3(256), 0, s, x_new, state, n_new, S,
                               Sessions<true>{slots, n_slots, 1});
        else
            hipLaunchKernelGGL(resample_stream_state_kernel<false>, dim3(B), dim3(256), 0, s, x_new, state, n_new, S, Sessions<false>{});
    }
    return hipGetLastError();
}

// desc == nullptr: the dense instantiation on `rows` rows with the one (fill, n, drop); else the group desc[G][5] of a pool of
// n_slots sessions, 2*G blocks (fill / n / drop unused).
hipError_t launch_stream_samples(float* buf, const int32_t* desc, const float* x_new, float* win, int fill, int n, int w, int drop,
                                 int cap, int rows, int n_slots, int x_total, hipStream_t s)
{
    if (rows == 0) return hipSuccess;
    if (desc) {
        hipLaunchKernelGGL(stream_samples_kernel<true>, dim3(2u * (unsigned)rows), dim3(SMP_THREADS), 0, s, buf, x_new, win, w, cap,
                           SampleRows<true>{desc, rows, n_slots, x_total});
        return hipGetLastError();
    }
    if (n == 0 && w == 0 && drop == 0) return hipSuccess;
    hipLaunchKernelGGL(stream_samples_kernel<false>, dim3((unsigned)rows), dim3(SMP_THREADS), 0, s, buf, x_new, win, w, cap,
                       SampleRows<false>{fill, n, drop});
    return hipGetLastError();
}

hipError_t launch_stream_rows(float* pool, const int32_t* slots, float* rows, int G, int C, int n_slots, int scatter, hipStream_t s)
{
    const int total = G * C;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(stream_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pool, slots, rows, C, n_slots,
                       total, scatter);
    return hipGetLastError();
}

}  // namespace mvq
