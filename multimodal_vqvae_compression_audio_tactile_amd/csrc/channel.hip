// channel.hip -- the loss-pattern generator of the training step (mvq_channel_draw_u8): packets.channel_counts on the device,
// expanded to the per-token layout of decode_latents' nb_valid / na_valid (token t takes packet t / packet_tok).
//
// A two-state Gilbert-Elliott chain per item over its packets, drawn from a STATELESS 32-bit hash of
// (seed, step, stream, item, packet, draw) -- pure uint32 / uint64 integer arithmetic, so host (numpy) and device agree bit for
// bit and row b depends on item_base + b alone:
//   mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
//   fold(h, f) = mix((h ^ f) + 0x9e3779b9)                                  (mod 2^32)
//   u(draw) = fold(fold(fold(fold(fold(fold(0, seed), step), stream), item), packet), draw)
// An event of probability q happens when u < thr(q), thr(q) = min(2^32, int(q * 2^32)) computed on the host (64-bit).
//   draw 0: the state moves BEFORE every packet (packet 0 included), from "good": good -> bad when u < thr_gb, bad -> good when
//           u < thr_bg;   draw 1: the packet is lost when u < (bad ? thr_loss_bad : thr_loss) -> count 0;
//   draw 2: a surviving packet is thinned when u < thr_thin and nb > min_books;
//   draw 3: books kept by a thinned packet = min_books + ((u * (nb - min_books)) >> 32), i.e. min_books .. nb-1.
// One thread walks one item's chain; plain byte stores, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_small.hpp"

namespace mvq {

__device__ __forceinline__ uint32_t chan_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t chan_fold(uint32_t h, uint32_t f) { return chan_mix((h ^ f) + 0x9e3779b9u); }

__global__ __launch_bounds__(64) void channel_draw_kernel(uint8_t* __restrict__ out, int B, int T, int ptok, int nb, int min_books,
                                                          uint64_t thr_loss, uint64_t thr_thin, uint64_t thr_gb, uint64_t thr_bg,
                                                          uint64_t thr_loss_bad, uint32_t h_stream, uint32_t item_base)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t h_item = chan_fold(h_stream, item_base + (uint32_t)b);
    uint8_t* row = out + (size_t)b * T;
    bool bad = false;
    for (int t0 = 0, p = 0; t0 < T; t0 += ptok, ++p) {
        const uint32_t h = chan_fold(h_item, (uint32_t)p);
        const uint64_t u0 = chan_fold(h, 0u);
        if (bad) { if (u0 < thr_bg) bad = false; }
        else if (u0 < thr_gb) bad = true;
        int count = nb;
        if ((uint64_t)chan_fold(h, 1u) < (bad ? thr_loss_bad : thr_loss)) count = 0;
        else if (nb > min_books && (uint64_t)chan_fold(h, 2u) < thr_thin)
            count = min_books + (int)(((uint64_t)chan_fold(h, 3u) * (uint64_t)(nb - min_books)) >> 32);
        const int t1 = min(T, t0 + ptok);
        for (int t = t0; t < t1; ++t) row[t] = (uint8_t)count;
    }
}

// h_stream = fold(fold(fold(0, seed), step), stream), folded on the host with the same integers
hipError_t launch_channel_draw(uint8_t* out, int B, int T, int ptok, int nb, int min_books, uint64_t thr_loss, uint64_t thr_thin,
                               uint64_t thr_gb, uint64_t thr_bg, uint64_t thr_loss_bad, uint32_t h_stream, uint32_t item_base,
                               hipStream_t s)
{
    if (B == 0 || T == 0) return hipSuccess;
    hipLaunchKernelGGL(channel_draw_kernel, dim3((B + 63) / 64), dim3(64), 0, s, out, B, T, ptok, nb, min_books, thr_loss, thr_thin,
                       thr_gb, thr_bg, thr_loss_bad, h_stream, item_base);
    return hipGetLastError();
}

}  // namespace mvq
