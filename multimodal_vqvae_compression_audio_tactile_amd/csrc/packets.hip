// packets.hip -- the lossy-channel receiver's index kernels (include/mvq.h: mvq_idx_pack_packets_u8, mvq_idx_unpack_packets,
// mvq_rvq_dequant_layers_f32).  The packet body layout is defined by packets.py (pack_bodies / unpack_bodies); the kernels equal
// it bit for bit:
//   packet p of an item carries tokens [p*ptok, min(T, (p+1)*ptok)), ntok of them; element e = book*ntok + j (BOOK-major) takes
//   bits [e*bits, (e+1)*bits) of the body, least-significant bit first, bits packed LSB-first into bytes; a row of
//   bodies[B, P, body_full] is zero past its last element.
// No atomics: one thread owns one output byte (pack) or one output index (unpack) and gathers what falls into it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_small.hpp"

namespace mvq {
namespace {
inline unsigned grid_1d(size_t n)
{
    size_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

__device__ __forceinline__ uint32_t clamp_index(int64_t v, int K)
{
    return v < 0 ? 0u : (v >= K ? (uint32_t)(K - 1) : (uint32_t)v);
}
}  // namespace

// One thread per output byte.  Byte y of packet (b, p) holds bits [8y, 8y+8) of the body: at most eight elements touch it.
__global__ __launch_bounds__(256) void idx_pack_packets_kernel(const int64_t* __restrict__ idx, uint8_t* __restrict__ bodies,
                                                               int P, int body_full, int nb, int T, int K, int bits, int ptok,
                                                               size_t s_book, size_t s_item, size_t total)
{
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(o % body_full);
        const size_t row = o / body_full;
        const int p = (int)(row % P);
        const size_t b = row / P;
        const int t0 = p * ptok;
        const int ntok = min(ptok, T - t0);
        const int n_elem = nb * ntok;
        const int bit0 = 8 * y;
        const int e_last = min((bit0 + 7) / bits, n_elem - 1);
        uint32_t byte = 0;
        for (int e = bit0 / bits; e <= e_last; ++e) {
            const int book = e / ntok, j = e - book * ntok;
            const uint32_t v = clamp_index(idx[(size_t)book * s_book + b * s_item + (size_t)(t0 + j)], K);
            const int sh = e * bits - bit0;                               // in (-bits, 8)
            byte |= sh >= 0 ? v << sh : v >> -sh;
        }
        bodies[o] = (uint8_t)(byte & 0xFFu);
    }
}

// One thread per output index (book i, token n = b*T + t); the thread of book 0 also writes nb_valid[n].  An index of up to 24
// bits at a bit offset of up to 7 spans at most four bytes, each read only when it lies inside the row.
__global__ __launch_bounds__(256) void idx_unpack_packets_kernel(const uint8_t* __restrict__ bodies, const uint8_t* __restrict__ nb_recv,
                                                                 int64_t* __restrict__ idx, uint8_t* __restrict__ nb_valid,
                                                                 int P, int body_full, int nb, int T, int K, int bits, int ptok,
                                                                 size_t N, size_t total)
{
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t n = o % N;
        const int i = (int)(o / N);
        const size_t b = n / T;
        const int t = (int)(n % T);
        const int p = t / ptok, j = t - p * ptok;
        const int ntok = min(ptok, T - p * ptok);
        const int got = min((int)nb_recv[b * P + p], nb);
        if (i == 0) nb_valid[n] = (uint8_t)got;
        if (nb == 0) continue;
        uint32_t v = 0;
        if (i < got && bits > 0) {
            const int bit = (i * ntok + j) * bits;
            const int y0 = bit >> 3;
            const uint8_t* row = bodies + (b * P + p) * (size_t)body_full;
            uint32_t w = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (y0 + u < body_full) w |= (uint32_t)row[y0 + u] << (8 * u);
            v = (w >> (bit & 7)) & ((1u << bits) - 1u);
            if (v >= (uint32_t)K) v = (uint32_t)(K - 1);
        }
        idx[(size_t)i * N + n] = (int64_t)v;
    }
}

// rvq_dequant_kernel (kernels_vq.hip) with a per-token book count: the same +0 start and book order, over the first
// min(nb, nb_valid[n]) books.  One thread per (token, 4-dim piece), tokens fastest across the lanes.
__global__ __launch_bounds__(256) void rvq_dequant_layers_kernel(const int64_t* __restrict__ idx, const float* __restrict__ books,
                                                                 const uint8_t* __restrict__ nb_valid, float* __restrict__ q,
                                                                 int B, int D, int T, int nb, int K, size_t out_sb, size_t out_sd)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    const size_t N = (size_t)B * T;
    const size_t total = N * (size_t)(D >> 2);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i % N;
        const int j = (int)(i / N);
        const int cnt = min(nb, (int)nb_valid[n]);
        v4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int bk = 0; bk < cnt; ++bk) {
            const int id = (int)clamp_index(idx[(size_t)bk * N + n], K);
            const v4 e = *reinterpret_cast<const v4*>(books + ((size_t)bk * K + id) * D + 4 * j);
            acc = acc + e;
        }
        const int b = (int)(n / T), t = (int)(n % T);
        float* o = q + (size_t)b * out_sb + (size_t)(4 * j) * out_sd + t;
        o[0] = acc.x;
        o[out_sd] = acc.y;
        o[2 * out_sd] = acc.z;
        o[3 * out_sd] = acc.w;
    }
}

hipError_t launch_idx_pack_packets(const int64_t* idx, uint8_t* bodies, int B, int nb, int T, int K, int bits, int ptok,
                                   size_t s_book, size_t s_item, hipStream_t s)
{
    const int P = (T + ptok - 1) / ptok;
    const int body_full = (nb * ptok * bits + 7) / 8;
    const size_t total = (size_t)B * P * body_full;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(idx_pack_packets_kernel, dim3(grid_1d(total)), dim3(256), 0, s, idx, bodies, P, body_full, nb, T, K, bits,
                       ptok, s_book, s_item, total);
    return hipGetLastError();
}

hipError_t launch_idx_unpack_packets(const uint8_t* bodies, const uint8_t* nb_recv, int64_t* idx, uint8_t* nb_valid, int B, int nb,
                                     int T, int K, int bits, int ptok, hipStream_t s)
{
    const size_t N = (size_t)B * T;
    if (N == 0) return hipSuccess;
    const int P = (T + ptok - 1) / ptok;
    const int body_full = (nb * ptok * bits + 7) / 8;
    const size_t total = N * (size_t)(nb > 0 ? nb : 1);
    hipLaunchKernelGGL(idx_unpack_packets_kernel, dim3(grid_1d(total)), dim3(256), 0, s, bodies, nb_recv, idx, nb_valid, P,
                       body_full, nb, T, K, bits, ptok, N, total);
    return hipGetLastError();
}

hipError_t launch_rvq_dequant_layers(const int64_t* idx, const float* books, const uint8_t* nb_valid, float* q, int B, int D, int T,
                                     int nb, int K, size_t out_sb, size_t out_sd, hipStream_t s)
{
    const size_t total = (size_t)B * T * (D / 4);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(rvq_dequant_layers_kernel, dim3(grid_1d(total)), dim3(256), 0, s, idx, books, nb_valid, q, B, D, T, nb, K,
                       out_sb, out_sd);
    return hipGetLastError();
}

}  // namespace mvq
