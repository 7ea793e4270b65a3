// fec.hip -- forward error correction over the packet bodies (include/mvq.h: mvq_fec_parity_u8, mvq_fec_recover_u8).  The
// format and THE recovery rule are defined by packets.py (fec_rows / fec_recover); the kernels equal them bit for bit:
//   parity group j of an item covers packets [j*g, min(P, (j+1)*g)); packet p is protected to c_p books; prefix(p) = the first
//   n_p = ceil(c_p*ntok_p*bits / 8) bytes of body row p with the bits of book c_p and above cleared in the last one;
//   row j of rows[B, G, g + W] = the g counts (0 in the slots of a short tail group), then the XOR of the prefixes, W bytes.
// Byte kernels: no atomics, no LDS, and the group's counts are re-read (L1 hits) instead of kept in an indexed local array.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_small.hpp"

namespace mvq {
namespace {
constexpr int FEC_MAX_GROUP = 16;
constexpr int FEC_BLOCK = 64;

// Byte y of prefix(p) at c books: 0 at and past n = ceil(c*ntok*bits / 8), the last byte masked to the bits of the kept books.
// c <= nb, so n <= body_full: the read stays inside the row.
__device__ __forceinline__ uint32_t prefix_byte(const uint8_t* __restrict__ row, int y, int c, int ntok, int bits)
{
    const int nbits = c * ntok * bits;
    const int n = (nbits + 7) >> 3;
    if (y >= n) return 0u;
    uint32_t v = row[y];
    const int used = nbits - 8 * y;                                       // >= 1; < 8 only in the last byte
    if (used < 8) v &= (1u << used) - 1u;
    return v;
}
}  // namespace

// One thread per output byte of rows[B, G, g + W].
__global__ __launch_bounds__(256) void fec_parity_kernel(const uint8_t* __restrict__ bodies, const uint8_t* __restrict__ nb_sent,
                                                         uint8_t* __restrict__ rows, int P, int G, int body_full, int nb, int T,
                                                         int bits, int ptok, int g, int m, int W, size_t total)
{
    const int rw = g + W;
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % rw);
        const size_t r = o / rw;
        const int j = (int)(r % G);
        const size_t b = r / G;
        const int p0 = j * g;
        const int gj = min(g, P - p0);
        uint32_t out = 0;
        if (x < g) {
            if (x < gj) out = (uint32_t)min(m, nb_sent ? (int)nb_sent[b * P + p0 + x] : nb);
        } else {
            const int y = x - g;
            for (int u = 0; u < gj; ++u) {
                const int p = p0 + u;
                const int c = min(m, nb_sent ? (int)nb_sent[b * P + p] : nb);
                out ^= prefix_byte(bodies + (b * P + p) * (size_t)body_full, y, c, min(ptok, T - p * ptok), bits);
            }
        }
        rows[o] = (uint8_t)out;
    }
}

// One block per (item, group).  Every thread forms the decision from the group's counts; the threads then share out the bytes of
// the one deficient row; its count is written behind a barrier, after every thread has decided.
__global__ __launch_bounds__(FEC_BLOCK) void fec_recover_kernel(uint8_t* __restrict__ bodies, uint8_t* __restrict__ nb_recv,
                                                                const uint8_t* __restrict__ rows, const uint8_t* __restrict__ got,
                                                                uint8_t* __restrict__ recovered, int P, int G, int body_full, int nb,
                                                                int T, int bits, int ptok, int g, int m, int W)
{
    const int j = blockIdx.x % G;
    const size_t b = blockIdx.x / G;
    const int p0 = j * g;
    const int gj = min(g, P - p0);
    const int cmax = min(m, nb);                                          // a corrupt count byte cannot make a read leave its row
    const uint8_t* prow = rows + (b * G + j) * (size_t)(g + W);
    uint8_t* cnt = nb_recv + b * P + p0;

    int ndef = 0, q = 0, cq = 0;
    if (got[b * G + j] != 0) {
#pragma unroll
        for (int u = 0; u < FEC_MAX_GROUP; ++u) {
            if (u < gj) {
                const int c = min((int)prow[u], cmax);
                if ((int)cnt[u] < c) { ++ndef; q = u; cq = c; }
            }
        }
    }
    const bool fix = ndef == 1;
    if (recovered && (int)threadIdx.x < gj) recovered[b * P + p0 + threadIdx.x] = (uint8_t)(fix && (int)threadIdx.x == q);
    if (fix) {
        const int nq = (cq * min(ptok, T - (p0 + q) * ptok) * bits + 7) >> 3;      // <= W <= body_full
        uint8_t* dst = bodies + (b * P + p0 + q) * (size_t)body_full;
        for (int y = threadIdx.x; y < body_full; y += FEC_BLOCK) {
            uint32_t v = 0;
            if (y < nq) {
                v = prow[g + y];
                for (int u = 0; u < gj; ++u) {
                    if (u == q) continue;
                    const int p = p0 + u;
                    v ^= prefix_byte(bodies + (b * P + p) * (size_t)body_full, y, min((int)prow[u], cmax), min(ptok, T - p * ptok), bits);
                }
            }
            dst[y] = (uint8_t)v;
        }
    }
    __syncthreads();                                                      // every thread has read the group's counts
    if (fix && threadIdx.x == 0) cnt[q] = (uint8_t)cq;
}

hipError_t launch_fec_parity(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows, int B, int nb, int T, int bits, int ptok,
                             int g, int m, hipStream_t s)
{
    const int P = (T + ptok - 1) / ptok;
    const int G = (P + g - 1) / g;
    const int body_full = (nb * ptok * bits + 7) / 8;
    const int W = (m * ptok * bits + 7) / 8;
    const size_t total = (size_t)B * G * (size_t)(g + W);
    if (total == 0) return hipSuccess;
    size_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    const int pi = prof_enabled() ? prof_begin("fec_parity_kernel", 0.0, s) : -1;
    hipLaunchKernelGGL(fec_parity_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bodies, nb_sent, rows, P, G, body_full, nb, T, bits,
                       ptok, g, m, W, total);
    prof_end(pi, s);
    return hipGetLastError();
}

hipError_t launch_fec_recover(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int B,
                              int nb, int T, int bits, int ptok, int g, int m, hipStream_t s)
{
    const int P = (T + ptok - 1) / ptok;
    const int G = (P + g - 1) / g;
    const int body_full = (nb * ptok * bits + 7) / 8;
    const int W = (m * ptok * bits + 7) / 8;
    if ((size_t)B * G == 0) return hipSuccess;
    const int pi = prof_enabled() ? prof_begin("fec_recover_kernel", 0.0, s) : -1;
    hipLaunchKernelGGL(fec_recover_kernel, dim3((unsigned)((size_t)B * G)), dim3(FEC_BLOCK), 0, s, bodies, nb_recv, rows, got, recovered,
                       P, G, body_full, nb, T, bits, ptok, g, m, W);
    prof_end(pi, s);
    return hipGetLastError();
}

}  // namespace mvq
