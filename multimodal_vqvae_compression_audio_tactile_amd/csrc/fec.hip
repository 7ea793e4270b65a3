// fec.hip -- forward error correction over the packet bodies (include/mvq.h: mvq_fec_parity_u8, mvq_fec_recover_u8,
// mvq_fec_rs_parity_u8, mvq_fec_rs_recover_u8): r <= 4 Reed-Solomon parity rows per group, of which XOR parity is the r = 1 case.
// The format and THE recovery rule are defined by packets.py (fec_rows / fec_recover with Fec.parity = r); the kernels equal them
// bit for bit:
//   parity group j of an item covers packets [j*g, min(P, (j+1)*g)); packet p is protected to c_p books; prefix(p) = the first
//   n_p = ceil(c_p*ntok_p*bits / 8) bytes of body row p with the bits of book c_p and above cleared in the last one;
//   GF(2^8), polynomial 0x11d, generator 2; packet u of its group (u < g <= 16) has coefficient A[i][u] = 2^(i*u) in parity i
//   (i*u <= 45: no exponent wraps); row [j, i] of rows[B, G, r, g + W] = the g counts (0 in the slots of a short tail group), then
//   the GF sum of A[i][u] * prefix(u), W bytes.  A[0][u] = 1: row [j, 0] is the XOR of the prefixes.
//   Every square submatrix of A (4 x 16) is nonsingular, so the d x d system of d deficient packets and any d arrived parities has
//   a solution and Gauss-Jordan on it needs no pivoting (its leading minors are such submatrices).
// One kernel pair, templated on R, the compile-time bound on the parity rows: <4> serves r = 2..4 with the runtime r; in <1> r is
// the constant 1, the one coefficient is 1 and the system is the 1 x 1 identity, so no GF multiply, no matrix and no inversion is
// compiled and what is left is XOR.
// Byte kernels: no atomics, no LDS, no tables (multiply by shift-and-xor), and no indexed local array: the group's counts are
// re-read (L1 hits), the matrix lives in named registers through fully unrolled loops, and the lists of deficient packets and
// arrived parities are bit masks.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_small.hpp"

namespace mvq {
namespace {
constexpr int FEC_MAX_GROUP = 16;
constexpr int FEC_MAX_PARITY = 4;
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

__device__ __forceinline__ uint32_t gf_xtime(uint32_t a) { return ((a << 1) ^ ((a & 0x80u) ? 0x11du : 0u)) & 0xffu; }

__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t acc = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        acc ^= ((b >> s) & 1u) ? a : 0u;
        a = gf_xtime(a);
    }
    return acc;
}

// a * 2^e, 0 <= e <= 3 (one step along a parity row: A[i][u+1] = A[i][u] * 2^i).
__device__ __forceinline__ uint32_t gf_step(uint32_t a, int e)
{
#pragma unroll
    for (int s = 0; s < FEC_MAX_PARITY - 1; ++s)
        if (s < e) a = gf_xtime(a);
    return a;
}

// 2^e for 0 <= e <= 45.
__device__ __forceinline__ uint32_t gf_exp2(int e)
{
    uint32_t a = 1;
    for (int s = 0; s < e; ++s) a = gf_xtime(a);
    return a;
}

// a^254 = a^-1 (a != 0): a^2 * a^4 * ... * a^128.
__device__ __forceinline__ uint32_t gf_inv(uint32_t a)
{
    uint32_t sq = gf_mul(a, a), acc = sq;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        sq = gf_mul(sq, sq);
        acc = gf_mul(acc, sq);
    }
    return acc;
}

// The position of the lowest set bit of mask (mask != 0), which is then cleared.
__device__ __forceinline__ int pop_lowest(uint32_t& mask)
{
    const int x = __ffs((int)mask) - 1;
    mask &= mask - 1u;
    return x;
}

// What both launchers derive from the entry points' arguments.
struct FecGeom {
    int P, G, body_full, W;                                               // packets, parity groups, bytes of a body row / a parity body
};

inline FecGeom fec_geom(int nb, int T, int bits, int ptok, int g, int m)
{
    const int P = (T + ptok - 1) / ptok;
    return {P, (P + g - 1) / g, (nb * ptok * bits + 7) / 8, (m * ptok * bits + 7) / 8};
}
}  // namespace

// One thread per output byte of rows[B, G, r, g + W] (r = 1 in <1>, whatever r_rt says).
template <int R>
__global__ __launch_bounds__(256) void fec_parity_kernel(const uint8_t* __restrict__ bodies, const uint8_t* __restrict__ nb_sent,
                                                         uint8_t* __restrict__ rows, int P, int G, int body_full, int nb, int T,
                                                         int bits, int ptok, int g, int m, int W, int r_rt, size_t total)
{
    const int r = R == 1 ? 1 : r_rt;
    const int rw = g + W;
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(o % rw);
        size_t rest = o / rw;
        const int i = (int)(rest % r);
        rest /= r;
        const int j = (int)(rest % G);
        const size_t b = rest / G;
        const int p0 = j * g;
        const int gj = min(g, P - p0);
        uint32_t out = 0;
        if (x < g) {
            if (x < gj) out = (uint32_t)min(m, nb_sent ? (int)nb_sent[b * P + p0 + x] : nb);
        } else {
            const int y = x - g;
            uint32_t coef = 1;                                            // A[i][u], stepped along the row
            for (int u = 0; u < gj; ++u) {
                const int p = p0 + u;
                const int c = min(m, nb_sent ? (int)nb_sent[b * P + p] : nb);
                const uint32_t v = prefix_byte(bodies + (b * P + p) * (size_t)body_full, y, c, min(ptok, T - p * ptok), bits);
                if constexpr (R == 1) {
                    out ^= v;
                } else {
                    out ^= gf_mul(coef, v);
                    coef = gf_step(coef, i);
                }
            }
        }
        rows[o] = (uint8_t)out;
    }
}

// One block per (item, group).  Every thread forms the same decision from the count bytes and got & got_mask (in <1>: arrived or
// not; else the bitmask of arrived parities): the deficient packets as a bit mask D over the group, the arrived parities as a bit
// mask over r; with 1 <= |D| <= |arrived| the |D| lowest arrived parities i_k and the deficient packets q_d give
// M[k][d] = A[i_k][q_d], padded with the identity to R x R and inverted by Gauss-Jordan (in <1>, M = A[0][q] = 1 is its own
// inverse).  The threads then share out the bytes y: |D| syndromes over the packets outside D (only read), |D| rows of D (only
// written).  The counts are written behind a barrier, after every thread has decided.
template <int R>
__global__ __launch_bounds__(FEC_BLOCK) void fec_recover_kernel(uint8_t* __restrict__ bodies, uint8_t* __restrict__ nb_recv,
                                                                const uint8_t* __restrict__ rows, const uint8_t* __restrict__ got,
                                                                uint8_t* __restrict__ recovered, int P, int G, int body_full, int nb,
                                                                int T, int bits, int ptok, int g, int m, int W, int r_rt,
                                                                uint32_t got_mask)
{
    const int r = R == 1 ? 1 : r_rt;
    const int j = blockIdx.x % G;
    const size_t b = blockIdx.x / G;
    const int p0 = j * g;
    const int gj = min(g, P - p0);
    const int cmax = min(m, nb);                                          // a corrupt count byte cannot make a read leave its row
    const int rw = g + W;
    const uint8_t* grows = rows + (b * G + j) * (size_t)r * rw;           // the group's r parity rows
    uint8_t* cnt = nb_recv + b * P + p0;

    uint32_t arrived = (uint32_t)got[b * G + j] & got_mask;
    if constexpr (R == 1) arrived = arrived != 0;
    const int na = __popc(arrived);
    const uint8_t* crow = grows + (arrived ? __ffs((int)arrived) - 1 : 0) * (size_t)rw;   // the counts: the lowest arrived parity's
    uint32_t D = 0;
    if (arrived) {
#pragma unroll
        for (int u = 0; u < FEC_MAX_GROUP; ++u)
            if (u < gj && (int)cnt[u] < min((int)crow[u], cmax)) D |= 1u << u;
    }
    const int nd = __popc(D);
    const bool fix = nd >= 1 && nd <= na;
    if (recovered && (int)threadIdx.x < gj) recovered[b * P + p0 + threadIdx.x] = (uint8_t)(fix && ((D >> threadIdx.x) & 1u));
    if (fix) {
        // i_k (k < nd): the nd lowest arrived parities; q_d (d < nd): the deficient packets, ascending.  Past nd: 0, unused.
        int ik[R], qd[R];
        uint32_t am = arrived, dm = D;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            ik[k] = (R > 1 && k < nd) ? pop_lowest(am) : 0;
            qd[k] = k < nd ? pop_lowest(dm) : 0;
        }
        uint32_t V[R][R];                                                 // the inverse of M
        if constexpr (R == 1) {
            V[0][0] = 1;
        } else {
            uint32_t M[R][R];                                             // M -> identity, V: identity -> the inverse of M
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int d = 0; d < R; ++d) {
                    M[k][d] = (k < nd && d < nd) ? gf_exp2(ik[k] * qd[d]) : (uint32_t)(k == d);
                    V[k][d] = (uint32_t)(k == d);
                }
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const uint32_t inv = gf_inv(M[k][k]);                     // nonzero: a leading minor of a nonsingular submatrix
#pragma unroll
                for (int d = 0; d < R; ++d) {
                    M[k][d] = gf_mul(inv, M[k][d]);
                    V[k][d] = gf_mul(inv, V[k][d]);
                }
#pragma unroll
                for (int e = 0; e < R; ++e) {
                    if (e == k) continue;
                    const uint32_t f = M[e][k];
#pragma unroll
                    for (int d = 0; d < R; ++d) {
                        M[e][d] ^= gf_mul(f, M[k][d]);
                        V[e][d] ^= gf_mul(f, V[k][d]);
                    }
                }
            }
        }
        for (int y = threadIdx.x; y < body_full; y += FEC_BLOCK) {
            uint32_t S[R];
#pragma unroll
            for (int k = 0; k < R; ++k) S[k] = (k < nd && y < W) ? (uint32_t)grows[ik[k] * (size_t)rw + g + y] : 0u;
            if (y < W) {
                uint32_t coef[R];                                         // A[i_k][u], stepped along the rows
#pragma unroll
                for (int k = 0; k < R; ++k) coef[k] = 1;
                for (int u = 0; u < gj; ++u) {
                    if (!((D >> u) & 1u)) {
                        const int p = p0 + u;
                        const uint32_t v = prefix_byte(bodies + (b * P + p) * (size_t)body_full, y, min((int)crow[u], cmax),
                                                       min(ptok, T - p * ptok), bits);
#pragma unroll
                        for (int k = 0; k < R; ++k)
                            if (k < nd) S[k] ^= R == 1 ? v : gf_mul(coef[k], v);
                    }
                    if constexpr (R > 1) {
#pragma unroll
                        for (int k = 0; k < R; ++k) coef[k] = gf_step(coef[k], ik[k]);
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < R; ++d) {
                if (d < nd) {
                    const int q = qd[d];
                    const int cq = min((int)crow[q], cmax);
                    const int nq = (cq * min(ptok, T - (p0 + q) * ptok) * bits + 7) >> 3;   // <= W <= body_full
                    uint32_t x = 0;
#pragma unroll
                    for (int k = 0; k < R; ++k) x ^= R == 1 ? S[k] : gf_mul(V[d][k], S[k]);
                    bodies[(b * P + p0 + q) * (size_t)body_full + y] = (uint8_t)(y < nq ? x : 0u);
                }
            }
        }
    }
    __syncthreads();                                                      // every thread has read the group's counts
    if (fix && (int)threadIdx.x < gj && ((D >> threadIdx.x) & 1u)) cnt[threadIdx.x] = (uint8_t)min((int)crow[threadIdx.x], cmax);
}

hipError_t launch_fec_parity(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows, int B, int nb, int T, int bits, int ptok,
                             int g, int m, int r, hipStream_t s)
{
    const FecGeom f = fec_geom(nb, T, bits, ptok, g, m);
    const size_t total = (size_t)B * f.G * (size_t)r * (size_t)(g + f.W);
    if (total == 0) return hipSuccess;
    size_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    const int pi = prof_enabled() ? prof_begin(r == 1 ? "fec_parity_kernel" : "fec_rs_parity_kernel", 0.0, s) : -1;
    hipLaunchKernelGGL(r == 1 ? fec_parity_kernel<1> : fec_parity_kernel<FEC_MAX_PARITY>, dim3((unsigned)blocks), dim3(256), 0, s, bodies,
                       nb_sent, rows, f.P, f.G, f.body_full, nb, T, bits, ptok, g, m, f.W, r, total);
    prof_end(pi, s);
    return hipGetLastError();
}

hipError_t launch_fec_recover(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int B,
                              int nb, int T, int bits, int ptok, int g, int m, int r, uint32_t got_mask, hipStream_t s)
{
    const FecGeom f = fec_geom(nb, T, bits, ptok, g, m);
    if ((size_t)B * f.G == 0) return hipSuccess;
    const int pi = prof_enabled() ? prof_begin(r == 1 ? "fec_recover_kernel" : "fec_rs_recover_kernel", 0.0, s) : -1;
    hipLaunchKernelGGL(r == 1 ? fec_recover_kernel<1> : fec_recover_kernel<FEC_MAX_PARITY>, dim3((unsigned)((size_t)B * f.G)),
                       dim3(FEC_BLOCK), 0, s, bodies, nb_recv, rows, got, recovered, f.P, f.G, f.body_full, nb, T, bits, ptok, g, m, f.W, r,
                       got_mask);
    prof_end(pi, s);
    return hipGetLastError();
}

}  // namespace mvq
