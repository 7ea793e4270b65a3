// dac_stage.hpp -- ONE stage of the DAC residual VQ's look-up, shared by dac_rvq_from_codes_kernel (kernels_vq.hip) and the energy
// kernel of the audio rate control (dac_rate.hip), so that the two chains cannot drift apart: for the lane's four channels
// c0, c0 + 16, c0 + 32, c0 + 48, zq_st(c) = the fma chain over the 8 code dims from +0, then + out_b; acc(c) = acc(c) + zq_st(c).
#pragma once
#include <hip/hip_runtime.h>
#include "det_math.hpp"

namespace mvq {

typedef float dac_v4 __attribute__((ext_vector_type(4)));

// pa / pb: the two halves of the token's raw codebook row of stage st.
__device__ __forceinline__ void dac_stage_accumulate(float (&acc)[4], const dac_v4 pa, const dac_v4 pb, const float* __restrict__ out_w,
                                                     const float* __restrict__ out_b, int st, int C, int c0)
{
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = c0 + 16 * u;
        const float* wr = out_w + ((size_t)st * C + c) * 8;
        const dac_v4 wa = *reinterpret_cast<const dac_v4*>(wr);
        const dac_v4 wb = *reinterpret_cast<const dac_v4*>(wr + 4);
        float a = 0.0f;
        a = dfma(wa.x, pa.x, a); a = dfma(wa.y, pa.y, a); a = dfma(wa.z, pa.z, a); a = dfma(wa.w, pa.w, a);
        a = dfma(wb.x, pb.x, a); a = dfma(wb.y, pb.y, a); a = dfma(wb.z, pb.z, a); a = dfma(wb.w, pb.w, a);
        const float zqi = a + out_b[(size_t)st * C + c];
        acc[u] = acc[u] + zqi;
    }
}

}  // namespace mvq
