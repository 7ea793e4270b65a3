// rate_decide.hpp -- the ONE statement of the sender's rate rule (include/mvq.h: mvq_rvq_rate_f32), shared by the tactile rate
// kernel (rate.hip) and the audio rate kernels (dac_rate.hip).  Include only from units compiled with -ffp-contract=off: the gain
// sums are separate fp32 subtractions and additions.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mvq.h"

namespace mvq {

constexpr int RATE_GROUP_MAX = 16;          // tokens of a group (and so packets of a group)
constexpr int RATE_NB_MAX = 32;

// The decision of one group, by ONE whole wave (all 64 lanes call it together): lane p = packet p of the group.  Es[(m)*16 + i] =
// E_m of token i of the group (LDS, m = 0 .. nb).  Constant quality: the max over a packet of the per-token need.  Constant rate:
// the greedy loop that gives the next book to the packet that gains most, the scan over candidates in ascending packet order
// exactly as the rule states it (a later candidate displaces only on a strictly greater gain).  -> the count of this lane's
// packet (meaningful for lane < npk).
__device__ __forceinline__ int rate_decide(const float* Es, int lane, int nb, int ntok, int npk, int pc, int ptok, int min_books,
                                           int mode, float tol2, int budget)
{
    const int pt0 = lane * ptok;                                           // first token of this lane's packet
    const int pnt = lane < npk ? min(ptok, ntok - pt0) : 0;
    int m = nb < min_books ? nb : min_books;                               // nb == 0: counts of 0
    if (mode == MVQ_RATE_FULL) {
        m = nb;
    } else if (mode == MVQ_RATE_TOL2) {
        int need_max = m;
        for (int jt = 0; jt < pnt; ++jt) {
            const int i = pt0 + jt;
            const float thr = tol2 * Es[i];
            int need = nb;
            for (int mm = nb - 1; mm >= m; --mm)                           // the smallest mm with E_mm <= thr (a NaN comparison is false)
                if (Es[mm * RATE_GROUP_MAX + i] <= thr) need = mm;
            need_max = need > need_max ? need : need_max;
        }
        m = need_max;
    } else if (nb > 0) {                                                   // MVQ_RATE_BUDGET
        auto gain = [&](int mm) {
            float s = 0.0f;
            for (int jt = 0; jt < pnt; ++jt)
                s = s + (Es[mm * RATE_GROUP_MAX + pt0 + jt] - Es[(mm + 1) * RATE_GROUP_MAX + pt0 + jt]);
            return s;
        };
        const int share = (int)(((long long)budget * npk) / pc);
        int left = (share > npk * m ? share : npk * m) - npk * m;
        float gn = (lane < npk && m < nb) ? gain(m) : 0.0f;
        while (left > 0) {
            int win = -1;
            float gw = 0.0f;
#pragma unroll
            for (int p = 0; p < RATE_GROUP_MAX; ++p) {
                const int mp = __builtin_amdgcn_readlane(m, p);
                const float gp = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gn), p));
                if (p < npk && mp < nb && (win < 0 || gp > gw)) { win = p; gw = gp; }
            }
            if (win < 0) break;                                            // every packet has all books
            if (lane == win) { m += 1; gn = m < nb ? gain(m) : 0.0f; }
            left -= 1;
        }
    }
    return m;
}

}  // namespace mvq
