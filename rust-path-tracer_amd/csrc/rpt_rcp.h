/*
 * rpt_rcp.h — the IEEE f32 reciprocal RN(1 / x) in four instructions on the device.
 *
 * With -fhip-fp32-correctly-rounded-divide-sqrt `1.0f / x` is the full division: 11 VALU instructions on gfx950 (v_div_scale x2,
 * v_rcp, five fma-class, v_mul, v_div_fmas, v_div_fixup), four of them in the slow issue class.  The dividend 1 needs none of the
 * scaling: with r0 = v_rcp_f32(x) (within 1 ulp), one residual step
 *     e = fma(-x, r0, 1);  r = fma(e, r0, r0)
 * is RN(1 / x) (Markstein) as long as r0 is a normal number.  On gfx950 in the mode these kernels are compiled in
 * (-fno-gpu-flush-denormals-to-zero) that is every |x| in [2^-126, 2^126] — the all-ones mantissas included, no second step needed —
 * and nothing else: v_rcp_f32 flushes denormal arguments (it answers inf) and denormal results (it answers 0), and answers 0 / inf /
 * NaN to inf / 0 / NaN.  Through the residual step an estimate of 0 stays 0 (NaN where x is inf) and inf / NaN become NaN, while a true
 * reciprocal inside the window is neither: the guard is ONE compare of the RESULT with the inline constant 0, no register for a threshold, and it is its own
 * lower and upper bound — a caller that knows ONE bound of x (the triangle test's |det| >= 1e-6) has nothing left to save.  Behind the
 * guard, for the rare lanes it catches, the device returns `1.0f / x`, the full sequence, so results never depend on which path ran.
 * A caller that has established BOTH bounds (fastdiv_divisor_ok of rpt_fastdiv.h: |x| in [2^-40, 4)) calls rcp_rn_window: the three
 * instructions and no guard.  The host returns `1.0f / x` from both.
 * Only for the dividend 1: x / y by a reciprocal needs operand guards (rpt_fastdiv.h).
 * Evidence: tests/test_gpu_rcp_exact.py (all 2^32 bit patterns, and rcp_rn_window on all of its window, on the device against the
 * compiler's division: 0 differences; the device against numpy on every exponent field and both sides of the guard) and
 * tests/test_gpu_rcp_walks.py (scenes that take the fallback, bitwise against the oracle).
 */
#ifndef RPT_RCP_H
#define RPT_RCP_H

#include "rpt_math.h"

namespace rptm {

RPT_HD float rcp_rn(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float r0 = __builtin_amdgcn_rcpf(x);
    float r = __builtin_fmaf(__builtin_fmaf(-x, r0, 1.0f), r0, r0);
    if (!(__builtin_fabsf(r) > 0.0f)) {                  /* 0 or NaN: x outside the window */
        asm volatile("");                                /* a real branch: left alone the optimiser runs the division on every lane and selects */
        r = 1.0f / x;
    }
    return r;
#else
    return 1.0f / x;
#endif
}

/* the same for a finite |x| in [2^-126, 2^126], which the CALLER has established: outside it the device's answer is 0 or NaN */
RPT_HD float rcp_rn_window(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float r0 = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r0, 1.0f), r0, r0);
#else
    return 1.0f / x;
#endif
}

}  // namespace rptm
#endif
