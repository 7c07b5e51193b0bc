// vbmath.h -- the arithmetic of VBEM's x_t = exp(psi(alpha_t) - c) / effLen_t (src/CollapsedEMOptimizer.cpp:300-320), usable from
// device code (hipcc: em.hip, em_persist.h) and, except for the two forms that need gfx950 instructions, from host code (g++:
// tests/test_vbmath_cpu.py compiles this header as plain C++ through tests/vbmath_harness.cpp and compares it with mpmath).
// sfgpu_vb_eval (em.hip) evaluates every form on the device, one lane per element, for tests/test_gpu_vbmath.py.
//
//   digamma_pos(x)          psi(x)                              host + device    k_vb_prepare, k_update, the normaliser c
//   vb_x_lean(a, c, len)    the x above, no log                 g++ + device     the fused sweep
//   vb_x_fast(a, c, len)    the x above, one division, own exp  g++ + device     SFGPU_P_OLDHEAD builds of the persistent loop
//   vb_x_head(a, c, len)    vb_x_fast with literals + fast_rcp  device           the persistent loop
//   fast_rcp(x)             1 / x by v_rcp_f64 + two Newton     device           the persistent loop
//
// Domain.  digamma_pos: every x > 0 (a denormal x whose -1/x overflows gives -inf, as psi does in binary64).  The three x forms:
// a >= kPriorAlpha (0.01), len >= 1, c < 50 -- the exponent then lies in (-200, 0], far from the ends of the binary64 range, and
// d y len stays normal.  The CALLERS guarantee it: new_alpha adds the prior to every alpha' before an x is formed from it, c is
// psi(M prior + numMapped) <= psi(2^63) < 44, and k_clamp_len clamps every effective length to >= 1.  Outside it vb_x_fast and
// vb_x_head are undefined (a = 1e-100: an argument of -1e100, which their own exp does not reduce -- the result is -inf); vb_x_lean and exp(digamma_pos(a) - c) / len still
// hold wherever the result is a normal number -- which is why the FIRST x of a run, whose alpha is N / n_active and may lie below
// the prior, comes from digamma_pos (k_vb_prepare).
//
// The host build must not contract: vb_x_lean and digamma_pos are written without fma, vb_x_fast with explicit fma, and the device
// build (-ffp-contract=off) keeps them so.  Compile host code with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SF_VB_HD __host__ __device__ __forceinline__
#define SF_VB_D __device__ __forceinline__
#define SF_VB_FMA(a, b, c) fma(a, b, c)
#else
#define SF_VB_HD inline
#define SF_VB_D inline
#define SF_VB_FMA(a, b, c) std::fma(a, b, c)
#endif

namespace sfgpu {

// psi(x), x > 0: the recurrence psi(x) = psi(x + 10) - sum_{k<10} 1/(x + k) for x < 10, then the asymptotic
// series through B_14 (boost::math::digamma at :303, :314 in the reference; |err| ~ 1e-15).
// The ten reciprocals are added as ONE fraction (pairwise n/d merges: every term is positive, so nothing
// cancels) -- a single f64 division instead of up to ten dependent ones (a wavefront always holds some
// low-abundance transcript, so the old loop ran all ten rounds for everybody).
SF_VB_HD double digamma_pos(double x) {
    double r = 0.0;
    if (x < 10.0) {
        const double a0 = x, a1 = x + 1.0, a2 = x + 2.0, a3 = x + 3.0, a4 = x + 4.0,
                     a5 = x + 5.0, a6 = x + 6.0, a7 = x + 7.0, a8 = x + 8.0, a9 = x + 9.0;
        double n01 = a0 + a1, d01 = a0 * a1, n23 = a2 + a3, d23 = a2 * a3, n45 = a4 + a5, d45 = a4 * a5,
               n67 = a6 + a7, d67 = a6 * a7, n89 = a8 + a9, d89 = a8 * a9;
        const double n03 = n01 * d23 + n23 * d01, d03 = d01 * d23;
        const double n47 = n45 * d67 + n67 * d45, d47 = d45 * d67;
        const double n07 = n03 * d47 + n47 * d03, d07 = d03 * d47;
        const double n09 = n07 * d89 + n89 * d07, d09 = d07 * d89;
        r = -(n09 / d09);
        x += 10.0;
    }
    double inv = 1.0 / x, inv2 = inv * inv;
    double s = inv2 * (1.0 / 12.0 - inv2 * (1.0 / 120.0 - inv2 * (1.0 / 252.0 - inv2 * (1.0 / 240.0
             - inv2 * (1.0 / 132.0 - inv2 * (691.0 / 32760.0 - inv2 * (1.0 / 12.0)))))));
    return r + log(x) - 0.5 * inv - s;
}

// VBEM's x_t = exp(psi(a) - c) / effLen (:300-320) for the FUSED sweep, whose 64-register budget has no room for digamma_pos's
// pairwise tree, a log and an exp.  Same recurrence and series as digamma_pos, but exp(log(y)) is y itself:
//   exp(psi(a) - c) = y exp(-(1 / (2y) + s(y) + r + c)),   y = a (+ 10 below 10),   r = sum_{k<10} 1 / (a + k),
// with r gathered as ONE fraction term by term (all terms positive: nothing cancels; ten numbers below 20 multiply to < 1e13).
// One exp, no log, ~10 live doubles; agrees with exp(digamma_pos(a) - c) to a few ulp of the exponent's size.
SF_VB_D double vb_x_lean(double a, double c, double len) {
    double y = a, q = c;
    if (a < 10.0) {
        double n = 1.0, d = a;
#pragma unroll
        for (int k = 1; k < 10; ++k) { const double t = a + (double)k; n = n * t + d; d = d * t; }
        q += n / d;
        y = a + 10.0;
    }
    const double inv = 1.0 / y, inv2 = inv * inv;
    const double s = inv2 * (1.0 / 12.0 - inv2 * (1.0 / 120.0 - inv2 * (1.0 / 252.0 - inv2 * (1.0 / 240.0
                   - inv2 * (1.0 / 132.0 - inv2 * (691.0 / 32760.0 - inv2 * (1.0 / 12.0)))))));
    q += 0.5 * inv + s;
    return y * exp(-q) / len;
}

// The same for the kernels that are short of registers AND of issue slots (the fused sweep, the persistent loop: every thread of a
// window slot evaluates this once per iteration, ~9 wavefronts per tile on a dependent chain).  One division instead of three
// (n / d, 1 / y and 1 / effLen share the reciprocal of d y effLen) and an exp of its own: k = rint(t log2 e), r = t - k ln 2 in two
// pieces, the Taylor polynomial to r^13 (|r| <= ln 2 / 2: the remainder is below 4e-18), ldexp -- no special cases: the argument lies
// in (-200, 0] (alpha >= the prior 0.01, c = psi(M prior + numMapped) < 50).  Its 15 constants sit in constant memory: as literals
// the compiler keeps them in VGPR pairs across the persistent loop and spills them.  ~70 instructions against ~150; agrees with
// exp(digamma_pos(a) - c) / len to ~1e-13 at alpha near the prior (the fraction of ten terms carries the rounding: tests/test_vbmath_cpu.py
// has the bound, per evaluation against mpmath).
struct VbConsts { double l2e, ln2_hi, ln2_lo, c[12]; double s[7]; };
#define SF_VB_CONSTS {                                                                                                              \
    1.4426950408889634074, 6.93147180369123816490e-01, 1.90821492927058770002e-10,                                                  \
    {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, \
     1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5},                                                                                      \
    {1.0 / 12.0, 691.0 / 32760.0, 1.0 / 132.0, 1.0 / 240.0, 1.0 / 252.0, 1.0 / 120.0, 1.0 / 12.0}}
#if defined(__HIPCC__)
__device__ __constant__ VbConsts kVb = SF_VB_CONSTS;
#else
static const VbConsts kVb = SF_VB_CONSTS;                   // the host's twin: the same initialiser in plain memory
#endif
SF_VB_D double vb_x_fast(double a, double c, double len) {
    double y = a, n = 0.0, d = 1.0;
    if (a < 10.0) {
        n = 1.0; d = a;
#pragma unroll
        for (int k = 1; k < 10; ++k) { const double t = a + (double)k; n = SF_VB_FMA(n, t, d); d = d * t; }
        y = a + 10.0;
    }
    const double dy = d * y;
    const double R = 1.0 / (dy * len);                                 // the one division
    const double inv = (d * len) * R;                                  // 1 / y
    const double rlen = dy * R;                                        // 1 / effLen
    const double inv2 = inv * inv;
    const VbConsts& K = kVb;
    double s = SF_VB_FMA(-inv2, K.s[0], K.s[1]);                        // inv2 (1/12 - inv2 (1/120 - inv2 (1/252 - inv2 (1/240 - inv2 (1/132 - inv2 (691/32760 - inv2 / 12))))))
    s = SF_VB_FMA(-inv2, s, K.s[2]); s = SF_VB_FMA(-inv2, s, K.s[3]); s = SF_VB_FMA(-inv2, s, K.s[4]); s = SF_VB_FMA(-inv2, s, K.s[5]); s = SF_VB_FMA(-inv2, s, K.s[6]);
    s = s * inv2;
    // t = -(c + n / d + 1 / (2 y) + s)   (n / d = n y effLen R)
    const double t = -(c + SF_VB_FMA(n * y, len * R, SF_VB_FMA(0.5, inv, s)));
    const double kf = rint(t * K.l2e);
    double r = SF_VB_FMA(-kf, K.ln2_hi, t);
    r = SF_VB_FMA(-kf, K.ln2_lo, r);
    double p = K.c[0];
#pragma unroll
    for (int i = 1; i < 12; ++i) p = SF_VB_FMA(p, r, K.c[i]);
    p = SF_VB_FMA(p, r, 1.0); p = SF_VB_FMA(p, r, 1.0);
    return ldexp(p * y, (int)kf) * rlen;
}

#if defined(__HIPCC__)
// The same arithmetic for the PERSISTENT loop's head (round 6).  There every tile is in the same phase at the same time (a tile needs its
// neighbours' sums of the step before: lockstep), so the head's instructions are not hidden under another block's LDS phases and every
// one of them is on the step's critical path -- and the constants of vb_x_fast arrived through 58 v_readlane per evaluation (22 doubles
// loaded once, far more than the kernel's SGPRs hold: spilled into VGPR lanes).  Here a constant is two s_mov_b32 with literals right where
// it is used (scalar ALU, no memory, no spill, never hoisted: the asm is volatile), and the two divisions are v_rcp_f64 + two Newton steps
// (the operands are far from the denormals: a >= the prior, effLen >= 1) instead of the IEEE sequence.
template <uint64_t B> SF_VB_D double kd_bits() {
    uint32_t lo, hi;
    asm volatile("s_mov_b32 %0, %1" : "=s"(lo) : "n"((uint32_t)B));
    asm volatile("s_mov_b32 %0, %1" : "=s"(hi) : "n"((uint32_t)(B >> 32)));
    return __hiloint2double((int)hi, (int)lo);
}
#define SF_KD(x) kd_bits<__builtin_bit_cast(uint64_t, (double)(x))>()
SF_VB_D double fast_rcp(double x) {                                    // 1 / x to ~1 ulp for normal x
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
SF_VB_D double vb_x_head(double a, double c, double len) {
    double y = a, n = 0.0, d = 1.0;
    if (a < 10.0) {
        n = 1.0; d = a;
#pragma unroll
        for (int k = 1; k < 10; ++k) { const double t = a + (double)k; n = fma(n, t, d); d = d * t; }
        y = a + 10.0;
    }
    const double dy = d * y;
    const double R = fast_rcp(dy * len);                               // the one reciprocal
    const double inv = (d * len) * R;                                  // 1 / y
    const double rlen = dy * R;                                        // 1 / effLen
    const double inv2 = inv * inv;
    double s = fma(-inv2, SF_KD(1.0 / 12.0), SF_KD(691.0 / 32760.0));   // inv2 (1/12 - inv2 (1/120 - inv2 (1/252 - inv2 (1/240 - inv2 (1/132 - inv2 (691/32760 - inv2 / 12))))))
    s = fma(-inv2, s, SF_KD(1.0 / 132.0)); s = fma(-inv2, s, SF_KD(1.0 / 240.0)); s = fma(-inv2, s, SF_KD(1.0 / 252.0));
    s = fma(-inv2, s, SF_KD(1.0 / 120.0)); s = fma(-inv2, s, SF_KD(1.0 / 12.0));
    s = s * inv2;
    const double t = -(c + fma(n * y, len * R, fma(0.5, inv, s)));      // -(c + n / d + 1 / (2 y) + s)   (n / d = n y effLen R)
    const double kf = rint(t * SF_KD(1.4426950408889634074));
    double r = fma(-kf, SF_KD(6.93147180369123816490e-01), t);
    r = fma(-kf, SF_KD(1.90821492927058770002e-10), r);
    double p = SF_KD(1.0 / 6227020800.0);
    p = fma(p, r, SF_KD(1.0 / 479001600.0)); p = fma(p, r, SF_KD(1.0 / 39916800.0)); p = fma(p, r, SF_KD(1.0 / 3628800.0));
    p = fma(p, r, SF_KD(1.0 / 362880.0)); p = fma(p, r, SF_KD(1.0 / 40320.0)); p = fma(p, r, SF_KD(1.0 / 5040.0)); p = fma(p, r, SF_KD(1.0 / 720.0));
    p = fma(p, r, SF_KD(1.0 / 120.0)); p = fma(p, r, SF_KD(1.0 / 24.0)); p = fma(p, r, SF_KD(1.0 / 6.0)); p = fma(p, r, 0.5);
    p = fma(p, r, 1.0); p = fma(p, r, 1.0);
    return ldexp(p * y, (int)kf) * rlen;
}
#endif  // __HIPCC__

}  // namespace sfgpu
