// gfmt.h -- printf("%g") of a binary64 (six significant digits, correctly rounded with ties to even on the exact binary value,
// fixed or scientific by the decimal exponent, trailing zeros stripped) without libc, usable from device code (hipcc) and from
// host code (g++: tests/test_gfmt_cpu.py compiles this header as plain C++ and compares it with snprintf).
// Used by quant_write.hip, which writes the rows of quant.sf on the device.  The bytes are Python's "%g" % x (writer.fmt_g);
// a NaN of either sign prints "nan", -0.0 prints "-0".  The longest token is 13 bytes ("-1.23456e-308").
//
//   gfmt_decode(x, &slow)   -> 32-bit record: D (the six digits as an integer, trailing zeros stripped) in bits 0 .. 19,
//                              X + 512 (the decimal exponent of the first digit) in bits 20 .. 29, the sign in bit 30; bit 31
//                              marks zero / inf / nan (then D holds the kind).  All wide arithmetic happens here, once per value.
//                              gfmt_decode_fast / gfmt_decode_slow are its two halves, for callers that run them apart.
//   gfmt_len(r)             -> bytes of the token
//   gfmt_put(r, put)        -> the token through put(i, ch), the convention of decfmt.h: i = 0 is the LAST byte
//
// With x = m 2^e (m < 2^53) and s = 5 - X the digits are D = round_half_even(m 2^e 10^s), an integer division.  X is estimated
// from the bit length, and corrected by comparing the FLOOR of the quotient with 10^5 and 10^6 (not the rounded value: a binary
// value just below a tie must not move up a decade); a rounded 1000000 carries into 100000, X + 1.
//   * 128-bit path: whenever numerator and denominator stay below 2^127 -- every x in [2^-56, 2^127), that is everything a
//     quant.sf column holds.  For s >= 0 the denominator is a power of two (a shift); otherwise the quotient is below 2^24 and
//     comes from 24 compare-and-subtract steps.  No division instruction, no table.
//   * slow path (*slow = true): the same scheme in 36 32-bit limbs, for denormals and the ends of the exponent range.  It is a
//     separate function that is never inlined; on the device its arrays live in scratch memory, so quant_write.hip runs
//     gfmt_decode_fast and gfmt_decode_slow in two kernels and the first one needs registers only.
#pragma once
#include <cstdint>
#include <cstring>

#include "decfmt.h"

#if defined(__HIPCC__)
#define SF_GFMT_HD __host__ __device__ __forceinline__
#define SF_GFMT_SLOW __host__ __device__ __noinline__ inline
#else
#define SF_GFMT_HD inline
#define SF_GFMT_SLOW __attribute__((noinline)) inline
#endif

namespace sfgpu {

__extension__ typedef unsigned __int128 gfmt_u128;

constexpr uint32_t kGfmtSpecial = 1u << 31, kGfmtSign = 1u << 30;
constexpr uint32_t kGfmtZero = 0, kGfmtInf = 1, kGfmtNan = 2;
constexpr uint32_t kGfmtPending = 0xffffffffu;    // no record: what gfmt_decode_fast returns outside its window
constexpr int kGfmtMaxLen = 13;
constexpr int kGfmtLimbs = 36;                     // 1152 bits: m 10^330 (denormals) and 10^304 << 23 (DBL_MAX) fit

SF_GFMT_HD int gfmt_bitlen_u64(uint64_t v) {
    int n = 0;
    if (v >> 32) { n += 32; v >>= 32; }
    if (v >> 16) { n += 16; v >>= 16; }
    if (v >> 8) { n += 8; v >>= 8; }
    if (v >> 4) { n += 4; v >>= 4; }
    if (v >> 2) { n += 2; v >>= 2; }
    if (v >> 1) { n += 1; v >>= 1; }
    return n + (int)v;
}

// floor(q) and round_half_even(q) of q = m 2^e 10^s in 128 bits; false when an operand would not stay below 2^127.
// The caller's estimate of the decimal exponent is off by at most one, so floor(q) < 10^7 < 2^24.
SF_GFMT_HD bool gfmt_scaled_u128(uint64_t m, int e, int s, uint32_t* F, uint32_t* D) {
    if (s >= 0) {
        if (e >= 0 || s > 22 || -e > 126) return false;           // (e >= 0 means x >= 2^52: then s < 0)
        gfmt_u128 num = m;
        for (int i = 0; i < s; ++i) num *= 10u;                   // m 10^22 < 2^127
        const int k = -e;
        const gfmt_u128 q = num >> k;
        const bool half = (uint32_t)(num >> (k - 1)) & 1u;
        const bool sticky = (num & ((((gfmt_u128)1) << (k - 1)) - 1u)) != 0;
        const uint32_t f = q > 0xfffffffeu ? 0xfffffffeu : (uint32_t)q;
        *F = f;
        *D = f + ((half && (sticky || (f & 1u))) ? 1u : 0u);
        return true;
    }
    const int ds = -s;
    gfmt_u128 num, den = 1;
    if (e >= 0) {
        if (gfmt_bitlen_u64(m) + e > 127 || ds > 38) return false;      // 10^38 < 2^127
        num = ((gfmt_u128)m) << e;
        for (int i = 0; i < ds; ++i) den *= 10u;
    } else {
        if (ds > 19 || -e > 63) return false;                     // (x < 2^53: ds <= 11)
        num = m;
        for (int i = 0; i < ds; ++i) den *= 10u;
        den <<= -e;
    }
    uint32_t f = 0;
    for (int bit = 23; bit >= 0; --bit) {
        if (bit && (den >> (128 - bit)) != 0) continue;           // den << bit leaves 128 bits: it is above num
        const gfmt_u128 t = den << bit;
        if (t <= num) { num -= t; f |= 1u << bit; }
    }
    const gfmt_u128 r2 = num << 1;                                // the remainder is below den < 2^127
    *F = f;
    *D = f + ((r2 > den || (r2 == den && (f & 1u))) ? 1u : 0u);
    return true;
}

// ---- the same in kGfmtLimbs 32-bit limbs (little endian)
SF_GFMT_HD void gfmt_big_mul(uint32_t* a, uint32_t f) {
    uint64_t carry = 0;
    for (int i = 0; i < kGfmtLimbs; ++i) {
        const uint64_t v = (uint64_t)a[i] * f + carry;
        a[i] = (uint32_t)v;
        carry = v >> 32;
    }
}
SF_GFMT_HD void gfmt_big_pow10(uint32_t* a, int p) {              // a *= 10^p
    for (; p >= 9; p -= 9) gfmt_big_mul(a, 1000000000u);
    uint32_t f = 1;
    for (int i = 0; i < p; ++i) f *= 10u;
    if (f > 1) gfmt_big_mul(a, f);
}
SF_GFMT_HD void gfmt_big_shl(uint32_t* a, int k) {                // a <<= k (the result fits by the caller's bounds)
    const int w = k >> 5, b = k & 31;
    for (int i = kGfmtLimbs - 1; i >= 0; --i) {
        const uint32_t hi = i - w >= 0 ? a[i - w] : 0u, lo = i - w - 1 >= 0 ? a[i - w - 1] : 0u;
        a[i] = b ? (hi << b) | (lo >> (32 - b)) : hi;
    }
}
SF_GFMT_HD void gfmt_big_shr1(uint32_t* a) {
    for (int i = 0; i < kGfmtLimbs; ++i) a[i] = (a[i] >> 1) | (i + 1 < kGfmtLimbs ? a[i + 1] << 31 : 0u);
}
SF_GFMT_HD int gfmt_big_cmp(const uint32_t* a, const uint32_t* b) {
    for (int i = kGfmtLimbs - 1; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
SF_GFMT_HD void gfmt_big_sub(uint32_t* a, const uint32_t* b) {    // a -= b, a >= b
    uint64_t borrow = 0;
    for (int i = 0; i < kGfmtLimbs; ++i) {
        const uint64_t v = (uint64_t)a[i] - b[i] - borrow;
        a[i] = (uint32_t)v;
        borrow = (v >> 32) & 1u;
    }
}

SF_GFMT_SLOW void gfmt_scaled_big(uint64_t m, int e, int s, uint32_t* F, uint32_t* D) {
    uint32_t num[kGfmtLimbs];
    for (int i = 0; i < kGfmtLimbs; ++i) num[i] = 0;
    num[0] = (uint32_t)m; num[1] = (uint32_t)(m >> 32);
    if (s >= 0) {
        gfmt_big_pow10(num, s);
        if (e >= 0) {                                             // (does not occur: x >= 2^52 has s < 0) an integer, exact
            gfmt_big_shl(num, e);
            *F = *D = num[1] ? 0xfffffffeu : num[0];
            return;
        }
        const int k = -e, w = k >> 5, b = k & 31;                 // k <= 1074
        uint32_t f = num[w] >> b;
        if (b) f |= num[w + 1] << (32 - b);
        const int hk = k - 1, hw = hk >> 5, hb = hk & 31;
        const bool half = (num[hw] >> hb) & 1u;
        bool sticky = (num[hw] & ((1u << hb) - 1u)) != 0;
        for (int i = 0; i < hw; ++i) sticky = sticky || num[i] != 0;
        *F = f;
        *D = f + ((half && (sticky || (f & 1u))) ? 1u : 0u);
        return;
    }
    uint32_t den[kGfmtLimbs], t[kGfmtLimbs];
    for (int i = 0; i < kGfmtLimbs; ++i) den[i] = 0;
    den[0] = 1;
    gfmt_big_pow10(den, -s);
    if (e >= 0) gfmt_big_shl(num, e); else gfmt_big_shl(den, -e);
    for (int i = 0; i < kGfmtLimbs; ++i) t[i] = den[i];
    gfmt_big_shl(t, 23);                                          // den < 2^1011: 23 more bits fit
    uint32_t f = 0;
    for (int bit = 23; bit >= 0; --bit) {
        if (gfmt_big_cmp(t, num) <= 0) { gfmt_big_sub(num, t); f |= 1u << bit; }
        gfmt_big_shr1(t);
    }
    gfmt_big_shl(num, 1);                                         // twice the remainder
    const int c = gfmt_big_cmp(num, den);
    *F = f;
    *D = f + ((c > 0 || (c == 0 && (f & 1u))) ? 1u : 0u);
}

// the six digits D (100000 .. 999999, before stripping) and the decimal exponent X of m 2^e, through `scaled`; false when
// `scaled` gives up
template <typename Scaled>
SF_GFMT_HD bool gfmt_digits(uint64_t m, int e, Scaled scaled, uint32_t* D_out, int* X_out) {
    const int bl = gfmt_bitlen_u64(m) + e;                        // x in [2^(bl-1), 2^bl)
    const int t = (bl - 1) * 1233;
    int X = t >= 0 ? t >> 12 : -((-t + 4095) >> 12);              // floor((bl-1) log10 2), off by at most one either way
    uint32_t F, D;
    if (!scaled(m, e, 5 - X, &F, &D)) return false;
    if (F >= 1000000u) { ++X; if (!scaled(m, e, 5 - X, &F, &D)) return false; }
    else if (F < 100000u) { --X; if (!scaled(m, e, 5 - X, &F, &D)) return false; }
    if (D == 1000000u) { D = 100000u; ++X; }
    *D_out = D; *X_out = X;
    return true;
}

SF_GFMT_HD uint32_t gfmt_pack(uint32_t sign, uint32_t D, int X) {
    for (int i = 0; i < 5; ++i) {                                 // strip the trailing zeros: D keeps its first digit
        const uint32_t q = dec_div10(D);
        if (q * 10u != D) break;
        D = q;
    }
    return sign | ((uint32_t)(X + 512) << 20) | D;
}

// sign, m and e of a finite nonzero x = m 2^e; false for zero, inf and nan, whose record is *special
SF_GFMT_HD bool gfmt_split(double x, uint32_t* sign, uint64_t* m, int* e, uint32_t* special) {
    uint64_t bits;
    memcpy(&bits, &x, 8);
    *sign = (bits >> 63) ? kGfmtSign : 0u;
    const uint32_t be = (uint32_t)(bits >> 52) & 0x7ffu;
    *m = bits & 0xfffffffffffffull;
    if (be == 0x7ffu) { *special = *m ? (kGfmtSpecial | kGfmtNan) : (kGfmtSpecial | *sign | kGfmtInf); return false; }
    if (be == 0 && *m == 0) { *special = kGfmtSpecial | *sign | kGfmtZero; return false; }
    *e = -1074;
    if (be) { *m |= 1ull << 52; *e = (int)be - 1075; }
    return true;
}

// the record of x by the 128-bit path; kGfmtPending when x lies outside its window (then gfmt_decode_slow gives the record)
SF_GFMT_HD uint32_t gfmt_decode_fast(double x) {
    uint32_t sign, special, D;
    uint64_t m;
    int e, X;
    if (!gfmt_split(x, &sign, &m, &e, &special)) return special;
    if (!gfmt_digits(m, e, [](uint64_t mm, int ee, int ss, uint32_t* F, uint32_t* DD) { return gfmt_scaled_u128(mm, ee, ss, F, DD); }, &D, &X))
        return kGfmtPending;
    return gfmt_pack(sign, D, X);
}

// the record of any x in multi-word integers
SF_GFMT_SLOW uint32_t gfmt_decode_slow(double x) {
    uint32_t sign, special, D;
    uint64_t m;
    int e, X;
    if (!gfmt_split(x, &sign, &m, &e, &special)) return special;
    (void)gfmt_digits(m, e, [](uint64_t mm, int ee, int ss, uint32_t* F, uint32_t* DD) { gfmt_scaled_big(mm, ee, ss, F, DD); return true; }, &D, &X);
    return gfmt_pack(sign, D, X);
}

SF_GFMT_HD uint32_t gfmt_decode(double x, bool* slow) {
    uint32_t r = gfmt_decode_fast(x);
    *slow = r == kGfmtPending;
    if (*slow) r = gfmt_decode_slow(x);
    return r;
}

SF_GFMT_HD int gfmt_len(uint32_t r) {
    const int sg = (r & kGfmtSign) ? 1 : 0;
    if (r & kGfmtSpecial) return (r & 3u) == kGfmtZero ? 1 + sg : (r & 3u) == kGfmtInf ? 3 + sg : 3;
    const int X = (int)((r >> 20) & 0x3ffu) - 512;
    const int nd = dec_len_u32(r & 0xfffffu);
    if (X >= -4 && X < 6) {
        if (X < 0) return sg + nd + 1 - X;                        // 0. zeros digits
        return sg + (nd <= X + 1 ? X + 1 : nd + 1);
    }
    const int ax = X < 0 ? -X : X;
    return sg + nd + (nd > 1 ? 1 : 0) + 2 + (ax >= 100 ? 3 : 2);
}

template <typename Put>
SF_GFMT_HD int gfmt_put(uint32_t r, Put put) {
    const int len = gfmt_len(r);
    const int sg = (r & kGfmtSign) ? 1 : 0;
    auto at = [&](int pos, char ch) { put(len - 1 - pos, ch); };  // pos counts from the left
    if (sg) at(0, '-');
    if (r & kGfmtSpecial) {
        const uint32_t kind = r & 3u;
        if (kind == kGfmtZero) at(sg, '0');
        else if (kind == kGfmtInf) { at(sg, 'i'); at(sg + 1, 'n'); at(sg + 2, 'f'); }
        else { at(0, 'n'); at(1, 'a'); at(2, 'n'); }
        return len;
    }
    const int X = (int)((r >> 20) & 0x3ffu) - 512;
    const uint32_t D = r & 0xfffffu;
    const int nd = dec_len_u32(D);
    if (X >= -4 && X < 6) {
        if (X < 0) {
            at(sg, '0'); at(sg + 1, '.');
            for (int i = 0; i < -X - 1; ++i) at(sg + 2 + i, '0');
            dec_put_fixed_u32(D, nd, 0, put);                     // the digits end the token
        } else if (nd <= X + 1) {
            for (int i = nd; i <= X; ++i) at(sg + i, '0');
            dec_put_fixed_u32(D, nd, X + 1 - nd, put);
        } else {
            at(sg + X + 1, '.');
            // digit k from the left sits at sg + k (k <= X) or sg + k + 1: j = nd - 1 - k from the right
            dec_put_fixed_u32(D, nd, 0, [&](int j, char ch) { const int k = nd - 1 - j; at(sg + k + (k > X ? 1 : 0), ch); });
        }
        return len;
    }
    const int ax = X < 0 ? -X : X;
    if (nd > 1) at(sg + 1, '.');
    dec_put_fixed_u32(D, nd, 0, [&](int j, char ch) { const int k = nd - 1 - j; at(k ? sg + 1 + k : sg, ch); });
    const int ne = ax >= 100 ? 3 : 2;
    dec_put_fixed_u32((uint32_t)ax, ne, 0, put);
    put(ne, X < 0 ? '-' : '+');
    put(ne + 1, 'e');
    return len;
}

}  // namespace sfgpu
