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
//   gfmt_value(r, &slow)    -> the double strtod reads back from that token (genes.hip folds printed values); at the end of the file
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

// ---- the other direction: the double that strtod reads back from the token of a record (genes.hip folds printed values).
// The token is D 10^k exactly, k = X - (digits(D) - 1), D < 10^6.
//   gfmt_value_fast(r, &pending)  |k| <= 22: D and 10^|k| = 5^|k| 2^|k| are exact doubles, so one IEEE multiply or divide is
//                                 the correctly rounded result; outside, *pending = true and gfmt_value_slow gives the value
//   gfmt_value_slow(r)            any record, in the limbs above: the integer D 10^k rounded to 53 bits (k >= 0), or the
//                                 quotient D 2^-e / 10^-k by compare and subtract with e chosen so that it has 53 bits -- fewer
//                                 when e stops at -1074: denormals -- and the remainder deciding the tie (k < 0)
SF_GFMT_HD double gfmt_from_bits(uint64_t bits) {
    double x;
    memcpy(&x, &bits, 8);
    return x;
}

// zero / inf / nan records; false for a record with digits, whose D and k come back
SF_GFMT_HD bool gfmt_value_split(uint32_t r, double* special, uint32_t* D, int* k) {
    const uint64_t sign = (r & kGfmtSign) ? 1ull << 63 : 0ull;
    if (r & kGfmtSpecial) {
        const uint32_t kind = r & 3u;
        *special = gfmt_from_bits(kind == kGfmtZero ? sign : kind == kGfmtInf ? (sign | 0x7ff0000000000000ull) : 0x7ff8000000000000ull);
        return false;
    }
    *D = r & 0xfffffu;
    *k = (int)((r >> 20) & 0x3ffu) - 512 - (dec_len_u32(*D) - 1);
    return true;
}

SF_GFMT_HD double gfmt_value_fast(uint32_t r, bool* pending) {
    double v;
    uint32_t D;
    int k;
    *pending = false;
    if (!gfmt_value_split(r, &v, &D, &k)) return v;
    const int ak = k < 0 ? -k : k;
    if (ak > 22) { *pending = true; return 0.0; }
    uint64_t p5 = 1;
    for (int i = 0; i < ak; ++i) p5 *= 5u;                         // 5^22 < 2^52
    const double p10 = (double)p5 * (double)(1u << ak);           // exact: 10^22 has 52 significant bits
    v = k < 0 ? (double)D / p10 : (double)D * p10;
    return (r & kGfmtSign) ? -v : v;
}

SF_GFMT_HD int gfmt_big_bitlen(const uint32_t* a) {
    for (int i = kGfmtLimbs - 1; i >= 0; --i)
        if (a[i]) return 32 * i + gfmt_bitlen_u64(a[i]);
    return 0;
}

SF_GFMT_SLOW double gfmt_value_slow(uint32_t r) {
    double special;
    uint32_t D;
    int k;
    if (!gfmt_value_split(r, &special, &D, &k)) return special;
    const uint64_t sign = (r & kGfmtSign) ? 1ull << 63 : 0ull;
    uint32_t num[kGfmtLimbs];
    for (int i = 0; i < kGfmtLimbs; ++i) num[i] = 0;
    num[0] = D;
    uint64_t q;                                                   // the value is q 2^e2 before rounding, q < 2^53
    int e2;
    bool up;                                                      // round q up
    if (k >= 0) {
        gfmt_big_pow10(num, k);                                   // D 10^k < 2^20 10^308 < 2^1044
        const int L = gfmt_big_bitlen(num);
        e2 = L - 53;
        if (e2 <= 0) {                                            // an integer below 2^53: exact
            q = ((uint64_t)num[0] | ((uint64_t)num[1] << 32)) << -e2;
            up = false;
        } else {                                                  // bits e2 .. e2 + 52 lie in at most three limbs
            const int w = e2 >> 5, b = e2 & 31;
            const uint64_t lo = (uint64_t)num[w] | ((uint64_t)(w + 1 < kGfmtLimbs ? num[w + 1] : 0u) << 32);
            const uint64_t hi = w + 2 < kGfmtLimbs ? num[w + 2] : 0u;
            q = (b ? (lo >> b) | (hi << (64 - b)) : lo) & ((1ull << 53) - 1u);
            const int hk = e2 - 1, hw = hk >> 5, hb = hk & 31;
            const bool half = (num[hw] >> hb) & 1u;
            bool sticky = (num[hw] & ((1u << hb) - 1u)) != 0;
            for (int i = 0; i < hw; ++i) sticky = sticky || num[i] != 0;
            up = half && (sticky || (q & 1u));
        }
    } else {
        uint32_t den[kGfmtLimbs], t[kGfmtLimbs];
        for (int i = 0; i < kGfmtLimbs; ++i) den[i] = 0;
        den[0] = 1;
        gfmt_big_pow10(den, -k);                                  // 10^329 < 2^1093
        // D / den lies in (2^(bn - bd - 1), 2^(bn - bd + 1)): with e2 = bn - bd - 52 the quotient is below 2^53, and one more
        // step of the division supplies the missing bit when it is below 2^52
        e2 = gfmt_bitlen_u64(D) - gfmt_big_bitlen(den) - 52;
        if (e2 < -1074) e2 = -1074;
        gfmt_big_shl(num, -e2);                                   // below den 2^53 < 2^1146
        for (int i = 0; i < kGfmtLimbs; ++i) t[i] = den[i];
        gfmt_big_shl(t, 52);
        q = 0;
        for (int bit = 52; bit >= 0; --bit) {
            if (gfmt_big_cmp(t, num) <= 0) { gfmt_big_sub(num, t); q |= 1ull << bit; }
            gfmt_big_shr1(t);
        }
        gfmt_big_shl(num, 1);                                     // twice the remainder
        if (q < (1ull << 52) && e2 > -1074) {
            --e2;
            q <<= 1;
            if (gfmt_big_cmp(num, den) >= 0) { gfmt_big_sub(num, den); q |= 1u; }
            gfmt_big_shl(num, 1);
        }
        const int c = gfmt_big_cmp(num, den);
        up = c > 0 || (c == 0 && (q & 1u));
    }
    if (up) ++q;
    if (q == (1ull << 53)) { q = 1ull << 52; ++e2; }
    // q in [2^52, 2^53) is a normal number with biased exponent e2 + 1075; below 2^52 (only with e2 = -1074) a denormal, whose
    // bits are q itself -- and q = 2^52 there is the smallest normal number by the same sum
    const int be = e2 + 1075;
    if (be >= 2047) return gfmt_from_bits(sign | 0x7ff0000000000000ull);
    return gfmt_from_bits(sign | (q + ((uint64_t)(be - 1) << 52)));
}

SF_GFMT_HD double gfmt_value(uint32_t r, bool* slow) {
    const double v = gfmt_value_fast(r, slow);
    return *slow ? gfmt_value_slow(r) : v;
}

}  // namespace sfgpu
