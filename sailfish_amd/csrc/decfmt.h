// decfmt.h -- decimal formatting of unsigned integers without division instructions, usable from device code (hipcc) and
// from host code (g++: tests/test_eqwrite_cpu.py compiles this header as plain C++ and compares it with snprintf).
// Used by eqtext_write.hip, which writes the class section of eq_classes.txt on the device.
//
//   dec_len_u32 / dec_len_u64   number of decimal digits (1 .. 10 / 1 .. 20; 0 has one digit)
//   dec_div10 / dec_div100      v / 10, v / 100 of a u32 by multiply-high (exact for every u32)
//   dec_put_fixed_u32           `len` digits of a u32 (zero-padded), two per step, right to left through put(i, ch)
//   dec_put_u32 / dec_put_u64   all digits of v, right to left, through put(i, ch): i = 0 is the LAST digit, i = len - 1 the first
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SF_DEC_HD __host__ __device__ __forceinline__
#else
#define SF_DEC_HD inline
#endif

namespace sfgpu {

SF_DEC_HD int dec_len_u32(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}

SF_DEC_HD int dec_len_u64(uint64_t v) {
    if (v <= 0xffffffffull) return dec_len_u32((uint32_t)v);
    int n = 10;                                  // 2^32 has 10 digits
    uint64_t p = 10000000000ull;                 // 10^10
    while (n < 20 && v >= p) { ++n; if (n < 20) p *= 10ull; }      // (10^20 does not fit: 20 digits is the end)
    return n;
}

// floor(v / 10) = (v * ceil(2^35 / 10)) >> 35 and floor(v / 100) = (v * ceil(2^37 / 100)) >> 37 hold for every v < 2^32
SF_DEC_HD uint32_t dec_div10(uint32_t v) { return (uint32_t)(((uint64_t)v * 0xCCCCCCCDull) >> 35); }
SF_DEC_HD uint32_t dec_div100(uint32_t v) { return (uint32_t)(((uint64_t)v * 0x51EB851Full) >> 37); }

// `len` digits of v (leading zeros if v is shorter), right to left, starting at index i0
template <typename Put>
SF_DEC_HD void dec_put_fixed_u32(uint32_t v, int len, int i0, Put put) {
    int i = 0;
    for (; i + 1 < len; i += 2) {
        const uint32_t q = dec_div100(v), r = v - 100u * q, t = dec_div10(r);
        put(i0 + i, (char)('0' + (r - 10u * t)));
        put(i0 + i + 1, (char)('0' + t));
        v = q;
    }
    if (i < len) put(i0 + i, (char)('0' + (v - 10u * dec_div10(v))));
}

template <typename Put>
SF_DEC_HD int dec_put_u32(uint32_t v, Put put) {
    const int len = dec_len_u32(v);
    dec_put_fixed_u32(v, len, 0, put);
    return len;
}

// v = hi * 10^18 + mid * 10^9 + lo with every part below 10^9: the 32-bit digit loop does the rest
template <typename Put>
SF_DEC_HD int dec_put_u64(uint64_t v, Put put) {
    if (v <= 0xffffffffull) return dec_put_u32((uint32_t)v, put);
    const uint64_t r = v / 1000000000ull;
    const uint32_t lo = (uint32_t)(v - r * 1000000000ull);
    dec_put_fixed_u32(lo, 9, 0, put);
    if (r < 1000000000ull) {
        const int len = dec_len_u32((uint32_t)r);
        dec_put_fixed_u32((uint32_t)r, len, 9, put);
        return 9 + len;
    }
    const uint64_t hi = r / 1000000000ull;                        // <= 18
    dec_put_fixed_u32((uint32_t)(r - hi * 1000000000ull), 9, 9, put);
    const int len = dec_len_u32((uint32_t)hi);
    dec_put_fixed_u32((uint32_t)hi, len, 18, put);
    return 18 + len;
}

}  // namespace sfgpu
