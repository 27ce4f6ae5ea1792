// vg_window.h — the window rule of the approximate extension for (aw, am) = (15, 7), branch-free.
// Plain C++ with no HIP dependency, so that the host test (tests/test_parse_window_rule.py) compiles this very
// function and checks it against the serial loop of the general parse kernel.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define VG_HD __host__ __device__ __forceinline__
#else
#define VG_HD inline
#endif

// First violating position of one lane's 32 positions: the smallest j with a mismatch at j (bit j of mm) whose window
// of aw = 15 positions j-14 .. j holds more than am = 7 mismatches; 32 if there is none.  prev_mm = the mismatch bits
// of the 32 positions in front (only its top 14 bits are read).
//
// Bit j of the 15 shifted copies c_t = {mm, prev_mm} >> (32 - t) is mismatch bit j - t, so the window count of every j
// is the column sum of c_0 .. c_14: a carry-save tree of full adders sums the 15 bit-columns at once.  Only the weight-8
// output is kept (count >= 8 <=> that bit, the count being <= 15), which drops the final sums of weights 1, 2 and 4.
// Each full adder is two three-input logic functions (v_bitop3_b32 on gfx950).
VG_HD uint32_t vg_sh64(uint32_t hi, uint32_t lo, int t) {   // ({hi, lo} >> (32 - t)), 0 < t < 32: bit j = bit j - t of hi
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (32 - t));
}
VG_HD void vg_fa(uint32_t a, uint32_t b, uint32_t c, uint32_t& s, uint32_t& cy) { s = a ^ b ^ c; cy = (a & b) | (c & (a ^ b)); }
VG_HD uint32_t vg_maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a ^ b)); }

// bit j = the window j-14 .. j holds more than 7 mismatches
VG_HD uint32_t vg_window_over_15_7(uint32_t mm, uint32_t prev_mm) {
    uint32_t c[15];
    c[0] = mm;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int t = 1; t < 15; ++t) c[t] = __builtin_amdgcn_alignbit(mm, prev_mm, (uint32_t)(32 - t));
#else
    for (int t = 1; t < 15; ++t) c[t] = vg_sh64(mm, prev_mm, t);
#endif
    // weight 1: 15 -> 5 sums + 5 carries; 5 sums -> the weight-2 carries of two more adders (their final sum is not needed)
    uint32_t s1[5], c2[7];
#pragma unroll
    for (int k = 0; k < 5; ++k) vg_fa(c[3 * k], c[3 * k + 1], c[3 * k + 2], s1[k], c2[k]);
    uint32_t s;
    vg_fa(s1[0], s1[1], s1[2], s, c2[5]);
    c2[6] = vg_maj(s1[3], s1[4], s);
    // weight 2: 7 -> carries of weight 4; weight 4: 3 -> the carry of weight 8
    uint32_t t0, t1, c4a, c4b;
    vg_fa(c2[0], c2[1], c2[2], t0, c4a);
    vg_fa(c2[3], c2[4], c2[5], t1, c4b);
    const uint32_t c4c = vg_maj(c2[6], t0, t1);
    return vg_maj(c4a, c4b, c4c);
}
VG_HD int vg_first_violation_15_7(uint32_t mm, uint32_t prev_mm) {
    const uint32_t v = vg_window_over_15_7(mm, prev_mm) & mm;
    return v ? __builtin_ctz(v) : 32;
}
