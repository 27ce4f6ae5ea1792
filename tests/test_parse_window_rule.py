"""The branch-free window rule of the FAST parse kernels (vclust_amd/csrc/vg_window.h, (aw, am) = (15, 7)) against a
restatement of the serial loop that the general kernel runs (extend() in vg_align.hip).  The header is plain C++: a small
host program includes it and checks, without a GPU,
  * by construction: for every lane position j and every one of the 2^15 contents of the window j-14 .. j (the rest of
    the 64 bits random), bit j of the window predicate is `more than 7 mismatches` -- the predicate of a column reads
    nothing but the 15 bits of its window, so this covers every (mm, prev_mm);
  * end to end: the first violation (popcount screen in front, as in the kernel) equals the loop's on every mm that
    is zero outside one 16-bit field (all 2^16 values, at every shift) times edge and random tails, and on 2^24 random
    pairs drawn with mismatch rates from 3 % to 60 %."""
import pathlib
import shutil
import subprocess

import pytest

HEADER_DIR = pathlib.Path(__file__).resolve().parent.parent / 'vclust_amd' / 'csrc'

DRIVER = r'''
#include "vg_window.h"
#include <cstdio>
#include <cstdint>

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static uint32_t rnd_mask(int pct) { uint32_t m = 0; for (int j = 0; j < 32; ++j) if ((int)(rnd() % 100) < pct) m |= 1u << j; return m; }

// the general kernel's block, restated: popcount screen, skip of the first am - |tail| mismatches, serial test
static int loop_viol(uint32_t mm, uint32_t prev_mm) {
    const int aw = 15, am = 7; const uint32_t awmask = (1u << aw) - 1u;
    int viol = 32;
    const uint32_t tail = prev_mm >> (32 - (aw - 1));
    if ((int)(__builtin_popcount(mm) + __builtin_popcount(tail)) > am) {
        uint32_t bits = mm;
        for (int skip = am - (int)__builtin_popcount(tail); skip > 0; --skip) bits &= bits - 1;
        while (bits) {
            const int j = __builtin_ctz(bits);
            const uint32_t hi = (j == 31) ? mm : (mm & ((2u << j) - 1u));
            int cnt;
            if (j + 1 >= aw) cnt = __builtin_popcount(hi & (awmask << (j + 1 - aw)));
            else cnt = __builtin_popcount(hi) + __builtin_popcount(prev_mm >> (32 - (aw - 1 - j)));
            if (cnt > am) { viol = j; break; }
            bits &= bits - 1;
        }
    }
    return viol;
}
// the FAST kernels' block
static int fast_viol(uint32_t mm, uint32_t prev_mm) {
    const uint32_t tail = prev_mm >> (32 - 14);
    return (int)(__builtin_popcount(mm) + __builtin_popcount(tail)) > 7 ? vg_first_violation_15_7(mm, prev_mm) : 32;
}

static long long bad = 0, n = 0;
static void check(uint32_t mm, uint32_t prev) {
    ++n;
    const int a = loop_viol(mm, prev), b = fast_viol(mm, prev);
    if (a != b && bad++ < 10) printf("MISMATCH mm=%08x prev=%08x loop=%d fast=%d\n", mm, prev, a, b);
}

int main() {
    // 1. the predicate of column j, by construction over its whole window
    long long pbad = 0;
    for (int j = 0; j < 32; ++j)
        for (uint32_t w = 0; w < (1u << 15); ++w)
            for (int r = 0; r < 2; ++r) {
                uint64_t x = rnd();                              // bits 32 + k = mm bit k, bits 0..31 = prev_mm
                const int lo = 32 + j - 14;                      // window = bits lo .. lo + 14 of x
                x = (x & ~(0x7fffull << lo)) | ((uint64_t)w << lo);
                const uint32_t got = (vg_window_over_15_7((uint32_t)(x >> 32), (uint32_t)x) >> j) & 1u;
                if (got != (uint32_t)(__builtin_popcount(w) > 7) && pbad++ < 10) printf("PREDICATE j=%d w=%04x\n", j, w);
            }
    // 2. end to end against the loop
    uint32_t tails[12] = {0u, ~0u, 0xfffc0000u, 0x7f000000u, 0xfe000000u, 0x01fc0000u, 0xaaaa0000u, 0x55540000u, 0, 0, 0, 0};
    for (int k = 8; k < 12; ++k) tails[k] = (uint32_t)rnd();
    for (int sh = 0; sh <= 16; sh += 4)
        for (uint32_t f = 0; f < (1u << 16); ++f)
            for (int k = 0; k < 12; ++k) check(f << sh, tails[k]);
    for (int k = 0; k < (1 << 24); ++k) {
        const int pct = 3 + (int)(rnd() % 58);
        check(rnd_mask(pct), rnd_mask(pct));
    }
    printf("checked %lld pairs, %lld mismatches, %lld predicate errors\n", n, bad, pbad);
    return (bad || pbad) ? 1 : 0;
}
'''


def _cxx():
    for c in ('c++', 'g++', 'clang++'):
        if shutil.which(c):
            return shutil.which(c)
    pytest.fail('no host C++ compiler on PATH')


def test_branch_free_window_rule_matches_the_loop(tmp_path):
    src = tmp_path / 'window_rule.cpp'
    exe = tmp_path / 'window_rule'
    src.write_text(DRIVER)
    r = subprocess.run([_cxx(), '-O2', '-std=c++17', f'-I{HEADER_DIR}', str(src), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 mismatches, 0 predicate errors' in r.stdout, r.stdout
