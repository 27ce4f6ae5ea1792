"""The two references of the coverage map held to each other, without a device: the event sweep (tests/cover_sweep.py) must return
what the mask restatement (tests/cover_restatement.py) returns -- records, segments, run counts -- on every input that
tests/test_cover_cpu.py and tests/test_gpu_cover.py construct, on the golden table, and on a few hundred small random inputs made to
hit the sweep's own edges: rows that touch, nest and repeat, self rows, rows that end at len - 1, lengths 0 and 1.  The sweep then
stands in for the restatement in tests/test_gpu_cover_sizes.py, at sizes and lengths the masks cannot hold."""
import numpy as np
import pytest

import cluster_stats_restatement as cs
import cover_restatement as cv
import cover_sweep as sw
import test_cover_cpu
import test_gpu_cover
import test_gpu_cover_sizes


def _same(lengths, rows, label=None, n_groups=None):
    arrays = {}
    want = cv.cover(lengths, rows, label, n_groups)
    got = sw.cover(lengths, rows, label, n_groups, arrays=arrays)
    assert got[2] == want[2]
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert sw.cover(lengths, rows, label, n_groups) == got                # (the arrays are a by-product)
    # the by-product: the kept rows in key order, one entry per breakpoint, depths that end every object at zero
    assert len(arrays['rows']) == want[2]['rows_kept'] and arrays['rows'] == sorted(arrays['rows'])
    assert len(arrays['breakpoints']) == len(arrays['depths']) == want[2]['breakpoints']
    assert arrays['breakpoints'] == sorted(set(arrays['breakpoints']))
    last = {o: d for (o, _), d in zip(arrays['breakpoints'], arrays['depths'])}
    assert all(d == (0, 0) for d in last.values())


@pytest.mark.parametrize('seed,n,density,groups', test_cover_cpu.CASES)
def test_inputs_of_the_cpu_test(seed, n, density, groups):
    rng = np.random.default_rng(seed)
    lengths, rows, label = test_cover_cpu.random_case(rng, n, 300, n * density, groups)
    _same(lengths, rows, label, groups or None)


def test_inputs_of_the_gpu_test():
    cases = test_gpu_cover.constructed_inputs()
    assert len(cases) == 17
    for lengths, rows, label, n_groups in cases:
        _same(lengths, rows, label, n_groups)


def test_golden_table(golden_dir):
    out = golden_dir / 'output'
    ids, lengths = cv.read_ids(out / 'ani.ids.tsv')
    rows = cv.read_aln(out / 'ani.aln.tsv', ids, lengths)
    names, label, text = cs.read_clusters(out / 'clusters.tsv', ids)
    _same(lengths, rows)
    _same(lengths, rows, label[0], len(text[0]))
    _same(lengths, rows[:1500], label[0], len(text[0]))


def test_key_width_inputs_the_masks_can_hold():
    """the power-of-two lengths and an object count above 2^16 of tests/test_gpu_cover_sizes.py (not its lengths near 2^31; the
    two object counts differ in a key width of the device only, so one of them serves here)"""
    for P in (1024, 2 ** 20):
        for lengths, rows in test_gpu_cover_sizes.power_of_two_cases(P):
            _same(lengths, rows)
            if P == 1024:
                _same(lengths, rows, [0, 1, 0], 2)
    lengths, rows = test_gpu_cover_sizes.object_count_input(65537, False)
    _same(lengths, rows, [k % 2 for k in range(65537)], 2)


def small_case(rng):
    """lengths 0..60, up to 6 partners; rows drawn so that touching, nested and repeated rows, self rows and rows that end at
    len - 1 or start at 0 are all common"""
    n = int(rng.integers(1, 8))
    lengths = [int(x) for x in rng.integers(0, 61, n)]
    if rng.integers(0, 4) == 0:
        lengths[int(rng.integers(0, n))] = int(rng.integers(0, 2))          # a length of 0 or 1
    live = [i for i in range(n) if lengths[i] > 0]
    rows = []
    for _ in range(int(rng.integers(0, 40)) if live else 0):
        q = int(rng.choice(live))
        L = lengths[q]
        kind = int(rng.integers(0, 8))
        mine = [t for t in rows if t[0] == q]
        if kind == 0 and mine:                          # touches an earlier row of the same pair, or of another partner
            _, r, s, e = mine[int(rng.integers(0, len(mine)))]
            if e + 1 < L:
                rows.append((q, r if rng.integers(0, 2) else int(rng.integers(0, n)), e + 1, int(rng.integers(e + 1, L))))
                continue
        if kind == 1 and mine:                          # nested in an earlier row, or that row again
            _, r, s, e = mine[int(rng.integers(0, len(mine)))]
            s2 = int(rng.integers(s, e + 1))
            rows.append((q, r, s2, int(rng.integers(s2, e + 1))) if rng.integers(0, 3) else (q, r, s, e))
            continue
        s = 0 if kind == 2 else int(rng.integers(0, L))
        e = L - 1 if kind == 3 else int(rng.integers(s, L))
        r = q if kind == 4 else int(rng.integers(0, n))
        rows.append((q, r, s, e))
    groups = int(rng.integers(0, 4))
    label = [int(x) for x in rng.integers(0, groups, n)] if groups else None
    return lengths, rows, label, groups or None


@pytest.mark.parametrize('block', range(4))
def test_small_random_inputs(block):
    rng = np.random.default_rng(1000 + block)
    seen = dict(touch=0, self_row=0, at_end=0, nested=0, grouped=0, plain=0, empty=0)
    for _ in range(100):
        lengths, rows, label, n_groups = small_case(rng)
        _same(lengths, rows, label, n_groups)
        seen['grouped' if label else 'plain'] += 1
        seen['empty'] += 0 in lengths
        for q, r, s, e in rows:
            seen['self_row'] += q == r
            seen['at_end'] += e == lengths[q] - 1
            seen['touch'] += any(t[0] == q and t[1] == r and t[3] + 1 == s for t in rows)
            seen['nested'] += any(t[0] == q and t[1] == r and t[2] <= s and e <= t[3] and (t[2], t[3]) != (s, e) for t in rows)
    assert all(v >= 10 for v in seen.values()), seen
