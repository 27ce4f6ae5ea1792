"""The average-linkage (UPGMA) merge table without a GPU: the restatement (tests/average_restatement.py) on hand cases and the
properties DESIGN.md section 9 states for it, a model of the library's parallel rounds against that sequential rule, the host
arithmetic entries (vg_cluster_average_similarity, the shared comparator), the C ABI and Python surface, and the CLI's usage
errors (no device needed for any of it)."""
import pathlib
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import average_restatement as av
import cluster_restatement as cr
import complete_restatement as cl
import linkage_restatement as lr
from vclust_amd import _lib, api

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
NEW_SYMBOLS = ('vg_cluster_average_linkage_graph', 'vg_cluster_average_levels_graph', 'vg_cluster_average_order_selftest')
U9, U8, U6 = 3865470566, 3435973837, 2576980378                 # 0.9, 0.8 and 0.6 in quanta of 2^-32


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


def wrap_cases():
    """candidates whose 64-bit cross products wrap: (S, size_c, size_d, c, d) per entry, neighbours compared"""
    big = (1 << 64) - 1
    rows = [(big, 0xffffffff, 0xffffffff, 0, 1), (big - 1, 0xffffffff, 0xffffffff, 0, 1),      # P = 2^64 - 2^33 + 1
            (1 << 63, 1 << 16, 1 << 16, 2, 3), (1 << 62, 1 << 15, 1 << 16, 2, 3),              # equal fractions, equal ids
            (1 << 62, 1 << 15, 1 << 16, 3, 2), (1 << 62, 1 << 15, 1 << 16, 2, 4),              # (the ids arrive in either order)
            (3 << 40, 3, 1 << 20, 7, 9), (1 << 60, 1 << 20, 1 << 20, 1, 9),                    # equal, the ids decide
            ((1 << 63) + 1, 0x80000000, 0x80000001, 5, 6), (1 << 63, 0x80000000, 0x80000000, 5, 6),
            (6148914691236517205, 3, 1, 0, 1), (12297829382473034410, 3, 2, 0, 1),             # (2^64 - 1) / 3: equal after cross products
            (12297829382473034411, 3, 2, 0, 1), (0, 1, 1, 0, 1), (0, 0xffffffff, 7, 0, 2), (1, 0xffffffff, 0xffffffff, 0, 1)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        s = int(rng.integers(0, 1 << 63)) << int(rng.integers(0, 2))
        rows.append((s, int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32)), int(rng.integers(0, 4)), int(rng.integers(4, 8))))
    want = []
    for x, y in zip(rows, rows[1:]):
        kx = (-Fraction(x[0], x[1] * x[2]), min(x[3], x[4]), max(x[3], x[4]))
        ky = (-Fraction(y[0], y[1] * y[2]), min(y[3], y[4]), max(y[3], y[4]))
        want.append(-1 if kx < ky else 1 if kx > ky else 0)
    return [np.array(col, dtype=np.uint64 if k == 0 else np.uint32) for k, col in enumerate(zip(*rows))], want


def rounds_model(n, e, floor=0.0):
    """The library's parallel rounds in plain Python: every cluster picks the candidate of smallest key in its row, mutual choices
    of sim >= floor and S > 0 merge at once; when a round finds none and records of S == 0 are left (floor 0), they merge one per
    round, smallest (c, d) first.  -> ([(c, d, S, P)] in table order, rounds)"""
    f = av.quantum(floor)
    size = [1] * n
    total = {pair: av.quantum(w) for pair, w in e.items()}
    done, rounds, zero_phase, in_key_order = [], 0, False, None
    while True:
        rounds += 1
        best = {}
        for (c, d), s in total.items():
            for x, y in ((c, d), (d, c)):
                k = (-Fraction(s, size[y]), c, d)                   # inside one row the cluster's own size cancels
                if x not in best or k < best[x][0]:
                    best[x] = (k, y)
        picked = [(c, d) for (c, d) in total if best[c][1] == d and best[d][1] == c]
        if zero_phase:
            picked = [p for p in picked if p == min(total)]
        else:
            picked = [(c, d) for c, d in picked if total[(c, d)] > 0 and total[(c, d)] >= f * size[c] * size[d]]
        if not picked:
            if f == 0 and total and not zero_phase:
                zero_phase, in_key_order = True, len(done)
                continue
            break
        parent = list(range(n))
        for c, d in picked:
            done.append((c, d, total[(c, d)], size[c] * size[d]))
            parent[d] = c
        for c, d in picked:
            size[c] += size[d]
        joined = {}
        for (x, y), v in total.items():
            x, y = parent[x], parent[y]
            if x != y:
                joined[(min(x, y), max(x, y))] = joined.get((min(x, y), max(x, y)), 0) + v
        total = joined
    cut_at = len(done) if in_key_order is None else in_key_order
    head = sorted(done[:cut_at], key=lambda m: (-Fraction(m[2], m[3]), m[0], m[1]))
    return head + done[cut_at:], rounds


def test_restatement_hand_cases():
    # the 4-object path 0.9 0.8 0.9: both ends merge first (the smaller ids first), then the two pairs through the one middle edge,
    # whose 0.8 is shared by four object pairs
    rows = [(0, 1, 0.9), (1, 2, 0.8), (2, 3, 0.9)]
    e = cr.edges(rows)
    assert av.quantum(0.9) == U9 and av.quantum(0.8) == U8 and av.quantum(0.6) == U6 and av.quantum(1.0) == 1 << 32 and av.quantum(-0.0) == 0
    assert av.merges(4, e) == [(0, 1, U9, 1), (2, 3, U9, 1), (0, 2, U8, 4)]
    assert av.linkage(4, rows) == [(0, 1, float(Fraction(U9, 1 << 32)), 2, 0, 1), (2, 3, float(Fraction(U9, 1 << 32)), 2, 2, 3),
                                   (4, 5, float(Fraction(U8, 4 << 32)), 4, 0, 2)]
    assert av.linkage(4, rows)[2][2] == pytest.approx(0.2) and av.linkage(4, rows)[0][2] == pytest.approx(0.9)
    assert av.merges(4, e, 0.3) == [(0, 1, U9, 1), (2, 3, U9, 1)] and av.cluster_ids(4, rows, 0.3) == [0, 0, 2, 2]
    assert av.cluster_ids(4, rows, 0.0, 0.2) == [0, 0, 0, 0] and av.cluster_ids(4, rows, 0.0, 0.21) == [0, 0, 2, 2]
    # a missing pair blocks a merge at the floor that single linkage makes: {0, 1} and 2 average (0.8 + 0) / 2 = 0.4 < 0.7
    rows = [(0, 1, 0.9), (1, 2, 0.8)]
    assert av.cluster_ids(3, rows, 0.7) == [0, 0, 2] and lr.cut(3, lr.forest(3, cr.edges(rows)), 0.7) == [0, 0, 0]
    assert av.merges(3, cr.edges(rows), 0.4) == [(0, 1, U9, 1), (0, 2, U8, 2)]              # 0.4 itself is reached: U8 >= 2 * quantum(0.4)
    # complete linkage splits on the missing pair {1, 2}; the average (0.9 + 0) / 2 = 0.45 passes a floor of 0.4
    rows = [(0, 1, 0.9), (0, 2, 0.9)]
    assert cl.cluster_ids(3, rows) == [0, 0, 2] and av.cluster_ids(3, rows, 0.4) == [0, 0, 0]
    assert av.merges(3, cr.edges(rows), 0.4) == [(0, 1, U9, 1), (0, 2, U9, 2)]
    # the cut at a level is not a rerun at that level: the row 0.6 lies below 0.7 and still counts in the average (0.9 + 0.6) / 2
    rows = [(0, 1, 0.9), (0, 2, 0.9), (1, 2, 0.6)]
    assert av.merges(3, cr.edges(rows), 0.5) == [(0, 1, U9, 1), (0, 2, U9 + U6, 2)]
    assert av.cluster_ids(3, rows, 0.5, 0.7) == [0, 0, 0]
    assert av.cluster_ids(3, [x for x in rows if x[2] >= 0.7], 0.7) == [0, 0, 2]
    # ties: an all-equal triangle merges (0, 1) and then 2; duplicate and reverse rows keep the maximum, self rows are dropped
    assert av.merges(3, cr.edges([(1, 2, 0.5), (0, 2, 0.5), (0, 1, 0.5)])) == [(0, 1, 1 << 31, 1), (0, 2, 1 << 32, 2)]
    rows = [(0, 1, 0.5), (1, 0, 0.9), (0, 1, 0.7), (1, 2, 0.8), (2, 1, 0.6), (3, 3, 1.0)]
    assert av.merges(4, cr.edges(rows)) == [(0, 1, U9, 1), (0, 2, U8, 2)] and av.cluster_ids(4, rows) == [0, 0, 0, 3]
    # no edges; no objects; one object
    assert av.linkage(5, []) == [] and av.cluster_ids(5, []) == [0, 1, 2, 3, 4]
    assert av.linkage(0, []) == [] and av.linkage(1, []) == [] and av.levels(0, [], [0.5]) == [([], [])]


def test_zero_weights_merge_last_and_in_the_sequential_order():
    """A pair without a record has the similarity 0 of a record of S == 0, and turns into a candidate when a merge gives it one: the
    keys of such merges need not rise, and the sequential rule decides.  Here {0, 3} (0.5) merges first; its new record with 1
    has the key (0, 0, 1), below the (0, 1, 2) that 1 and 2 held from the start."""
    e = {(1, 2): 0.0, (1, 3): 0.0, (0, 3): 0.5}
    want = [(0, 3, 1 << 31, 1), (0, 1, 0, 2), (0, 2, 0, 3)]
    assert av.merges(4, e) == want and rounds_model(4, e)[0] == want
    assert av.merges(4, e, 0.1) == want[:1] and rounds_model(4, e, 0.1)[0] == want[:1]
    # (0, 5) and (2, 3) are both mutual choices of S == 0; after (0, 5) the pair (0, 2) precedes (2, 3)
    e = {(0, 5): 0.0, (2, 5): 0.0, (2, 3): 0.0}
    want = [(0, 5, 0, 1), (0, 2, 0, 2), (0, 3, 0, 3)]
    assert av.merges(6, e) == want and rounds_model(6, e)[0] == want


@pytest.mark.parametrize('seed', range(6))
def test_restatement_properties_and_the_round_model(seed):
    """heavy ties (three weights, or one): nested cuts, a monotone table, inside single linkage -- and the parallel rounds of the
    library, modelled in Python, give the table of the sequential rule"""
    rng = np.random.default_rng(seed)
    n = 60
    weights = ([0.5, 0.75, 1.0], [0.7], [0.0, 0.5, 1.0])[seed % 3]
    q, r, w = av.random_graph(rng, n, (90, 240)[seed // 3], weights)
    e = cr.edges(zip(q.tolist(), r.tolist(), w.tolist()))
    single = lr.forest(n, e)
    for floor in (0.0, 0.6):
        m = av.merges(n, e, floor)
        assert rounds_model(n, e, floor)[0] == m, floor
        sims = [Fraction(s, p) for _, _, s, p in m]
        assert all(x >= y for x, y in zip(sims, sims[1:]))                                  # similarity never rises
        tab = av.table(n, m)
        assert all(x[2] >= y[2] for x, y in zip(tab, tab[1:])) and all(a < b for a, b, _, _ in m)
        assert all(s >= av.quantum(floor) * p for _, _, s, p in m)
        previous = None
        for t in (1.0, 0.8, 0.75, 0.6, 0.3, 0.0):
            if t < floor:
                continue
            cid = av.cut(n, m, t)
            members = {}
            for i, c in enumerate(cid):
                members.setdefault(c, []).append(i)
            sl = lr.cut(n, single, floor)
            assert all(len({sl[i] for i in mem}) == 1 for mem in members.values()), t    # inside one single-linkage cluster at the floor
            if previous is not None:                                                       # nested: descending levels only join
                assert all(len({cid[i] for i in mem}) == 1 for mem in previous.values()), t
            previous = members


def test_equal_weight_cliques_are_the_clusters_of_single_and_complete():
    rng = np.random.default_rng(11)
    q, r, w = cl.planted_cliques(rng, 80, 9, lambda g, k: np.full(k, 0.8), 0, lambda g, k: np.zeros(k))
    rows = list(zip(q.tolist(), r.tolist(), w.tolist()))
    e = cr.edges(rows)
    assert av.cluster_ids(80, rows, 0.7) == cl.cluster_ids(80, rows) == lr.cut(80, lr.forest(80, e), 0.7)
    assert rounds_model(80, e, 0.7)[0] == av.merges(80, e, 0.7)


def test_similarity_is_the_nearest_double():
    sim = api.cluster_average_similarity
    cases = [(0, 1), (0, (1 << 64) - 1), (1, 1), (1 << 32, 1), (U9, 1), (U8, 4), (U9 + U6, 2), (1, (1 << 64) - 1), ((1 << 64) - 1, 1),
             ((1 << 64) - 1, (1 << 64) - 1), ((1 << 64) - 1, (1 << 62) - 1), ((1 << 53) + 1, 1), ((1 << 53) + 1, 3), ((1 << 53) - 1, (1 << 53) + 1),
             ((1 << 53) + 1, (1 << 53) - 1), ((1 << 54) + 2, 1), ((1 << 54) + 6, 1),              # exact ties: to even, down and up
             ((1 << 54) + 2, 1 << 10), ((1 << 54) + 6, 1 << 31), ((1 << 54) + 3, 1), ((1 << 63) + (1 << 10), 1), ((1 << 63) + (3 << 10), 1),
             ((1 << 63) + (1 << 10) + 1, 1), (3 * ((1 << 54) + 2), 3), (5 * ((1 << 54) + 6), 5 << 20)]
    rng = np.random.default_rng(2)
    for _ in range(2000):
        cases.append((int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) >> int(rng.integers(0, 64)),
                      (int(rng.integers(0, 1 << 63)) * 2 + 1 >> int(rng.integers(0, 64))) or 1))
    for s, p in cases:
        assert sim(s, p) == float(Fraction(s, p << 32)), (s, p)
    assert sim(1 << 32, 1) == 1.0 and sim(0, 5) == 0.0 and not np.signbit(sim(0, 5))
    assert sim((1 << 54) + 2, 1) == float(1 << 22) and sim((1 << 54) + 6, 1) == float((1 << 54) + 8) / 2**32


def test_host_comparator_on_products_that_wrap():
    cols, want = wrap_cases()
    assert api.cluster_average_order_selftest(*cols).tolist() == want
    assert sorted(set(want)) == [-1, 0, 1]
    # a 64-bit product gets these wrong: S1 * P2 and S2 * P1 agree modulo 2^64
    assert api.cluster_average_order_selftest([1 << 63, 1 << 62], [1 << 16, 1 << 15], [1 << 16, 1 << 16], [2, 2], [3, 3]).tolist() == [0]
    assert api.cluster_average_order_selftest([(1 << 63) + 1, 1 << 63], [2, 4], [1, 1], [0, 0], [1, 1]).tolist() == [-1]
    assert len(api.cluster_average_order_selftest([], [], [], [], [])) == 0 and len(api.cluster_average_order_selftest([1], [1], [1], [0], [1])) == 0


def test_new_symbols_exported_declared_and_pinned():
    lib = _lib.load()
    header = (ROOT / 'include' / 'vclust_gpu.h').read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header, name
    assert hasattr(lib, 'vg_cluster_average_similarity') and 'double vg_cluster_average_similarity(' in header
    assert 'VG_CLUSTER_COMPLETE = 4' in header and 'VG_CLUSTER_AVERAGE = 5' in header
    assert len(_lib.SYMBOLS['vg_cluster_average_linkage_graph'][1]) == 16 and len(_lib.SYMBOLS['vg_cluster_average_levels_graph'][1]) == 11
    assert _lib.HIERARCHY_ALGORITHMS == {'single': 0, 'complete': 4, 'average': 5}
    assert _lib.LINKAGE_ALGORITHMS == {'single': 0, 'complete': 4}
    assert _lib.CLUSTER_ALGORITHMS == {'single': 0, 'cd-hit': 1, 'uclust': 2, 'set-cover': 3}
    assert api.AVERAGE_LINKAGE_DTYPE.names == api.LINKAGE_DTYPE.names + ('sum', 'pairs')


def test_argument_errors_need_no_device(out_dir, tmp_path):
    calls = (lambda n, q, r, w: api.cluster_average_linkage_graph(n, q, r, w, 0.5),
             lambda n, q, r, w: api.cluster_average_levels_graph(n, q, r, w, [0.6], 0.5))
    for call in calls:
        for bad, word in ((1.5, 'outside [0, 1]'), (-0.1, 'outside [0, 1]'), (float('nan'), 'NaN'), (float('inf'), 'outside [0, 1]')):
            with pytest.raises(_lib.VclustGpuError) as e:
                call(3, [0, 1], [1, 2], [0.9, bad])
            assert e.value.code == -1 and word in str(e.value), bad
        with pytest.raises(_lib.VclustGpuError) as e:
            call(3, [0], [3], [1.0])
        assert e.value.code == -1 and 'outside' in str(e.value)
        with pytest.raises(_lib.VclustGpuError) as e:
            call(1 << 31, [], [], [])
        assert e.value.code == -6
    for floor in (-0.1, 1.5, float('nan')):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster_average_linkage_graph(3, [0], [1], [0.9], floor)
        assert e.value.code == -1 and 'floor' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_average_levels_graph(3, [0, 1], [1, 2], [0.9, 0.8], [0.9, 0.4], 0.5)       # a level below the floor
    assert e.value.code == -1 and 'below' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_average_levels_graph(3, [0], [1], [0.5], [float('nan')])
    assert e.value.code == -1
    with pytest.raises(_lib.VclustGpuError) as e:                                               # no floor argument: not this call's algorithm
        _lib.check(_lib.load().vg_cluster_graph(0, None, None, None, 0, 5, None, None, None))
    assert e.value.code == -1 and 'unknown algorithm' in str(e.value)
    with pytest.raises(ValueError):
        api.cluster_graph(2, [0], [1], [1.0], 'average')
    table, stats = api.cluster_average_linkage_graph(0, [], [], [])
    assert len(table) == 0 and table.dtype == api.AVERAGE_LINKAGE_DTYPE and stats == dict(rounds=0, n_edges=0, n_merges=0)
    label, rep, stats = api.cluster_average_levels_graph(0, [], [], [], [0.9, 0.5])
    assert label.shape == rep.shape == (2, 0) and stats['n_merges'] == 0
    files = (out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster(*files, algorithm='average', tani=0.95, levels=[0.9])
    assert e.value.code == -1 and 'below' in str(e.value) and not (tmp_path / 'c.tsv').exists()


def test_without_device_fails_loudly(out_dir, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    for call in (lambda: api.cluster_average_linkage_graph(3, [0, 1], [1, 2], [0.9, 0.8]),
                 lambda: api.cluster_average_levels_graph(3, [0, 1], [1, 2], [0.9, 0.8], [0.85]),
                 lambda: api.cluster_average_order_selftest([1, 2], [1, 1], [1, 1], [0, 0], [1, 1], on_device=True),
                 lambda: api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv', algorithm='average', tani=0.7)):
        with pytest.raises(_lib.VclustGpuError) as e:
            call()
        assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    assert not (tmp_path / 'c.tsv').exists()


def test_cli_usage_errors_then_the_library(out_dir, tmp_path):
    args = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv']
    p = run(*args, '--tani', '0.7', '--levels', '0.9', '--algorithm', 'cd-hit')
    assert p.returncode == 2 and all(f'--algorithm {x}' in p.stderr for x in ('single', 'complete', 'average')), p.stderr
    p = run(*args, '--algorithm', 'average')
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr, p.stderr
    p = run(*args, '--algorithm', 'average', '--levels', '0.9')
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr, p.stderr
    p = run(*args, '--tani', '0.95', '--levels', '0.9', '--algorithm', 'average')
    assert p.returncode == 2 and 'below --tani 0.95' in p.stderr, p.stderr
    assert not (tmp_path / 'c.tsv').exists()
    if api.device_count() > 0:
        return                                                                                  # (tests/test_gpu_average.py runs it there)
    # a plain `--algorithm average` reaches the library and never asks for bin/clusty, which has no such algorithm
    assert not (ROOT / 'bin' / 'clusty').exists()
    p = run(*args, '--tani', '0.95', '--algorithm', 'average')
    assert p.returncode == 1 and 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'bin/clusty' not in p.stderr, p.stderr
    assert '--algorithm average' in p.stderr and not (tmp_path / 'c.tsv').exists()             # the Running: line names it
