"""The average-linkage (UPGMA) merge table and its cuts on the MI355X (vg_cluster_average_linkage_graph /
vg_cluster_average_levels_graph / vg_cluster_linkage and vg_cluster with algorithm average) against the sequential restatement
(tests/average_restatement.py): every case compares tables, sums, labels or bytes for exact equality."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import average_restatement as av
import cluster_restatement as cr
import complete_restatement as cl
import linkage_restatement as lr
from test_average_cpu import U6, U8, U9, wrap_cases

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'


def run(*args, timeout=300):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


def _records(table):
    return [(int(t['object_a']), int(t['object_b']), int(t['sum']), int(t['pairs'])) for t in table]


def _as_rows(table):
    return [(int(t['node_a']), int(t['node_b']), float(t['similarity']), int(t['size']), int(t['object_a']), int(t['object_b']))
            for t in table]


def _check(api, n, q, r, w, floor=0.0, lv=()):
    """merge records (ids, S, P), table and cuts are exactly the restatement's"""
    q, r, w = np.asarray(q, np.uint32), np.asarray(r, np.uint32), np.asarray(w, np.float64)
    e = cr.edges(zip(q.tolist(), r.tolist(), w.tolist()))
    m = av.merges(n, e, floor)
    table, stats = api.cluster_average_linkage_graph(n, q, r, w, floor)
    assert _records(table) == m
    assert _as_rows(table) == av.table(n, m)
    assert stats['n_merges'] == len(m) and stats['n_edges'] == len(e) and stats['rounds'] >= (1 if e else 0)
    lv = [t for t in lv if t >= floor]
    label, rep, st2 = api.cluster_average_levels_graph(n, q, r, w, lv + [floor], floor)
    assert label.shape == rep.shape == (len(lv) + 1, n) and st2 == stats
    for k, t in enumerate(lv + [floor]):
        want_label, want_rep = cr.labels(av.cut(n, m, t))
        assert rep[k].tolist() == want_rep and label[k].tolist() == want_label, t
    assert rep[len(lv)].tolist() == cr.labels(av.cut(n, m, 0.0))[1]                        # the floor cut joins every merge
    return table, stats, m


def test_no_rows_self_rows_one_edge(api):
    table, stats, _ = _check(api, 5, [], [], [], 0.0, [0.5])
    assert len(table) == 0 and stats == dict(rounds=0, n_edges=0, n_merges=0)
    table, stats = api.cluster_average_linkage_graph(1, [], [], [])
    assert len(table) == 0 and stats == dict(rounds=0, n_edges=0, n_merges=0)
    label, rep, _ = api.cluster_average_levels_graph(1, [0], [0], [1.0], [0.5])
    assert label.tolist() == [[0]] and rep.tolist() == [[0]]
    table, stats, _ = _check(api, 5, [3, 3], [3, 3], [1.0, 0.5], 0.0, [0.5])                 # self rows only
    assert len(table) == 0 and stats['rounds'] == 0
    table, stats, _ = _check(api, 3, [2], [0], [0.9], 0.5, [0.9, 0.95])                      # one edge
    assert _records(table) == [(0, 2, U9, 1)] and stats == dict(rounds=2, n_edges=1, n_merges=1)
    table, stats, _ = _check(api, 3, [2], [0], [0.9], 0.95)                                  # ... below the floor
    assert len(table) == 0 and stats == dict(rounds=1, n_edges=1, n_merges=0)


def test_hand_cases(api):
    path = ([0, 1, 2], [1, 2, 3], [0.9, 0.8, 0.9])
    table, stats, _ = _check(api, 4, *path, 0.0, [0.9, 0.21, 0.2])
    assert _records(table) == [(0, 1, U9, 1), (2, 3, U9, 1), (0, 2, U8, 4)] and stats['rounds'] == 3
    assert _as_rows(table) == [(0, 1, U9 / 2**32, 2, 0, 1), (2, 3, U9 / 2**32, 2, 2, 3), (4, 5, U8 / 2**34, 4, 0, 2)]
    table, stats, _ = _check(api, 4, *path, 0.3, [0.9])
    assert _records(table) == [(0, 1, U9, 1), (2, 3, U9, 1)] and stats['rounds'] == 2
    table, _, _ = _check(api, 3, [0, 1], [1, 2], [0.9, 0.8], 0.7)                            # the missing pair blocks what single joins
    assert _records(table) == [(0, 1, U9, 1)]
    assert api.cluster_levels(3, [0, 1], [1, 2], [0.9, 0.8], [0.7])[1].tolist() == [[0, 0, 0]]
    table, _, _ = _check(api, 3, [0, 1], [1, 2], [0.9, 0.8], 0.4)
    assert _records(table) == [(0, 1, U9, 1), (0, 2, U8, 2)]
    table, _, _ = _check(api, 3, [0, 0], [1, 2], [0.9, 0.9], 0.4)                            # complete linkage splits here
    assert _records(table) == [(0, 1, U9, 1), (0, 2, U9, 2)]
    assert api.cluster_graph(3, [0, 0], [1, 2], [0.9, 0.9], 'complete')[1].tolist() == [0, 0, 2]
    tri = ([0, 0, 1], [1, 2, 2], [0.9, 0.9, 0.6])                                            # the cut at a level is not a rerun
    table, _, _ = _check(api, 3, *tri, 0.5, [0.7])
    assert _records(table) == [(0, 1, U9, 1), (0, 2, U9 + U6, 2)]
    assert api.cluster_average_levels_graph(3, *tri, [0.7], 0.5)[1].tolist() == [[0, 0, 0]]
    assert api.cluster_average_levels_graph(3, [0, 0], [1, 2], [0.9, 0.9], [0.7], 0.7)[1].tolist() == [[0, 0, 2]]
    # duplicate and reverse rows with different weights keep the maximum, self rows are dropped, -0.0 is 0
    table, _, _ = _check(api, 4, [0, 1, 0, 1, 2, 3], [1, 0, 1, 2, 1, 3], [0.5, 0.9, 0.7, 0.8, 0.6, 1.0], 0.0, [0.9, 0.4])
    assert _records(table) == [(0, 1, U9, 1), (0, 2, U8, 2)]
    table, _, _ = _check(api, 3, [0, 1, 1], [1, 0, 2], [-0.0, 0.0, 1.0])
    assert _records(table) == [(1, 2, 1 << 32, 1), (0, 1, 0, 2)] and not np.signbit(table['similarity']).any()


def test_zero_weights_follow_the_sequential_rule(api):
    table, stats, _ = _check(api, 4, [1, 1, 0], [2, 3, 3], [0.0, 0.0, 0.5], 0.0, [0.5])
    assert _records(table) == [(0, 3, 1 << 31, 1), (0, 1, 0, 2), (0, 2, 0, 3)] and stats['rounds'] == 5
    table, _, _ = _check(api, 6, [0, 2, 2], [5, 5, 3], [0.0, 0.0, 0.0])
    assert _records(table) == [(0, 5, 0, 1), (0, 2, 0, 2), (0, 3, 0, 3)]
    _check(api, 4, [1, 1, 0], [2, 3, 3], [0.0, 0.0, 0.5], 0.25)


@pytest.mark.parametrize('degree', [1, 15, 16, 17, 33])
def test_rows_around_the_lane_count(api, degree):
    """a star of `degree` neighbours plus random extra edges: rows of 1, 15, 16, 17 and 33 records (ROW_LANES = 16)"""
    rng = np.random.default_rng(degree)
    n = degree + 8
    q = np.concatenate([np.zeros(degree, np.uint32), rng.integers(1, n, 12).astype(np.uint32)])
    r = np.concatenate([np.arange(1, degree + 1, dtype=np.uint32), rng.integers(1, n, 12).astype(np.uint32)])
    w = rng.choice([0.5, 0.75, 1.0], len(q))
    w[rng.integers(0, degree)] = 1.0                                # the star's best record sits in any lane
    _check(api, n, q, r, w, 0.0, [0.75])
    _, stats = api.cluster_average_linkage_graph(n, q[:degree], r[:degree], np.full(degree, 0.5))
    assert stats['n_edges'] == degree and stats['n_merges'] == degree


def test_all_weights_equal(api):
    """ties decide everything: the table equals the restatement row for row"""
    q, r = np.triu_indices(40, 1)
    table, stats, _ = _check(api, 40, q, r, np.full(len(q), 0.7), 0.0, [0.7, 0.71])
    assert stats['n_merges'] == 39 and set(table['similarity'].tolist()) == {av.similarity(av.quantum(0.7), 1)}
    rng = np.random.default_rng(7)
    q, r, w = av.random_graph(rng, 60, 150, [0.7])
    _check(api, 60, q, r, w, 0.0, [0.7, 0.3])
    _check(api, 60, q, r, w, 0.6)


@pytest.mark.parametrize('seed', range(20))
def test_random_graphs_with_tied_weights(api, seed):
    """200 objects, weights from {0.5, 0.75, 1.0}, three densities, floors 0, 0.6 and 0.9"""
    rng = np.random.default_rng(seed)
    for rows in (150, 400, 1200):
        q, r, w = av.random_graph(rng, 200, rows, [0.5, 0.75, 1.0])
        floor = (0.0, 0.6, 0.9)[(seed + rows) % 3]
        _check(api, 200, q, r, w, floor, [1.0, 0.75, 0.6])


def test_levels_in_any_order_and_the_four_properties(api):
    rng = np.random.default_rng(23)
    n = 200
    q, r, w = av.random_graph(rng, n, 500, [0.5, 0.75, 1.0])
    m = av.merges(n, cr.edges(zip(q.tolist(), r.tolist(), w.tolist())), 0.5)
    table, _ = api.cluster_average_linkage_graph(n, q, r, w, 0.5)
    assert _records(table) == m and np.all(np.diff(table['similarity']) <= 0)                # similarity never rises
    for lv in ([0.5, 0.6, 0.75, 1.0], [1.0, 0.75, 0.6, 0.5], [0.75, 0.6, 0.75, 0.75, 1.0]):   # ascending, descending, repeated
        label, rep, _ = api.cluster_average_levels_graph(n, q, r, w, lv, 0.5)
        for k, t in enumerate(lv):
            assert (label[k].tolist(), rep[k].tolist()) == cr.labels(av.cut(n, m, t)), (lv, t)
    label, rep, _ = api.cluster_average_levels_graph(n, q, r, w, [1.0, 0.75, 0.6, 0.5], 0.5)
    for hi, lo in ((0, 1), (1, 2), (2, 3)):                                                   # nested: descending levels only join
        assert all(len(set(rep[lo][rep[hi] == c].tolist())) == 1 for c in set(rep[hi].tolist()))
    single = api.cluster_levels(n, q, r, w, [0.5])[1][0]                                      # inside single linkage at the floor
    assert all(len(set(single[rep[3] == c].tolist())) == 1 for c in set(rep[3].tolist()))
    assert len(set(rep[3].tolist())) > len(set(single.tolist()))
    # every component a clique of equal weights: the floor clusters of single, complete and average are the same
    q, r, w = cl.planted_cliques(rng, 120, 12, lambda g, k: np.full(k, 0.8), 0, lambda g, k: np.zeros(k))
    a_rep = api.cluster_average_levels_graph(120, q, r, w, [0.7], 0.7)[1][0]
    assert np.array_equal(a_rep, api.cluster_graph(120, q, r, w, 'single')[1]) and np.array_equal(a_rep, api.cluster_graph(120, q, r, w, 'complete')[1])


def test_chain_of_one_merge_per_round(api):
    """a clique with w(i, j) = 1 - 0.001 * max(i, j): every object prefers the grown cluster 0, which takes the smallest one --
    object k joins {0 .. k-1} in round k, and the last round finds nothing"""
    n = 64
    q, r = np.triu_indices(n, 1)
    table, stats, m = _check(api, n, q, r, 1.0 - 0.001 * np.maximum(q, r), 0.0, [0.95])
    assert stats['n_merges'] == n - 1 and stats['rounds'] == stats['n_merges'] + 1
    assert table['object_a'].tolist() == [0] * (n - 1) and table['object_b'].tolist() == list(range(1, n))
    assert [p for _, _, _, p in m] == list(range(1, n))


def test_device_comparator_on_products_that_wrap(api):
    cols, want = wrap_cases()
    assert api.cluster_average_order_selftest(*cols, on_device=True).tolist() == want
    assert api.cluster_average_order_selftest(*cols, on_device=False).tolist() == want


def test_5000_objects_more_than_one_workgroup(api):
    rng = np.random.default_rng(17)
    n = 5000
    q, r, w = cl.planted_cliques(rng, n, 24, lambda g, k: g.choice([0.8, 0.9, 1.0], k), 3000, lambda g, k: g.choice([0.5, 0.9], k))
    table, stats = api.cluster_average_linkage_graph(n, q, r, w, 0.6)
    again, stats2 = api.cluster_average_linkage_graph(n, q, r, w, 0.6)
    assert table.tobytes() == again.tobytes() and stats == stats2
    assert stats['n_edges'] > 30000 and stats['rounds'] < stats['n_merges'] and np.all(np.diff(table['similarity']) <= 0)
    e = cr.edges(zip(q.tolist(), r.tolist(), w.tolist()))
    total = {}                                                      # every record's (S, P) from the members of its two clusters
    members = {i: [i] for i in range(n)}
    for c, d, s, p in _records(table):
        assert p == len(members[c]) * len(members[d]) and c < d
        assert s == sum(av.quantum(e[(min(a, b), max(a, b))]) for a in members[c] for b in members[d] if (min(a, b), max(a, b)) in e)
        assert s >= av.quantum(0.6) * p
        members[c] += members.pop(d)


@pytest.mark.parametrize('repr_', [False, True])
def test_cli_golden_example(api, out_dir, tmp_path, repr_):
    files = ['-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv']
    extra = ['-r'] if repr_ else []
    out, link = tmp_path / 'c.tsv', tmp_path / 'l.tsv'
    p = run('cluster', *files, '-o', out, '--algorithm', 'average', '--tani', '0.7', '--levels', '0.95', '0.9', '--out-linkage', link,
            '-v', '0', *extra)
    assert p.returncode == 0 and p.stderr == '', p.stderr
    want, want_link = av.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'tani', [0.95, 0.9], representatives=repr_, tani=0.7)
    assert out.read_bytes() == want and link.read_bytes() == want_link
    cols = [ln.split('\t') for ln in out.read_text().split('\n') if ln]
    assert cols[0] == ['object', 'cluster', 'tani_0.95', 'tani_0.9']
    # a plain `--algorithm average`: the floor cut of the hierarchy that stops at 0.95, in the library
    plain = tmp_path / 'plain.tsv'
    p = run('cluster', *files, '-o', plain, '--algorithm', 'average', '--tani', '0.95', *extra)
    assert p.returncode == 0 and 'Running' in p.stderr and '--algorithm average' in p.stderr and 'clusty' not in p.stderr, p.stderr
    assert plain.read_bytes() == av.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'tani', [], representatives=repr_, tani=0.95)[0]
    assert len({ln.split('\t')[1] for ln in plain.read_text().split('\n')[1:] if ln}) > 1
