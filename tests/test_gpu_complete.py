"""The complete-linkage merge table and its cuts on the MI355X (vg_cluster_complete_linkage_graph /
vg_cluster_complete_levels_graph / vg_cluster_linkage and vg_cluster_graph with algorithm complete) against the sequential
restatement (tests/complete_restatement.py): every case compares tables, labels or bytes for exact equality."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import average_restatement as av
import cluster_restatement as cr
import complete_restatement as cl
import linkage_restatement as lr

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


@pytest.fixture(scope='module')
def graph300():
    """300 objects: planted cliques of 2-40 members, three tied weights, noise edges, rows duplicated and reversed"""
    rng = np.random.default_rng(5)
    q, r, w = cl.planted_cliques(rng, 300, 40, lambda g, k: g.choice([0.75, 0.85, 0.95], k), 200, lambda g, k: g.choice([0.7, 0.85], k))
    sel = rng.random(len(q)) < 0.3                   # reverse copies with another weight: the maximum counts
    q, r, w = np.concatenate([q, r[sel]]), np.concatenate([r, q[sel]]), np.concatenate([w, rng.choice([0.7, 0.95], int(sel.sum()))])
    merges = cl.merges(300, cr.edges(zip(q.tolist(), r.tolist(), w.tolist())))
    return q, r, w, merges


def _as_rows(table):
    return [(int(t['node_a']), int(t['node_b']), float(t['similarity']), int(t['size']), int(t['object_a']), int(t['object_b']))
            for t in table]


def _check(api, n, q, r, w, lv, merges=None):
    """table, cuts and the floor clustering are exactly the restatement's; each cut is also the floor clustering of the rows at
    that level"""
    q, r, w = np.asarray(q, np.uint32), np.asarray(r, np.uint32), np.asarray(w, np.float64)
    e = cr.edges(zip(q.tolist(), r.tolist(), w.tolist()))
    if merges is None:
        merges = cl.merges(n, e)
    table, stats = api.cluster_complete_linkage_graph(n, q, r, w)
    assert _as_rows(table) == lr.table(n, merges)
    assert table['similarity'].tobytes() == np.array([m[2] for m in merges], np.float64).tobytes()      # bit for bit, -0.0 is +0.0
    assert stats['n_merges'] == len(merges) and stats['n_edges'] == len(e) and stats['rounds'] >= (1 if e else 0)
    label, rep, st2 = api.cluster_complete_levels_graph(n, q, r, w, lv)
    assert label.shape == rep.shape == (len(lv), n) and st2 == stats
    for k, t in enumerate(lv):
        want_label, want_rep = cr.labels(lr.cut(n, merges, t))
        assert rep[k].tolist() == want_rep and label[k].tolist() == want_label, t
        sel = w >= t
        l1, r1, _ = api.cluster_graph(n, q[sel], r[sel], w[sel], 'complete')
        assert np.array_equal(l1, label[k]) and np.array_equal(r1, rep[k]), t
    want_label, want_rep = cr.labels(lr.cut(n, merges, float('-inf')))
    l0, r0, st0 = api.cluster_graph(n, q, r, w, 'complete')
    assert l0.tolist() == want_label and r0.tolist() == want_rep
    assert st0 == dict(rounds=stats['rounds'], sweep_objects=0, n_edges=len(e))
    return table, stats


def test_hand_cases(api):
    table, stats = _check(api, 3, [0, 1], [1, 2], [0.9, 0.8], [0.9, 0.8, 0.0])                  # path: 2 stays alone
    assert _as_rows(table) == [(0, 1, 0.9, 2, 0, 1)] and stats['rounds'] == 2
    table, _ = _check(api, 3, [1, 0, 0], [2, 2, 1], [0.9, 0.9, 0.9], [0.9, 0.95])                # tied triangle
    assert _as_rows(table) == [(0, 1, 0.9, 2, 0, 1), (2, 3, 0.9, 3, 1, 2)]
    table, _ = _check(api, 4, [0, 0, 0, 1, 1], [1, 2, 3, 2, 3], [0.9, 0.8, 0.7, 0.85, 0.75], [0.8, 0.7])     # K4 without {2, 3}
    assert _as_rows(table) == [(0, 1, 0.9, 2, 0, 1), (2, 4, 0.8, 3, 0, 2)]
    table, _ = _check(api, 4, [0, 0, 0, 1, 1], [1, 2, 3, 2, 3], [0.9, 0.7, 0.8, 0.75, 0.85], [0.8])
    assert _as_rows(table) == [(0, 1, 0.9, 2, 0, 1), (3, 4, 0.8, 3, 0, 3)]
    table, stats = _check(api, 5, [], [], [], [0.5])                                             # no rows
    assert len(table) == 0 and stats == dict(rounds=0, n_edges=0, n_merges=0)
    table, stats = api.cluster_complete_linkage_graph(1, [], [], [])
    assert len(table) == 0 and stats == dict(rounds=0, n_edges=0, n_merges=0)
    label, rep, _ = api.cluster_complete_levels_graph(1, [0], [0], [1.0], [0.5])
    assert label.tolist() == [[0]] and rep.tolist() == [[0]]
    table, _ = _check(api, 5, [3, 3], [3, 3], [1.0, 0.5], [0.5])                                 # self rows only
    assert len(table) == 0
    # duplicate and reverse rows keep the maximum, self rows are dropped, -0.0 is +0.0
    table, _ = _check(api, 3, [0, 1, 1, 2, 0, 2], [1, 0, 2, 2, 2, 0], [-0.0, 0.0, 0.0, 1.0, -0.0, -1.0], [0.0, 0.5])
    assert _as_rows(table) == [(0, 1, 0.0, 2, 0, 1), (2, 3, 0.0, 3, 1, 2)] and not np.signbit(table['similarity']).any()
    table, _ = _check(api, 4, [0, 1, 0, 1, 2, 0, 3], [1, 0, 1, 2, 1, 2, 3], [0.5, 0.9, 0.7, 0.95, 0.6, 0.8, 1.0], [0.95, 0.8, 0.95])
    assert _as_rows(table) == [(1, 2, 0.95, 2, 1, 2), (0, 4, 0.8, 3, 0, 2)]


def test_two_mutual_pairs_need_all_four_cross_pairs(api):
    """{0, 1} and {2, 3} merge in the same round; the two merged clusters then join only if all four cross pairs are edges"""
    q, r = [0, 2, 0, 0, 1, 1], [1, 3, 2, 3, 2, 3]
    w = [0.95, 0.9, 0.8, 0.6, 0.7, 0.75]
    table, stats = _check(api, 4, q, r, w, [0.9, 0.6])
    assert _as_rows(table) == [(0, 1, 0.95, 2, 0, 1), (2, 3, 0.9, 2, 2, 3), (4, 5, 0.6, 4, 0, 3)] and stats['rounds'] == 3
    for drop in range(2, 6):                                                                     # any one cross pair removed
        keep = [k for k in range(6) if k != drop]
        table, stats = _check(api, 4, [q[k] for k in keep], [r[k] for k in keep], [w[k] for k in keep], [0.9, 0.6])
        assert _as_rows(table) == [(0, 1, 0.95, 2, 0, 1), (2, 3, 0.9, 2, 2, 3)] and stats['rounds'] == 2, drop


def test_clique_of_200_merges_once_per_round(api):
    """w(i, j) = 1 - 0.001 * max(i, j): object k joins {0 .. k-1} in round k -- 199 rounds of one merge and a contraction each"""
    n = 200
    q, r = np.triu_indices(n, 1)
    w = 1.0 - 0.001 * np.maximum(q, r)
    table, stats = _check(api, n, q, r, w, [0.95, 0.9, 0.85])
    assert stats['n_merges'] == n - 1 and stats['rounds'] == n and table['size'][-1] == n
    assert table['object_a'].tolist() == list(range(n - 1)) and table['object_b'].tolist() == list(range(1, n))      # the worst pair: (k - 1, k)


@pytest.mark.parametrize('degree', [1, 15, 16, 17, 33])
def test_rows_around_the_lane_count(api, degree):
    """a clique of `degree` + 1 objects with distinct weights plus random extra rows: rows of 1, 15, 16, 17 and 33 records
    (ROW_LANES = 16) that shrink through the contractions; 4, 15, 17, 17 and 34 merges by the restatement"""
    rng = np.random.default_rng(degree)
    n = degree + 9
    q, r = np.triu_indices(degree + 1, 1)
    w = 0.5 + 1e-4 * rng.permutation(len(q))
    q = np.concatenate([q, rng.integers(0, n, 12)]).astype(np.uint32)
    r = np.concatenate([r, rng.integers(0, n, 12)]).astype(np.uint32)
    w = np.concatenate([w, rng.choice([0.5, 0.75, 1.0], 12)])
    _, stats = _check(api, n, q, r, w, [0.75, 0.5])
    assert stats['n_merges'] >= degree


def test_complete_then_average_then_complete(api, graph300):
    """the loop the two linkages share carries no state from one to the next"""
    q, r, w, _ = graph300
    t0, s0 = api.cluster_complete_linkage_graph(300, q, r, w)
    ta, _ = api.cluster_average_linkage_graph(300, q, r, w, 0.7)
    t1, s1 = api.cluster_complete_linkage_graph(300, q, r, w)
    assert t0.tobytes() == t1.tobytes() and s0 == s1
    want = av.merges(300, cr.edges(zip(q.tolist(), r.tolist(), w.tolist())), 0.7)
    assert [(int(t['object_a']), int(t['object_b']), int(t['sum']), int(t['pairs'])) for t in ta] == want
    assert _as_rows(ta) == av.table(300, want)


def test_planted_cliques_with_ties(api, graph300):
    q, r, w, merges = graph300
    table, stats = _check(api, 300, q, r, w, [0.95, 0.85, 0.75, 0.7, 0.0], merges)
    assert 3 <= stats['rounds'] < stats['n_merges']                                              # several merges per round


def test_levels_are_nested_cuts_of_one_hierarchy(api, graph300):
    q, r, w, merges = graph300
    lv = [0.95, 0.9, 0.7, 0.9]
    label, rep, _ = api.cluster_complete_levels_graph(300, q, r, w, lv)
    for k, t in enumerate(lv):
        assert (label[k].tolist(), rep[k].tolist()) == cr.labels(lr.cut(300, merges, t)), t
        sel = w >= t                                                                             # the floor cut of the filtered rows
        l1, r1, _ = api.cluster_graph(300, q[sel], r[sel], w[sel], 'complete')
        assert np.array_equal(l1, label[k]) and np.array_equal(r1, rep[k]), t
        single = api.cluster_levels(300, q, r, w, [t])[1][0]
        assert all(len(set(single[rep[k] == c].tolist())) == 1 for c in set(rep[k].tolist())), t # inside one single-linkage cluster
    assert np.array_equal(label[1], label[3]) and np.array_equal(rep[1], rep[3])                 # the repeated level
    for hi, lo in ((0, 1), (1, 2)):                                                              # descending levels only join
        assert all(len(set(rep[lo][rep[hi] == c].tolist())) == 1 for c in set(rep[hi].tolist()))


def test_5000_objects_continuous_weights(api):
    """more than one workgroup in every kernel; cliques up to 64 members, weights all distinct"""
    rng = np.random.default_rng(17)
    n = 5000
    q, r, w = cl.planted_cliques(rng, n, 64, lambda g, k: g.uniform(0.7, 1.0, k), 3000, lambda g, k: g.uniform(0.5, 1.0, k))
    table, stats = _check(api, n, q, r, w, [0.9, 0.8])
    assert stats['n_edges'] > 65536 and stats['rounds'] < stats['n_merges']


def test_same_call_twice(api, graph300):
    q, r, w, _ = graph300
    got = [(api.cluster_complete_linkage_graph(300, q, r, w), api.cluster_complete_levels_graph(300, q, r, w, [0.9, 0.7])) for _ in range(2)]
    (t0, s0), (l0, r0, _) = got[0]
    (t1, s1), (l1, r1, _) = got[1]
    assert t0.tobytes() == t1.tobytes() and s0 == s1 and np.array_equal(l0, l1) and np.array_equal(r0, r1)


@pytest.mark.parametrize('repr_', [False, True])
def test_cli_golden_example(api, out_dir, tmp_path, repr_):
    files = ['-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv']
    extra = ['-r'] if repr_ else []
    out, link = tmp_path / 'c.tsv', tmp_path / 'l.tsv'
    p = run('cluster', *files, '-o', out, '--algorithm', 'complete', '--tani', '0.7', '--out-linkage', link, '--levels', '0.95', '0.9',
            '-v', '0', *extra)
    assert p.returncode == 0 and p.stderr == '', p.stderr
    want, want_link = cl.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'tani', [0.95, 0.9], representatives=repr_, tani=0.7)
    assert out.read_bytes() == want and link.read_bytes() == want_link
    # the `cluster` column is the array-level complete clustering of the passing rows
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    rows = cr.read_rows(out_dir / 'ani.tsv', len(ids), 'tani', tani=0.7)
    label, rep, _ = api.cluster_graph(len(ids), *zip(*rows), 'complete')
    cols = [ln.split('\t') for ln in out.read_text().split('\n') if ln]
    assert cols[0] == ['object', 'cluster', 'tani_0.95', 'tani_0.9']
    assert [c[1] for c in cols[1:]] == ([ids[x] for x in rep.tolist()] if repr_ else [str(x) for x in label.tolist()])
    # the whole-stage library call without levels: the same floor clustering as a plain clusters.tsv
    plain = tmp_path / 'plain.tsv'
    api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', plain, algorithm='complete', tani=0.7, representatives=repr_)
    assert [ln for ln in plain.read_text().split('\n') if ln] == ['\t'.join(c[:2]) for c in cols]
    if not repr_:
        p = run('cluster', *files, '-o', out, '--algorithm', 'complete', '--tani', '0.7', '--levels', '0.9')
        assert p.returncode == 0 and 'Running' in p.stderr and '--algorithm complete' in p.stderr and '--levels 0.9' in p.stderr, p.stderr
