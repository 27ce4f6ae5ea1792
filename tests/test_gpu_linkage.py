"""The single-linkage merge table and its cuts on the MI355X (vg_cluster_linkage_graph / vg_cluster_levels_graph /
vg_cluster_linkage) against the sequential restatement (tests/linkage_restatement.py): every case compares arrays or bytes."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
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


def _as_rows(table):
    return [(int(t['node_a']), int(t['node_b']), float(t['similarity']), int(t['size']), int(t['object_a']), int(t['object_b']))
            for t in table]


def _check(api, n, q, r, w, lv):
    """table and cuts are exactly the restatement's; each cut is also `single` on the rows at that level"""
    q, r, w = np.asarray(q, np.uint32), np.asarray(r, np.uint32), np.asarray(w, np.float64)
    rows = list(zip(q.tolist(), r.tolist(), w.tolist()))
    e = cr.edges(rows)
    merges = lr.forest(n, e)
    table, stats = api.cluster_linkage(n, q, r, w)
    assert _as_rows(table) == lr.table(n, merges)
    assert not (np.signbit(table['similarity']) & (table['similarity'] == 0)).any()           # -0.0 is +0.0
    assert stats['n_merges'] == len(merges) == n - len(set(lr.cut(n, merges, float('-inf')))) and stats['n_edges'] == len(e)
    label, rep, st2 = api.cluster_levels(n, q, r, w, lv)
    assert label.shape == rep.shape == (len(lv), n) and st2 == stats
    for k, t in enumerate(lv):
        want_label, want_rep = cr.labels(lr.cut(n, merges, t))
        assert rep[k].tolist() == want_rep and label[k].tolist() == want_label, t
        sel = w >= t
        l1, r1, _ = api.cluster_graph(n, q[sel], r[sel], w[sel], 'single')
        assert np.array_equal(l1, label[k]) and np.array_equal(r1, rep[k]), t
    return table, stats


@pytest.mark.parametrize('repr_', [False, True])
def test_cli_golden_example(api, out_dir, tmp_path, repr_):
    files = ['-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv']
    extra = ['--out-repr'] if repr_ else []
    out, link, plain = tmp_path / 'c.tsv', tmp_path / 'l.tsv', tmp_path / 'plain.tsv'
    p = run('cluster', *files, '-o', out, '--tani', '0.7', '--levels', '0.95', '0.9', '0.8', '--out-linkage', link, '-v', '0', *extra)
    assert p.returncode == 0 and p.stderr == '', p.stderr
    want, want_link = lr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'tani', [0.95, 0.9, 0.8], representatives=repr_, tani=0.7)
    assert out.read_bytes() == want and link.read_bytes() == want_link
    p = run('cluster', *files, '-o', plain, '--tani', '0.7', '-v', '0', *extra)
    assert p.returncode == 0, p.stderr
    cols = [ln.split('\t') for ln in out.read_text().split('\n') if ln]
    assert ['\t'.join(c[:2]) for c in cols] == [ln for ln in plain.read_text().split('\n') if ln]
    assert cols[0][2:] == ['tani_0.95', 'tani_0.9', 'tani_0.8']
    if not repr_:
        golden = [ln.split('\t')[1] for ln in (out_dir / 'clusters.tsv').read_text().split('\n') if ln]
        assert [c[2] for c in cols][1:] == golden[1:]
    p = run('cluster', *files, '-o', out, '--tani', '0.7', '--levels', '0.9', '--out-linkage', link)
    assert p.returncode == 0 and 'Running' in p.stderr and '--levels 0.9' in p.stderr and f'--out-linkage {link}' in p.stderr, p.stderr


def _random_graph(rng, n, rows, weights):
    q = rng.integers(0, n, rows)
    r = np.where(rng.random(rows) < 0.7, np.clip(q + rng.integers(-20, 21, rows), 0, n - 1), rng.integers(0, n, rows))   # families; self rows
    w = rng.choice(weights, rows)
    sel = rng.random(rows) < 0.3                                             # duplicates and reverse rows with other weights
    return (np.concatenate([q, r[sel]]).astype(np.uint32), np.concatenate([r, q[sel]]).astype(np.uint32),
            np.concatenate([w, rng.choice(weights, int(sel.sum()))]))


ULP = [0.9, np.nextafter(0.9, 1), np.nextafter(np.nextafter(0.9, 1), 1), np.nextafter(0.9, 0)]


@pytest.mark.parametrize('seed,weights,lv', [
    (1, [0.5, 0.7, 0.9], [0.9, 0.7, 0.6, 0.5, 0.0]),                         # ties dominate
    (2, ULP, [ULP[2], ULP[1], ULP[0], ULP[3]]),                              # weights that differ in the last ulp only
    (3, [0.8], [0.8, 0.81, 0.0]),                                            # all equal
    (4, [-1.5, -0.0, 0.0, 2.5, 1e-300], [2.5, 1e-300, 0.0, -2.0]),           # signs: the full double order
])
def test_random_graphs(api, seed, weights, lv):
    rng = np.random.default_rng(seed)
    q, r, w = _random_graph(rng, 2000, 8000, weights)
    _check(api, 2000, q, r, w, lv)


@pytest.mark.parametrize('kind', ['equal', 'increasing'])
def test_path_in_index_order(api, kind):
    n = 4096
    q, r = np.arange(n - 1), np.arange(1, n)
    w = np.full(n - 1, 0.9) if kind == 'equal' else 0.5 + np.arange(n - 1) / (4.0 * n)
    table, stats = _check(api, n, q, r, w, [0.95, 0.9, float(w[n // 2]), 0.0])
    assert stats['n_merges'] == n - 1 and table['size'][-1] == n
    assert stats['rounds'] <= 13          # every round at least halves the components that still have a leaving edge


def test_star_with_70000_leaves(api):
    n, hub = 70001, 35000                 # one root receives more atomics than a workgroup has lanes; its row is 70 000 long
    leaves = np.array([j for j in range(n) if j != hub])
    rng = np.random.default_rng(7)
    w = rng.choice([0.8, 0.9], n - 1)
    flip = rng.random(n - 1) < 0.5
    table, stats = _check(api, n, np.where(flip, hub, leaves), np.where(flip, leaves, hub), w, [0.9, 0.8])
    assert stats['n_merges'] == n - 1 and stats['n_edges'] == n - 1


def test_two_families_joined_by_their_weakest_edge(api):
    rng = np.random.default_rng(9)
    k = 60
    rows = [(a, b, float(rng.choice([0.85, 0.9, 0.95]))) for f in (0, k) for a in range(f, f + k) for b in range(a + 1, f + k)]
    rows.append((k + 7, 11, 0.3))
    q, r, w = zip(*rows)
    table, stats = _check(api, 2 * k, q, r, w, [0.5, 0.3])
    assert _as_rows(table)[-1][2:] == (0.3, 2 * k, 11, k + 7)               # that edge is the last merge
    label, rep, _ = api.cluster_levels(2 * k, q, r, w, [0.5])
    assert rep[0].tolist() == [0] * k + [k] * k


def test_edge_cases(api):
    table, stats = api.cluster_linkage(1, [], [], [])
    assert len(table) == 0 and stats == dict(rounds=0, n_edges=0, n_merges=0)
    label, rep, _ = api.cluster_levels(1, [0], [0], [1.0], [0.5])
    assert label.tolist() == [[0]] and rep.tolist() == [[0]]
    table, stats = _check(api, 5, [], [], [], [0.5])
    assert len(table) == 0 and stats['n_edges'] == 0
    table, _ = _check(api, 5, [3, 3], [3, 3], [1.0, 0.5], [0.5])             # self rows only
    assert len(table) == 0
    table, _ = _check(api, 3, [0, 1, 1, 2], [1, 0, 2, 2], [-0.0, 0.0, 0.0, 1.0], [0.0, 0.5])
    assert _as_rows(table) == [(0, 1, 0.0, 2, 0, 1), (2, 3, 0.0, 3, 1, 2)] and not np.signbit(table['similarity']).any()
    table, _ = _check(api, 2, [1], [0], [-0.0], [0.0])
    assert not np.signbit(table['similarity']).any()
    # levels in ascending order and a repeated level: columns in the order given
    rng = np.random.default_rng(11)
    q, r, w = _random_graph(rng, 200, 500, [0.5, 0.7, 0.9])
    _check(api, 200, q, r, w, [0.5, 0.7, 0.9, 0.7])


def test_levels_file_keeps_the_order_given(api, out_dir, tmp_path):
    out = tmp_path / 'c.tsv'
    api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', out, tani=0.7, levels=[0.8, 0.95, 0.8])
    assert out.read_bytes() == lr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'tani', [0.8, 0.95, 0.8], tani=0.7)[0]
    assert out.read_text().split('\n')[0] == 'object\tcluster\ttani_0.8\ttani_0.95\ttani_0.8'
    link = tmp_path / 'l.tsv'
    api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', out, metric='ani', ani=0.9, out_linkage=link)
    want, want_link = lr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'ani', ani=0.9)
    assert out.read_bytes() == want == cr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'single', 'ani', ani=0.9)
    assert link.read_bytes() == want_link


DETERMINISM_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from vclust_amd import api
d = np.load(sys.argv[2])
table, stats = api.cluster_linkage(int(d['n']), d['q'], d['r'], d['w'])
label, rep, _ = api.cluster_levels(int(d['n']), d['q'], d['r'], d['w'], d['lv'])
print(json.dumps(dict(table=table.tobytes().hex(), label=label.tobytes().hex(), rep=rep.tobytes().hex(), stats=stats)))
"""


def test_determinism(api, tmp_path):
    rng = np.random.default_rng(13)
    n, lv = 3000, [0.9, 0.7]
    q, r, w = _random_graph(rng, n, 12000, [0.5, 0.7, 0.9])
    got = [(api.cluster_linkage(n, q, r, w), api.cluster_levels(n, q, r, w, lv)) for _ in range(2)]
    (t0, s0), (l0, r0, _) = got[0]
    (t1, s1), (l1, r1, _) = got[1]
    assert t0.tobytes() == t1.tobytes() and s0 == s1 and np.array_equal(l0, l1) and np.array_equal(r0, r1)
    np.savez(tmp_path / 'g.npz', n=n, q=q, r=r, w=w, lv=np.array(lv))
    p = subprocess.run([sys.executable, '-c', DETERMINISM_CHILD, str(ROOT), str(tmp_path / 'g.npz')], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child == dict(table=t0.tobytes().hex(), label=l0.tobytes().hex(), rep=r0.tobytes().hex(), stats=s0)
