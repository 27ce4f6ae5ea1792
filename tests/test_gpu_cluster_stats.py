"""The cluster report on the MI355X (vg_cluster_stats_graph, vg_cluster_stats_file, `cluster --out-stats`) against the sequential
restatement (tests/cluster_stats_restatement.py): every field of every record and every per-object value is an integer and must be
equal, and the report file must equal the restatement's text byte for byte."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_stats_restatement as cs

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


def _check(api, n, q, r, w, label, k=None):
    """the library's report of this labelling equals the restatement's, field by field; -> the library's raw bytes"""
    label = np.asarray(label, np.int32)
    k = (int(label.max()) + 1 if n else 0) if k is None else k
    rec, own, oth_max, oth = api.cluster_stats_graph(n, q, r, w, label, k)
    want, want_own, want_max, want_oth = cs.stats_graph(n, list(zip(map(int, q), map(int, r), map(float, w))), label.tolist(), k)
    assert len(rec) == k
    for f in cs.FIELDS:
        assert rec[f].tolist() == [x[f] for x in want], f
    assert own.tolist() == want_own and oth_max.tolist() == want_max and oth.tolist() == want_oth
    return rec.tobytes() + own.tobytes() + oth_max.tobytes() + oth.tobytes()


def _random_graph(rng, n, rows, weights):
    q = rng.integers(0, n, rows)
    r = np.where(rng.random(rows) < 0.7, np.clip(q + rng.integers(-20, 21, rows), 0, n - 1), rng.integers(0, n, rows))    # families: close in index
    w = rng.choice(weights, rows) if not callable(weights) else weights(rows)
    return q.astype(np.uint32), r.astype(np.uint32), np.asarray(w, np.float64)


def _scattered_labels(rng, n, k):
    """a random labelling over 2 k labels of which about half stay unused, in no relation to the index order"""
    names = rng.permutation(2 * k)[:k]
    return names[rng.integers(0, k, n)].astype(np.int32), 2 * k


@pytest.mark.parametrize('seed,n,rows', [(1, 1, 0), (2, 1, 3), (3, 2, 1), (4, 63, 50), (5, 65, 300), (6, 500, 2000), (7, 3000, 9000)])
def test_random_graphs_with_the_labels_of_every_algorithm(api, seed, n, rows):
    rng = np.random.default_rng(seed)
    if rows:
        q, r, w = _random_graph(rng, n, rows, lambda m: rng.uniform(0.5, 1.0, m).round(3))
        sel = rng.random(rows) < 0.3                                            # duplicates and reverse rows with other weights
        q, r, w = np.concatenate([q, r[sel]]), np.concatenate([r, q[sel]]), np.concatenate([w, rng.choice([0.6, 0.95], sel.sum())])
    else:
        q = r = np.zeros(0, np.uint32); w = np.zeros(0)
    for algo in ('single', 'cd-hit', 'uclust', 'set-cover', 'complete'):
        _check(api, n, q, r, w, api.cluster_graph(n, q, r, w, algo)[0])
    _check(api, n, q, r, w, api.cluster_average_levels_graph(n, q, r, w, [0.7], 0.0)[0][0])
    label, k = _scattered_labels(rng, n, max(1, n // 7))
    _check(api, n, q, r, w, label, k)


@pytest.fixture(scope='module')
def hub_graph():
    """6 000 objects; object 17 has a row to 5 500 of them (one CSR row of more than 5 000 entries), the others ~6 rows each"""
    rng = np.random.default_rng(11)
    n = 6000
    q, r, w = _random_graph(rng, n, 18000, lambda m: rng.uniform(0.0, 1.0, m).round(4))
    others = rng.permutation(np.setdiff1d(np.arange(n), [17]))[:5500]
    q = np.concatenate([q, np.full(5500, 17, np.uint32)]); r = np.concatenate([r, others.astype(np.uint32)])
    w = np.concatenate([w, rng.uniform(0.0, 1.0, 5500).round(4)])
    return n, q, r, w


def test_a_row_of_more_than_5000_entries(api, hub_graph):
    n, q, r, w = hub_graph
    rng = np.random.default_rng(12)
    _check(api, n, q, r, w, rng.integers(0, 40, n))                             # the hub's row crosses 40 clusters
    _check(api, n, q, r, w, api.cluster_graph(n, q, r, w, 'cd-hit')[0])


def test_every_object_in_one_cluster(api, hub_graph):
    n, q, r, w = hub_graph
    _check(api, n, q, r, w, np.zeros(n, np.int32))                              # one record takes every piece
    _check(api, n, q, r, w, np.full(n, 3, np.int32), 5)                         # ... beside labels without a member


def test_singletons_without_rows_and_no_object_at_all(api):
    none = np.zeros(0, np.uint32)
    _check(api, 1000, none, none, np.zeros(0), np.arange(1000)[::-1])
    _check(api, 0, none, none, np.zeros(0), np.zeros(0, np.int32), 0)
    _check(api, 0, none, none, np.zeros(0), np.zeros(0, np.int32), 3)
    _check(api, 700, [5, 9, 9], [5, 9, 9], [1.0, 0.5, 0.25], np.arange(700) // 2)     # self rows only: no edge


@pytest.mark.parametrize('weight', [1.0, 0.0, 0.5])
def test_one_weight_everywhere(api, weight):
    """1.0: every u is 2^32 (the 33-bit key); 0.0: edges that add nothing and still count; any: every tie is decided by label alone"""
    rng = np.random.default_rng(13)
    n = 2000
    q, r, _ = _random_graph(rng, n, 12000, [weight])
    w = np.full(len(q), weight)
    label, k = _scattered_labels(rng, n, 150)
    _check(api, n, q, r, w, label, k)
    _check(api, n, q, r, w, np.arange(n) % 7)
    _check(api, n, q, r, w, api.cluster_graph(n, q, r, w, 'uclust')[0])


def test_family_graph_of_20000_objects_twice(api):
    rng = np.random.default_rng(14)
    n, rows = 20000, 300000
    q, r, w = _random_graph(rng, n, rows, lambda m: rng.uniform(0.8, 1.0, m).round(4))
    q, r, w = np.concatenate([q, r]), np.concatenate([r, q]), np.concatenate([w, w])      # both directions: ~30 rows per object
    label = api.cluster_graph(n, q, r, w, 'cd-hit')[0]
    first = _check(api, n, q, r, w, label)
    rec, own, oth_max, oth = api.cluster_stats_graph(n, q, r, w, label)
    assert rec.tobytes() + own.tobytes() + oth_max.tobytes() + oth.tobytes() == first


# ---------------------------------------------------------------- end to end through the command line
CASES = {
    'single': ['--algorithm', 'single', '--tani', '0.95'],
    'cd-hit': ['--algorithm', 'cd-hit', '--tani', '0.95'],
    'uclust': ['--algorithm', 'uclust', '--ani', '0.9', '--metric', 'ani', '--qcov', '0.5'],
    'set-cover': ['--algorithm', 'set-cover', '--tani', '0.7', '--num_alns', '40'],
    'average': ['--algorithm', 'average', '--tani', '0.9'],
    'complete-levels': ['--algorithm', 'complete', '--tani', '0.9', '--levels', '0.95', '0.9'],
    'single-levels-repr': ['--algorithm', 'single', '--gani', '0.5', '--metric', 'gani', '--levels', '0.9', '--out-repr'],
    'cd-hit-repr': ['--algorithm', 'cd-hit', '--tani', '0.95', '--out-repr'],
    'prior': ['--algorithm', 'uclust', '--tani', '0.95', '--prior', 'PRIOR'],
}


def _options(argv):
    """the restatement's keywords for a command line of CASES"""
    kw, it = {}, iter(argv)
    for a in it:
        if a in ('--tani', '--gani', '--ani', '--qcov'):
            kw[a[2:]] = float(next(it))
        elif a == '--metric':
            kw['metric'] = next(it)
        elif a == '--num_alns':
            kw['num_alns'] = int(next(it))
    return kw


@pytest.mark.parametrize('case', list(CASES))
def test_cli_report_equals_restatement_and_leaves_clusters_alone(api, out_dir, tmp_path, case):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    prior = tmp_path / 'prior.tsv'
    prior.write_text('object\tcluster\n' + ''.join(f'{x}\t{k // 2}\n' for k, x in enumerate(ids[:8])))
    argv = [str(prior) if a == 'PRIOR' else a for a in CASES[case]]
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', *argv]
    plain, out, stats = tmp_path / 'plain.tsv', tmp_path / 'c.tsv', tmp_path / 's.tsv'
    p = run(*base, '-o', plain, '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    p = run(*base, '-o', out, '--out-stats', stats)
    assert p.returncode == 0 and p.stderr.count('Running: ') == 2 and p.stderr.count('Completed') == 2, p.stderr
    assert out.read_bytes() == plain.read_bytes()
    want = cs.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', out, '--out-repr' in argv, **_options(argv))
    assert stats.read_bytes() == want
    blocks = [ln.split('\t')[0] for ln in want.decode().split('\n')[1:-1]]
    assert sorted(set(blocks), key=blocks.index) == out.read_text().split('\n')[0].split('\t')[1:]


def test_file_call_on_a_clustering_the_library_did_not_make(api, out_dir, tmp_path):
    """any partition of the ids file, numbered any way, with several columns -- as bin/clusty or another tool may write it"""
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    rng = np.random.default_rng(15)
    path = tmp_path / 'foreign.tsv'
    order = rng.permutation(len(ids))
    path.write_text('object\tleiden\tother\n' + ''.join(f'{ids[i]}\t{1000 - i % 3}\t{i // 5 + 40}\n' for i in order))
    api.cluster_stats(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', path, tmp_path / 's.tsv', metric='ani', ani=0.5, len_ratio=0.5)
    assert (tmp_path / 's.tsv').read_bytes() == cs.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', path, metric='ani', ani=0.5, len_ratio=0.5)
