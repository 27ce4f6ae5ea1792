"""The cluster stage on the MI355X (vg_cluster / vg_cluster_graph) against the sequential restatement
(tests/cluster_restatement.py) and, for single linkage at tANI >= 0.95, against the golden clusters.tsv byte for byte."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
ALGOS = ('single', 'cd-hit', 'uclust', 'set-cover')


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


def test_cli_reproduces_golden_clusters(api, out_dir, tmp_path):
    out = tmp_path / 'clusters.tsv'
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', out,
            '--algorithm', 'single', '--metric', 'tani', '--tani', '0.95', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    assert out.read_bytes() == (out_dir / 'clusters.tsv').read_bytes()


@pytest.mark.parametrize('algo', ALGOS)
def test_cli_checks_of_the_reference(api, out_dir, tmp_path, algo):
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '--algorithm', algo]
    p = run(*base, '-o', tmp_path / 'a.tsv', '--tani', '0.95', '-v', '0')
    assert p.returncode == 0 and p.stderr == '' and (tmp_path / 'a.tsv').stat().st_size > 0, p.stderr
    p = run(*base, '-o', tmp_path / 'b.tsv', '--tani', '0.95', '--gani', '0.85', '--ani', '0.85', '--qcov', '0.85', '--rcov', '0.85', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    assert (tmp_path / 'b.tsv').read_bytes() == cr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', algo, 'tani', tani=0.95, gani=0.85,
                                                        ani=0.85, qcov=0.85, rcov=0.85)
    p = run(*base, '-o', tmp_path / 'c.tsv', '--tani', '0.95')
    assert p.returncode == 0 and 'Running' in p.stderr and 'Completed' in p.stderr and 'INFO' in p.stderr


@pytest.mark.parametrize('repr_', [False, True])
@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('metric,thr', [('tani', 0.95), ('ani', 0.9), ('gani', 0.5)])
def test_golden_files_equal_restatement(api, out_dir, tmp_path, algo, repr_, metric, thr):
    out = tmp_path / 'c.tsv'
    api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', out, algorithm=algo, metric=metric, representatives=repr_, **{metric: thr})
    assert out.read_bytes() == cr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', algo, metric, representatives=repr_, **{metric: thr})


def test_large_file_parsed_by_four_threads_equals_restatement(api, tmp_path):
    """About 3 000 objects and 60 000 rows in a file above 2 MiB (every one of four threads parses a chunk), blank lines, rows
    below an active minimum: the clusters of the restatement on the same file."""
    from test_cluster_cpu import big_ani_file
    path, ids, lines = big_ani_file(tmp_path)
    path.write_text('\n'.join(lines) + '\n')
    assert path.stat().st_size > (2 << 20) + (1 << 19)
    api.cluster(path, ids, tmp_path / 'c.tsv', algorithm='single', tani=0.97, ani=0.3, num_threads=4)
    assert (tmp_path / 'c.tsv').read_bytes() == cr.run(path, ids, 'single', 'tani', tani=0.97, ani=0.3)


def _check(api, n, q, r, w, algo):
    label, rep, stats = api.cluster_graph(n, q, r, w, algo)
    want_label, want_rep = cr.cluster_graph(n, list(zip(map(int, q), map(int, r), map(float, w))), algo)
    assert list(rep) == want_rep, algo
    assert list(label) == want_label, algo
    return stats


def _random_graph(rng, n, rows, weights):
    q = rng.integers(0, n, rows)
    # family structure: most rows stay close in index
    r = np.where(rng.random(rows) < 0.7, np.clip(q + rng.integers(-20, 21, rows), 0, n - 1), rng.integers(0, n, rows))
    w = rng.choice(weights, rows)
    return q.astype(np.uint32), r.astype(np.uint32), w


@pytest.mark.parametrize('seed,n,rows', [(1, 1, 0), (2, 1, 3), (3, 2, 1), (4, 50, 40), (5, 500, 2000), (6, 3000, 6000),
                                         (7, 20000, 60000), (8, 20000, 500000)])
def test_random_graphs_equal_restatement(api, seed, n, rows):
    rng = np.random.default_rng(seed)
    if rows:
        q, r, w = _random_graph(rng, n, rows, [0.5, 0.75, 0.75, 0.9, 1.0])    # tied weights (uclust), self rows when n is small
        sel = rng.random(rows) < 0.3                                            # duplicates and reverse rows with other weights
        q = np.concatenate([q, r[sel]]); r = np.concatenate([r, q[:rows][sel]]); w = np.concatenate([w, rng.choice([0.6, 0.95], sel.sum())])
    else:
        q = r = np.zeros(0, np.uint32); w = np.zeros(0)
    for algo in ALGOS:
        _check(api, n, q, r, w, algo)


def test_hub_cliques_and_isolated_objects(api):
    n = 12000
    rows = [(5000, j, 0.9) for j in range(0, n, 3) if j != 5000]                  # a hub joined to a third of the objects
    for c in range(0, 6000, 6):                                                  # many equal cliques of 6 with equal weights
        rows += [(c + a, c + b, 0.8) for a in range(6) for b in range(a + 1, 6)]
    rows += [(7, 7, 1.0), (11000, 11001, 0.7), (11001, 11000, 0.75)]             # a self row, an asymmetric couple
    q, r, w = (np.array(x) for x in zip(*rows))
    for algo in ALGOS:
        _check(api, n, q.astype(np.uint32), r.astype(np.uint32), w.astype(np.float64), algo)


TAIL_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import cluster_restatement as cr
from vclust_amd import api
n, shape = 100000, sys.argv[2]
if shape == 'path':
    q, r = np.arange(n - 1), np.arange(1, n)
else:
    hub = 0 if shape == 'star-first' else n - 1
    q = np.full(n - 1, hub); r = np.array([j for j in range(n) if j != hub])
w = np.full(len(q), 0.9)
out = {}
for algo in ('cd-hit', 'uclust', 'set-cover'):
    label, rep, stats = api.cluster_graph(n, q, r, w, algo)
    want_label, want_rep = cr.cluster_graph(n, list(zip(q.tolist(), r.tolist(), w.tolist())), algo)
    out[algo] = dict(stats, equal=list(rep) == want_rep and list(label) == want_label)
print(json.dumps(out))
"""


@pytest.mark.parametrize('shape', ['path', 'star-first', 'star-last'])
def test_tail_sweep(api, shape):
    """A 100 000-object path in index order is one long dependency chain: the rounds stall and the one-workgroup sweep
    finishes it.  Run in a child with a time limit (tools/cluster_timing.py measured well under a second per algorithm)."""
    import json
    p = subprocess.run([sys.executable, '-c', TAIL_CHILD, str(ROOT), shape], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for algo, st in res.items():
        assert st['equal'], (shape, algo, st)
        assert st['n_edges'] == 100000 - 1
        if shape == 'path':
            assert st['sweep_objects'] > 100000 // 2, (algo, st)


def test_end_to_end_synthetic_families(api, tmp_path):
    from vclust_amd import synth
    codes, offsets, names = synth.make_families(6, 5, length=6000, seed=3)
    fna = tmp_path / 'in.fna'
    synth.write_fasta(str(fna), codes, offsets, names)
    assert run('prefilter', '-i', fna, '-o', tmp_path / 'fltr.txt', '-v', '0').returncode == 0
    p = run('align', '-i', fna, '-o', tmp_path / 'ani.tsv', '--filter', tmp_path / 'fltr.txt', '-v', '0')
    assert p.returncode == 0, p.stderr
    for algo in ALGOS:
        out = tmp_path / f'{algo}.tsv'
        p = run('cluster', '-i', tmp_path / 'ani.tsv', '--ids', tmp_path / 'ani.ids.tsv', '-o', out, '--algorithm', algo, '--tani', '0.7', '-v', '0')
        assert p.returncode == 0 and p.stderr == '', p.stderr
        assert out.read_bytes() == cr.run(tmp_path / 'ani.tsv', tmp_path / 'ani.ids.tsv', algo, 'tani', tani=0.7)
