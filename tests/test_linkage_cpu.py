"""The single-linkage merge table without a GPU: the restatement (tests/linkage_restatement.py) against `single` and the
golden clusters.tsv, the C ABI and Python surface of vg_cluster_linkage_graph / vg_cluster_levels_graph / vg_cluster_linkage,
and the CLI's usage errors (no device needed for any of it)."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import linkage_restatement as lr
from vclust_amd import _lib, api

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
NEW_SYMBOLS = ('vg_cluster_linkage_graph', 'vg_cluster_levels_graph', 'vg_cluster_linkage')


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


def test_restatement_cuts_equal_single_on_the_golden_example(out_dir):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    n = len(ids)
    lv = [0.95, 0.9, 0.8, 0.7]
    rows = cr.read_rows(out_dir / 'ani.tsv', n, 'tani', tani=0.7)
    cuts = lr.levels(n, rows, lv)
    for t, got in zip(lv, cuts):
        assert got == cr.cluster_graph(n, cr.read_rows(out_dir / 'ani.tsv', n, 'tani', tani=t), 'single'), t
    assert cr.clusters_tsv(ids, *cuts[0]) == (out_dir / 'clusters.tsv').read_bytes()
    # the file: `object`, the cut at the floor, then the levels in the order given; the 0.95 column is the golden file's
    text, link = lr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'tani', lv, tani=0.7)
    lines = text.decode().split('\n')
    assert lines[0] == 'object\tcluster\ttani_0.95\ttani_0.9\ttani_0.8\ttani_0.7'
    golden = (out_dir / 'clusters.tsv').read_text().split('\n')
    assert ['\t'.join(ln.split('\t')[i] for i in (0, 2)) for ln in lines[1:] if ln] == [ln for ln in golden[1:] if ln]
    assert [ln.split('\t')[1] for ln in lines[1:] if ln] == [ln.split('\t')[5] for ln in lines[1:] if ln]     # floor = 0.7
    assert link.decode().split('\n')[0] == 'node_a\tnode_b\tsimilarity\tsize\tobject_a\tobject_b'


def test_restatement_table_on_a_random_graph():
    rng = np.random.default_rng(5)
    n = 300
    rows = [(int(a), int(b), float(w)) for a, b, w in zip(rng.integers(0, n, 900), rng.integers(0, n, 900), rng.choice([0.5, 0.7, 0.9], 900))]
    e = cr.edges(rows)
    tab = lr.linkage(n, rows)
    components = len(set(cr.cluster_ids(n, e, 'single')))
    assert len(tab) == n - components
    sims = [row[2] for row in tab]
    assert all(x >= y for x, y in zip(sims, sims[1:]))
    size = {i: 1 for i in range(n)}
    used = set()
    for k, (na, nb, w, sz, a, b) in enumerate(tab):
        assert na < nb < n + k and na not in used and nb not in used       # a node is merged once
        assert sz == size[na] + size[nb] and e[(a, b)] == w and a < b
        used.update((na, nb))
        size[n + k] = sz
    assert sum(size[x] for x in size if x not in used) == n                 # the nodes left over are the components
    for t in (0.9, 0.7, 0.5, 0.0, 0.95):
        assert cr.labels(lr.cut(n, lr.forest(n, e), t)) == cr.cluster_graph(n, [x for x in rows if x[2] >= t], 'single')
    # ties: the key (-w, a, b) decides, so the first merge is the (a, b)-smallest edge of the highest weight
    assert tab[0][4:] == min(k for k, w in e.items() if w == 0.9)


def test_restatement_small_cases():
    assert lr.linkage(1, []) == [] and lr.linkage(5, []) == []
    rows = [(0, 1, -0.0), (1, 0, 0.0), (1, 2, 0.0), (2, 2, 1.0)]
    assert lr.linkage(3, rows) == [(0, 1, 0.0, 2, 0, 1), (2, 3, 0.0, 3, 1, 2)]
    assert b'-' not in lr.linkage_tsv(lr.linkage(3, rows))
    # 0-1 (0.9), 1-2 (0.95), 0-2 (0.5: inside a cluster by then), 3-4 (0.7)
    rows = [(0, 1, 0.9), (2, 0, 0.5), (1, 2, 0.95), (2, 1, 0.6), (3, 4, 0.7)]
    assert lr.linkage(6, rows) == [(1, 2, 0.95, 2, 1, 2), (0, 6, 0.9, 3, 0, 1), (3, 4, 0.7, 2, 3, 4)]
    assert lr.levels(6, rows, [0.95, 0.6, 0.95]) == [([1, 0, 0, 2, 3, 4], [0, 1, 1, 3, 4, 5]), ([0, 0, 0, 1, 1, 2], [0, 0, 0, 3, 3, 5]),
                                                    ([1, 0, 0, 2, 3, 4], [0, 1, 1, 3, 4, 5])]


def test_new_symbols_exported_declared_and_callable():
    lib = _lib.load()
    header = (ROOT / 'include' / 'vclust_gpu.h').read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header, name
    assert 'vg_linkage_stats' in header
    assert callable(api.cluster_linkage) and callable(api.cluster_levels)
    assert _lib.CLUSTER_ALGORITHMS == {'single': 0, 'cd-hit': 1, 'uclust': 2, 'set-cover': 3}


def test_argument_errors_need_no_device():
    for call in (lambda *a: api.cluster_linkage(*a), lambda *a: api.cluster_levels(*a, [0.5])):
        with pytest.raises(_lib.VclustGpuError) as e:
            call(3, [0], [3], [1.0])
        assert e.value.code == -1 and 'outside' in str(e.value)
        with pytest.raises(_lib.VclustGpuError) as e:
            call(3, [0], [1], [float('nan')])
        assert e.value.code == -1 and 'NaN' in str(e.value)
        with pytest.raises(_lib.VclustGpuError) as e:
            call(1 << 31, [], [], [])
        assert e.value.code == -6
    table, stats = api.cluster_linkage(0, [], [], [])
    assert len(table) == 0 and table.dtype == api.LINKAGE_DTYPE and stats == dict(rounds=0, n_edges=0, n_merges=0)
    label, rep, stats = api.cluster_levels(0, [], [], [], [0.9, 0.5])
    assert label.shape == rep.shape == (2, 0) and stats['n_merges'] == 0
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_levels(3, [0], [1], [0.5], [float('nan')])
    assert e.value.code == -1


def test_file_call_refuses_other_algorithms_and_levels_below_the_floor(out_dir, tmp_path):
    files = (out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv')
    with pytest.raises(ValueError):
        api.cluster(*files, algorithm='cd-hit', tani=0.7, levels=[0.9])
    p = _lib.ClusterParams(algorithm=1, metric=b'tani', min_tani=0.7)
    import ctypes as C
    rc = _lib.load().vg_cluster_linkage(*(str(f).encode() for f in files), C.byref(p), None, None, 0)
    assert rc == -1 and 'single' in _lib.load().vg_last_error().decode()
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster(*files, tani=0.95, levels=[0.9])
    assert e.value.code == -1 and 'below' in str(e.value)
    assert not (tmp_path / 'c.tsv').exists()


def test_without_device_fails_loudly(out_dir, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_linkage(3, [0, 1], [1, 2], [0.9, 0.8])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_levels(3, [0, 1], [1, 2], [0.9, 0.8], [0.85])
    assert e.value.code == -3
    assert not (ROOT / 'bin' / 'clusty').exists()
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.7',
            '--out-linkage', tmp_path / 'l.tsv')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'bin/clusty' not in p.stderr, p.stderr
    assert '--out-linkage' in p.stderr                      # the Running: line names the flag
    assert not (tmp_path / 'c.tsv').exists() and not (tmp_path / 'l.tsv').exists()


def test_cli_usage_errors(out_dir, tmp_path):
    args = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv']
    p = run(*args, '--levels', '0.9', '--algorithm', 'cd-hit')
    assert p.returncode == 2 and '--algorithm single' in p.stderr, p.stderr
    p = run(*args, '--tani', '0.7', '--out-linkage', tmp_path / 'l.tsv', '--algorithm', 'uclust')
    assert p.returncode == 2 and '--algorithm single' in p.stderr, p.stderr
    p = run(*args, '--tani', '0.95', '--levels', '0.9')
    assert p.returncode == 2 and 'below --tani 0.95' in p.stderr, p.stderr
    p = run(*args, '--levels', '0.9')
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr, p.stderr
    assert not (tmp_path / 'c.tsv').exists() and not (tmp_path / 'l.tsv').exists()
