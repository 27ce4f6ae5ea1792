"""The complete-linkage merge table without a GPU: the restatement (tests/complete_restatement.py) on hand cases and the
properties DESIGN.md section 9 states for it, the C ABI and Python surface of vg_cluster_complete_linkage_graph /
vg_cluster_complete_levels_graph, and the CLI's usage errors (no device needed for any of it)."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import complete_restatement as cl
import linkage_restatement as lr
from vclust_amd import _lib, api

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
NEW_SYMBOLS = ('vg_cluster_complete_linkage_graph', 'vg_cluster_complete_levels_graph')


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


def test_restatement_hand_cases():
    # path 0-1-2: one merge; the pair (0, 2) has no edge, so the third object stays alone
    rows = [(0, 1, 0.9), (1, 2, 0.8)]
    assert cl.linkage(3, rows) == [(0, 1, 0.9, 2, 0, 1)] and cl.cluster_ids(3, rows) == [0, 0, 2]
    # triangle with tied weights: (a, b) decides -- (0, 1) first, and the worst pair of {0, 1} with 2 is (1, 2)
    rows = [(1, 2, 0.9), (0, 2, 0.9), (0, 1, 0.9)]
    assert cl.linkage(3, rows) == [(0, 1, 0.9, 2, 0, 1), (2, 3, 0.9, 3, 1, 2)]
    # K4 without {2, 3}: {0, 1}, then 2 joins by its worst edge (0, 2); 3 cannot join {0, 1, 2} and stays alone
    rows = [(0, 1, 0.9), (0, 2, 0.8), (0, 3, 0.7), (1, 2, 0.85), (1, 3, 0.75)]
    assert cl.linkage(4, rows) == [(0, 1, 0.9, 2, 0, 1), (2, 4, 0.8, 3, 0, 2)] and cl.cluster_ids(4, rows) == [0, 0, 0, 3]
    # ... and with 3 closer than 2: {0, 1, 3}, 2 alone
    rows = [(0, 1, 0.9), (0, 2, 0.7), (0, 3, 0.8), (1, 2, 0.75), (1, 3, 0.85)]
    assert cl.linkage(4, rows) == [(0, 1, 0.9, 2, 0, 1), (3, 4, 0.8, 3, 0, 3)] and cl.cluster_ids(4, rows) == [0, 0, 2, 0]
    # no edges; no objects; one object
    assert cl.linkage(5, []) == [] and cl.cluster_ids(5, []) == [0, 1, 2, 3, 4]
    assert cl.linkage(0, []) == [] and cl.linkage(1, []) == [] and cl.levels(0, [], [0.5]) == [([], [])]
    # duplicate and reverse rows keep the maximum, self rows are dropped, -0.0 is +0.0
    rows = [(0, 1, -0.0), (1, 0, 0.0), (1, 2, 0.0), (2, 2, 1.0), (0, 2, -0.0), (2, 0, -1.0)]
    tab = cl.linkage(3, rows)
    assert tab == [(0, 1, 0.0, 2, 0, 1), (2, 3, 0.0, 3, 1, 2)] and b'-' not in lr.linkage_tsv(tab)
    rows = [(0, 1, 0.5), (1, 0, 0.9), (0, 1, 0.7), (1, 2, 0.95), (2, 1, 0.6), (0, 2, 0.8), (3, 3, 1.0)]
    assert cl.linkage(4, rows) == [(1, 2, 0.95, 2, 1, 2), (0, 4, 0.8, 3, 0, 2)]
    assert cl.levels(4, rows, [0.95, 0.8, 0.95]) == [([1, 0, 0, 2], [0, 1, 1, 3]), ([0, 0, 0, 1], [0, 0, 0, 3]), ([1, 0, 0, 2], [0, 1, 1, 3])]


def test_restatement_properties_on_a_random_graph():
    rng = np.random.default_rng(5)
    n = 300
    q, r, w = cl.planted_cliques(rng, n, 40, lambda g, k: g.choice([0.75, 0.85, 0.95], k), 200, lambda g, k: g.choice([0.7, 0.85], k))
    rows = list(zip(q.tolist(), r.tolist(), w.tolist()))
    e = cr.edges(rows)
    merges = cl.merges(n, e)
    tab = lr.table(n, merges)
    sims = [row[2] for row in tab]
    assert len(tab) > 100 and all(x >= y for x, y in zip(sims, sims[1:]))              # similarity never rises
    keys = [(-w_, a, b) for a, b, w_ in merges]
    assert keys == sorted(keys) and all(e[(a, b)] == w_ and a < b for a, b, w_ in merges)
    single = lr.forest(n, e)
    previous = None
    for t in (0.95, 0.85, 0.75, 0.7, 0.0):
        cid = lr.cut(n, merges, t)
        at_level = [x for x in rows if x[2] >= t]
        assert cid == cl.cluster_ids(n, at_level), t                                   # the floor cut of a run on the rows >= t
        members = {}
        for i, c in enumerate(cid):
            members.setdefault(c, []).append(i)
        ok = {k for k, w_ in e.items() if w_ >= t}
        assert all((a, b) in ok for m in members.values() for i, a in enumerate(m) for b in m[i + 1:]), t     # cliques
        sl = lr.cut(n, single, t)
        assert all(len({sl[i] for i in m}) == 1 for m in members.values()), t         # inside one single-linkage cluster
        if previous is not None:                                                       # nested: descending levels only join
            assert all(len({cid[i] for i in m}) == 1 for m in previous.values()), t
        previous = members
    assert len(set(lr.cut(n, merges, 0.0))) > len(set(lr.cut(n, single, 0.0)))         # and it is not single linkage


def test_new_symbols_exported_declared_and_callable():
    lib = _lib.load()
    header = (ROOT / 'include' / 'vclust_gpu.h').read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header, name
    assert 'VG_CLUSTER_COMPLETE = 4' in header
    assert callable(api.cluster_complete_linkage_graph) and callable(api.cluster_complete_levels_graph)
    assert _lib.LINKAGE_ALGORITHMS == {'single': 0, 'complete': 4}
    assert _lib.CLUSTER_ALGORITHMS == {'single': 0, 'cd-hit': 1, 'uclust': 2, 'set-cover': 3}


def test_argument_errors_need_no_device():
    for call in (lambda *a: api.cluster_complete_linkage_graph(*a), lambda *a: api.cluster_complete_levels_graph(*a, [0.5]),
                 lambda *a: api.cluster_graph(*a, 'complete')):
        with pytest.raises(_lib.VclustGpuError) as e:
            call(3, [0], [3], [1.0])
        assert e.value.code == -1 and 'outside' in str(e.value)
        with pytest.raises(_lib.VclustGpuError) as e:
            call(3, [0], [1], [float('nan')])
        assert e.value.code == -1 and 'NaN' in str(e.value)
        with pytest.raises(_lib.VclustGpuError) as e:
            call(1 << 31, [], [], [])
        assert e.value.code == -6
    table, stats = api.cluster_complete_linkage_graph(0, [], [], [])
    assert len(table) == 0 and table.dtype == api.LINKAGE_DTYPE and stats == dict(rounds=0, n_edges=0, n_merges=0)
    label, rep, stats = api.cluster_complete_levels_graph(0, [], [], [], [0.9, 0.5])
    assert label.shape == rep.shape == (2, 0) and stats['n_merges'] == 0
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_complete_levels_graph(3, [0], [1], [0.5], [float('nan')])
    assert e.value.code == -1
    label, rep, stats = api.cluster_graph(0, [], [], [], 'complete')
    assert len(label) == len(rep) == 0 and stats['n_edges'] == 0


def test_file_call_takes_complete_and_refuses_levels_below_the_floor(out_dir, tmp_path):
    files = (out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster(*files, algorithm='complete', tani=0.95, levels=[0.9])
    assert e.value.code == -1 and 'below' in str(e.value)
    with pytest.raises(ValueError):
        api.cluster(*files, algorithm='leiden', tani=0.7, levels=[0.9])
    assert not (tmp_path / 'c.tsv').exists()


def test_without_device_fails_loudly(out_dir, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_complete_linkage_graph(3, [0, 1], [1, 2], [0.9, 0.8])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_complete_levels_graph(3, [0, 1], [1, 2], [0.9, 0.8], [0.85])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_graph(3, [0, 1], [1, 2], [0.9, 0.8], 'complete')
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    assert not (ROOT / 'bin' / 'clusty').exists()
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.7',
            '--algorithm', 'complete', '--out-linkage', tmp_path / 'l.tsv')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'bin/clusty' not in p.stderr, p.stderr
    assert '--algorithm complete' in p.stderr and '--out-linkage' in p.stderr          # the Running: line names both
    assert not (tmp_path / 'c.tsv').exists() and not (tmp_path / 'l.tsv').exists()


def test_cli_usage_errors(out_dir, tmp_path):
    args = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv']
    p = run(*args, '--tani', '0.7', '--levels', '0.9', '--algorithm', 'cd-hit')
    assert p.returncode == 2 and '--algorithm single' in p.stderr and '--algorithm complete' in p.stderr, p.stderr
    p = run(*args, '--tani', '0.7', '--out-linkage', tmp_path / 'l.tsv', '--algorithm', 'leiden')
    assert p.returncode == 2 and '--algorithm complete' in p.stderr, p.stderr
    p = run(*args, '--tani', '0.95', '--levels', '0.9', '--algorithm', 'complete')
    assert p.returncode == 2 and 'below --tani 0.95' in p.stderr, p.stderr
    p = run(*args, '--levels', '0.9', '--algorithm', 'complete')
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr, p.stderr
    assert not (tmp_path / 'c.tsv').exists() and not (tmp_path / 'l.tsv').exists()
