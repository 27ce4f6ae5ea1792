"""Markov clustering without a GPU: the restatement (tests/mcl_restatement.py) on fixed graphs and at the ends of its arithmetic,
the graphs of the GPU test under the restatement alone (each must converge inside the default limit), the C ABI and Python
surface, the argument checks (all on the host) and the CLI's usage errors."""
import math
import pathlib
import subprocess
import sys
import types

import pytest

import cluster_restatement as cr
import mcl_cases
import mcl_restatement as mr
from vclust_amd import _lib, api, cli

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
NEW_SYMBOLS = ('vg_cluster_mcl_graph', 'vg_cluster_mcl')
ONE = mr.ONE


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


def test_bridged_cliques_are_two_clusters():
    n, rows = mcl_cases.bridged_cliques()
    e = cr.edges(rows)
    cid, iterations, converged, matrix = mr.mcl(n, e)
    assert cid == [0] * 6 + [6] * 6 and converged == 1 and iterations <= 27
    assert cr.single(n, cr.adjacency(n, e)) == [0] * 12
    assert all(sum(row.values()) <= ONE and min(row.values()) > 0 for row in matrix)


def test_golden_example(out_dir):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    want = {0.7: [0, 1, 1, 1, 4, 4, 0, 0, 8, 8, 8, 8], 0.95: [0, 1, 1, 1, 4, 4, 6, 7, 8, 8, 8, 8]}
    for tani, cid in want.items():
        rows = cr.read_rows(out_dir / 'ani.tsv', len(ids), 'tani', tani=tani)
        assert mr.mcl(len(ids), cr.edges(rows))[0] == cid, tani
    head = mr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tani=0.7, representatives=True).split(b'\n')
    assert head[0] == b'object\tcluster' and len(head) == len(ids) + 2 and head[1].split(b'\t')[1] == ids[0].encode()


def test_object_without_rows_stays_a_singleton():
    cid, iterations, converged, matrix = mr.mcl(4, cr.edges([(0, 1, 0.9), (1, 3, 0.8), (2, 2, 1.0)]))
    assert cid[2] == 2 and matrix[2] == {2: ONE} and cid[0] == cid[1] == cid[3] == 0 and converged == 1
    assert mr.start(3, {})[1] == {1: ONE}
    assert mr.mcl(0, {}) == ([], 0, 0, [])


def test_arithmetic_at_the_ends():
    for a in range(3, 13):
        assert mr.power(0, a) == 0 and mr.power(ONE, a) == ONE, a
        # 2^-30 to any power above 1 is below one quantum; ONE - 1 stays below ONE and falls with the exponent
        assert mr.power(1, a) == 0, a
        t = mr.power(ONE - 1, a)
        assert 0 < t < ONE and t <= mr.power(ONE - 1, a - 1), a
        exact = (ONE - 1) ** a / ONE ** (a - 2)                # (t / ONE)^2 against ((ONE - 1) / ONE)^a: off by the floors only
        assert abs(t * t - exact) <= 2.0 * (a + 1) * ONE, a
    assert mr.power(1, 2) == 1 and mr.power(ONE - 1, 2) == ONE - 1
    for y in (0, 1, 2, 3, ONE - 1, ONE, 12345678):
        s = math.isqrt(y << 30)
        assert s * s <= y << 30 < (s + 1) * (s + 1) and mr.power(y, 1) == s
    assert mr.quantise(1.0) == 1 << 32 and mr.quantise(mcl_cases.SMALLEST) == 1 and mr.quantise(2.0 ** -33) == 0 and mr.quantise(1.5 * 2.0 ** -32) == 2
    assert mr.normalise({0: 1, 1: ONE}) == {1: ONE * ONE // (ONE + 1)}
    assert mr.prune({3: 5, 1: 5, 2: 9, 7: 1}, 2, 2) == {2: 9, 1: 5} and mr.prune({3: 5, 1: 5}, 9, 2) == {1: 5}


def test_the_cases_of_the_gpu_test_converge():
    for name, n, rows, params in mcl_cases.all_cases():
        last = mr.trace(n, cr.edges(rows), **params)[-1]
        assert last['converged'] == 1 and last['iterations'] <= 27, name
    n, rows = mcl_cases.planted()
    assert len(set(mr.mcl(n, cr.edges(rows))[0])) == 20
    n, rows = mcl_cases.path()
    assert mr.iterate(n, cr.edges(rows))['iterations'] == 57 and mr.iterate(n, cr.edges(rows), max_iterations=1)['converged'] == 0
    for distinct in (False, True):                         # the hub's first row is cut to the 8 leaves of lowest index / highest weight
        n, rows = mcl_cases.hub(distinct)
        first = mr.trace(n, cr.edges(rows), max_row=8, max_iterations=1)[0]['matrix'][0]
        assert sorted(first) == list(range(8)), distinct


def test_the_table_size_cases_reach_their_paths():
    """the cases of the GPU test at the real table: what the predictor says of each (rows tried, distinct columns of the named row,
    rows and records spilled, per iteration) is what the case states, so a changed case cannot stop reaching its path unnoticed"""
    cases = mcl_cases.table_size_cases()
    assert [c[4] for c in cases].count(64) == 1 and len({c[0] for c in cases}) == len(cases) == 8
    for case in cases:
        name, n, rows, params, slots, expected = case
        e = cr.edges(rows)
        trace = mr.trace(n, e, **params)
        figures = mcl_cases.reaches_its_path(case, mr.start(n, e), trace)
        assert 'max_iterations' in params or trace[-1]['converged'] == 1, name
        if slots == 64:
            assert figures[1]['records'] > 1 << 25, name
    # the crowns differ by one leaf, the limit by one column: 3/4 of 4 096
    assert cases[0][5]['figures'][0]['distinct'] == 4096 - 4096 // 4 == cases[1][5]['figures'][0]['distinct'] - 1


def test_symbols_exported_declared_and_listed():
    lib = _lib.load()
    header = (ROOT / 'include' / 'vclust_gpu.h').read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header, name
    assert hasattr(lib, 'vg_cluster_mcl_set_table_slots') and 'void vg_cluster_mcl_set_table_slots(' in header
    assert 'VG_CLUSTER_MCL = 6' in header and '} vg_mcl_params;' in header and '} vg_mcl_stats;' in header
    assert len(_lib.SYMBOLS['vg_cluster_mcl_graph'][1]) == 12 and len(_lib.SYMBOLS['vg_cluster_mcl'][1]) == 6
    assert _lib.FLOW_ALGORITHMS == {'mcl': 6}
    assert [f for f, _ in _lib.MclParams._fields_] == ['inflation', 'prune', 'chaos_eps', 'max_row', 'max_iterations']
    assert [f for f, _ in _lib.MclStats._fields_] == ['iterations', 'converged', 'n_edges', 'nnz', 'max_row_seen', 'lds_rows', 'spill_rows', 'chaos']
    assert 'mcl' not in {**_lib.CLUSTER_ALGORITHMS, **_lib.HIERARCHY_ALGORITHMS, **_lib.UPDATE_ALGORITHMS}


def test_the_general_calls_still_refuse_it(out_dir, tmp_path):
    with pytest.raises(_lib.VclustGpuError) as e:
        _lib.check(_lib.load().vg_cluster_graph(0, None, None, None, 0, 6, None, None, None))
    assert e.value.code == -1 and 'unknown algorithm' in str(e.value)
    with pytest.raises(ValueError):
        api.cluster_graph(2, [0], [1], [1.0], 'mcl')
    files = (out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv')
    for extra in (dict(levels=[0.9]), dict(out_linkage=tmp_path / 'l.tsv'), dict(prior_path=tmp_path / 'p.tsv')):
        with pytest.raises(ValueError):
            api.cluster(*files, algorithm='mcl', tani=0.7, **extra)
    with pytest.raises(ValueError):
        api.cluster(*files, algorithm='single', tani=0.7, mcl_inflation=2.0)
    assert not (tmp_path / 'c.tsv').exists()


def test_parameter_ranges_need_no_device():
    rows = (3, [0, 1], [1, 2], [0.9, 0.8])
    for bad, word in ((dict(inflation=1.7), 'inflation'), (dict(inflation=1.0), 'inflation'), (dict(inflation=6.5), 'inflation'),
                      (dict(inflation=float('nan')), 'inflation'), (dict(prune=0.2), 'prune'), (dict(prune=-1e-9), 'prune'),
                      (dict(max_row=1), 'max_row'), (dict(max_row=4097), 'max_row'), (dict(chaos_eps=1.0), 'chaos_eps'),
                      (dict(chaos_eps=-0.1), 'chaos_eps'), (dict(max_iterations=0), 'max_iterations'), (dict(max_iterations=1001), 'max_iterations')):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster_mcl_graph(*rows, **bad)
        assert e.value.code == -1 and word in str(e.value), bad
        with pytest.raises(ValueError):
            mr.check_params(**{**mr.DEFAULTS, **bad})
    for w, word in ((float('nan'), 'NaN'), (1.5, 'outside [0, 1]'), (-0.1, 'outside [0, 1]')):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster_mcl_graph(3, [0, 1], [1, 2], [0.9, w])
        assert e.value.code == -1 and 'weight' in str(e.value) and word in str(e.value), w
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_mcl_graph(3, [0], [3], [1.0])
    assert e.value.code == -1 and 'outside' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_mcl_graph(1 << 31, [], [], [])
    assert e.value.code == -6
    with pytest.raises(_lib.VclustGpuError) as e:          # null parameters
        _lib.check(_lib.load().vg_cluster_mcl_graph(0, None, None, None, 0, None, None, None, None, None, None, None))
    assert e.value.code == -1


def test_zero_objects_need_no_device():
    label, rep, stats = api.cluster_mcl_graph(0, [], [], [])
    assert len(label) == 0 and len(rep) == 0 and stats['iterations'] == 0 and stats['converged'] == 0 and stats['nnz'] == 0
    label, rep, stats, (off, col, val) = api.cluster_mcl_graph(0, [], [], [], matrix=True)
    assert off.tolist() == [0] and len(col) == 0 and len(val) == 0
    assert (mr.csr(mr.iterate(0, {})['matrix'])) == ([0], [], [])


def test_without_device_fails_loudly(out_dir, tmp_path):
    if api.device_count() > 0:
        return                                                 # (tests/test_gpu_mcl.py runs the calls there)
    for call in (lambda: api.cluster_mcl_graph(3, [0, 1], [1, 2], [0.9, 0.8]),
                 lambda: api.cluster_mcl_graph(3, [0, 1], [1, 2], [0.9, 0.8], matrix=True),
                 lambda: api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv', algorithm='mcl', tani=0.7)):
        with pytest.raises(_lib.VclustGpuError) as e:
            call()
        assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    assert not (tmp_path / 'c.tsv').exists()


def test_cli_usage_errors_then_the_library(out_dir, tmp_path):
    args = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--algorithm', 'mcl']
    prior = tmp_path / 'prior.tsv'
    prior.write_text('object\tcluster\n')
    for extra, word in ((['--prior', prior], 'not under mcl'), (['--levels', '0.9'], 'linkage hierarchy'),
                        (['--out-linkage', tmp_path / 'l.tsv'], 'linkage hierarchy')):
        p = run(*args, '--tani', '0.7', *extra)
        assert p.returncode == 2 and word in p.stderr and 'usage' in p.stderr, p.stderr
    p = run(*args)
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr, p.stderr
    for extra, word in ((['--mcl-inflation', '1.7'], '--mcl-inflation'), (['--mcl-prune', '0.5'], '--mcl-prune'),
                        (['--mcl-max-row', '1'], '--mcl-max-row'), (['--mcl-iterations', '0'], '--mcl-iterations')):
        p = run(*args, '--tani', '0.7', *extra)
        assert p.returncode == 2 and word in p.stderr, p.stderr
    assert not (tmp_path / 'c.tsv').exists()
    if api.device_count() > 0:
        return                                                 # (tests/test_gpu_mcl.py runs it there)
    assert not (ROOT / 'bin' / 'clusty').exists()
    p = run(*args, '--tani', '0.7', '--mcl-inflation', '2.5')
    assert p.returncode == 1 and 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'bin/clusty' not in p.stderr, p.stderr
    assert '--algorithm mcl --mcl-inflation 2.5' in p.stderr and not (tmp_path / 'c.tsv').exists()


def test_cluster_call_carries_the_mcl_keys_only_under_mcl():
    base = dict(input_path='a', ids_path='b', output_path='c', metric='tani', num_alns=0, representatives=False, tani=0.7, gani=0, ani=0,
                qcov=0, rcov=0, len_ratio=0, mcl_inflation=2.5, mcl_prune=1e-4, mcl_max_row=128, mcl_iterations=100)
    call = cli.cluster_call(types.SimpleNamespace(algorithm='mcl', **base))
    assert {k: v for k, v in call.items() if k.startswith('mcl_')} == dict(mcl_inflation=2.5, mcl_prune=1e-4, mcl_max_row=128, mcl_iterations=100)
    for algo in ('single', 'average', 'leiden'):
        assert not [k for k in cli.cluster_call(types.SimpleNamespace(algorithm=algo, **base)) if k.startswith('mcl_')], algo
    sub = next(x for x in cli.get_parser()._actions if getattr(x, 'choices', None) and 'cluster' in x.choices).choices['cluster']
    assert 'mcl' in next(x for x in sub._actions if x.dest == 'algorithm').choices
    assert 'multiple of 0.5' in next(x for x in sub._actions if x.dest == 'mcl_inflation').help
