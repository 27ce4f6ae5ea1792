"""The update of a prior clustering (`cluster --prior`) without a GPU: the restatement's hand cases and its three properties
against cluster_restatement, the C ABI and Python surface of vg_cluster_update / vg_cluster_update_graph, and the CLI's usage
errors, prior-file errors and `Running:` lines (no device needed for any of it)."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_update_restatement as cu
from vclust_amd import _lib, api

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


# ---------------------------------------------------------------- hand cases of the restatement
def test_a_longer_new_object_joins_the_prior_representative_and_does_not_replace_it():
    prior = [-1, 1, 1]                       # object 0 (the longest) is new; {1, 2} is a prior cluster of representative 1
    for algo in ('cd-hit', 'uclust'):
        label, rep, st = cu.update_graph(3, [(0, 1, 0.9)], prior, algo)
        assert (label, rep) == ([0, 0, 0], [1, 1, 1])
        assert (st['joined_prior'], st['joined_new'], st['founded']) == (1, 0, 0)
    # single: same cluster, and the representative is the earliest member
    assert cu.update_graph(3, [(0, 1, 0.9)], prior, 'single')[:2] == ([0, 0, 0], [0, 0, 0])


def test_an_edge_to_a_prior_member_only_founds_a_cluster():
    prior = [-1, 1, 1]
    for algo in ('cd-hit', 'uclust'):
        label, rep, st = cu.update_graph(3, [(0, 2, 0.9)], prior, algo)
        assert (label, rep) == ([1, 0, 0], [0, 1, 1]) and st['founded'] == 1
    assert cu.update_graph(3, [(0, 2, 0.9)], prior, 'single')[:2] == ([0, 0, 0], [0, 0, 0])


def test_a_uclust_tie_between_a_prior_and_a_new_representative_goes_to_the_prior_one():
    prior = [-1, -1, 2]                      # visit order 2, 0, 1: object 1 is tied between 0 (new, founded) and 2 (prior)
    rows = [(1, 0, 0.9), (1, 2, 0.9)]
    label, rep, st = cu.update_graph(3, rows, prior, 'uclust')
    assert rep == [0, 2, 2] and label == [1, 0, 0]
    assert (st['joined_prior'], st['joined_new'], st['founded']) == (1, 0, 1)
    assert cr.cluster_graph(3, rows, 'uclust')[1] == [0, 0, 2]            # (the plain run gives it to the earlier index)
    assert cu.update_graph(3, [(1, 0, 0.95), (1, 2, 0.9)], prior, 'uclust')[1] == [0, 0, 2]       # no tie: the heavier one


def test_a_new_object_bridges_two_prior_clusters():
    prior = [0, 0, 2, 2, -1]
    rows = [(4, 1, 0.9), (4, 2, 0.9)]
    label, rep, st = cu.update_graph(5, rows, prior, 'single')
    assert (label, rep) == ([0] * 5, [0] * 5) and st['prior_merged'] == 1 and st['joined_prior'] == 1
    for algo in ('cd-hit', 'uclust'):        # 1 is a member: the only representative 4 is linked to is 2
        label, rep, st = cu.update_graph(5, rows, prior, algo)
        assert (label, rep) == ([0, 0, 1, 1, 1], [0, 0, 2, 2, 2]) and st['prior_merged'] == 0


def test_a_row_between_two_prior_clusters_is_ignored():
    prior = [0, 1, -1]
    for algo in cu.ALGORITHMS:
        label, rep, st = cu.update_graph(3, [(0, 1, 1.0), (1, 0, 0.99)], prior, algo)
        assert (label, rep) == ([0, 1, 2], [0, 1, 2]) and st['n_edges'] == 0 and st['prior_merged'] == 0


def test_a_prior_representative_need_not_be_the_earliest_member():
    prior = [2, -1, 2]                       # as --prior-repr may say: the representative of {0, 2} is 2
    label, rep, _ = cu.update_graph(3, [(1, 2, 0.9)], prior, 'cd-hit')
    assert (label, rep) == ([0, 0, 0], [2, 2, 2])
    label, rep, _ = cu.update_graph(3, [(1, 0, 0.9)], prior, 'cd-hit')     # 0 is a member here
    assert (label, rep) == ([0, 1, 0], [2, 1, 2])


# ---------------------------------------------------------------- properties P1, P2, P3 of the restatement
def _random_graph(seed, n=200, rows=700):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, n, rows)
    r = np.where(rng.random(rows) < 0.7, np.clip(q + rng.integers(-8, 9, rows), 0, n - 1), rng.integers(0, n, rows))
    w = np.round(rng.uniform(0.7, 1.0, rows), 2)                           # two decimals: ties occur
    return rng, [(int(a), int(b), float(x)) for a, b, x in zip(q, r, w)]


def _inside(rows, members):
    return [(a, b, w) for a, b, w in rows if a in members and b in members]


def _with_new_end(rows, members):
    return [(a, b, w) for a, b, w in rows if a not in members or b not in members]


@pytest.mark.parametrize('seed', range(6))
def test_p1_single_update_equals_single_on_the_whole_graph(seed):
    n = 200
    rng, rows = _random_graph(seed)
    D = set(np.flatnonzero(rng.random(n) < rng.choice([0.3, 0.7, 0.95])).tolist())
    cid = cr.cluster_ids(n, cr.edges(_inside(rows, D)), 'single')
    prior = cu.prior_of(cid, D)
    want = cr.cluster_graph(n, rows, 'single')
    assert cu.update_graph(n, _with_new_end(rows, D), prior, 'single')[:2] == want
    assert cu.update_graph(n, rows, prior, 'single')[:2] == want           # rows inside D change nothing


@pytest.mark.parametrize('algo', ['cd-hit', 'uclust'])
@pytest.mark.parametrize('seed', range(6))
def test_p2_frozen_update_equals_the_plain_run_when_prior_objects_come_first(seed, algo):
    n = 200
    rng, rows = _random_graph(seed)
    D = set(range(int(rng.integers(1, n))))
    prior = cu.prior_of(cr.cluster_ids(n, cr.edges(_inside(rows, D)), algo), D)
    want_label, want_rep = cr.cluster_graph(n, rows, algo)
    label, rep, st = cu.update_graph(n, _with_new_end(rows, D), prior, algo)
    assert (label, rep) == (want_label, want_rep)
    assert st['joined_prior'] + st['joined_new'] + st['founded'] == st['n_new'] == n - len(D)


@pytest.mark.parametrize('algo', cu.ALGORITHMS)
@pytest.mark.parametrize('seed', range(3))
def test_p3_empty_and_full_priors(seed, algo):
    n = 200
    rng, rows = _random_graph(seed)
    assert cu.update_graph(n, rows, [-1] * n, algo)[:2] == cr.cluster_graph(n, rows, algo)
    # a prior that covers every object comes back, renumbered by the output rule, whatever the rows say
    cluster_of = rng.integers(0, 40, n)
    heads = {}
    for i in rng.permutation(n):             # any member may be the representative
        heads.setdefault(int(cluster_of[i]), int(i))
    prior = [heads[int(c)] for c in cluster_of]
    label, rep, st = cu.update_graph(n, rows, prior, algo)
    assert label == cr.labels(prior)[0] and st['n_edges'] == 0 and st['n_new'] == 0
    assert rep == (cr.labels(prior)[1] if algo == 'single' else prior)


# ---------------------------------------------------------------- the C ABI and the Python surface
def test_update_symbols_exported_and_callable():
    lib = _lib.load()
    for name in ('vg_cluster_update', 'vg_cluster_update_graph'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert callable(api.cluster_update) and callable(api.cluster_update_graph)
    assert _lib.UPDATE_ALGORITHMS == {'single': 0, 'cd-hit': 1, 'uclust': 2}
    assert _lib.CLUSTER_ALGORITHMS == {'single': 0, 'cd-hit': 1, 'uclust': 2, 'set-cover': 3}
    assert _lib.LINKAGE_ALGORITHMS == {'single': 0, 'complete': 4}
    with pytest.raises(ValueError):
        api.cluster_update_graph(2, [0], [1], [1.0], [-1, -1], 'set-cover')


def _update_rc(n, q, r, w, prior, algorithm):
    """the raw C call (any algorithm number) -> its return code"""
    import ctypes as C
    P = C.POINTER
    q, r, w = np.asarray(q, np.uint32), np.asarray(r, np.uint32), np.asarray(w, np.float64)
    prior = np.asarray(prior, np.int32)
    label, rep = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    return _lib.load().vg_cluster_update_graph(n, q.ctypes.data_as(P(C.c_uint32)), r.ctypes.data_as(P(C.c_uint32)), w.ctypes.data_as(P(C.c_double)),
                                               len(q), algorithm, prior.ctypes.data_as(P(C.c_int32)), label.ctypes.data_as(P(C.c_int32)),
                                               rep.ctypes.data_as(P(C.c_int32)), None)


def test_update_graph_argument_errors_need_no_device():
    for prior, msg in (([-1, 3, -1], 'outside'), ([-2, -1, -1], 'outside'), ([1, 2, 2], 'not its own representative'), ([-1, 0, -1], 'not its own')):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster_update_graph(3, [0], [1], [0.9], prior, 'cd-hit')
        assert e.value.code == -1 and msg in str(e.value), str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_update_graph(3, [0], [3], [1.0], [-1, -1, -1])
    assert e.value.code == -1 and 'outside' in str(e.value)
    for algorithm in (3, 4, 5, -1):          # set-cover and the hierarchies
        assert _update_rc(3, [0], [1], [0.9], [-1, -1, -1], algorithm) == -1
    assert 'single, cd-hit or uclust' in _lib.load().vg_last_error().decode()
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_update_graph(1 << 31, [], [], [], [])
    assert e.value.code == -6
    label, rep, stats = api.cluster_update_graph(0, [], [], [], [])
    assert len(label) == len(rep) == 0 and stats['n_edges'] == stats['n_new'] == 0


def test_update_graph_without_device_fails_loudly():
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_update_graph(3, [0, 1], [1, 2], [0.9, 0.8], [0, -1, -1], 'uclust')
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)


# ---------------------------------------------------------------- the CLI
def _prior_file(tmp_path, out_dir, keep=8, representatives=False, name='prior.tsv'):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    path = tmp_path / name
    path.write_text('object\tcluster\n' + ''.join(f'{x}\t{x if representatives else k}\n' for k, x in enumerate(ids[:keep])))
    return path


def test_cli_usage_errors_exit_2(out_dir, tmp_path):
    prior = _prior_file(tmp_path, out_dir)
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.95']
    for algo in ('set-cover', 'complete', 'average', 'leiden'):
        p = run(*base, '--prior', prior, '--algorithm', algo)
        assert p.returncode == 2 and '--prior' in p.stderr and algo in p.stderr, (algo, p.stderr)
    for extra in (['--out-linkage', tmp_path / 'l.tsv'], ['--levels', '0.97']):
        p = run(*base, '--prior', prior, *extra)
        assert p.returncode == 2 and '--prior' in p.stderr, p.stderr
    p = run(*base, '--prior-repr')
    assert p.returncode == 2 and '--prior-repr' in p.stderr and 'needs --prior' in p.stderr, p.stderr
    p = run(*base, '--prior', tmp_path / 'missing.tsv')
    assert p.returncode == 2
    assert not (tmp_path / 'c.tsv').exists()


def _mutated(tmp_path, out_dir, mutate, representatives):
    path = _prior_file(tmp_path, out_dir, representatives=representatives, name='bad_prior.tsv')
    lines = path.read_text().split('\n')
    mutate(lines)
    path.write_text('\n'.join(lines))
    return path


# the library's full message of every case below, behind "<file>:<line>: " (recorded before the two label-file parsers became one)
PRIOR_MESSAGES = {
    'unknown name': "object 'no_such_genome' is not in the ids file",
    'listed twice': "object 'NC_005091.alt2' is listed twice",
    'no tab': 'malformed line (expected <object><TAB><cluster>)',
    'three fields': 'malformed line (expected <object><TAB><cluster>)',
    'not a number': "malformed cluster number 'x7'",
    'bad header': 'malformed header (expected object<TAB>cluster)',
    'representative outside the file': "representative 'no_such_genome' is not an object of this file",
    'representative is a member': "representative 'NC_005091' is not its own representative",
}


@pytest.mark.parametrize('case,representatives,mutate,line,msg', [
    ('unknown name', False, lambda ls: ls.__setitem__(3, 'no_such_genome\t2'), 4, 'not in the ids file'),
    ('listed twice', False, lambda ls: ls.__setitem__(5, ls[2]), 6, 'listed twice'),
    ('no tab', False, lambda ls: ls.__setitem__(4, ls[4].replace('\t', ' ')), 5, 'malformed'),
    ('three fields', False, lambda ls: ls.__setitem__(4, ls[4] + '\t1'), 5, 'malformed'),
    ('not a number', False, lambda ls: ls.__setitem__(6, ls[6].split('\t')[0] + '\tx7'), 7, 'malformed'),
    ('bad header', False, lambda ls: ls.__setitem__(0, 'object\tclusters'), 1, 'malformed'),
    ('representative outside the file', True, lambda ls: ls.__setitem__(2, ls[2].split('\t')[0] + '\tno_such_genome'), 3, 'not an object of this file'),
    ('representative is a member', True, lambda ls: (ls.__setitem__(2, ls[2].split('\t')[0] + '\t' + ls[3].split('\t')[0]),
                                                     ls.__setitem__(3, ls[3].split('\t')[0] + '\t' + ls[4].split('\t')[0])), 3,
     'not its own representative'),
])
def test_prior_file_errors_before_device_use(case, representatives, mutate, line, msg, tmp_path, out_dir):
    """Each error exits 1 with file and line, on a machine with or without a device (the parse runs first)."""
    bad = _mutated(tmp_path, out_dir, mutate, representatives)
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    with pytest.raises(cu.PriorError) as pe:
        cu.read_prior(bad, ids, representatives)
    assert f'{bad}:{line}: ' in str(pe.value)
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.95',
            '--prior', bad, *(['--prior-repr'] if representatives else []))
    assert p.returncode == 1 and 'ERROR' in p.stderr
    assert f'{bad}:{line}: ' in p.stderr and msg in p.stderr, p.stderr
    assert not (tmp_path / 'c.tsv').exists()
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_update(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', bad, tmp_path / 'c.tsv', prior_repr=representatives, tani=0.95)
    assert e.value.code == -1 and str(e.value) == f'libvclust_gpu error -1: {bad}:{line}: {PRIOR_MESSAGES[case]}'


def test_restatement_reads_both_forms_of_the_prior_file(tmp_path, out_dir):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    path = tmp_path / 'p.tsv'
    path.write_text(f'object\tcluster\n{ids[5]}\t1\n{ids[2]}\t0\n{ids[7]}\t1\n\n{ids[0]}\t0\n')
    want = [-1] * len(ids)
    want[0] = want[2] = 0
    want[5] = want[7] = 5
    assert cu.read_prior(path, ids) == want
    path.write_text(f'object\tcluster\n{ids[5]}\t{ids[7]}\n{ids[2]}\t{ids[2]}\n{ids[7]}\t{ids[7]}\n{ids[0]}\t{ids[2]}\n')
    want[0] = want[2] = 2
    want[5] = want[7] = 7
    assert cu.read_prior(path, ids, True) == want


def test_stage_call_rejects_excluded_combinations(tmp_path, out_dir):
    prior = _prior_file(tmp_path, out_dir)
    paths = (out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv')
    with pytest.raises(ValueError):
        api.cluster(*paths, algorithm='set-cover', prior_path=prior, tani=0.95)
    with pytest.raises(ValueError):
        api.cluster(*paths, algorithm='single', prior_path=prior, levels=[0.97], tani=0.95)
    with pytest.raises(ValueError):
        api.cluster(*paths, prior_repr=True, tani=0.95)


def test_running_lines_with_and_without_prior(out_dir, tmp_path):
    """Without --prior the `Running:` line and the call are those of the commit before --prior existed; with it, the line names
    the file (and the run goes to the library even where bin/clusty exists)."""
    from vclust_amd import cli
    prior = _prior_file(tmp_path, out_dir, representatives=True)
    out = tmp_path / 'c.tsv'
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', out, '--algorithm', 'cd-hit', '--tani', '0.95', '-r']
    plain = f'Running: libvclust_gpu cluster --algorithm cd-hit --metric tani --tani 0.95 --out-repr [1 GPU] -> {out}'
    p = run(*base)
    assert plain in p.stderr and '--prior' not in p.stderr, p.stderr
    p = run(*base, '--prior', prior, '--prior-repr')
    want = f'Running: libvclust_gpu cluster --algorithm cd-hit --metric tani --tani 0.95 --out-repr --prior {prior} --prior-repr [1 GPU] -> {out}'
    assert want in p.stderr, p.stderr
    if api.device_count() > 0:
        assert p.returncode == 0 and 'Prior clustering updated: 8 prior + 4 new genomes' in p.stderr, p.stderr
    else:
        assert p.returncode == 1 and 'no HIP device' in p.stderr and not out.exists(), p.stderr
    # the call: no new key without --prior
    old = sys.argv
    try:
        sys.argv = ['vclust.py', *map(str, base)]
        call = cli.cluster_call(cli.get_parser().parse_args(sys.argv[1:]))
        assert 'prior_path' not in call and 'prior_repr' not in call
        sys.argv = ['vclust.py', *map(str, base), '--prior', str(prior)]
        call = cli.cluster_call(cli.get_parser().parse_args(sys.argv[1:]))
        assert call['prior_path'] == prior and call['prior_repr'] is False
    finally:
        sys.argv = old
