"""The cluster report (`cluster --out-stats`) without a GPU: hand-worked cases of the restatement with the expected integers and the
expected text written out, the golden example, the reader of clusters.tsv (restatement and library give the same file:line), the C
ABI and Python surface of vg_cluster_stats_graph / vg_cluster_stats_file, and the argument and CLI errors that need no device."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_stats_restatement as cs
from vclust_amd import _lib, api

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
U = 1 << 32


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


def record(**kw):
    base = dict(size=0, rep=-1, pairs=0, linked=0, sum=0, min=0, external=0, nearest=-1, nearest_max=0, nearest_sum=0, misfits=0)
    base.update(kw)
    return base


# ---------------------------------------------------------------- hand-worked cases
def test_a_triangle_with_one_missing_pair_and_a_singleton_beside_it():
    rows = [(0, 1, 0.5), (2, 1, 0.25), (1, 2, 0.125), (3, 0, 0.125), (3, 3, 1.0)]      # a reverse row (the max counts), a self row
    rec, own, oth_max, oth = cs.stats_graph(4, rows, [0, 0, 0, 1], 2)
    assert rec[0] == record(size=3, rep=0, pairs=3, linked=2, sum=3 * U // 4, min=U // 4, external=1, nearest=1, nearest_max=U // 8,
                            nearest_sum=U // 8)
    assert rec[1] == record(size=1, rep=3, external=1, nearest=0, nearest_max=U // 8, nearest_sum=U // 8, misfits=1)
    assert own == [U // 2, U // 2, U // 4, 0] and oth_max == [U // 8, 0, 0, U // 8] and oth == [1, -1, -1, 0]
    text = cs.report(['a', 'b', 'c', 'd'], rows, ['cluster'], [[0, 0, 0, 1]], [['7', '4']]).decode()
    assert text == ('column\tcluster\tsize\trepresentative\tpairs\tlinked\tmin_tani\tmean_linked\tmean_all\texternal\tnearest\tnearest_tani\t'
                    'nearest_mean\tmisfits\n'
                    'cluster\t7\t3\ta\t3\t2\t0.25\t0.375\t0.25\t1\t4\t0.125\t0.0416667\t0\n'
                    'cluster\t4\t1\td\t0\t0\t-\t-\t-\t1\t7\t0.125\t0.0416667\t1\n')


def test_an_isolated_singleton_and_an_unused_label():
    rec, own, oth_max, oth = cs.stats_graph(1, [], [2], 3)
    assert rec == [record(), record(), record(size=1, rep=0)]
    assert (own, oth_max, oth) == ([0], [0], [-1])
    assert cs.report(['x'], [], ['tani_0.9'], [[0]], [['x']], 'ani').decode().split('\n')[1] == 'tani_0.9\tx\t1\tx\t0\t0\t-\t-\t-\t0\t-\t-\t-\t0'


def test_a_tie_of_the_strongest_link_goes_to_the_smallest_label():
    rows = [(0, 1, 0.5), (0, 2, 0.5), (0, 3, 0.25)]
    rec, own, oth_max, oth = cs.stats_graph(4, rows, [0, 2, 1, 1], 3)            # object 1 is cluster 2; objects 2, 3 are cluster 1
    assert (rec[0]['nearest'], rec[0]['nearest_max'], rec[0]['nearest_sum'], rec[0]['external']) == (1, U // 2, 3 * U // 4, 3)
    assert oth == [1, 0, 0, 0] and oth_max == [U // 2, U // 2, U // 2, U // 4]
    assert (rec[1]['nearest'], rec[1]['rep'], rec[1]['size']) == (0, 2, 2) and (rec[2]['nearest'], rec[2]['rep']) == (0, 1)
    assert [r['misfits'] for r in rec] == [1, 2, 1]                              # no object has an edge inside its cluster


def test_a_misfit_and_an_equality_that_is_none():
    rows = [(0, 1, 0.5), (1, 2, 0.75), (2, 3, 0.75)]
    rec, own, oth_max, oth = cs.stats_graph(4, rows, [0, 0, 1, 1], 2)
    assert own == [U // 2, U // 2, 3 * U // 4, 3 * U // 4] and oth_max == [0, 3 * U // 4, 3 * U // 4, 0]
    assert (rec[0]['misfits'], rec[1]['misfits']) == (1, 0)                      # object 1 is closer to cluster 1; object 2 is tied
    assert (rec[0]['linked'], rec[0]['min'], rec[1]['sum']) == (1, U // 2, 3 * U // 4)


def test_weight_one_needs_33_bits_and_weight_zero_is_an_edge():
    rows = [(0, 1, 1.0), (1, 2, 0.0)]
    rec, own, oth_max, oth = cs.stats_graph(3, rows, [0, 0, 1], 2)
    assert rec[0] == record(size=2, rep=0, pairs=1, linked=1, sum=U, min=U, external=1, nearest=1)
    assert rec[1] == record(size=1, rep=2, external=1, nearest=0)
    assert own == [U, U, 0] and oth_max == [0, 0, 0] and oth == [-1, 1, 0]
    lines = cs.report(['a', 'b', 'c'], rows, ['cluster'], [[0, 0, 1]], [['0', '1']]).decode().split('\n')
    assert lines[1] == 'cluster\t0\t2\ta\t1\t1\t1\t1\t1\t1\t1\t0\t0\t0'
    assert lines[2] == 'cluster\t1\t1\tc\t0\t0\t-\t-\t-\t1\t0\t0\t0\t0'
    assert cs.quanta(1.0) == U and cs.quanta(0.5 + 2.0 ** -33) == U // 2 and cs.quanta(0.5 + 3 * 2.0 ** -33) == U // 2 + 2    # ties to even
    with pytest.raises(ValueError):
        cs.quanta(1.5)
    with pytest.raises(ValueError):
        cs.quanta(float('nan'))


def test_printed_quotients_are_the_exact_division():
    # 1 / 3 of 2^32-quanta, a quotient that a division of rounded operands gets wrong in the last place, and the library's division
    assert cs.quotient(U, 3) == '0.333333' and cs.quotient(2 * U, 3) == '0.666667' and cs.quotient(0, 5) == '0' and cs.quotient(7, 0) == '-'
    rng = np.random.default_rng(4)
    for _ in range(2000):
        s, p = int(rng.integers(0, 1 << 62)), int(rng.integers(1, 1 << 40))
        assert '%.6g' % api.cluster_average_similarity(s, p) == cs.quotient(s, p)


# ---------------------------------------------------------------- the golden example
def test_golden_example(out_dir):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    rows = cr.read_rows(out_dir / 'ani.tsv', len(ids), 'tani', tani=0.95)
    names, label, text = cs.read_clusters(out_dir / 'clusters.tsv', ids)
    assert names == ['cluster'] and text == [['3', '0', '1', '4', '5', '2']] and label[0] == [0, 1, 1, 1, 2, 2, 3, 4, 5, 5, 5, 5]
    rec = cs.stats_graph(len(ids), rows, label[0], len(text[0]))[0]
    assert sum(r['size'] for r in rec) == len(ids)
    assert all(r['linked'] <= r['pairs'] for r in rec)
    assert sum(r['external'] for r in rec) % 2 == 0
    assert all(r['nearest'] != k for k, r in enumerate(rec))
    assert [r['rep'] for r in rec] == sorted(r['rep'] for r in rec)
    report = cs.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', out_dir / 'clusters.tsv', tani=0.95).decode().split('\n')
    assert len(report) == 8 and report[1].split('\t')[:4] == ['cluster', '3', '1', 'NC_025457.alt2']
    # without a filter every row is an edge: the clusters are less separate, the sizes are the same
    loose = cs.stats_graph(len(ids), cr.read_rows(out_dir / 'ani.tsv', len(ids), 'tani'), label[0], len(text[0]))[0]
    assert [r['size'] for r in loose] == [r['size'] for r in rec] and sum(r['external'] for r in loose) >= sum(r['external'] for r in rec)


# ---------------------------------------------------------------- the reader of clusters.tsv
def _clusters_file(tmp_path, out_dir, representatives=False):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    lines = (out_dir / 'clusters.tsv').read_text().split('\n')
    if representatives:                      # every cluster named by its LAST member
        last = {}
        for ln in lines[1:-1]:
            last[ln.split('\t')[1]] = ln.split('\t')[0]
        lines = [lines[0]] + [ln.split('\t')[0] + '\t' + last[ln.split('\t')[1]] for ln in lines[1:-1]] + ['']
    return ids, lines


# the library's full message of every case below, behind "<file>:<line>: " (recorded before the two label-file parsers became one)
CLUSTERS_MESSAGES = {
    'unknown id': "object 'no_such_genome' is not in the ids file",
    'repeated id': "object 'NC_005091.alt2' is listed twice",
    'missing id': "object 'NC_005091.alt1' of the ids file is missing",
    'negative label': "malformed cluster number '-1'",
    'representative is not a member': "representative 'NC_002486' is not a member of its cluster",
    'representative outside the ids': "representative 'no_such_genome' is not in the ids file",
    'bad header': 'malformed header (expected object<TAB>cluster, then further label columns)',
    'a field too many': 'malformed line (expected 2 fields)',
}


@pytest.mark.parametrize('case,representatives,mutate,line,msg', [
    ('unknown id', False, lambda ls: ls.__setitem__(3, 'no_such_genome\t2'), 4, 'not in the ids file'),
    ('repeated id', False, lambda ls: ls.__setitem__(5, ls[2]), 6, 'listed twice'),
    ('missing id', False, lambda ls: ls.__delitem__(4), 12, 'is missing'),
    ('negative label', False, lambda ls: ls.__setitem__(6, ls[6].split('\t')[0] + '\t-1'), 7, 'malformed cluster number'),
    ('representative is not a member', True, lambda ls: ls.__setitem__(2, ls[2].split('\t')[0] + '\t' + ls[5].split('\t')[0]), 3,
     'not a member of its cluster'),
    ('representative outside the ids', True, lambda ls: ls.__setitem__(2, ls[2].split('\t')[0] + '\tno_such_genome'), 3, 'not in the ids file'),
    ('bad header', False, lambda ls: ls.__setitem__(0, 'objects\tcluster'), 1, 'malformed header'),
    ('a field too many', False, lambda ls: ls.__setitem__(4, ls[4] + '\t1'), 5, 'malformed line'),
])
def test_clusters_file_errors_before_device_use(case, representatives, mutate, line, msg, tmp_path, out_dir):
    """Restatement and library refuse the same line, on a machine with or without a device (the parse runs first)."""
    ids, lines = _clusters_file(tmp_path, out_dir, representatives)
    mutate(lines)
    bad = tmp_path / 'bad_clusters.tsv'
    bad.write_text('\n'.join(lines))
    with pytest.raises(cs.ClustersError) as ce:
        cs.read_clusters(bad, ids, representatives)
    assert f'{bad}:{line}: ' in str(ce.value) and msg in str(ce.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_stats(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', bad, tmp_path / 's.tsv', clusters_repr=representatives, tani=0.95)
    assert e.value.code == -1 and str(e.value) == f'libvclust_gpu error -1: {bad}:{line}: {CLUSTERS_MESSAGES[case]}', str(e.value)
    assert not (tmp_path / 's.tsv').exists()


def test_restatement_reads_numbers_ids_and_several_columns(tmp_path, out_dir):
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')[:4]
    path = tmp_path / 'c.tsv'
    path.write_text(f'object\tcluster\ttani_0.9\r\n{ids[2]}\t7\t007\r\n{ids[0]}\t12\t7\r\n\r\n{ids[3]}\t7\t3\r\n{ids[1]}\t12\t3')
    names, label, text = cs.read_clusters(path, ids)
    assert names == ['cluster', 'tani_0.9'] and label == [[0, 0, 1, 1], [0, 1, 0, 1]] and text == [['12', '7'], ['7', '3']]
    path.write_text(f'object\tcluster\n{ids[2]}\t{ids[3]}\n{ids[0]}\t{ids[0]}\n{ids[3]}\t{ids[3]}\n{ids[1]}\t{ids[0]}\n')
    names, label, text = cs.read_clusters(path, ids, True)
    assert label == [[0, 0, 1, 1]] and text == [[ids[0], ids[3]]]


# ---------------------------------------------------------------- the C ABI and the Python surface
def test_stats_symbols_exported_and_callable():
    header = (_lib.PKG_DIR.parent / 'include' / 'vclust_gpu.h').read_text()
    lib = _lib.load()
    for name in ('vg_cluster_stats_graph', 'vg_cluster_stats_file'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header, name
    assert '} vg_cluster_stat;' in header
    assert len(_lib.SYMBOLS['vg_cluster_stats_graph'][1]) == 11 and len(_lib.SYMBOLS['vg_cluster_stats_file'][1]) == 6
    assert callable(api.cluster_stats_graph) and callable(api.cluster_stats)
    assert api.CLUSTER_STAT_DTYPE.names == cs.FIELDS and api.CLUSTER_STAT_DTYPE.itemsize == 88
    # what exists keeps its shape
    assert len(_lib.SYMBOLS['vg_cluster'][1]) == 4 and len(_lib.SYMBOLS['vg_cluster_update'][1]) == 7 and len(_lib.SYMBOLS['vg_cluster_linkage'][1]) == 7
    assert len(_lib.ClusterParams._fields_) == 12


def test_bad_array_arguments_are_refused_before_any_device_use():
    for w, msg in (([0.9, 1.5], 'outside [0, 1]'), ([float('nan'), 0.5], 'NaN'), ([-0.25, 0.5], 'outside [0, 1]'), ([float('inf'), 0.5], 'outside [0, 1]')):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster_stats_graph(3, [0, 1], [1, 2], w, [0, 0, 1])
        assert e.value.code == -1 and msg in str(e.value), str(e.value)
    for label, k in (([0, 2, 1], 2), ([0, -1, 1], 2), ([0, 0, 0], 0)):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster_stats_graph(3, [0, 1], [1, 2], [0.9, 0.8], label, k)
        assert e.value.code == -1 and 'label[' in str(e.value), str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_stats_graph(3, [0], [3], [0.9], [0, 0, 0])
    assert e.value.code == -1 and 'outside' in str(e.value)
    with pytest.raises(ValueError):
        api.cluster_stats_graph(3, [0], [1], [0.9], [0, 0])
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_stats_graph(1 << 31, [], [], [], [])
    assert e.value.code == -6
    # no object: valid, and no device is needed for it
    rec, own, oth_max, oth = api.cluster_stats_graph(0, [], [], [], [], 2)
    assert len(own) == len(oth_max) == len(oth) == 0
    assert [{f: int(r[f]) for f in cs.FIELDS} for r in rec] == cs.stats_graph(0, [], [], 2)[0]


def test_stats_graph_without_device_fails_loudly():
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_stats_graph(3, [0, 1], [1, 2], [0.9, 0.8], [0, 0, 1])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)


# ---------------------------------------------------------------- the CLI
def test_cli_without_out_stats_is_unchanged_and_with_it_makes_a_second_call(out_dir, tmp_path):
    from vclust_amd import cli
    out, stats = tmp_path / 'c.tsv', tmp_path / 's.tsv'
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', out, '--algorithm', 'cd-hit', '--tani', '0.95', '-r']
    plain = f'Running: libvclust_gpu cluster --algorithm cd-hit --metric tani --tani 0.95 --out-repr [1 GPU] -> {out}'
    p = run(*base, '-v', '1')
    assert plain in p.stderr and 'cluster-stats' not in p.stderr, p.stderr
    p = run(*base, '--out-stats', stats, '-v', '1')
    assert plain in p.stderr, p.stderr
    second = f'Running: libvclust_gpu cluster-stats --metric tani --tani 0.95 --out-repr --clusters {out} [1 GPU] -> {stats}'
    if api.device_count() > 0:
        assert p.returncode == 0 and second in p.stderr and p.stderr.count('Completed') == 2 and stats.exists(), p.stderr
    else:
        assert p.returncode == 1 and 'ERROR' in p.stderr and 'no HIP device' in p.stderr, p.stderr
        assert 'bin/clusty' not in p.stderr and not stats.exists() and not out.exists()
    assert '--out-stats' in run('cluster', '--help').stdout
    old = sys.argv
    try:
        sys.argv = ['vclust.py', *map(str, base)]
        args = cli.get_parser().parse_args(sys.argv[1:])
        assert args.stats_path is None and 'stats_path' not in cli.cluster_call(args) and 'out_stats' not in cli.cluster_call(args)
        sys.argv = ['vclust.py', *map(str, base), '--out-stats', str(stats), '--qcov', '0.5', '--num_alns', '3']
        args = cli.get_parser().parse_args(sys.argv[1:])
        assert cli.cluster_stats_call(args) == dict(ani_path=out_dir / 'ani.tsv', ids_path=out_dir / 'ani.ids.tsv', clusters_path=out,
                                                    out_path=stats, clusters_repr=True, metric='tani', num_alns=3, tani=0.95, qcov=0.5)
    finally:
        sys.argv = old


def test_cli_metric_threshold_is_required_as_before(out_dir, tmp_path):
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--out-stats', tmp_path / 's.tsv')
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr
    assert not (tmp_path / 's.tsv').exists()
