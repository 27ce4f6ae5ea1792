"""The cluster stage without a GPU: the restatement against the golden clusters.tsv, the C ABI and Python surface of
vg_cluster / vg_cluster_graph, and the CLI's dispatch and host-side validation (no device needed for any of it)."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
from vclust_amd import _lib, api

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


def test_restatement_reproduces_golden_clusters(out_dir):
    got = cr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', 'single', 'tani', tani=0.95)
    assert got == (out_dir / 'clusters.tsv').read_bytes()


def test_restatement_partition_equals_the_handoff_check(out_dir):
    import test_oracle_golden as tog
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    label, _ = cr.cluster_graph(len(ids), cr.read_rows(out_dir / 'ani.tsv', len(ids), 'tani', tani=0.95), 'single')
    groups = {}
    for x, lab in zip(ids, label):
        groups.setdefault(lab, set()).add(x)
    assert sorted(sorted(g) for g in groups.values()) == tog.single_linkage_partition(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv')


def test_restatement_algorithms_on_a_small_graph():
    # 0-1 (0.9), 0-2 (0.5), 1-2 (0.95), 3-4 (0.7), 5 alone
    rows = [(0, 1, 0.9), (2, 0, 0.5), (1, 2, 0.95), (2, 1, 0.6), (3, 4, 0.7), (4, 4, 1.0)]
    assert cr.cluster_graph(6, rows, 'single') == ([0, 0, 0, 1, 1, 2], [0, 0, 0, 3, 3, 5])
    assert cr.cluster_graph(6, rows, 'cd-hit') == ([0, 0, 0, 1, 1, 2], [0, 0, 0, 3, 3, 5])
    # uclust: 2 is linked to rep 0 only (1 is a member): joins 0
    assert cr.cluster_graph(6, rows, 'uclust')[0] == [0, 0, 0, 1, 1, 2]
    # a path 0-1-2-3: set cover picks 1 ({0, 1, 2}), then 3 alone; cd-hit: 0 {0, 1}, 2 {2, 3}
    path = [(0, 1, 1.0), (1, 2, 1.0), (2, 3, 1.0)]
    assert cr.cluster_graph(4, path, 'set-cover') == ([0, 0, 0, 1], [0, 0, 0, 3])
    assert cr.cluster_graph(4, path, 'cd-hit') == ([0, 0, 1, 1], [0, 0, 2, 2])
    # uclust picks the heavier representative; a tie goes to the earlier one
    tri = [(0, 2, 0.5), (1, 2, 0.8)]
    assert cr.cluster_graph(3, tri, 'uclust')[1] == [0, 1, 1]
    assert cr.cluster_graph(3, [(0, 2, 0.8), (1, 2, 0.8)], 'uclust')[1] == [0, 1, 0]


def test_new_symbols_exported_and_callable():
    lib = _lib.load()
    for name in ('vg_cluster', 'vg_cluster_graph'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert callable(api.cluster) and callable(api.cluster_graph)
    assert _lib.CLUSTER_ALGORITHMS == {'single': 0, 'cd-hit': 1, 'uclust': 2, 'set-cover': 3}
    with pytest.raises(ValueError):
        api.cluster_graph(2, [0], [1], [1.0], 'leiden')


def test_cluster_graph_argument_errors_need_no_device():
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_graph(3, [0], [3], [1.0])
    assert e.value.code == -1 and 'outside' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_graph(3, [0], [1], [float('nan')])
    assert e.value.code == -1
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_graph(1 << 31, [], [], [])
    assert e.value.code == -6
    label, rep, stats = api.cluster_graph(0, [], [], [])
    assert len(label) == len(rep) == 0 and stats['n_edges'] == 0


def test_cluster_graph_without_device_fails_loudly():
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster_graph(3, [0, 1], [1, 2], [0.9, 0.8], 'uclust')
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)


def test_cli_without_clusty_names_the_missing_device(out_dir, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    assert not (ROOT / 'bin' / 'clusty').exists()
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.95')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'bin/clusty' not in p.stderr, p.stderr
    assert not (tmp_path / 'c.tsv').exists()


def test_cli_keeps_clusty_only_algorithms_and_the_threshold_check(out_dir, tmp_path):
    args = ['-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv']
    for algo in ('complete', 'leiden'):
        p = run('cluster', *args, '--algorithm', algo, '--tani', '0.95')
        assert p.returncode == 1 and 'bin/clusty' in p.stderr
    p = run('cluster', *args, '--algorithm', 'cd-hit')
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr


def _bad_file(tmp_path, out_dir, mutate):
    lines = (out_dir / 'ani.tsv').read_text().split('\n')
    mutate(lines)
    path = tmp_path / 'bad.tsv'
    path.write_text('\n'.join(lines))
    return path


@pytest.mark.parametrize('case,mutate,line,msg', [
    ('missing column', lambda ls: ls.__setitem__(0, ls[0].replace('tani', 'xani')), 1, 'missing column tani'),
    ('qidx out of range', lambda ls: ls.__setitem__(7, '12' + ls[7][ls[7].index('\t'):]), 8, 'outside the ids file'),
    ('malformed number', lambda ls: ls.__setitem__(20, ls[20].replace('\t0.', '\t0.x', 1)), 21, 'malformed'),
])
def test_host_side_validation_before_device_use(case, mutate, line, msg, tmp_path, out_dir):
    """Each error exits 1 with file and line, on a machine with or without a device (the parse runs first)."""
    bad = _bad_file(tmp_path, out_dir, mutate)
    with pytest.raises(cr.RowError):
        cr.read_rows(bad, 12, 'tani', tani=0.95)
    p = run('cluster', '-i', bad, '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.95')
    assert p.returncode == 1 and 'ERROR' in p.stderr
    assert f'{bad}:{line}: ' in p.stderr and msg in p.stderr, p.stderr
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cluster(bad, out_dir / 'ani.ids.tsv', tmp_path / 'c.tsv', tani=0.95)
    assert e.value.code == -1


def big_ani_file(tmp_path, n=3000, rows=60000, seed=17):
    """An ids file and an ani.tsv above 2 MiB (so that four threads each parse a chunk of it): `rows` rows over n objects, a
    blank line here and there.  -> (ani path, ids path, the lines of the ani file)"""
    rng = np.random.default_rng(seed)
    ids = tmp_path / 'big.ids.tsv'
    ids.write_text('id\tseq_len\tno_parts\n' + ''.join('object_%06d\t1000\t1\n' % i for i in range(n)))
    q = rng.integers(0, n, size=rows); r = (q + rng.integers(1, 4, size=rows) * rng.integers(0, 2, size=rows) * 7) % n
    tani = rng.random(rows); ani = rng.random(rows)
    lines = ['qidx\tridx\tquery\treference\ttani\tani']
    for i in range(rows):
        lines.append('%d\t%d\tobject_%06d\tobject_%06d\t%.6f\t%.6f' % (q[i], r[i], q[i], r[i], tani[i], ani[i]))
        if i % 997 == 0:
            lines.append('')
    return tmp_path / 'big.tsv', ids, lines


def test_row_error_names_the_same_line_for_every_thread_count(tmp_path):
    """A malformed number deep in the last quarter of a file that four threads parse in chunks: the message, with its
    file:line, is that of one thread, and the line is the right one."""
    path, ids, lines = big_ani_file(tmp_path)
    at = len(lines) - len(lines) // 7
    while not lines[at]:
        at += 1
    f = lines[at].split('\t'); f[4] = '0.x5'; lines[at] = '\t'.join(f)
    path.write_text('\n'.join(lines) + '\n')
    assert path.stat().st_size > (2 << 20) + (1 << 19)
    seen = []
    for threads in (1, 4):
        with pytest.raises(_lib.VclustGpuError) as e:
            api.cluster(path, ids, tmp_path / 'c.tsv', tani=0.5, num_threads=threads)
        assert e.value.code == -1
        seen.append(str(e.value))
    assert seen[0] == seen[1] and seen[0].endswith(f"{path}:{at + 1}: malformed tani '0.x5'"), seen
    assert not (tmp_path / 'c.tsv').exists()


def test_filter_columns_are_required_only_when_used(tmp_path, out_dir):
    """`lite` has no query/reference columns; len_ratio / num_alns are needed only when their filter is on."""
    lines = (out_dir / 'ani.tsv').read_text().split('\n')
    head = lines[0].split('\t')
    keep = [i for i, h in enumerate(head) if h not in ('query', 'reference', 'len_ratio', 'num_alns')]
    path = tmp_path / 'cut.tsv'
    path.write_text('\n'.join('\t'.join(ln.split('\t')[i] for i in keep) for ln in lines if ln) + '\n')
    assert len(cr.read_rows(path, 12, 'tani', tani=0.95)) > 0
    with pytest.raises(cr.RowError):
        cr.read_rows(path, 12, 'tani', tani=0.95, len_ratio=0.5)
    for extra, msg in ((['--len_ratio', '0.5'], 'missing column len_ratio'), (['--num_alns', '3'], 'missing column num_alns')):
        p = run('cluster', '-i', path, '--ids', out_dir / 'ani.ids.tsv', '-o', tmp_path / 'c.tsv', '--tani', '0.95', *extra)
        assert p.returncode == 1 and msg in p.stderr, p.stderr


def test_restatement_random_graphs_are_self_consistent():
    """cd-hit / uclust representatives are earlier REPs linked to the member; set cover clusters are stars of their pick."""
    rng = np.random.default_rng(5)
    n = 300
    rows = [(int(a), int(b), float(w)) for a, b, w in zip(rng.integers(0, n, 900), rng.integers(0, n, 900), rng.choice([0.5, 0.7, 0.9], 900))]
    e = cr.edges(rows)
    adj = cr.adjacency(n, e)
    for algo in ('cd-hit', 'uclust'):
        rep = cr.cluster_ids(n, e, algo)
        for i in range(n):
            assert rep[rep[i]] == rep[i] and (rep[i] == i or rep[i] in adj[i] and rep[i] < i)
    asg = cr.cluster_ids(n, e, 'set-cover')
    for i in range(n):
        assert asg[asg[i]] == asg[i] and (asg[i] == i or asg[i] in adj[i])
