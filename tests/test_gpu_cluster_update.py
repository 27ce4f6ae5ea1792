"""The update of a prior clustering on the MI355X (vg_cluster_update / vg_cluster_update_graph, `cluster --prior`) against the
sequential restatement (tests/cluster_update_restatement.py), labels and representatives compared exactly; the properties P1
and P2 of DESIGN.md section 9 against the plain run on the device and against the golden clusters.tsv byte for byte."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_update_restatement as cu
from test_new2all_cpu import N_DB_EXAMPLE, write_split

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
EX = ROOT / 'tests' / 'golden' / 'example'


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


def _rows(q, r, w):
    return list(zip(map(int, q), map(int, r), map(float, w)))


def _check(api, n, q, r, w, prior, algo):
    """the device against the restatement: labels, representatives and every count the restatement has"""
    label, rep, stats = api.cluster_update_graph(n, q, r, w, prior, algo)
    want_label, want_rep, want_stats = cu.update_graph(n, _rows(q, r, w), list(prior), algo)
    assert list(rep) == want_rep, algo
    assert list(label) == want_label, algo
    assert {k: stats[k] for k in want_stats} == want_stats, algo
    return stats


# ---------------------------------------------------------------- random family graphs
def family_graph(seed, n=3000):
    """families of 5-60 objects in index order, rows inside them with two-decimal weights (ties), 2 % weak rows anywhere, and
    duplicate, reverse and self rows"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(5, 61, n // 5 + 1)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    starts = starts[starts < n]
    bounds = np.concatenate([starts, [n]])
    fam_start, fam_size = np.repeat(starts, np.diff(bounds)), np.repeat(np.diff(bounds), np.diff(bounds))
    rows = 6 * n
    q = rng.integers(0, n, rows)
    r = fam_start[q] + rng.integers(0, 1 << 30, rows) % fam_size[q]          # (q == r now and then: self rows)
    w = np.round(rng.uniform(0.8, 1.0, rows), 2)
    weak = rng.random(rows) < 0.02
    r[weak] = rng.integers(0, n, weak.sum())
    w[weak] = 0.5
    dup = rng.random(rows) < 0.2                                             # reverse rows of other weights, and plain duplicates
    q, r, w = (np.concatenate([q, r[dup], q[:50]]), np.concatenate([r, q[dup], r[:50]]),
               np.concatenate([w, np.round(rng.uniform(0.8, 1.0, dup.sum()), 2), w[:50]]))
    assert (q == r).any()
    return rng, q.astype(np.uint32), r.astype(np.uint32), w


@pytest.fixture(scope='module')
def graphs():
    """seed -> (n, q, r, w, D as a mask, the rows as tuples): built once, shared, never changed"""
    out = {}
    for seed in (11, 12, 13):
        rng, q, r, w = family_graph(seed)
        out[seed] = (3000, q, r, w, rng.random(3000) < 0.7, _rows(q, r, w))
    return out


def _prior_run(n, rows, mask, algo):
    """the plain run of the restatement on the graph among the objects of the mask, as a prior_rep"""
    D = set(np.flatnonzero(mask).tolist())
    inside = [(a, b, x) for a, b, x in rows if a in D and b in D]
    return np.array(cu.prior_of(cr.cluster_ids(n, cr.edges(inside), algo), D), np.int32)


@pytest.mark.parametrize('algo', cu.ALGORITHMS)
@pytest.mark.parametrize('seed', [11, 12, 13])
def test_family_graphs_equal_restatement(api, graphs, seed, algo):
    n, q, r, w, mask, rows = graphs[seed]
    prior = _prior_run(n, rows, mask, algo)
    st = _check(api, n, q, r, w, prior, algo)                 # (all the rows: those inside D are dropped on the device)
    assert 0 < st['n_prior'] < n and st['joined_prior'] > 0
    if algo == 'single':
        assert st['prior_merged'] > 0                         # new objects bridge prior clusters
    else:
        assert st['joined_new'] > 0 and st['founded'] > 0     # every outcome of a new object occurs


@pytest.mark.parametrize('seed', [11, 12])
def test_p1_single_on_the_device(api, graphs, seed):
    """update(single on G[D], the rows with an end outside D) == single on G, computed by the plain call"""
    n, q, r, w, mask, rows = graphs[seed]
    prior = _prior_run(n, rows, mask, 'single')
    keep = ~(mask[q] & mask[r])
    label, rep, _ = api.cluster_update_graph(n, q[keep], r[keep], w[keep], prior, 'single')
    want_label, want_rep, _ = api.cluster_graph(n, q, r, w, 'single')
    assert list(label) == list(want_label) and list(rep) == list(want_rep)


@pytest.mark.parametrize('algo', ['cd-hit', 'uclust'])
@pytest.mark.parametrize('seed', [11, 12])
def test_p2_frozen_update_on_the_device(api, graphs, seed, algo):
    """every prior object before every new one, prior = the plain run on G[D]: the update is the plain run on G"""
    n, q, r, w, _, rows = graphs[seed]
    mask = np.arange(n) < 2100
    plabel, prep, _ = api.cluster_graph(2100, *(x[mask[q] & mask[r]] for x in (q, r, w)), algo)
    prior = np.concatenate([prep, np.full(n - 2100, -1, np.int32)])
    keep = ~(mask[q] & mask[r])
    label, rep, st = api.cluster_update_graph(n, q[keep], r[keep], w[keep], prior, algo)
    want_label, want_rep, _ = api.cluster_graph(n, q, r, w, algo)
    assert list(label) == list(want_label) and list(rep) == list(want_rep)
    assert st['joined_prior'] + st['joined_new'] + st['founded'] == st['n_new'] == n - 2100


# ---------------------------------------------------------------- edge sizes and hand cases
@pytest.mark.parametrize('algo', cu.ALGORITHMS)
def test_sizes_0_and_1_and_the_two_trivial_priors(api, graphs, algo):
    empty = np.zeros(0, np.uint32)
    label, rep, st = api.cluster_update_graph(0, empty, empty, np.zeros(0), [], algo)
    assert len(label) == len(rep) == 0 and st['n_new'] == 0
    for prior in ([-1], [0]):
        _check(api, 1, empty, empty, np.zeros(0), prior, algo)
        _check(api, 1, np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.ones(2), prior, algo)       # self rows only
    n, q, r, w, mask, rows = graphs[13]
    # P3: no prior object -> the plain run; every object prior -> the prior, renumbered, whatever the rows say
    label, rep, st = api.cluster_update_graph(n, q, r, w, np.full(n, -1, np.int32), algo)
    want_label, want_rep, _ = api.cluster_graph(n, q, r, w, algo)
    assert list(label) == list(want_label) and list(rep) == list(want_rep) and st['n_prior'] == 0
    rng = np.random.default_rng(5)
    cluster_of, heads = rng.integers(0, 400, n), {}
    for i in rng.permutation(n):
        heads.setdefault(int(cluster_of[i]), int(i))          # (any member may be the representative)
    prior = np.array([heads[int(c)] for c in cluster_of], np.int32)
    st = _check(api, n, q, r, w, prior, algo)
    assert st['n_new'] == 0 and st['n_edges'] == 0 and st['sweep_objects'] == 0


HAND_CASES = [
    # (n, rows, prior_rep): the cases of test_cluster_update_cpu.py
    (3, [(0, 1, 0.9)], [-1, 1, 1]),                           # a longer new object joins the prior representative
    (3, [(0, 2, 0.9)], [-1, 1, 1]),                           # an edge to a prior member only
    (3, [(1, 0, 0.9), (1, 2, 0.9)], [-1, -1, 2]),             # a uclust tie between a prior and a new representative
    (3, [(1, 0, 0.95), (1, 2, 0.9)], [-1, -1, 2]),
    (5, [(4, 1, 0.9), (4, 2, 0.9)], [0, 0, 2, 2, -1]),        # two prior clusters bridged by a new object
    (3, [(0, 1, 1.0), (1, 0, 0.99)], [0, 1, -1]),             # a row between two prior clusters
    (3, [(1, 2, 0.9)], [2, -1, 2]),                           # a prior representative that is not the earliest member
    (3, [(1, 0, 0.9)], [2, -1, 2]),
    (6, [(1, 5, 0.9), (3, 5, 0.9), (3, 4, 0.8), (0, 4, 0.7)], [5, -1, 4, -1, 4, 5]),
]


@pytest.mark.parametrize('algo', cu.ALGORITHMS)
def test_hand_cases_on_the_device(api, algo):
    for n, rows, prior in HAND_CASES:
        q, r, w = (np.array(x) for x in zip(*rows))
        _check(api, n, q.astype(np.uint32), r.astype(np.uint32), w.astype(np.float64), prior, algo)
    label, rep, st = api.cluster_update_graph(3, [1, 1], [0, 2], [0.9, 0.9], [-1, -1, 2], 'uclust')
    assert list(rep) == [0, 2, 2] and list(label) == [1, 0, 0]                # (spelled out: the tie goes to the prior one)
    label, rep, st = api.cluster_update_graph(3, [0], [1], [0.9], [-1, 1, 1], 'cd-hit')
    assert list(rep) == [1, 1, 1] and st['joined_prior'] == 1


@pytest.mark.parametrize('algo', cu.ALGORITHMS)
def test_representatives_that_are_not_the_earliest_member(api, graphs, algo):
    """as --prior-repr may say: every prior cluster is represented by its LAST member, so a member's state points forward"""
    n, q, r, w, mask, rows = graphs[12]
    prior = _prior_run(n, rows, mask, 'cd-hit')
    last = {}
    for i, p in enumerate(prior):
        if p >= 0:
            last[int(p)] = i
    prior = np.array([last[int(p)] if p >= 0 else -1 for p in prior], np.int32)
    assert (prior > np.arange(n)).any()
    _check(api, n, q, r, w, prior, algo)


# ---------------------------------------------------------------- the tail sweep from seeded states
TAIL_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import cluster_restatement as cr
import cluster_update_restatement as cu
from vclust_amd import api
n, n_prior = 100000, 10000
q, r = np.arange(n - 1), np.arange(1, n)
w = np.full(len(q), 0.9)
rows = list(zip(q.tolist(), r.tolist(), w.tolist()))
out = {}
for algo in ('cd-hit', 'uclust'):
    inside = [x for x in rows if x[1] < n_prior]
    prior = cu.prior_of(cr.cluster_ids(n, cr.edges(inside), algo), range(n_prior))
    label, rep, stats = api.cluster_update_graph(n, q, r, w, prior, algo)
    want_label, want_rep, want = cu.update_graph(n, rows, prior, algo)
    out[algo] = dict(stats, equal=list(rep) == want_rep and list(label) == want_label, want_edges=want['n_edges'])
print(json.dumps(out))
"""


def test_tail_sweep_from_seeded_states(api):
    """The 100 000-object path in index order of test_gpu_cluster.py::test_tail_sweep with its first tenth prior: the rounds
    stall on the one dependency chain and the one-workgroup sweep, started behind the prior objects, finishes it.  Run in a
    child with a time limit, as that test is."""
    p = subprocess.run([sys.executable, '-c', TAIL_CHILD, str(ROOT)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for algo, st in res.items():
        print(algo, st)
        assert st['equal'], (algo, st)
        assert st['n_prior'] == 10000 and st['n_new'] == 90000 and st['n_edges'] == st['want_edges'] == 90000
        assert st['sweep_objects'] > st['n_new'] // 2, (algo, st)


# ---------------------------------------------------------------- files: the golden example
GOLDEN_PRIOR = (0, 1, 3, 4, 6, 8, 9, 11)         # 8 of the 12 genomes


def _golden_split(out_dir, tmp_path, members=GOLDEN_PRIOR, representatives=False):
    """-> (prior clusters.tsv = single at tANI 0.95 on the golden rows among `members`, ani.tsv of the rows with another genome)"""
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    lines = (out_dir / 'ani.tsv').read_text().split('\n')
    head = lines[0].split('\t')
    qc, rc = head.index('qidx'), head.index('ridx')
    D = set(members)
    both = lambda ln: int(ln.split('\t')[qc]) in D and int(ln.split('\t')[rc]) in D       # noqa: E731
    inside, rest = tmp_path / 'inside.tsv', tmp_path / 'new_rows.tsv'
    inside.write_text('\n'.join([lines[0]] + [ln for ln in lines[1:] if ln and both(ln)]) + '\n')
    rest.write_text('\n'.join([lines[0]] + [ln for ln in lines[1:] if ln and not both(ln)]) + '\n')
    cid = cr.cluster_ids(len(ids), cr.edges(cr.read_rows(inside, len(ids), 'tani', tani=0.95)), 'single')
    prior = tmp_path / 'prior.tsv'
    prior.write_text('object\tcluster\n' + ''.join(f'{ids[i]}\t{ids[cid[i]] if representatives else cid[i]}\n' for i in sorted(D)))
    return prior, rest


@pytest.mark.parametrize('representatives', [False, True])
def test_p1_reproduces_the_golden_clusters_byte_for_byte(api, out_dir, tmp_path, representatives):
    prior, rest = _golden_split(out_dir, tmp_path, representatives=representatives)
    out = tmp_path / 'clusters.tsv'
    p = run('cluster', '-i', rest, '--ids', out_dir / 'ani.ids.tsv', '--prior', prior, *(['--prior-repr'] if representatives else []),
            '--algorithm', 'single', '--tani', '0.95', '-o', out, '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    assert out.read_bytes() == (out_dir / 'clusters.tsv').read_bytes()
    # ... and from the whole golden table: the rows among the 8 are ignored
    p = run('cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '--prior', prior,
            *(['--prior-repr'] if representatives else []), '--tani', '0.95', '-o', out)
    assert p.returncode == 0 and f'--prior {prior}' in p.stderr and 'Prior clustering updated: 8 prior + 4 new genomes' in p.stderr, p.stderr
    assert out.read_bytes() == (out_dir / 'clusters.tsv').read_bytes()


@pytest.mark.parametrize('repr_', [False, True])
@pytest.mark.parametrize('algo', cu.ALGORITHMS)
def test_golden_files_equal_restatement(api, out_dir, tmp_path, algo, repr_):
    prior, rest = _golden_split(out_dir, tmp_path, members=(2, 3, 5, 7, 10, 11), representatives=True)
    out = tmp_path / 'c.tsv'
    for metric, thr in (('tani', 0.95), ('ani', 0.9), ('gani', 0.5)):
        st = api.cluster_update(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', prior, out, algorithm=algo, prior_repr=True, metric=metric,
                                representatives=repr_, **{metric: thr})
        assert st['n_prior'] == 6 and st['n_new'] == 6
        assert out.read_bytes() == cu.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', prior, algo, metric, representatives=repr_,
                                          prior_repr=True, **{metric: thr})


@pytest.mark.parametrize('algo', ['single', 'cd-hit', 'uclust', 'set-cover'])
def test_without_prior_the_files_are_those_of_the_plain_stage(api, out_dir, tmp_path, algo):
    """`cluster` without --prior writes what the restatement of the plain stage writes; with a prior file that lists nobody
    (P3) the three algorithms of the update write the same bytes through the other entry."""
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '--algorithm', algo, '--tani', '0.95', '-v', '0']
    empty = tmp_path / 'empty_prior.tsv'
    empty.write_text('object\tcluster\n')
    for extra in ([], ['-r']):
        want = cr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', algo, 'tani', representatives=bool(extra), tani=0.95)
        p = run(*base, *extra, '-o', tmp_path / 'plain.tsv')
        assert p.returncode == 0 and p.stderr == '', p.stderr
        assert (tmp_path / 'plain.tsv').read_bytes() == want
        if algo in cu.ALGORITHMS:
            p = run(*base, *extra, '--prior', empty, '-o', tmp_path / 'updated.tsv')
            assert p.returncode == 0 and p.stderr == '', p.stderr
            assert (tmp_path / 'updated.tsv').read_bytes() == want


# ---------------------------------------------------------------- the whole workflow: 8 genomes, then 4 more
def _partition(path):
    groups = {}
    for line in path.read_text().splitlines()[1:]:
        name, c = line.split('\t')
        groups.setdefault(c, set()).add(name)
    return sorted(sorted(g) for g in groups.values())


def test_whole_workflow_db_then_prior(api, tmp_path):
    names = write_split(tmp_path)
    db, new, whole = tmp_path / 'db.fna', tmp_path / 'new.fna', EX / 'multifasta.fna'
    old, upd, full = tmp_path / 'old', tmp_path / 'upd', tmp_path / 'full'
    for d in (old, upd, full):
        d.mkdir()

    def ok(*args):
        p = run(*args, '-v', '0')
        assert p.returncode == 0 and p.stderr == '', (args, p.stderr)
    for d, inputs in ((old, ['-i', db]), (full, ['-i', whole]), (upd, ['-i', new, '--db', db])):
        ok('prefilter', *inputs, '-o', d / 'fltr.txt')
        ok('align', *inputs, '--filter', d / 'fltr.txt', '-o', d / 'ani.tsv')
    assert cr.read_ids(upd / 'ani.ids.tsv') == cr.read_ids(full / 'ani.ids.tsv')
    for algo in ('single', 'cd-hit'):
        for d in (old, full):
            ok('cluster', '-i', d / 'ani.tsv', '--ids', d / 'ani.ids.tsv', '--algorithm', algo, '--tani', '0.95', '-r', '-o', d / f'{algo}.tsv')
        ok('cluster', '-i', upd / 'ani.tsv', '--ids', upd / 'ani.ids.tsv', '--prior', old / f'{algo}.tsv', '--prior-repr',
           '--algorithm', algo, '--tani', '0.95', '-r', '-o', upd / f'{algo}.tsv')
    # single: the partition of the all-vs-all run on all 12, by name
    assert _partition(upd / 'single.tsv') == _partition(full / 'single.tsv')
    assert len(_partition(full / 'single.tsv')) < 12
    # cd-hit: every one of the 8 keeps its representative
    before = dict(ln.split('\t') for ln in (old / 'cd-hit.tsv').read_text().splitlines()[1:])
    after = dict(ln.split('\t') for ln in (upd / 'cd-hit.tsv').read_text().splitlines()[1:])
    assert set(before) == set(names[:N_DB_EXAMPLE]) and set(after) == set(names)
    assert all(after[x] == before[x] for x in before)
