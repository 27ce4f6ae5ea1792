"""`dereplicate --db --prior` without a GPU: the update procedure's restatement against the update of a prior clustering on the whole
graph (the lemma of DESIGN.md section 13 and the pairs it never asks for: none with a prior member, none between two prior objects),
the C ABI and Python surface of vg_genomes_extend / vg_genomes_truncate / vg_genomes_reserve / vg_dereplicate_update_set /
vg_dereplicate_update, their argument errors (raised before any device use) and the CLI's usage errors."""
import ctypes as C
import os
import pathlib
import random
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_update_restatement as cu
import derep_restatement as dr
import derep_update_restatement as du
from vclust_amd import _lib, api, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'


def run(*args, env=None):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120, env={**os.environ, **(env or {})})


# ---------------------------------------------------------------- the restatement
def _random_graph(rng, n, density):
    return {(a, b): round(rng.random(), 2) for a in range(n) for b in range(a + 1, n) if rng.random() < density}


def _cd_hit_prior(n, e, members):
    """prior_rep of plain cd-hit over the graph induced on `members` (ascending), -1 for the others"""
    pos = {m: i for i, m in enumerate(members)}
    rows = [(pos[b], pos[a], w) for (a, b), w in e.items() if a in pos and b in pos]
    rep = cr.cluster_graph(len(members), rows, 'cd-hit')[1] if members else []
    prior = [-1] * n
    for i, m in enumerate(members):
        prior[m] = members[rep[i]]
    return prior


def _priors(rng, n, e):
    """the three shapes: the first half clustered by cd-hit; a random subset clustered by cd-hit; the first half again with the LAST
    member of every cluster as its representative (what --prior-repr can name: a representative behind its members)"""
    half = _cd_hit_prior(n, e, list(range(n // 2)))
    subset = _cd_hit_prior(n, e, sorted(rng.sample(range(n), rng.randint(0, n))))
    last = {}
    for i, r in enumerate(half):
        if r >= 0:
            last[r] = i
    behind = [last[r] if r >= 0 else -1 for r in half]
    return {'first half': half, 'random subset': subset, 'representative behind its members': behind}


def test_a_row_to_a_prior_member_joins_nothing():
    """prior cluster {0, 1} with representative 0; the new object 2 has an edge to the member 1 only: it founds a cluster, and the
    pair (1, 2) is never asked"""
    e = {(0, 1): 0.9, (1, 2): 0.9}
    label, rep, asked, st = du.dereplicate_update(3, lambda a, b: e.get((a, b)), 4, [0, 0, -1])
    assert rep == [0, 0, 2] and label == [0, 0, 1] and asked == [(0, 2, 'rep')]
    assert st['founded'] == 1 and st['joined_prior_cluster'] == 0 and st['prior_objects'] == 2 and st['prior_representatives'] == 1
    # ... and a new object longer than the representative (a lower index) still joins it: position in R is visit order, not index
    label, rep, asked, st = du.dereplicate_update(3, lambda a, b: {(0, 1): 0.9}.get((a, b)), 1, [-1, 1, 1])
    assert rep == [1, 1, 1] and st['joined_prior_cluster'] == 1 and asked == [(0, 1, 'rep')]


@pytest.mark.parametrize('density', [0.05, 0.15, 0.4, 0.8])
def test_update_batches_equal_the_update_of_the_whole_graph_and_never_ask_for_a_prior_member(density):
    rng = random.Random(1000 + int(density * 100))
    never_asked = total = 0
    seen_shapes = set()
    for trial in range(60):
        n = rng.randint(1, 40)
        e = _random_graph(rng, n, density)
        rows = [(b, a, w) for (a, b), w in e.items()]
        for shape, prior in _priors(rng, n, e).items():
            want = cu.update_graph(n, rows, prior, 'cd-hit')
            n_new = sum(p < 0 for p in prior)
            for batch in (1, 2, 3, 7, n, n + 5):
                label, rep, asked, st = du.dereplicate_update(n, lambda a, b: e.get((a, b)), batch, prior)
                assert (label, rep) == (want[0], want[1]), (n, shape, batch)
                # the update on the asked edges alone
                pairs = {(a, b) for a, b, _ in asked}
                assert len(pairs) == len(asked)                       # no pair is asked twice
                alone = cu.update_graph(n, [(b, a, w) for (a, b), w in e.items() if (a, b) in pairs], prior, 'cd-hit')
                assert (alone[0], alone[1]) == (want[0], want[1])
                for a, b, kind in asked:
                    assert a < b
                    for x in (a, b):                                  # no prior member
                        assert prior[x] < 0 or prior[x] == x, (shape, a, b)
                    assert prior[a] < 0 or prior[b] < 0               # not two prior ends
                    if kind == 'U':
                        assert prior[a] < 0 and prior[b] < 0
                assert st['joined_prior'] + st['joined_new'] + st['founded'] == n_new
                assert st['founded'] + st['prior_representatives'] == st['representatives']
                assert st['joined_prior_cluster'] == want[2]['joined_prior']
                assert st['prior_objects'] == n - n_new and st['batches'] == -(-n_new // batch)
                never_asked += n * (n - 1) // 2 - len(asked)
                total += n * (n - 1) // 2
            if any(0 <= p != i and p > i for i, p in enumerate(prior)):
                seen_shapes.add(shape)
    assert never_asked > 0 and total > 0
    assert 'representative behind its members' in seen_shapes


def test_empty_prior_is_the_plain_procedure_and_a_full_prior_comes_back():
    rng = random.Random(5)
    for trial in range(60):
        n = rng.randint(1, 40)
        e = _random_graph(rng, n, rng.choice([0.05, 0.15, 0.4, 0.8]))
        for batch in (1, 2, 3, 7, n, n + 5):
            label, rep, asked, st = du.dereplicate_update(n, lambda a, b: e.get((a, b)), batch, [-1] * n)
            plabel, prep, pasked, pst = dr.dereplicate(n, lambda a, b: e.get((a, b)), batch)
            assert (label, rep, asked) == (plabel, prep, pasked)
            assert {k: st[k] for k in pst} == pst and st['prior_objects'] == 0 and st['joined_prior_cluster'] == 0
            full = cr.cluster_graph(n, [(b, a, w) for (a, b), w in e.items()], 'single')[1]
            label, rep, asked, st = du.dereplicate_update(n, lambda a, b: e.get((a, b)), batch, full)
            assert rep == full and label == cu.update_graph(n, [], full, 'cd-hit')[0] and asked == []
            assert st['batches'] == 0 and st['prior_objects'] == n


# ---------------------------------------------------------------- the ABI
NEW_SYMBOLS = ('vg_genomes_extend', 'vg_genomes_truncate', 'vg_genomes_reserve', 'vg_dereplicate_update_set', 'vg_dereplicate_update')


def test_new_symbols_exported_declared_and_bound():
    lib = _lib.load()
    header = (ROOT / 'include' / 'vclust_gpu.h').read_text()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and f'{name}(' in header
    for name in ('extend', 'truncate', 'reserve'):
        assert callable(getattr(api.GenomeSet, name))
    # the structs of the plain command keep their layouts; the update's counts are a struct of their own
    assert C.sizeof(_lib.DerepStats) == 64 and C.sizeof(_lib.DerepUpdateStats) == 24
    assert [n for n, _ in _lib.DerepUpdateStats._fields_] == ['prior_objects', 'prior_representatives', 'joined_prior_cluster']
    assert 'vg_derep_update_stats' in header


def _small_set():
    codes = np.array([0, 1, 2, 3] * 30, dtype=np.uint8)
    return api.GenomeSet.from_codes(codes, np.array([0, 40, 80, 120], dtype=np.int64), ['a', 'b', 'c'])


def _error(fn):
    with pytest.raises(_lib.VclustGpuError) as e:
        fn()
    return e.value


def test_extend_truncate_reserve_argument_errors_need_no_device():
    lib = _lib.load()
    gs, other = _small_set(), _small_set()
    ids = (C.c_int32 * 2)(0, 1)
    assert lib.vg_genomes_extend(None, gs._h, ids, 2) == -1 and b'null argument' in lib.vg_last_error()
    assert lib.vg_genomes_extend(gs._h, None, ids, 2) == -1
    assert lib.vg_genomes_extend(gs._h, other._h, None, 2) == -1
    assert lib.vg_genomes_extend(gs._h, other._h, ids, -1) == -1
    assert lib.vg_genomes_truncate(None, 0) == -1 and lib.vg_genomes_reserve(None, 0, 0) == -1
    err = _error(lambda: gs.extend(other, [0, 3]))
    assert err.code == -1 and 'ids[1] = 3' in str(err) and 'outside 0..2' in str(err)
    err = _error(lambda: gs.extend(other, [-1]))
    assert err.code == -1 and 'ids[0] = -1' in str(err)
    err = _error(lambda: gs.extend(other, [2, 0, 2]))
    assert err.code == -1 and 'ids[2] = 2 is listed twice' in str(err)
    # a loaded set is no subset: it has a host copy, which would not follow
    err = _error(lambda: gs.extend(other, [0]))
    assert err.code == -1 and 'vg_genomes_subset' in str(err)
    err = _error(lambda: gs.truncate(4))
    assert err.code == -1 and 'n_keep = 4' in str(err) and 'outside 0..3' in str(err)
    err = _error(lambda: gs.truncate(-1))
    assert err.code == -1 and 'n_keep = -1' in str(err)
    err = _error(lambda: gs.truncate(1))
    assert err.code == -1 and 'vg_genomes_subset' in str(err)
    err = _error(lambda: gs.reserve(-1, 0))
    assert err.code == -1 and 'negative' in str(err)
    err = _error(lambda: gs.reserve(0, -1))
    assert err.code == -1
    err = _error(lambda: gs.reserve(100, 1))
    assert err.code == -1 and 'vg_genomes_subset' in str(err)
    assert len(gs) == 3 and gs.names() == ['a', 'b', 'c']


def test_update_set_argument_errors_need_no_device():
    gs = _small_set()
    err = _error(lambda: gs.dereplicate_set(tani=0.9, n_db=4, prior_rep=[-1, -1, -1]))
    assert err.code == -1 and 'n_db = 4' in str(err)
    err = _error(lambda: gs.dereplicate_set(tani=0.9, n_db=-1))
    assert err.code == -1 and 'n_db = -1' in str(err)
    err = _error(lambda: gs.dereplicate_set(tani=0.9, n_db=2, prior_rep=[0, 3, -1]))
    assert err.code == -1 and 'prior_rep[1] = 3' in str(err)
    err = _error(lambda: gs.dereplicate_set(tani=0.9, n_db=2, prior_rep=[1, 0, -1]))
    assert err.code == -1 and 'is not its own representative' in str(err)
    with pytest.raises(ValueError):
        gs.dereplicate_set(tani=0.9, n_db=2, prior_rep=[0, 0])
    # what the plain call refuses stays refused
    err = _error(lambda: gs.dereplicate_set(batch_genomes=0, tani=0.9, n_db=2, prior_rep=[0, 0, -1]))
    assert err.code == -1 and 'batch_genomes must be at least 1' in str(err)
    err = _error(lambda: gs.dereplicate_set(algorithm='uclust', tani=0.9, n_db=2, prior_rep=[0, 0, -1]))
    assert err.code == -1 and 'VG_CLUSTER_CDHIT' in str(err)
    err = _error(lambda: gs.dereplicate_set(n_db=2, prior_rep=[0, 0, -1]))
    assert err.code == -1 and 'tani threshold must be above 0' in str(err)


def test_file_level_argument_errors_need_no_device(golden_dir, tmp_path):
    out, fasta = tmp_path / 'clusters.tsv', golden_dir / 'multifasta.fna'
    prior = tmp_path / 'prior.tsv'
    prior.write_text('object\tcluster\n')
    with pytest.raises(ValueError, match='db_paths and prior_path'):
        stages.dereplicate([fasta], out, True, tani=0.95, db_paths=[fasta])
    with pytest.raises(ValueError, match='db_paths and prior_path'):
        stages.dereplicate([fasta], out, True, tani=0.95, prior_path=prior)
    with pytest.raises(ValueError, match='prior_repr'):
        stages.dereplicate([fasta], out, True, tani=0.95, prior_repr=True)
    err = _error(lambda: stages.dereplicate([fasta], out, True, db_paths=[fasta], prior_path=prior, batch_genomes=0, tani=0.95))
    assert err.code == -1 and 'batch_genomes' in str(err)
    err = _error(lambda: stages.dereplicate([fasta], out, True, db_paths=[fasta], prior_path=prior, algorithm='uclust', tani=0.95))
    assert err.code == -1 and 'VG_CLUSTER_CDHIT' in str(err)
    files = sorted((golden_dir / 'fna').iterdir())
    err = _error(lambda: stages.dereplicate(files[8:], out, False, db_paths=files[:8], prior_path=prior, tani=0.95, out_repr_fasta=tmp_path / 'r.fna'))
    assert err.code == -1 and 'multi-FASTA' in str(err)
    assert not out.exists()


# ---------------------------------------------------------------- the command line
def test_cli_help_names_the_new_flags():
    p = run('dereplicate')
    assert p.returncode == 0 and '--db' in p.stdout and '--prior' in p.stdout and '--prior-repr' in p.stdout


def test_cli_usage_errors(golden_dir, tmp_path):
    fasta, out = golden_dir / 'multifasta.fna', tmp_path / 'clusters.tsv'
    prior = tmp_path / 'prior.tsv'
    prior.write_text('object\tcluster\n')
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--prior', prior)
    assert p.returncode == 2 and '--prior' in p.stderr and 'needs --db' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--db', fasta)
    assert p.returncode == 2 and '--db' in p.stderr and '--prior' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--prior-repr')
    assert p.returncode == 2 and '--prior-repr' in p.stderr and 'needs --prior' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--db', golden_dir / 'fna', '--prior', prior)
    assert p.returncode == 2 and '-i and --db must both be' in p.stderr
    p = run('dereplicate', '-i', golden_dir / 'fna', '-o', out, '--tani', 0.95, '--db', fasta, '--prior', prior)
    assert p.returncode == 2 and '-i and --db must both be' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--db', fasta, '--prior', tmp_path / 'missing.tsv')
    assert p.returncode == 2 and 'missing.tsv' in p.stderr
    # everything the plain command refuses stays refused beside the new flags
    p = run('dereplicate', '-i', fasta, '-o', out, '--db', fasta, '--prior', prior)
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--db', fasta, '--prior', prior, env={'WORLD_SIZE': '2'})
    assert p.returncode == 2 and 'WORLD_SIZE must be 1' in p.stderr
    p = run('dereplicate', '-i', golden_dir / 'fna', '-o', out, '--tani', 0.95, '--db', golden_dir / 'fna', '--prior', prior,
            '--out-repr-fasta', tmp_path / 'r.fna')
    assert p.returncode == 2 and '--out-repr-fasta' in p.stderr
    assert not out.exists()


def test_cli_without_a_device_fails_loudly(golden_dir, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    out, fasta = tmp_path / 'clusters.tsv', golden_dir / 'multifasta.fna'
    prior = tmp_path / 'prior.tsv'
    prior.write_text('object\tcluster\n')
    p = run('dereplicate', '-i', fasta, '--db', fasta, '--prior', prior, '--prior-repr', '-o', out, '--tani', 0.95)
    assert p.returncode == 1 and 'ERROR' in p.stderr and 'no HIP device' in p.stderr, p.stderr
    assert 'Running: libvclust_gpu dereplicate' in p.stderr and f'--db {fasta}' in p.stderr and f'--prior {prior} --prior-repr' in p.stderr
    assert not out.exists()
