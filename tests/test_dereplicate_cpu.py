"""`dereplicate` without a GPU: the batch procedure's restatement against plain cd-hit (the lemma of DESIGN.md section 13 and the
pairs it never asks for), the C ABI and Python surface of vg_genomes_subset / vg_dereplicate_set / vg_dereplicate, their argument
errors (raised before any device use) and the CLI's usage errors."""
import ctypes as C
import os
import pathlib
import random
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import derep_restatement as dr
from vclust_amd import _lib, api, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'


def run(*args, env=None):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120, env={**os.environ, **(env or {})})


# ---------------------------------------------------------------- the restatement
def test_an_edge_to_a_member_does_not_join():
    """edges 0-1 and 1-2 only: object 2 founds a cluster, because object 1 is a member and not a representative"""
    e = {(0, 1): 0.9, (1, 2): 0.9}
    for batch in (1, 2, 3, 8):
        label, rep, asked, st = dr.dereplicate(3, lambda a, b: e.get((a, b)), batch)
        assert rep == [0, 0, 2] and label == [0, 0, 1]
        assert st['founded'] == 2 and st['joined_prior'] + st['joined_new'] == 1
    # batch 2: object 1 joined nothing EARLIER (0 is a batch-mate), so 0-1 is a U pair; then 2 is asked against 0 alone
    assert dr.dereplicate(3, lambda a, b: e.get((a, b)), 2)[2] == [(0, 1, 'U'), (0, 2, 'rep')]


def _random_graph(rng, n, density):
    return {(a, b): round(rng.random(), 2) for a in range(n) for b in range(a + 1, n) if rng.random() < density}


@pytest.mark.parametrize('density', [0.05, 0.15, 0.4, 0.8])
def test_batches_equal_cd_hit_and_ask_only_what_the_lemma_allows(density):
    rng = random.Random(int(density * 100))
    never_asked = total = 0
    for trial in range(150):
        n = rng.randint(1, 40)
        e = _random_graph(rng, n, density)
        rows = [(b, a, w) for (a, b), w in e.items()]
        want = cr.cluster_graph(n, rows, 'cd-hit')
        for batch in (1, 2, 3, 7, n, n + 5):
            label, rep, asked, st = dr.dereplicate(n, lambda a, b: e.get((a, b)), batch)
            assert (label, rep) == want, (n, batch)
            # plain cd-hit on the asked edges alone
            pairs = {(a, b) for a, b, _ in asked}
            assert len(pairs) == len(asked)                       # no pair is asked twice
            assert cr.cluster_graph(n, [(b, a, w) for (a, b), w in e.items() if (a, b) in pairs], 'cd-hit') == want
            # every asked pair is (batch object, representative of an earlier batch) or lies inside U
            for a, b, kind in asked:
                assert a < b
                if kind == 'rep':
                    assert rep[a] == a and a // batch < b // batch
                else:
                    assert a // batch == b // batch
                    for x in (a, b):                              # no edge to a representative of an earlier batch
                        assert not any(rep[r] == r and r // batch < x // batch and (r, x) in e for r in range(x))
            assert st['joined_prior'] + st['joined_new'] + st['founded'] == n and st['founded'] == st['representatives']
            assert st['batches'] == -(-n // batch)
            never_asked += n * (n - 1) // 2 - len(asked)
            total += n * (n - 1) // 2
    assert never_asked > 0 and total > 0


# ---------------------------------------------------------------- the ABI
NEW_SYMBOLS = ('vg_genomes_subset', 'vg_dereplicate_set', 'vg_dereplicate')


def test_new_symbols_exported_declared_and_bound():
    lib = _lib.load()
    header = (ROOT / 'include' / 'vclust_gpu.h').read_text()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and f'{name}(' in header
    assert callable(api.GenomeSet.subset) and callable(api.GenomeSet.dereplicate_set) and callable(stages.dereplicate)
    assert api.dereplicate is stages.dereplicate
    assert C.sizeof(_lib.DerepStats) == 64


def _small_set():
    codes = np.array([0, 1, 2, 3] * 30, dtype=np.uint8)
    return api.GenomeSet.from_codes(codes, np.array([0, 40, 80, 120], dtype=np.int64), ['a', 'b', 'c'])


def _error(fn):
    with pytest.raises(_lib.VclustGpuError) as e:
        fn()
    return e.value


def test_subset_argument_errors_need_no_device():
    gs = _small_set()
    err = _error(lambda: gs.subset([0, 3]))
    assert err.code == -1 and 'ids[1] = 3' in str(err) and 'outside 0..2' in str(err)
    err = _error(lambda: gs.subset([-1]))
    assert err.code == -1 and 'ids[0] = -1' in str(err)
    err = _error(lambda: gs.subset([2, 0, 2]))
    assert err.code == -1 and 'ids[2] = 2 is listed twice' in str(err)
    if api.device_count() == 0:           # a host-only set is not resident: refused as an argument, not as a missing device
        err = _error(lambda: gs.subset([0, 1]))
        assert err.code == -1 and 'not resident' in str(err)


def test_dereplicate_set_argument_errors_need_no_device():
    gs = _small_set()
    err = _error(lambda: gs.dereplicate_set(batch_genomes=0, tani=0.9))
    assert err.code == -1 and 'batch_genomes must be at least 1' in str(err)
    err = _error(lambda: gs.dereplicate_set(batch_genomes=4))                       # no threshold for the metric
    assert err.code == -1 and 'tani threshold must be above 0' in str(err)
    err = _error(lambda: gs.dereplicate_set(batch_genomes=4, metric='ani', tani=0.9))
    assert err.code == -1 and 'ani threshold must be above 0' in str(err)
    for algo in ('uclust', 'single', 'set-cover'):
        err = _error(lambda: gs.dereplicate_set(batch_genomes=4, algorithm=algo, tani=0.9))
        assert err.code == -1 and 'VG_CLUSTER_CDHIT' in str(err)
    with pytest.raises(ValueError):
        gs.dereplicate_set(algorithm='kmeans', tani=0.9)
    err = _error(lambda: gs.dereplicate_set(k=14, tani=0.9))
    assert err.code == -1


def test_file_level_argument_errors_need_no_device(golden_dir, tmp_path):
    out = tmp_path / 'clusters.tsv'
    fasta = golden_dir / 'multifasta.fna'
    err = _error(lambda: stages.dereplicate([fasta], out, True, batch_genomes=0, tani=0.95))
    assert err.code == -1 and 'batch_genomes' in str(err)
    err = _error(lambda: stages.dereplicate([fasta], out, True))
    assert err.code == -1 and 'threshold must be above 0' in str(err)
    err = _error(lambda: stages.dereplicate([fasta], out, True, algorithm='uclust', tani=0.95))
    assert err.code == -1 and 'VG_CLUSTER_CDHIT' in str(err)
    files = sorted((golden_dir / 'fna').iterdir())
    err = _error(lambda: stages.dereplicate(files, out, False, tani=0.95, out_repr_fasta=tmp_path / 'r.fna'))
    assert err.code == -1 and 'multi-FASTA' in str(err)
    assert not out.exists()


# ---------------------------------------------------------------- the command line
def test_cli_without_arguments_prints_help():
    p = run('dereplicate')
    assert p.returncode == 0 and 'usage:' in p.stdout and '--batch-genomes' in p.stdout and '--out-repr-fasta' in p.stdout
    assert '--max-seqs' not in p.stdout
    assert 'dereplicate' in run().stdout


def test_cli_usage_errors(golden_dir, tmp_path):
    fasta, out = golden_dir / 'multifasta.fna', tmp_path / 'clusters.tsv'
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--max-seqs', 3)
    assert p.returncode == 2 and 'unrecognized arguments: --max-seqs' in p.stderr
    p = run('dereplicate', '-i', golden_dir / 'fna', '-o', out, '--tani', 0.95, '--out-repr-fasta', tmp_path / 'r.fna')
    assert p.returncode == 2 and '--out-repr-fasta' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, env={'WORLD_SIZE': '2'})
    assert p.returncode == 2 and 'WORLD_SIZE must be 1' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out)
    assert p.returncode == 2 and 'tani threshold must be above 0' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--metric', 'ani', '--tani', 0.95)
    assert p.returncode == 2 and 'ani threshold must be above 0' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--batch-genomes', 0)
    assert p.returncode == 2 and '--batch-genomes must be at least 1' in p.stderr
    p = run('dereplicate', '-i', fasta, '-o', out, '--tani', 0.95, '--algorithm', 'uclust')
    assert p.returncode == 2 and 'invalid choice' in p.stderr
    assert not out.exists()


def test_cli_without_a_device_fails_loudly(golden_dir, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    out = tmp_path / 'clusters.tsv'
    p = run('dereplicate', '-i', golden_dir / 'multifasta.fna', '-o', out, '--tani', 0.95, '--batch-genomes', 5, '--out-table', tmp_path / 'ani.tsv')
    assert p.returncode == 1 and 'ERROR' in p.stderr and 'no HIP device' in p.stderr, p.stderr
    assert 'Running: libvclust_gpu dereplicate' in p.stderr and '--batch-genomes 5' in p.stderr and '[1 GPU]' in p.stderr
    assert not out.exists() and not (tmp_path / 'ani.tsv').exists()
