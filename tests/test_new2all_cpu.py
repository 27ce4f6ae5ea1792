"""New genomes against a database (`--db`, vg_*_new): everything that needs no device -- the definition as a small Python
restatement (the GPU tests import it), the command line, the ABI symbols, the argument errors that must come before any
device work, and the loud failure without a device."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
EX = ROOT / 'tests' / 'golden' / 'example'
N_DB_EXAMPLE = 8            # the golden example split into its first 8 records (the database) and its last 4 (the new genomes)


# ---------------------------------------------------------------- the definition
def restrict_new(sizes, pairs, n_db):
    """All-vs-all, then restrict: `sizes` (one per genome) and `pairs` ({(a, b): shared}, a > b) of the all-vs-all result over
    database + new genomes -> what kmer_shared_new(n_db) returns: the pairs with a >= n_db, and the sizes with -1 for every
    database genome (id < n_db) that no kept pair names."""
    kept = {(a, b): s for (a, b), s in pairs.items() if a >= n_db}
    assert all(a > b for a, b in kept)
    named = {b for _, b in kept if b < n_db}
    return [int(s) if i >= n_db or i in named else -1 for i, s in enumerate(sizes)], kept


def test_restatement():
    sizes = [10, 11, 12, 13, 14]
    pairs = {(1, 0): 3, (2, 1): 4, (3, 0): 5, (4, 3): 6, (4, 2): 1}
    assert restrict_new(sizes, pairs, 0) == (sizes, pairs)
    assert restrict_new(sizes, pairs, 5) == ([-1] * 5, {})
    assert restrict_new(sizes, pairs, 3) == ([10, -1, 12, 13, 14], {(3, 0): 5, (4, 3): 6, (4, 2): 1})
    assert restrict_new(sizes, pairs, 4) == ([-1, -1, 12, 13, 14], {(4, 3): 6, (4, 2): 1})


# ---------------------------------------------------------------- inputs: the golden example, split
def split_records(path):
    """-> [(first header token, text of the record)] of a FASTA file"""
    recs = ['>' + r for r in pathlib.Path(path).read_text().split('>')[1:]]
    return [(r[1:].split()[0], r) for r in recs]


def write_split(tmp, n_db=N_DB_EXAMPLE):
    """The golden multi-FASTA as db.fna (first n_db records) + new.fna, and as directories db/ + new/ of one file per record;
    the files are numbered so that the sorted directory order is the record order: a genome of the directories is called
    `<2 digits>_<record name>`."""
    recs = split_records(EX / 'multifasta.fna')
    tmp = pathlib.Path(tmp)
    (tmp / 'db.fna').write_text(''.join(r for _, r in recs[:n_db]))
    (tmp / 'new.fna').write_text(''.join(r for _, r in recs[n_db:]))
    for d in ('db', 'new'):
        (tmp / d).mkdir()
    for i, (name, r) in enumerate(recs):
        (tmp / ('db' if i < n_db else 'new') / f'{i:02d}_{name}').write_text(r)
    return [name for name, _ in recs]


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('new2all')
    return tmp, write_split(tmp)


# ---------------------------------------------------------------- the library, without a device
def test_abi_symbols():
    from vclust_amd import _lib
    lib = _lib.load()
    for name in ('vg_genomes_load_db_new', 'vg_kmer_shared_new', 'vg_prefilter_new', 'vg_align_new', 'vg_set_new_path'):
        assert name in _lib.SYMBOLS and getattr(lib, name)


def test_loader_is_the_concatenated_set(split):
    from vclust_amd import api
    tmp, names = split
    whole = api.GenomeSet.load([EX / 'multifasta.fna'], multisample=True)
    gs, n_db = api.GenomeSet.load_db_new([tmp / 'db.fna'], [tmp / 'new.fna'], multisample=True)
    assert n_db == N_DB_EXAMPLE and gs.names() == names == whole.names() and list(gs.lengths()) == list(whole.lengths())
    for i in (0, 7, 8, 11):
        assert np.array_equal(gs.codes(i), whole.codes(i))
    db, new = sorted((tmp / 'db').iterdir()), sorted((tmp / 'new').iterdir())
    gd, n_db = api.GenomeSet.load_db_new(db, new, multisample=False)
    assert n_db == N_DB_EXAMPLE and gd.names() == [f'{i:02d}_{n}' for i, n in enumerate(names)]
    assert list(gd.lengths()) == list(whole.lengths())
    g1, n_db = api.GenomeSet.load_db_new(db[:1], new, multisample=False)       # a database of one file
    assert n_db == 1 and len(g1) == 5


def test_loader_errors(split, tmp_path):
    from vclust_amd import api
    from vclust_amd._lib import VclustGpuError
    tmp, names = split
    (tmp_path / 'again.fna').write_text('>fresh\nACGTACGTAC\n>' + names[2] + ' once more\nACGTTTGACA\n')
    with pytest.raises(VclustGpuError) as e:
        api.GenomeSet.load_db_new([tmp / 'db.fna'], [tmp_path / 'again.fna'], multisample=True)
    assert e.value.code == -1 and names[2] in str(e.value) and 'database' in str(e.value)
    with pytest.raises(VclustGpuError) as e:            # directory mode: the genome is the file name
        api.GenomeSet.load_db_new(sorted((tmp / 'db').iterdir()), [tmp / 'db' / f'03_{names[3]}'], multisample=False)
    assert e.value.code == -1 and f'03_{names[3]}' in str(e.value)
    with pytest.raises(VclustGpuError) as e:            # multi-FASTA mode is one file on each side
        api.GenomeSet.load_db_new([tmp / 'db.fna', tmp / 'new.fna'], [tmp / 'new.fna'], multisample=True)
    assert e.value.code == -1
    with pytest.raises(VclustGpuError) as e:
        api.GenomeSet.load_db_new([tmp / 'db.fna'], [tmp / 'missing.fna'], multisample=True)
    assert e.value.code == -2
    # the combined set needs two genomes: one database record and no new record is an error, before any device work
    (tmp_path / 'one.fna').write_text('>only\nACGTACGTACGTTTGACA\n')
    (tmp_path / 'none.fna').write_text('')
    with pytest.raises(VclustGpuError) as e:
        api.GenomeSet.load_db_new([tmp_path / 'one.fna'], [tmp_path / 'none.fna'], multisample=True)
    assert e.value.code == -1 and 'at least 2' in str(e.value)
    gs, n_db = api.GenomeSet.load_db_new([tmp / 'db.fna'], [tmp_path / 'none.fna'], multisample=True)      # (n_db = n is no error)
    assert n_db == len(gs) == N_DB_EXAMPLE
    for sub in ('prefilter', 'align'):
        p = run(sub, '-i', tmp_path / 'none.fna', '--db', tmp_path / 'one.fna', '-o', tmp_path / 'o.txt')
        assert p.returncode == 1 and 'ERROR' in p.stderr and 'at least 2' in p.stderr and not (tmp_path / 'o.txt').exists()


def test_argument_errors_come_before_any_device_work(split, tmp_path):
    """VG_EINVAL (-1), not VG_ENODEV (-3), also on a machine without a device."""
    from vclust_amd import api, stages
    from vclust_amd._lib import VclustGpuError
    tmp, names = split
    gs, n_db = api.GenomeSet.load_db_new([tmp / 'db.fna'], [tmp / 'new.fna'], multisample=True)
    for bad in (-1, len(gs) + 1):
        with pytest.raises(VclustGpuError) as e:
            gs.kmer_shared_new(bad)
        assert e.value.code == -1 and 'n_db' in str(e.value)
    (tmp_path / 'again.fna').write_text('>' + names[0] + '\nACGTACGTAC\n')
    with pytest.raises(VclustGpuError) as e:
        stages.prefilter([tmp_path / 'again.fna'], tmp_path / 'f.txt', True, db_paths=[tmp / 'db.fna'])
    assert e.value.code == -1 and names[0] in str(e.value)
    with pytest.raises(VclustGpuError) as e:
        stages.align([tmp_path / 'again.fna'], tmp_path / 'a.tsv', True, ['qidx', 'ridx', 'tani'], db_paths=[tmp / 'db.fna'])
    assert e.value.code == -1 and names[0] in str(e.value)
    assert not (tmp_path / 'f.txt').exists() and not (tmp_path / 'a.tsv').exists()


# ---------------------------------------------------------------- the command line
def run(*args, env=None):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          env={**os.environ, **(env or {})})


@pytest.mark.parametrize('sub', ['prefilter', 'align'])
def test_usage_errors(split, tmp_path, sub):
    tmp, _ = split
    out = tmp_path / 'out'
    p = run(sub, '-i', tmp / 'new.fna', '--db', tmp / 'db', '-o', out)
    assert p.returncode == 2 and '-i and --db must both be' in p.stderr
    p = run(sub, '-i', tmp / 'new', '--db', tmp / 'db.fna', '-o', out)
    assert p.returncode == 2 and '-i and --db must both be' in p.stderr
    p = run(sub, '-i', tmp / 'new.fna', '--db', tmp / 'nothing.fna', '-o', out)
    assert p.returncode == 2 and 'does not exist' in p.stderr
    p = run(sub, '-i', tmp / 'new.fna', '--db', tmp / 'db.fna', '-o', out, env={'WORLD_SIZE': '2', 'RANK': '0'})
    assert p.returncode == 2 and '--db' in p.stderr and 'WORLD_SIZE' in p.stderr
    (tmp_path / 'empty').mkdir()
    p = run(sub, '-i', tmp / 'new', '--db', tmp_path / 'empty', '-o', out)
    assert p.returncode == 2 and 'No fasta files found' in p.stderr
    assert not out.exists()


def _parsed(argv):
    from vclust_amd import cli
    sys.argv = ['vclust.py'] + argv
    parser = cli.get_parser()
    args = parser.parse_args(argv)
    if args.command == 'prefilter':
        args = cli.validate_args_prefilter(args, parser)
    return cli, cli.validate_args_fasta_input(args, parser)


def test_call_dictionaries(split, tmp_path):
    """--db adds db_paths to what the stage call receives and changes nothing else; without it the dictionary is today's."""
    tmp, _ = split
    db_files, new_files = sorted((tmp / 'db').iterdir()), sorted((tmp / 'new').iterdir())
    flt = tmp_path / 'fltr.txt'; flt.write_text('x')
    for inp, db, paths, db_paths, multi in ((tmp / 'new.fna', tmp / 'db.fna', [tmp / 'new.fna'], [tmp / 'db.fna'], True),
                                            (tmp / 'new', tmp / 'db', new_files, db_files, False)):
        base = ['-i', str(inp), '-o', str(tmp_path / 'o'), '-t', '3']
        cli, args = _parsed(['prefilter'] + base + ['-k', '21', '--max-seqs', '5'])
        plain = cli.prefilter_call(args)
        assert plain == dict(paths=paths, out_path=tmp_path / 'o', is_multifasta=multi, k=21, min_kmers=20, min_ident=0.7, kmers_fraction=1.0,
                             max_seqs=5, num_threads=3)
        cli, args = _parsed(['prefilter'] + base + ['-k', '21', '--max-seqs', '5', '--db', str(db)])
        assert cli.prefilter_call(args) == {**plain, 'db_paths': db_paths}
        assert f'--db {db}' in cli._db_description(args) and f'{len(db_paths)} database + {len(paths)} new' in cli._db_description(args)
        cli, args = _parsed(['align'] + base + ['--filter', str(flt), '--out-ani', '0.9'])
        plain = cli.align_call(args)
        assert set(plain) == {'paths', 'out_path', 'is_multifasta', 'columns', 'filter_path', 'filter_threshold', 'out_aln', 'lz',
                              'out_filters', 'num_threads'}
        assert plain['paths'] == paths and plain['filter_path'] == flt and plain['out_filters'] == {'ani': 0.9}
        cli, args = _parsed(['align'] + base + ['--filter', str(flt), '--out-ani', '0.9', '--db', str(db)])
        assert cli.align_call(args) == {**plain, 'db_paths': db_paths}
    # --batch-size stays accepted (and ignored) beside --db; a database directory of one file is enough
    cli, args = _parsed(['prefilter', '-i', str(tmp / 'new.fna'), '-o', 'o', '--db', str(tmp / 'db.fna'), '--batch-size', '4'])
    assert cli.prefilter_call(args)['db_paths'] == [tmp / 'db.fna']
    one = tmp_path / 'one'; one.mkdir(); (one / 'a.fna').write_text((tmp / 'db' / db_files[0].name).read_text())
    cli, args = _parsed(['align', '-i', str(tmp / 'new'), '-o', 'o', '--db', str(one)])
    assert cli.align_call(args)['db_paths'] == [one / 'a.fna']


def test_stages_take_the_call_dictionary():
    """cli hands the dictionary to stages.prefilter / stages.align as keywords: both must accept db_paths."""
    import inspect
    from vclust_amd import stages
    for fn in (stages.prefilter, stages.align):
        assert inspect.signature(fn).parameters['db_paths'].default is None


@pytest.mark.parametrize('sub', ['prefilter', 'align'])
def test_without_gpu_db_mode_fails_loudly(split, tmp_path, sub):
    """No CPU fallback: VG_ENODEV arrives as an ERROR line and exit status 1, and nothing is written."""
    from vclust_amd import api
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    tmp, _ = split
    out = tmp_path / 'out.txt'
    p = run(sub, '-i', tmp / 'new.fna', '--db', tmp / 'db.fna', '-o', out)
    assert p.returncode == 1
    assert 'Running' in p.stderr and f'--db {tmp / "db.fna"}' in p.stderr and 'ERROR' in p.stderr and 'no CPU fallback' in p.stderr
    assert not out.exists()
