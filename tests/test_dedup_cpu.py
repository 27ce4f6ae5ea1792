"""The deduplicate stage without a GPU: the restatement against the fixture's README.txt, the C ABI and Python surface of
vg_deduplicate / vg_dedup_seqs, and the CLI's dispatch and host-side validation (no device needed for any of it)."""
import os
import pathlib
import subprocess
import sys

import pytest

import dedup_restatement as dr
from vclust_amd import _lib, api, cli

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
DATASETS = ROOT / 'tests' / 'golden' / 'datasets'
# the fixture files are kept gzip-compressed (the reader takes plain, gzip and BGZF input alike)
INPUTS = [DATASETS / 'refseq.fna.gz', DATASETS / 'genbank.fna.gz', DATASETS / 'other.fna.gz']

EXPECTED_IDS = ['refseq|NC_002486.1', 'refseq|NC_005091.2', 'refseq|NC_010807.1', 'refseq|NC_025457.1',
                'genbank|MN428048.1', 'genbank|MK937595.1', 'other|Mushuvirus']
EXPECTED_DUPLICATES = (
    'representative\tduplicate\tstrand\n'
    'refseq|NC_002486.1\tgenbank|AB044554.1\t+\n'
    'refseq|NC_005091.2\tgenbank|AY357582.2\t+\n'
    'refseq|NC_010807.1\tgenbank|EU547803.1\t+\n'
    'refseq|NC_025457.1\tgenbank|KJ473423.1\t+\n'
    'refseq|NC_005091.2\tother|AY357582.2_duplicate\t+\n'
    'refseq|NC_010807.1\tother|NC_010807.1_duplicate\t+\n'
    'genbank|MN428048.1\tother|MN428048.1_revcomp\t-\n'
    'other|Mushuvirus\tother|Mushuvirus_copy\t+\n')


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def readme_groups():
    """The duplicate groups README.txt lists: every table row is one group of names joined by '='."""
    groups = []
    for line in (DATASETS / 'README.txt').read_text().splitlines():
        if '=' in line or line.strip() == 'MK937595.1':
            groups.append(sorted(x.strip() for x in line.split('=') if x.strip()))
    return sorted(groups)


def test_restatement_gives_the_readme_groups():
    fasta, dup, (rep, strand) = dr.run(INPUTS, dr.default_prefixes(INPUTS))
    ids = [h.split()[0][1:].decode() for h in fasta.split(b'\n') if h.startswith(b'>')]
    assert ids == EXPECTED_IDS
    assert dup.decode() == EXPECTED_DUPLICATES
    names = [dr.first_token(h).decode() for p in INPUTS for h, _, _ in dr.records(dr.read_text(p))]
    groups = {}
    for i, r in enumerate(rep):
        groups.setdefault(r, []).append(names[i])
    assert len(names) == 15 and sorted(sorted(g) for g in groups.values()) == readme_groups()
    assert len(readme_groups()) == 7
    assert [names[i] for i in range(15) if strand[i]] == ['MN428048.1_revcomp']


def test_restatement_definitions():
    assert dr.revcomp(b'ACGTRYKMBVDHSWN-') == b'-NWSDHBVKMRYACGT'
    for s in (b'', b'A', b'ACGT', b'RYKMBVDHSWN-A'):
        assert dr.revcomp(dr.revcomp(s)) == s
    # palindrome: '+'; reverse complement only: '-'; lower case and white space do not count; empty records form one group
    rep, strand = dr.run_seqs(['ACGT', 'acgt', 'AAC', 'GTT', 'G T\nT\r\n', '', '', 'N', 'n'])
    assert rep == [0, 0, 2, 2, 2, 5, 5, 7, 7] and strand == [0, 0, 0, 1, 1, 0, 0, 0, 0]
    with pytest.raises(dr.NotIupac, match="'X' is not an IUPAC"):
        dr.run_seqs(['ACXG'])


def test_new_symbols_exported_and_bound():
    lib = _lib.load()
    for name in ('vg_deduplicate', 'vg_dedup_seqs', 'vg_dedup_set_hash_bits'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert [f for f, _ in _lib.DedupStats._fields_] == ['records', 'unique', 'removed', 'reverse', 'rounds', 'collisions']
    assert [f for f, _ in _lib.DedupParams._fields_] == ['gzip_level', 'num_threads', 'verbosity']
    assert callable(api.deduplicate) and callable(api.dedup_set_hash_bits) and callable(api.deduplicate_files)


def test_seqs_argument_errors_need_no_device():
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGT', 'ACJT'])
    assert e.value.code == -1 and "record 1: 'J' is not an IUPAC nucleotide code" in str(e.value)
    rep, strand, stats = api.deduplicate([])
    assert len(rep) == len(strand) == 0 and stats['records'] == 0


def test_without_device_fails_loudly(tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGT', 'ACGT'])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    assert not (ROOT / 'bin' / 'mfasta-tool').exists()
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--add-prefixes')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'mfasta-tool' not in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()


@pytest.mark.parametrize('extra,msg', [
    (['--add-prefixes', 'a|', 'b|'], 'Number of prefixes must match the number of input files.'),
    (['--add-prefixes', 'a|', 'b,|', 'c|'], 'Prefixes cannot contain commas.'),
    (['--gzip-level', '0'], 'Compression level must be between 1 and 9.'),
    (['--gzip-level', '10'], 'Compression level must be between 1 and 9.'),
])
def test_usage_errors(tmp_path, extra, msg):
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', *extra)
    assert p.returncode == 2 and f'error: {msg}' in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()


def test_directory_input_is_a_usage_error(tmp_path):
    p = run('deduplicate', '-i', INPUTS[0], DATASETS, '-o', tmp_path / 'nr.fna')
    assert p.returncode == 2 and 'is a directory' in p.stderr, p.stderr


@pytest.mark.parametrize('where', ['middle', 'lower', 'gz'])
def test_non_iupac_byte_names_file_and_line(tmp_path, where):
    import gzip
    text = dr.read_text(DATASETS / 'other.fna.gz').split(b'\n')
    # line 7 (1-based) is a sequence line of the first record
    text[6] = text[6][:10] + (b'u' if where == 'lower' else b'Z') + text[6][11:]
    bad = tmp_path / ('bad.fna.gz' if where == 'gz' else 'bad.fna')
    data = b'\n'.join(text)
    bad.write_bytes(gzip.compress(data) if where == 'gz' else data)
    ch = 'u' if where == 'lower' else 'Z'
    with pytest.raises(dr.NotIupac, match=f"{bad}:7: '{ch}'"):
        dr.run([INPUTS[0], bad])
    p = run('deduplicate', '-i', INPUTS[0], bad, '-o', tmp_path / 'nr.fna')
    assert p.returncode == 1 and 'ERROR' in p.stderr
    assert f"{bad}:7: '{ch}' is not an IUPAC nucleotide code" in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()


def _args(argv):
    parser = cli.get_parser()
    return parser, parser.parse_args(argv)


def test_prefix_defaults_and_gz_naming(tmp_path):
    parser, a = _args(['deduplicate', '-i', *map(str, INPUTS), '-o', str(tmp_path / 'nr.fna'), '--add-prefixes'])
    a = cli.validate_args_deduplicate(a, parser)
    assert a.add_prefixes == ['refseq|', 'genbank|', 'other|'] == dr.default_prefixes(INPUTS)
    assert a.output_duplicates_path == tmp_path / 'nr.fna.duplicates.txt'
    call = cli.deduplicate_call(a)
    assert call['prefixes'] == ['refseq|', 'genbank|', 'other|'] and call['gzip_level'] == 0
    parser, a = _args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--gzip-output', '--gzip-level', '7'])
    a = cli.validate_args_deduplicate(a, parser)
    assert a.output_path == tmp_path / 'nr.fna.gz' and a.output_duplicates_path == tmp_path / 'nr.fna.gz.duplicates.txt'
    assert a.add_prefixes is False and cli.deduplicate_call(a)['prefixes'] is None and cli.deduplicate_call(a)['gzip_level'] == 7
    parser, a = _args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna.gz'), '--gzip-output'])
    assert cli.validate_args_deduplicate(a, parser).output_path == tmp_path / 'nr.fna.gz'
    parser, a = _args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'x.tar.fna.gz'), '--add-prefixes', 'p'])
    assert cli.validate_args_deduplicate(a, parser).add_prefixes == ['p']
    assert dr.default_prefixes([tmp_path / 'x.tar.fna.gz']) == ['x|']


def test_mfasta_tool_pass_through_is_unchanged(tmp_path, monkeypatch):
    log = tmp_path / 'argv.txt'
    fake = tmp_path / 'mfasta-tool'
    fake.write_text(f'#!/bin/sh\nprintf "%s\\n" "$@" > {log}\n')
    fake.chmod(0o755)
    monkeypatch.setattr(cli, 'BIN_MFASTA', fake)
    out = tmp_path / 'nr.fna'
    argv = ['vclust.py', 'deduplicate', '-i', *map(str, INPUTS), '-o', str(out), '--add-prefixes', 'a', 'b', 'c',
            '--gzip-output', '--gzip-level', '6', '-t', '3']
    monkeypatch.setattr(sys, 'argv', argv)
    cli.main()
    assert log.read_text().split('\n')[:-1] == [
        'mrds', '-i', ','.join(map(str, INPUTS)), '-o', str(out), '--out-duplicates', f'{out}.duplicates.txt',
        '--remove-duplicates', '--mark-duplicates-orientation', '--rev-comp-as-equivalent', '-t', '3',
        '--verbosity', '1', '--in-prefixes', 'a,b,c', '--gzipped-output', '--gzip-level', '6']
    # the pass-through does not validate: a bare --add-prefixes and a level outside 1..9 go through as before
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(out), '--add-prefixes',
                                      '--gzip-level', '0', '-v', '0', '-t', '1'])
    cli.main()
    assert log.read_text().split('\n')[:-1] == [
        'mrds', '-i', str(INPUTS[0]), '-o', str(out), '--out-duplicates', f'{out}.duplicates.txt', '--remove-duplicates',
        '--mark-duplicates-orientation', '--rev-comp-as-equivalent', '-t', '1']
    assert os.access(fake, os.X_OK)
