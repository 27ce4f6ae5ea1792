"""Terminal repeats of the circular deduplicate mode without a GPU: the restatement (tests/dedup_trepeat_restatement.py) on
hand-worked cases, the reason for the feature (two assemblies of one circle with different overlaps are one group, where
the plain circular mode keeps them apart), the new C symbols and Python surface, the CLI option and its usage errors."""
import inspect
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_circular_restatement as dcr
import dedup_restatement as dr
import dedup_trepeat_restatement as dtr
from test_dedup_cpu import INPUTS
from vclust_amd import _lib, api, cli, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
HEADER = ROOT / 'include' / 'vclust_gpu.h'
HELP = ('Min. length of an exact terminal repeat (the same bases at both ends of a record, as assemblers leave on circular '
        'contigs) taken off before rotations are compared; needs --circular')


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def rand(rng, L):
    return np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()


def test_hand_worked_repeats():
    # borders of ACACACA: 5, 3 and 1; 5 exceeds L / 2 and is not looked at
    assert dtr.tr(b'ACACACA', 1) == 3 and dtr.circ(b'ACACACA', 1) == b'ACAC'
    assert dtr.tr(b'ACACACA', 4) == 0
    rng = np.random.default_rng(1)
    c = rand(rng, 300)
    for k in (21, 55, 127, 150):
        assert dtr.tr(c + c[:k], 20) == k and dtr.circ(c + c[:k], 20) == c
    # the only border has m - 1 symbols
    x = b'ACGTGGCCGGACGT'
    assert [t for t in range(1, len(x)) if x[:t] == x[len(x) - t:]] == [4]
    assert dtr.tr(x, 5) == 0 and dtr.tr(x, 4) == 4 and dtr.tr(x, 1) == 4
    # m above L // 2
    assert dtr.tr(b'ACGTACGT', 4) == 4 and dtr.tr(b'ACGTACGT', 5) == 0 and dtr.tr(b'ACGTAACGT', 5) == 0
    # literal symbols: N equals only N, an IUPAC code only itself; case is ignored
    assert dtr.tr(b'NCGTTTACGT', 4) == 0 and dtr.tr(b'RCGTTTACGT', 4) == 0
    assert dtr.tr(b'NCGTTTNCGT', 4) == 4 and dtr.tr(b'RCGTTTRCGT', 4) == 4
    assert dtr.run_seqs(['acgtTTACGT', 'ac gt\nTTACGN'], 4)[3] == [4, 0]
    assert dtr.tr(b'', 1) == 0 and dtr.circ(b'', 1) == b''
    # a circle is never shorter than half the record
    assert dtr.tr(b'AAAA', 1) == 2 and dtr.tr(b'AAAAA', 1) == 2 and dtr.tr(b'A', 1) == 0


def test_two_assemblies_of_one_circle_are_one_group():
    """The reason for the feature: the same circle opened at two bases, assembled with k = 21 and k = 55, and a third copy on
    the other strand with k = 127.  Raw lengths differ; the circles are rotations."""
    rng = np.random.default_rng(2)
    c = rand(rng, 500)
    r = dcr.rot(c, 137)
    o = dr.revcomp(dcr.rot(c, 200))                # == rot(revcomp(c), 500 - 200)
    seqs = [c + c[:21], r + r[:55], o + o[:127], c, rand(rng, 521)]
    rep, strand, offset, repeat = dtr.group(seqs, 20)
    assert rep == [0, 0, 0, 0, 4] and strand == [0, 0, 1, 0, 0] and offset == [0, 137, 300, 0, 0] and repeat == [21, 55, 127, 0, 0]
    # the kept record is the earliest, with or without a repeat
    assert dtr.group([c, c + c[:21]], 20)[0] == [0, 0] and dtr.group([c, c + c[:21]], 20)[3] == [0, 21]
    # the plain circular mode keeps every one of them apart, also the two of equal raw length
    r2 = dcr.rot(c, 137)
    same_len = [c + c[:55], r2 + r2[:55]]
    assert len(same_len[0]) == len(same_len[1]) and dcr.group(same_len)[0] == [0, 1]
    assert dtr.group(same_len, 20)[:3] == ([0, 0], [0, 0], [0, 137])
    assert dcr.group(seqs)[0] == [0, 1, 2, 3, 4]
    # a minimum above every repeat gives the plain circular groups
    assert dtr.group(seqs, 300)[:3] == dcr.group(seqs) and dtr.group(seqs, 300)[3] == [0] * 5
    # all empty records form one group
    assert dtr.group([b'', b'A', b''], 1)[0] == [0, 1, 0]


def test_restatement_files(tmp_path):
    c = b'ACGGTCATTGCAGGCTTAACGATCGATCCGAT'
    a = tmp_path / 'a.fna'
    a.write_bytes(b'>one first\n' + c + c[:9] + b'\n>two\n' + dcr.rot(c, 5) + b'\n' + dcr.rot(c, 5)[:12] + b'\n')
    fasta, dup, (rep, strand, offset, repeat) = dtr.run([a], ['P|'], 8)
    assert (rep, strand, offset, repeat) == ([0, 0], [0, 0], [0, 5], [9, 12])
    assert fasta == b'>P|one first\n' + c + c[:9] + b'\n'
    assert dup == b'representative\tduplicate\tstrand\toffset\trepeat\trepresentative_repeat\nP|one\tP|two\t+\t5\t12\t9\n'


def test_new_symbols_exported_and_bound():
    lib = _lib.load()
    header = HEADER.read_text()
    for name in ('vg_dedup_terminal_repeats', 'vg_dedup_seqs_circular_tr', 'vg_deduplicate_circular_tr'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header
    assert 'vg_dedup_repeat_stats' in header
    assert [f for f, _ in _lib.DedupRepeatStats._fields_] == ['with_repeat', 'repeat_symbols', 'candidates', 'equal', 'batches']
    # the pinned layouts and signatures beside them have not moved
    assert [f for f, _ in _lib.DedupOptions._fields_] == ['circular']
    assert [f for f, _ in _lib.DedupStats._fields_] == ['records', 'unique', 'removed', 'reverse', 'rounds', 'collisions']
    assert len(_lib.SYMBOLS['vg_deduplicate_ex'][1]) == 7 and len(_lib.SYMBOLS['vg_dedup_seqs_ex'][1]) == 8
    assert len(_lib.SYMBOLS['vg_dedup_terminal_repeats'][1]) == 5 and len(_lib.SYMBOLS['vg_dedup_seqs_circular_tr'][1]) == 10
    assert len(_lib.SYMBOLS['vg_deduplicate_circular_tr'][1]) == 7
    assert list(inspect.signature(api.terminal_repeats).parameters) == ['seqs', 'min_repeat']
    # api.deduplicate takes the option by keyword only, on top of its three parameters (which keep their order)
    assert list(inspect.signature(api.deduplicate).parameters)[:3] == ['seqs', 'circular', 'contained']
    assert len(api.deduplicate([], circular=True, terminal_repeat=5)) == 4
    with pytest.raises(TypeError):
        api.deduplicate([], circular=True, terminal_repeats=5)
    assert inspect.signature(stages.deduplicate).parameters['terminal_repeat'].default == 0


def test_argument_errors_need_no_device():
    with pytest.raises(_lib.VclustGpuError) as e:
        api.terminal_repeats(['ACGTACGT'], 0)
    assert e.value.code == -1 and 'min_repeat' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGTACGT'], circular=True, terminal_repeat=0)
    assert e.value.code == -1 and 'min_repeat' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.deduplicate([INPUTS[0]], 'unused.fna', 'unused.txt', circular=True, terminal_repeat=-3)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        api.deduplicate(['ACGT'], terminal_repeat=4)
    with pytest.raises(ValueError):
        api.deduplicate(['ACGT'], contained=True, terminal_repeat=4)
    with pytest.raises(ValueError):
        stages.deduplicate([INPUTS[0]], 'unused.fna', 'unused.txt', terminal_repeat=4)
    # the alphabet is checked on the host, and nothing to do needs no device
    with pytest.raises(_lib.VclustGpuError) as e:
        api.terminal_repeats(['ACGT', 'ACJT'], 2)
    assert e.value.code == -1 and "record 1: 'J' is not an IUPAC nucleotide code" in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGT', 'ACJT'], circular=True, terminal_repeat=2)
    assert e.value.code == -1 and "record 1: 'J' is not an IUPAC nucleotide code" in str(e.value)
    t = api.terminal_repeats([], 3)
    assert len(t) == 0 and t.dtype == np.int64
    rep, strand, offset, stats = api.deduplicate([], circular=True, terminal_repeat=3)
    assert len(rep) == len(strand) == len(offset) == len(stats['repeat']) == 0 and stats['repeat'].dtype == np.int64
    assert stats['records'] == 0 and stats['with_repeat'] == 0 and stats['batches'] == 0
    # without the keyword the results keep their shape
    assert len(api.deduplicate([])) == 3 and len(api.deduplicate([], circular=True)) == 4
    assert 'repeat' not in api.deduplicate([], circular=True)[3]


def test_usage_errors(tmp_path):
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *INPUTS, '-o', out, '--terminal-repeat', '20')
    assert p.returncode == 2 and '--terminal-repeat needs --circular' in p.stderr, p.stderr
    p = run('deduplicate', '-i', *INPUTS, '-o', out, '--circular', '--terminal-repeat', '0')
    assert p.returncode == 2 and '--terminal-repeat must be at least 1' in p.stderr, p.stderr
    p = run('deduplicate', '-i', *INPUTS, '-o', out, '--circular', '--terminal-repeat', '-5')
    assert p.returncode == 2
    p = run('deduplicate', '-i', *INPUTS, '-o', out, '--contained', '--terminal-repeat', '20')
    assert p.returncode == 2
    p = run('deduplicate', '-i', *INPUTS, '-o', out, '--circular', '--contained', '--terminal-repeat', '20')
    assert p.returncode == 2 and 'exclude each other' in p.stderr
    assert not out.exists()


def test_without_device_fails_loudly(tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.terminal_repeats(['ACGTACGT'], 2)
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGTACGT', 'CGTA'], circular=True, terminal_repeat=2)
    assert e.value.code == -3
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--add-prefixes', '--circular', '--terminal-repeat', '20')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'mfasta-tool' not in p.stderr, p.stderr
    assert 'Running: libvclust_gpu deduplicate' in p.stderr and ' --circular --terminal-repeat 20 [1 GPU]' in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()
    # a byte outside the alphabet is named before the device is missed
    bad = tmp_path / 'bad.fna'
    bad.write_bytes(b'>x\nACGT\nACZT\n')
    p = run('deduplicate', '-i', bad, '-o', tmp_path / 'nr.fna', '--circular', '--terminal-repeat', '20')
    assert p.returncode == 1 and f"{bad}:3: 'Z' is not an IUPAC nucleotide code" in p.stderr, p.stderr


def test_option_parses_and_reaches_the_library_call(tmp_path, monkeypatch):
    parser = cli.get_parser()
    a = parser.parse_args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--circular'])
    assert a.terminal_repeat is None
    a = parser.parse_args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--circular', '--terminal-repeat', '55'])
    assert a.terminal_repeat == 55
    sub = next(x for x in parser._actions if getattr(x, 'choices', None) and 'deduplicate' in x.choices).choices['deduplicate']
    assert next(x for x in sub._actions if '--terminal-repeat' in x.option_strings).help == HELP
    assert '--terminal-repeat' in run('deduplicate', '--help').stdout
    # the stage runs in the library also where bin/mfasta-tool exists
    fake = tmp_path / 'mfasta-tool'
    fake.write_text(f'#!/bin/sh\necho called > {tmp_path}/called\n')
    fake.chmod(0o755)
    monkeypatch.setattr(cli, 'BIN_MFASTA', fake)
    seen = {}
    monkeypatch.setattr(stages, 'deduplicate', lambda **kw: seen.update(kw))
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--circular',
                                      '--terminal-repeat', '55', '-v', '0'])
    cli.main()
    assert seen['circular'] is True and seen['terminal_repeat'] == 55 and not (tmp_path / 'called').exists()
    seen.clear()
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--circular', '-v', '0'])
    cli.main()
    assert seen['circular'] is True and 'terminal_repeat' not in seen
