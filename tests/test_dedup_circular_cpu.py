"""Circular mode of the deduplicate stage without a GPU: the restatement (tests/dedup_circular_restatement.py) on hand-written
cases and against a brute force over all rotations of both strands, the new C symbols and Python surface, the CLI flag,
and the unchanged non-circular output on the fixture."""
import itertools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_circular_restatement as dcr
import dedup_restatement as dr
from test_dedup_cpu import EXPECTED_DUPLICATES, EXPECTED_IDS, INPUTS
from vclust_amd import _lib, api, cli, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
HEADER = ROOT / 'include' / 'vclust_gpu.h'


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def pair(kept, removed):
    rep, strand, offset = dcr.run_seqs([kept, removed])
    assert rep == [0, 0]
    return '-' if strand[1] else '+', offset[1]


def test_hand_written_cases():
    assert pair('ACGTT', 'GTTAC') == ('+', 2)
    assert dr.revcomp(b'ACGTT') == b'AACGT' and dcr.rot(b'AACGT', 2) == b'CGTAA'
    assert pair('ACGTT', 'AACGT') == ('-', 0)
    assert pair('ACGTT', 'CGTAA') == ('-', 2)
    assert pair('A' * 9, 'T' * 9) == ('-', 0)
    assert pair('AC' * 4, 'CA' * 4) == ('+', 1)
    # a palindromic circle is '+', the smallest offset wins, other lengths and other circles stay apart
    assert pair('ACGT', 'ACGT') == ('+', 0) and pair('ACGT', 'CGTA') == ('+', 1)
    rep, strand, offset = dcr.run_seqs(['ACGTT', 'ACGTC', 'ACGT', '', 'acg tt\n', '', 'TTACG', 'TAACG'])
    assert rep == [0, 1, 2, 3, 0, 3, 0, 0] and strand == [0, 0, 0, 0, 0, 0, 0, 1] and offset == [0, 0, 0, 0, 0, 0, 3, 4]


def test_reverse_complement_rotated_the_other_way():
    """revcomp(ACGTT) = AACGT rotated by 2 in the contract's sense, rot(X, s)[i] = X[(i + s) mod L], is CGTAA: '-', offset 2
    (test_hand_written_cases).  GTAAC is the same circle opened two symbols to the other side, rot(AACGT, 3), so the
    contract and the restatement's (Y + Y).find give it '-' with offset 3, not 2."""
    assert dcr.rot(b'AACGT', 3) == b'GTAAC' and (b'AACGT' * 2).find(b'GTAAC') == 3
    assert pair('ACGTT', 'GTAAC') == ('-', 3)


def brute(seqs):
    """Minimum over all rotations of both strands as the canonical form of a circle; the earliest record with the same form
    is kept; strand and offset by trying every s, forward strand first."""
    first, out = {}, []
    for i, s in enumerate(seqs):
        forms = [dcr.rot(y, k) for y in (s, dr.revcomp(s)) for k in range(max(len(s), 1))]
        j = first.setdefault((len(s), min(forms)), i)
        if j == i:
            out.append((i, 0, 0))
            continue
        hit = [(st, k) for st, y in enumerate((seqs[j], dr.revcomp(seqs[j]))) for k in range(max(len(s), 1)) if dcr.rot(y, k) == s]
        out.append((j, *hit[0]))
    return [list(x) for x in zip(*out)] if out else [[], [], []]


@pytest.mark.parametrize('alphabet', [b'AC', b'ACGT', b'ACGTRYSWKMBDHVN-'])
def test_restatement_equals_brute_force(alphabet):
    rng = np.random.default_rng(len(alphabet))
    sym = np.frombuffer(alphabet, dtype=np.uint8)
    seqs = []
    for L in list(range(0, 20)) + [31, 32, 33, 63, 64]:
        for _ in range(3):
            s = sym[rng.integers(0, len(sym), L)].tobytes()
            if L >= 4 and rng.random() < 0.5:                       # periodic: many equal rotations
                s = (s[:int(rng.integers(1, 4))] * L)[:L]
            seqs.append(s)
            for _ in range(3):
                k = int(rng.integers(0, max(L, 1)))
                seqs.append(dcr.rot(s if rng.random() < 0.5 else dr.revcomp(s), k))
    order = rng.permutation(len(seqs))
    seqs = [seqs[int(k)] for k in order]
    assert list(dcr.group(seqs)) == brute(seqs)


def test_every_binary_circle_up_to_length_8():
    seqs = [bytes(t) for L in range(0, 9) for t in itertools.product(b'AC', repeat=L)]
    assert list(dcr.group(seqs)) == brute(seqs)


def test_without_the_flag_the_groups_are_the_plain_ones():
    rng = np.random.default_rng(5)
    sym = np.frombuffer(b'ACGT', dtype=np.uint8)
    seqs = []
    for _ in range(300):
        s = sym[rng.integers(0, 4, int(rng.integers(0, 12)))].tobytes()
        seqs += [s, dr.revcomp(s), dcr.rot(s, len(s) // 2)]
    rep, strand, offset = dcr.group(seqs, circular=False)
    assert (rep, strand) == dr.group(seqs) and offset == [0] * len(seqs)
    # the circular groups are unions of the plain ones
    crep = dcr.group(seqs)[0]
    assert all(crep[i] == crep[r] for i, r in enumerate(rep))
    assert len(set(crep)) < len(set(rep))


def test_new_symbols_exported_and_bound():
    lib = _lib.load()
    header = HEADER.read_text()
    for name in ('vg_deduplicate_ex', 'vg_dedup_seqs_ex'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header
    assert 'vg_dedup_options' in header
    assert [f for f, _ in _lib.DedupOptions._fields_] == ['circular']
    # the pinned layouts and signatures beside them have not moved
    assert [f for f, _ in _lib.DedupParams._fields_] == ['gzip_level', 'num_threads', 'verbosity']
    assert len(_lib.SYMBOLS['vg_deduplicate'][1]) == 6 and len(_lib.SYMBOLS['vg_dedup_seqs'][1]) == 6
    assert len(_lib.SYMBOLS['vg_deduplicate_ex'][1]) == 7 and len(_lib.SYMBOLS['vg_dedup_seqs_ex'][1]) == 8
    import inspect
    assert inspect.signature(api.deduplicate).parameters['circular'].default is False
    assert inspect.signature(stages.deduplicate).parameters['circular'].default is False
    assert list(inspect.signature(stages.deduplicate).parameters)[:7] == ['paths', 'out_path', 'dup_path', 'prefixes', 'gzip_level',
                                                                         'num_threads', 'verbosity']


def test_argument_errors_need_no_device():
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGT', 'ACJT'], circular=True)
    assert e.value.code == -1 and "record 1: 'J' is not an IUPAC nucleotide code" in str(e.value)
    rep, strand, offset, stats = api.deduplicate([], circular=True)
    assert len(rep) == len(strand) == len(offset) == 0 and offset.dtype == np.int64 and stats['records'] == 0
    assert len(api.deduplicate([])) == 3


def test_without_device_fails_loudly(tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGT', 'CGTA'], circular=True)
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--add-prefixes', '--circular')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'mfasta-tool' not in p.stderr, p.stderr
    assert 'Running: libvclust_gpu deduplicate' in p.stderr and ' --circular [1 GPU]' in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()
    # validation comes first: a usage error is exit 2, and a byte outside the alphabet is named before the device is missed
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--circular', '--gzip-level', '0')
    assert p.returncode == 2 and 'Compression level must be between 1 and 9.' in p.stderr
    bad = tmp_path / 'bad.fna'
    bad.write_bytes(b'>x\nACGT\nACZT\n')
    p = run('deduplicate', '-i', bad, '-o', tmp_path / 'nr.fna', '--circular')
    assert p.returncode == 1 and f"{bad}:3: 'Z' is not an IUPAC nucleotide code" in p.stderr, p.stderr


def test_flag_parses_and_reaches_the_library_call(tmp_path, monkeypatch):
    parser = cli.get_parser()
    a = parser.parse_args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna')])
    assert a.circular is False
    a = parser.parse_args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--circular'])
    assert a.circular is True
    sub = next(x for x in parser._actions if getattr(x, 'choices', None) and 'deduplicate' in x.choices).choices['deduplicate']
    text = next(x for x in sub._actions if '--circular' in x.option_strings).help
    assert '\n' not in text and 'rotations' in text and 'reverse complement' in text
    assert '--circular' in run('deduplicate', '--help').stdout
    # with the flag the stage runs in the library also when bin/mfasta-tool exists; without it the tool is still called
    fake = tmp_path / 'mfasta-tool'
    fake.write_text(f'#!/bin/sh\necho called > {tmp_path}/called\n')
    fake.chmod(0o755)
    monkeypatch.setattr(cli, 'BIN_MFASTA', fake)
    seen = {}
    monkeypatch.setattr(stages, 'deduplicate', lambda **kw: seen.update(kw))
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--circular', '-v', '0'])
    cli.main()
    assert seen['circular'] is True and seen['paths'] == [INPUTS[0]] and not (tmp_path / 'called').exists()
    seen.clear()
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '-v', '0'])
    cli.main()
    assert seen == {} and (tmp_path / 'called').exists()


def test_fixture_output_without_the_flag_is_unchanged(tmp_path):
    """The non-circular bytes on the fixture: the restatement's (both modules agree) and, where a device is visible, the
    CLI's.  In circular mode the fixture has the same groups (it holds no rotated copy), every offset 0."""
    fasta, dup, _ = dcr.run(INPUTS, dr.default_prefixes(INPUTS), circular=False)
    assert (fasta, dup) == dr.run(INPUTS, dr.default_prefixes(INPUTS))[:2] and dup.decode() == EXPECTED_DUPLICATES
    cfasta, cdup, (rep, strand, offset) = dcr.run(INPUTS, dr.default_prefixes(INPUTS))
    assert cfasta == fasta and set(offset) == {0}
    assert cdup.decode() == '\n'.join(ln + '\t' + ('offset' if k == 0 else '0')
                                      for k, ln in enumerate(EXPECTED_DUPLICATES.splitlines())) + '\n'
    if api.device_count() > 0:
        out = tmp_path / 'nr.fna'
        p = run('deduplicate', '-i', *INPUTS, '-o', out, '--add-prefixes', '-v', '0')
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
        assert [ln.split()[0][1:] for ln in out.read_text().splitlines() if ln.startswith('>')] == EXPECTED_IDS
