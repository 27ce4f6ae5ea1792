"""Contained mode of the deduplicate stage without a GPU: the restatement (tests/dedup_contained_restatement.py) on
hand-written cases and against a brute force over every position of both strands, the new C symbols and Python surface,
the CLI flag, and the unchanged output without the flag on the fixture."""
import inspect
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_contained_restatement as dcn
import dedup_restatement as dr
from test_dedup_cpu import EXPECTED_DUPLICATES, EXPECTED_IDS, INPUTS
from vclust_amd import _lib, api, cli, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
HEADER = ROOT / 'include' / 'vclust_gpu.h'

Y = 'ACGGTCATTGCAAGCTTAGGCATCGA'         # 26 symbols, no repeated 4-mer on either strand


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def answer(seqs):
    rep, strand, offset = dcn.run_seqs(seqs)
    return [(r, '-' if s else '+', o) for r, s, o in zip(rep, strand, offset)]


def test_fragment_at_start_middle_and_end():
    assert answer([Y, Y[:7], Y[9:20], Y[-5:]]) == [(0, '+', 0), (0, '+', 0), (0, '+', 9), (0, '+', 21)]
    # the container may come after its fragments
    assert answer([Y[9:20], Y[-5:], Y]) == [(2, '+', 9), (2, '+', 21), (2, '+', 0)]


def test_reverse_strand_fragment():
    rc = dr.revcomp(Y.encode()).decode()
    assert answer([Y, rc[3:12]]) == [(0, '+', 0), (0, '-', 3)]
    assert answer([Y, rc]) == [(0, '+', 0), (0, '-', 0)]
    # the offset counts in revcomp(representative): the fragment revcomp(Y[2:8]) starts at 26 - 8 there
    assert answer([Y, dr.revcomp(Y[2:8].encode())]) == [(0, '+', 0), (0, '-', 18)]


def test_chain_names_the_outermost():
    a, b, c = Y[8:14], Y[5:20], Y
    assert answer([a, b, c]) == [(2, '+', 8), (2, '+', 5), (2, '+', 0)]
    assert answer([c, b, a]) == [(0, '+', 0), (0, '+', 5), (0, '+', 8)]
    # also when the middle link holds the innermost on the other strand
    assert answer([a, dr.revcomp(b.encode()), c]) == [(2, '+', 8), (2, '-', 26 - 20), (2, '+', 0)]


def test_two_equal_length_kept_containers_the_earliest_wins():
    x = 'GATTACA'
    c1, c2 = 'CC' + x + 'TTG', 'AG' + x + 'CCA'
    assert answer([c2, x, c1]) == [(0, '+', 0), (0, '+', 2), (2, '+', 0)]
    assert answer([c1, x, c2]) == [(0, '+', 0), (0, '+', 2), (2, '+', 0)]


def test_a_longer_container_beats_an_earlier_shorter_one():
    x = 'GATTACA'
    short, long_ = 'C' + x + 'C', 'TTT' + x + 'GGGG'
    assert answer([short, x, long_]) == [(0, '+', 0), (2, '+', 3), (2, '+', 0)]


def test_palindrome_is_plus_and_the_smallest_offset_is_reported():
    assert answer(['TTACGTAA', 'ACGT']) == [(0, '+', 0), (0, '+', 2)]
    assert answer(['A' * 30, 'A' * 5, 'T' * 5]) == [(0, '+', 0), (0, '+', 0), (0, '-', 0)]
    assert answer(['ACACACACAC', 'CAC', 'GTG']) == [(0, '+', 0), (0, '+', 1), (0, '-', 0)]


def test_near_miss_stays():
    near = Y[9:19] + ('A' if Y[19] != 'A' else 'C')
    assert answer([Y, near, Y[9:20]]) == [(0, '+', 0), (1, '+', 0), (0, '+', 9)]


def test_empty_records():
    assert answer(['', Y, '', Y[3:9], '\n']) == [(0, '+', 0), (1, '+', 0), (0, '+', 0), (1, '+', 3), (0, '+', 0)]
    assert answer([]) == []


def test_n_matches_only_n():
    assert answer(['ACNGT', 'CNG', 'CAG', 'CRG', 'NNNNN', 'N']) == [(0, '+', 0), (0, '+', 1), (2, '+', 0), (3, '+', 0), (4, '+', 0), (0, '+', 2)]
    # an IUPAC code is not expanded: R is complementary to Y and nothing else
    assert answer(['AARCC', 'GGYTT', 'GGCTT']) == [(0, '+', 0), (0, '-', 0), (2, '+', 0)]


def test_equal_records_keep_the_plain_rule():
    seqs = ['ACGTT', 'AACGT', 'ACGTT', 'acg tt\n', 'ACGTTT']
    assert answer(seqs) == [(4, '+', 0), (4, '-', 1), (4, '+', 0), (4, '+', 0), (4, '+', 0)]
    assert answer(seqs[:4]) == [(0, '+', 0), (0, '-', 0), (0, '+', 0), (0, '+', 0)]


def brute(seqs):
    """The definition by trying every position of every other record, forward strand first."""
    n = len(seqs)
    rc = [dr.revcomp(s) for s in seqs]

    def hits(i, j):
        x = seqs[i]
        return [(st, s) for st, y in enumerate((seqs[j], rc[j])) for s in range(len(y) - len(x) + 1) if y[s:s + len(x)] == x]
    removed = [bool(seqs[i]) and any(hits(i, j) for j in range(n)
                                     if len(seqs[j]) > len(seqs[i]) or (len(seqs[j]) == len(seqs[i]) and j < i)) for i in range(n)]
    out = []
    first_empty = next((i for i in range(n) if not seqs[i]), None)
    for i in range(n):
        if not seqs[i]:
            out.append((first_empty, 0, 0))
        elif not removed[i]:
            out.append((i, 0, 0))
        else:
            best = None
            for j in range(n):
                if j != i and not removed[j] and len(seqs[j]) >= len(seqs[i]) and hits(i, j):
                    if best is None or len(seqs[j]) > len(seqs[best]):
                        best = j
            out.append((best, *hits(i, best)[0]))
    return [list(x) for x in zip(*out)] if out else [[], [], []]


@pytest.mark.parametrize('alphabet', [b'A', b'AC', b'ACGT', b'ACGTRYSWKMBDHVN-'])
def test_restatement_equals_brute_force(alphabet):
    rng = np.random.default_rng(len(alphabet))
    sym = np.frombuffer(alphabet, dtype=np.uint8)
    seqs = [b'', b'']
    for L in (1, 2, 3, 5, 8, 9, 16, 17, 24, 40):
        for _ in range(3):
            s = sym[rng.integers(0, len(sym), L)].tobytes()
            seqs.append(s)
            for _ in range(3):
                a = int(rng.integers(0, L))
                b = int(rng.integers(a, L)) + 1
                f = s[a:b] if rng.random() < 0.5 else dr.revcomp(s[a:b])
                seqs.append(f)
    seqs = [seqs[int(k)] for k in rng.permutation(len(seqs))]
    assert list(dcn.group(seqs)) == brute(seqs)


def test_plain_groups_are_a_subset_of_contained_groups():
    rng = np.random.default_rng(5)
    sym = np.frombuffer(b'ACGT', dtype=np.uint8)
    seqs = []
    for _ in range(150):
        s = sym[rng.integers(0, 4, int(rng.integers(0, 14)))].tobytes()
        seqs += [s, dr.revcomp(s), s[len(s) // 3:]]
    rep, strand, offset = dcn.group(seqs, contained=False)
    assert (rep, strand) == dr.group(seqs) and offset == [0] * len(seqs)
    crep = dcn.group(seqs)[0]
    assert all(crep[i] == crep[r] for i, r in enumerate(rep))
    assert len(set(crep)) < len(set(rep))
    assert all(crep[r] == r for r in set(crep))                  # a representative is a kept record


def test_new_symbols_exported_and_bound():
    lib = _lib.load()
    header = HEADER.read_text()
    for name in ('vg_deduplicate_contained', 'vg_dedup_seqs_contained'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'int {name}(' in header
    for name in ('vg_dedup_set_anchor_symbols', 'vg_dedup_set_index_positions'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS and f'void {name}(' in header
    assert 'vg_dedup_contained_stats' in header
    # the pinned layouts and signatures beside them have not moved
    assert [f for f, _ in _lib.DedupOptions._fields_] == ['circular']
    assert [f for f, _ in _lib.DedupStats._fields_] == ['records', 'unique', 'removed', 'reverse', 'rounds', 'collisions']
    assert len(_lib.SYMBOLS['vg_deduplicate'][1]) == 6 and len(_lib.SYMBOLS['vg_deduplicate_contained'][1]) == 6
    assert len(_lib.SYMBOLS['vg_dedup_seqs_ex'][1]) == 8 and len(_lib.SYMBOLS['vg_dedup_seqs_contained'][1]) == 8
    for f in (api.deduplicate, stages.deduplicate):
        p = inspect.signature(f).parameters
        assert p['circular'].default is False and p['contained'].default is False
    assert list(inspect.signature(api.deduplicate).parameters) == ['seqs', 'circular', 'contained']
    assert list(inspect.signature(stages.deduplicate).parameters)[:8] == ['paths', 'out_path', 'dup_path', 'prefixes', 'gzip_level',
                                                                         'num_threads', 'verbosity', 'circular']
    # the knobs clamp and can be restored without a device
    api.dedup_set_anchor_symbols(1)
    api.dedup_set_index_positions(1000)
    api.dedup_set_anchor_symbols()
    api.dedup_set_index_positions()


def test_both_modes_together_are_refused(tmp_path):
    with pytest.raises(ValueError):
        api.deduplicate(['ACGT'], circular=True, contained=True)
    with pytest.raises(ValueError):
        stages.deduplicate([INPUTS[0]], tmp_path / 'a', tmp_path / 'b', circular=True, contained=True)
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--contained', '--circular')
    assert p.returncode == 2 and '--contained' in p.stderr and '--circular' in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()


def test_argument_errors_need_no_device():
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGT', 'ACJT'], contained=True)
    assert e.value.code == -1 and "record 1: 'J' is not an IUPAC nucleotide code" in str(e.value)
    rep, strand, offset, stats = api.deduplicate([], contained=True)
    assert len(rep) == len(strand) == len(offset) == 0 and offset.dtype == np.int64
    assert stats['records'] == 0 and stats['passes'] == 0 and stats['candidates'] == 0
    assert len(api.deduplicate([])) == 3


def test_without_device_fails_loudly(tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        api.deduplicate(['ACGTAC', 'CGTA'], contained=True)
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--add-prefixes', '--contained')
    assert p.returncode == 1
    assert 'ERROR' in p.stderr and 'no HIP device' in p.stderr and 'mfasta-tool' not in p.stderr, p.stderr
    assert 'Running: libvclust_gpu deduplicate' in p.stderr and ' --contained [1 GPU]' in p.stderr, p.stderr
    assert not (tmp_path / 'nr.fna').exists()
    # validation comes first: a usage error is exit 2, and a byte outside the alphabet is named before the device is missed
    p = run('deduplicate', '-i', *INPUTS, '-o', tmp_path / 'nr.fna', '--contained', '--gzip-level', '0')
    assert p.returncode == 2 and 'Compression level must be between 1 and 9.' in p.stderr
    bad = tmp_path / 'bad.fna'
    bad.write_bytes(b'>x\nACGT\nACZT\n')
    p = run('deduplicate', '-i', bad, '-o', tmp_path / 'nr.fna', '--contained')
    assert p.returncode == 1 and f"{bad}:3: 'Z' is not an IUPAC nucleotide code" in p.stderr, p.stderr


def test_flag_parses_and_reaches_the_library_call(tmp_path, monkeypatch):
    parser = cli.get_parser()
    a = parser.parse_args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna')])
    assert a.contained is False and a.circular is False
    a = parser.parse_args(['deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--contained'])
    assert a.contained is True and a.circular is False
    sub = next(x for x in parser._actions if getattr(x, 'choices', None) and 'deduplicate' in x.choices).choices['deduplicate']
    text = next(x for x in sub._actions if '--contained' in x.option_strings).help
    assert '\n' not in text and 'substring' in text and 'longer' in text and 'reverse complement' in text
    assert '--contained' in run('deduplicate', '--help').stdout
    # with the flag the stage runs in the library also when bin/mfasta-tool exists; without it the tool is still called
    fake = tmp_path / 'mfasta-tool'
    fake.write_text(f'#!/bin/sh\necho called > {tmp_path}/called\n')
    fake.chmod(0o755)
    monkeypatch.setattr(cli, 'BIN_MFASTA', fake)
    seen = {}
    monkeypatch.setattr(stages, 'deduplicate', lambda **kw: seen.update(kw))
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '--contained', '-v', '0'])
    cli.main()
    assert seen['contained'] is True and 'circular' not in seen and seen['paths'] == [INPUTS[0]] and not (tmp_path / 'called').exists()
    seen.clear()
    monkeypatch.setattr(sys, 'argv', ['vclust.py', 'deduplicate', '-i', str(INPUTS[0]), '-o', str(tmp_path / 'nr.fna'), '-v', '0'])
    cli.main()
    assert seen == {} and (tmp_path / 'called').exists()


def test_fixture_output_without_the_flag_is_unchanged(tmp_path):
    """The bytes without the flag on the 15-record fixture: the plain restatement's and, where a device is visible, the
    CLI's.  In contained mode the fixture has the same groups (it holds no fragment), every offset 0."""
    fasta, dup, _ = dcn.run(INPUTS, dr.default_prefixes(INPUTS), contained=False)
    assert (fasta, dup) == dr.run(INPUTS, dr.default_prefixes(INPUTS))[:2] and dup.decode() == EXPECTED_DUPLICATES
    cfasta, cdup, (rep, strand, offset) = dcn.run(INPUTS, dr.default_prefixes(INPUTS))
    assert cfasta == fasta and set(offset) == {0}
    assert cdup.decode() == '\n'.join(ln + '\t' + ('offset' if k == 0 else '0')
                                      for k, ln in enumerate(EXPECTED_DUPLICATES.splitlines())) + '\n'
    if api.device_count() > 0:
        out = tmp_path / 'nr.fna'
        p = run('deduplicate', '-i', *INPUTS, '-o', out, '--add-prefixes', '-v', '0')
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
        assert [ln.split()[0][1:] for ln in out.read_text().splitlines() if ln.startswith('>')] == EXPECTED_IDS
