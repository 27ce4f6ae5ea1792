"""Terminal repeats of the circular deduplicate mode on the GPU against the sequential restatement
(tests/dedup_trepeat_restatement.py): the repeat pass alone on planted repeats of every framing, false candidates, many
candidates in several batches, low complexity, the chunk boundary, the full alphabet; then the grouping over circles with
forced hash collisions, the CLI, and a plain circular call after a trimming one."""
import gzip
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_circular_restatement as dcr
import dedup_restatement as dr
import dedup_trepeat_restatement as dtr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
SYMBOLS = np.frombuffer(b'ACGTRYSWKMBDHVN-', dtype=np.uint8)
CHUNK = 16384            # symbols per (record, chunk) task: 2 048 words


def run(*args, timeout=600):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


def rand(rng, L, k=4):
    return SYMBOLS[:k][rng.integers(0, k, L)].tobytes()


def other(ch: int) -> bytes:
    return b'A' if ch != ord('A') else b'C'


def plant(s: bytes, t: int) -> bytes:
    """s with its first t symbols copied over its last t (t <= len(s) // 2)."""
    assert 0 <= t <= len(s) // 2
    return s[:len(s) - t] + s[:t]


def check_repeats(api, seqs, m):
    got = api.terminal_repeats(seqs, m)
    want = [dtr.tr(dr.normalise(s), m) for s in seqs]
    assert got.dtype == np.int64 and got.tolist() == want
    return want


def check_seqs(api, seqs, m):
    rep, strand, offset, st = api.deduplicate(seqs, circular=True, terminal_repeat=m)
    erep, estrand, eoffset, erepeat = dtr.run_seqs(seqs, m)
    assert st['repeat'].tolist() == erepeat and st['repeat'].dtype == np.int64
    assert rep.tolist() == erep
    assert strand.tolist() == estrand
    assert offset.tolist() == eoffset and offset.dtype == np.int64
    assert st['records'] == len(seqs) and st['unique'] == sum(r == i for i, r in enumerate(erep))
    assert st['removed'] == len(seqs) - st['unique']
    assert st['reverse'] == sum(s for i, s in enumerate(estrand) if erep[i] != i)
    assert st['with_repeat'] == sum(t > 0 for t in erepeat) and st['repeat_symbols'] == sum(erepeat)
    assert st['candidates'] >= st['equal'] >= st['with_repeat']
    return erep, estrand, eoffset, erepeat, st


LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200)
MINIMA = (1, 5, 15, 16, 17, 20)


def planted_cases(m):
    """(L, t) for the minimum m: t in {m - 1, m, m + 1, L // 2 - 1, L // 2} within 0 .. L // 2; -> (cases, combinations left out)"""
    cases, left_out = [], 0
    for L in LENGTHS:
        for t in (m - 1, m, m + 1, L // 2 - 1, L // 2):
            if 0 <= t <= L // 2:
                cases.append((L, t))
            else:
                left_out += 1
    return cases, left_out


def test_planted_cases_cover_every_framing():
    """What test_planted_repeats runs.  12 lengths x 5 repeats x 6 minima = 360 combinations; those with a
    repeat below 0 or above L // 2 do not exist and are left out, counted here."""
    used = [(L, t, m) for m in MINIMA for L, t in planted_cases(m)[0]]
    left_out = sum(planted_cases(m)[1] for m in MINIMA)
    assert len(used) + left_out == len(LENGTHS) * 5 * len(MINIMA) == 360
    assert left_out == 96, left_out
    found = [(L, t) for L, t, m in used if t >= m]
    assert {(L - t) % 8 for L, t in found} == set(range(8)) and {t % 8 for L, t in found} == set(range(8))


@pytest.mark.parametrize('m', MINIMA)
def test_planted_repeats(api, m):
    rng = np.random.default_rng(m)
    cases, _ = planted_cases(m)
    seqs = [plant(rand(rng, L), t) for L, t in cases]
    want = check_repeats(api, seqs, m)
    # the planted repeat is found when it reaches the minimum (a longer chance border of random bases may hide it)
    assert sum(w == t for (L, t), w in zip(cases, want) if t >= m) >= sum(t >= m for _, t in cases) - 3
    assert all(w == 0 or w >= m for w in want)


@pytest.mark.parametrize('m', [5, 16, 20])
def test_false_candidate(api, m):
    """The first window recurs in the second half, but the suffix differs from the prefix in its last symbol only."""
    rng = np.random.default_rng(30 + m)
    seqs = []
    for L, t in ((200, 60), (200, 100), (65, 32), (CHUNK + 50, 300), (2 * CHUNK + 100, CHUNK + 9)):
        s = bytearray(plant(rand(rng, L), t))
        s[-1:] = other(s[-1])
        seqs += [bytes(s), plant(rand(rng, L), t)]
    want = check_repeats(api, seqs, m)
    assert want[0::2] == [0] * 5 and want[1::2] == [60, 100, 32, 300, CHUNK + 9]


def test_many_candidates_take_several_batches(api):
    """The record's first 16 symbols recur 300 times in its second half, each time followed by other symbols; only the last
    occurrence starts the repeat.  Candidates are tried by increasing start, so it has rank 299: 9 batches."""
    rng = np.random.default_rng(3)
    unit = rand(rng, 16)
    head = unit + rand(rng, 40)
    rec = head + rand(rng, 6400) + b''.join(unit + rand(rng, 5) for _ in range(299)) + head
    assert len(rec) - len(rec) // 2 <= len(head) + 6400
    assert check_repeats(api, [rec, rand(rng, 500)], 16) == [56, 0]
    _, _, _, erepeat, st = check_seqs(api, [rec, rec[:-56], rand(rng, 500)], 16)
    assert erepeat == [56, 0, 0]
    assert st['batches'] >= 2 and st['batches'] == 9 and st['candidates'] == 300 + 299 and st['equal'] == 1, st
    # a minimum below 16 compares fewer symbols per start: more candidates, the same answer
    assert check_repeats(api, [rec], 3) == [56]


def test_candidate_list_grows_and_takes_many_batches(api):
    """As above with 1 201 occurrences in a set of 2 records: more candidates than the list's first 2 * 2 + 1 024 slots, so
    the candidate pass runs again on a grown list; the last occurrence has rank 1 200, the 11th batch.  Then poly-A with a
    minimum of 1: 2 500 candidates per record, a grown list whose answer is the candidate of rank 0."""
    rng = np.random.default_rng(3)
    unit = rand(rng, 16)
    head = unit + rand(rng, 40)
    rec = head + rand(rng, 27000) + b''.join(unit + rand(rng, 5) for _ in range(1200)) + head
    L = len(rec)
    starts = [u for u in range(L - L // 2, L - 16 + 1) if rec.startswith(unit, u)]
    assert L == 52312 and len(starts) == 1201 > 2 * 2 + 1024 and starts[-1] == L - 56
    batches = len(starts).bit_length()                    # batch b holds the ranks 2^b - 1 .. 2^(b+1) - 2
    _, _, _, erepeat, st = check_seqs(api, [rec, rand(rng, 500)], 16)
    assert erepeat[0] == 56
    assert st['batches'] == batches == 11 and st['equal'] == 1 and st['candidates'] == min(len(starts), 2 ** batches - 1), st
    assert check_repeats(api, [b'A' * 5000, b'A' * 4999], 1) == [2500, 2499]


def test_poly_a(api):
    """Every start is a candidate and the first one is equal: one batch."""
    seqs = [b'A' * 1000, b'A' * 999]
    assert check_repeats(api, seqs, 20) == [500, 499]
    erep, _, _, _, st = check_seqs(api, seqs, 20)
    assert erep == [0, 0] and st['batches'] == 1 and st['candidates'] == 2 and st['equal'] == 2, st
    assert check_repeats(api, [b'AC' * 500, b'ACG' * 333], 1) == [500, 498]


def test_chunk_boundary(api):
    """40 000 symbols with a 17 000-symbol repeat: the candidate starts and the compare both cross the 16 384-symbol chunk
    boundary; a copy that differs in the repeat's second chunk only; a repeat that starts in the record's third chunk."""
    rng = np.random.default_rng(4)
    s = rand(rng, 40000)
    long = plant(s, 17000)
    near = bytearray(long)
    near[23000 + CHUNK + 100:23000 + CHUNK + 101] = other(near[23000 + CHUNK + 100])
    late = plant(rand(rng, 40000), 5000)
    assert check_repeats(api, [long, bytes(near), late], 100) == [17000, 0, 5000]
    erep, _, eoffset, _, _ = check_seqs(api, [dcr.rot(s[:23000], 777), long, late, late[:35000]], 100)
    assert erep == [0, 0, 2, 2] and eoffset[1] == 23000 - 777


def test_full_alphabet_inside_the_repeat(api):
    rng = np.random.default_rng(5)
    seqs = []
    for L, t in ((40, 20), (64, 17), (333, 100), (4097, 2048), (100, 16)):
        s = plant(rand(rng, L, 16), t)
        seqs += [s, s.lower(), s[:L - t] + s[L - t:].lower()]
    seqs += [b'-' * 41, b'N' * 40, b'ACGT' + b'-' * 30 + b'ACGT', b'-' * 20 + b'ACGTA' + b'-' * 20, b'n' * 21 + b'N' * 20]
    want = check_repeats(api, seqs, 16)
    assert want[-5:] == [20, 20, 0, 20, 20] and all(w >= 16 for w in want[:15])
    check_repeats(api, seqs, 1)
    erep, _, _, _, _ = check_seqs(api, seqs, 16)
    assert erep[:15] == [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9, 12, 12, 12]


def test_n_equals_only_n(api):
    """Records whose ends would be equal only if N matched A (or an IUPAC code one of its bases): no repeat."""
    rng = np.random.default_rng(6)
    seqs = []
    for L, t, j in ((100, 30, 0), (100, 30, 17), (100, 30, 29), (257, 128, 64), (64, 32, 31)):
        for code in (b'N', b'R'):
            s = bytearray(plant(rand(rng, L), t))
            s[j:j + 1] = b'A'
            s[L - t + j:L - t + j + 1] = code
            seqs.append(bytes(s))
            s[j:j + 1] = code                         # the same code at both ends: a repeat
            seqs.append(bytes(s))
    want = check_repeats(api, seqs, 20)
    assert want[0::2] == [0] * 10 and want[1::2] == [30, 30, 30, 30, 30, 30, 128, 128, 32, 32]


N_CIRCLES = 40 + 1 + 2 + 60      # the circles of circle_set: 40, the empty one, two of 1 000 symbols, 60 of 300


@pytest.fixture(scope='module')
def circle_set():
    """40 circles of 300 to 5 000 symbols, four copies each (random rotation, random strand, overlap of 0, 21, 55 or 127
    symbols), shuffled, with plain duplicates, empty records, two different circles of one length and 60 more different
    circles of 300 symbols (enough for two of them to share 8 hash bits); and the restatement's answer for the minimum 20."""
    rng = np.random.default_rng(7)
    seqs = []
    for _ in range(40):
        c = rand(rng, int(rng.integers(300, 5001)))
        for _ in range(4):
            r = dcr.rot(c, int(rng.integers(0, len(c))))
            if rng.random() < 0.5:
                r = dr.revcomp(r)
            seqs.append(r + r[:int(rng.choice([0, 21, 55, 127]))])
    seqs += [seqs[3], seqs[50].lower(), dr.revcomp(seqs[77]), b'', b'', b'\n']
    a, b = rand(rng, 1000), rand(rng, 1000)
    seqs += [a + a[:55], b + b[:55], a + a[:21], b]
    for _ in range(60):
        c = rand(rng, 300)
        seqs.append(c + c[:21])
    seqs = [seqs[int(k)] for k in rng.permutation(len(seqs))]
    return seqs, dtr.run_seqs(seqs, 20)


@pytest.mark.parametrize('bits', [128, 0, 8])
def test_grouping_over_circles(api, circle_set, bits):
    seqs, (erep, estrand, eoffset, erepeat) = circle_set
    assert sum(r == i for i, r in enumerate(erep)) == N_CIRCLES and sorted(set(erepeat)) == [0, 21, 55, 127]
    try:
        api.dedup_set_hash_bits(bits)
        rep, strand, offset, st = api.deduplicate(seqs, circular=True, terminal_repeat=20)
    finally:
        api.dedup_set_hash_bits(128)
    assert st['repeat'].tolist() == erepeat
    assert rep.tolist() == erep and strand.tolist() == estrand and offset.tolist() == eoffset
    assert st['unique'] == N_CIRCLES and st['with_repeat'] == sum(t > 0 for t in erepeat)
    assert (st['collisions'] > 0 and st['rounds'] > 1) if bits < 128 else (st['collisions'] == 0 and st['rounds'] == 1), st


def test_minimum_above_every_repeat_is_the_plain_circular_mode(api, circle_set):
    seqs, _ = circle_set
    rep, strand, offset, st = api.deduplicate(seqs, circular=True, terminal_repeat=1 + max(len(s) for s in seqs) // 2)
    prep, pstrand, poffset, pst = api.deduplicate(seqs, circular=True)
    erep, estrand, eoffset = dcr.run_seqs(seqs)
    assert rep.tolist() == prep.tolist() == erep and strand.tolist() == pstrand.tolist() == estrand
    assert offset.tolist() == poffset.tolist() == eoffset
    assert st['repeat'].tolist() == [0] * len(seqs) and st['with_repeat'] == 0 and st['candidates'] == 0 and st['batches'] == 0
    assert {k: st[k] for k in pst} == pst and 'repeat' not in pst


def test_a_plain_circular_call_after_a_trimming_one(api, circle_set):
    """The trim happens in the device copy of one call: a later call on the same input in the same process gives the plain
    circular answer, and the repeat pass gives the same repeats again."""
    seqs, (erep, _, _, erepeat) = circle_set
    rep, _, _, st = api.deduplicate(seqs, circular=True, terminal_repeat=20)
    assert rep.tolist() == erep
    prep, pstrand, poffset, _ = api.deduplicate(seqs, circular=True)
    assert (prep.tolist(), pstrand.tolist(), poffset.tolist()) == dcr.run_seqs(seqs)
    assert prep.tolist() != erep
    assert api.terminal_repeats(seqs, 20).tolist() == erepeat
    rep, strand, _ = api.deduplicate(seqs)
    assert (rep.tolist(), strand.tolist()) == dr.group([dr.normalise(s) for s in seqs])


@pytest.fixture(scope='module')
def cli_input(tmp_path_factory):
    d = tmp_path_factory.mktemp('trepeat')
    rng = np.random.default_rng(8)
    g1, g2, g3 = rand(rng, 5000), rand(rng, 777), rand(rng, 90)

    def wrap(s, w=60):
        return b'\n'.join(s[k:k + w] for k in range(0, len(s), w)) + b'\n'
    r1, r2 = dcr.rot(g1, 1234), dr.revcomp(dcr.rot(g2, 500))
    a = d / 'first.fna'
    a.write_bytes(b'>g1 phage one\n' + wrap(g1 + g1[:55]) + b'>g2\n' + wrap(g2, 70) + b'>g3 short\n' + g3 + b'\n>e1\n')
    b = d / 'second.fna.gz'
    b.write_bytes(gzip.compress(b'>g1_rot k=127\n' + wrap(r1 + r1[:127]) + b'>g2_rc_rot\r\n' + wrap((r2 + r2[:21]).lower(), 50)
                                + b'>g3_copy\n' + g3 + g3[:19] + b'\n>g3_k20\n' + g3 + g3[:20] + b'\n>e2\n\n>new\n' + wrap(rand(rng, 777))))
    return [a, b]


@pytest.mark.parametrize('gz', [False, True])
def test_cli_end_to_end(api, cli_input, tmp_path, gz):
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '--circular', '--terminal-repeat', '20', '-v', '1',
            *(['--gzip-output', '--gzip-level', '5'] if gz else []))
    assert p.returncode == 0, p.stderr
    assert ' --circular --terminal-repeat 20 [1 GPU]' in p.stderr and '4 records with a terminal repeat' in p.stderr, p.stderr
    fasta, dup, (rep, strand, offset, repeat) = dtr.run(cli_input, ['A|', 'B|'], 20)
    written = tmp_path / ('nr.fna.gz' if gz else 'nr.fna')
    assert (gzip.decompress(written.read_bytes()) if gz else written.read_bytes()) == fasta
    assert pathlib.Path(f'{written}.duplicates.txt').read_bytes() == dup
    assert dup.splitlines()[:3] == [b'representative\tduplicate\tstrand\toffset\trepeat\trepresentative_repeat',
                                    b'A|g1\tB|g1_rot\t+\t1234\t127\t55', b'A|g2\tB|g2_rc_rot\t-\t%d\t21\t0' % offset[5]]
    assert b'A|g3\tB|g3_k20\t+\t0\t20\t0' in dup and b'A|e1\tB|e2\t+\t0\t0\t0' in dup and len(dup.splitlines()) == 5
    assert b'>B|g3_copy\n' in fasta and repeat == [55, 0, 0, 0, 127, 21, 0, 20, 0, 0]


def test_cli_without_the_option_is_the_circular_file(api, cli_input, tmp_path):
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '--circular', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    fasta, dup, _ = dcr.run(cli_input, ['A|', 'B|'])
    assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
    assert dup == b'representative\tduplicate\tstrand\toffset\nA|e1\tB|e2\t+\t0\n' and b'>B|g1_rot ' in fasta
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '-v', '0')
    assert p.returncode == 0, p.stderr
    assert (out.read_bytes(), (tmp_path / 'nr.fna.duplicates.txt').read_bytes()) == dr.run(cli_input, ['A|', 'B|'])[:2]
