"""Circular mode of the deduplicate stage on the GPU against the sequential restatement
(tests/dedup_circular_restatement.py): representative, strand and offset of every record, on edge lengths, chunk
boundaries, periodic records, the full alphabet, forced hash collisions, one long record, random sets and the CLI."""
import gzip
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_circular_restatement as dcr
import dedup_restatement as dr

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


def check_seqs(api, seqs):
    rep, strand, offset, st = api.deduplicate(seqs, circular=True)
    erep, estrand, eoffset = dcr.run_seqs(seqs)
    assert rep.tolist() == erep
    assert strand.tolist() == estrand
    assert offset.tolist() == eoffset and offset.dtype == np.int64
    assert st['records'] == len(seqs) and st['unique'] == sum(r == i for i, r in enumerate(erep))
    assert st['removed'] == len(seqs) - st['unique']
    assert st['reverse'] == sum(s for i, s in enumerate(estrand) if erep[i] != i)
    return erep, estrand, eoffset, st


def edge_set(rng, L):
    """A record, its rotations by 1, 7, 8, 9, L - 1 (those below L), the reverse complement of each, an unrelated record of
    the same length, and a rotation with one symbol changed at the wrap point (the rotated record's last original symbol)."""
    s = rand(rng, L)
    seqs = [s]
    for k in sorted({k for k in (1, 7, 8, 9, L - 1) if 0 < k < L}):
        r = dcr.rot(s, k)
        seqs += [r, dr.revcomp(r)]
    seqs.append(dr.revcomp(s))
    seqs.append(rand(rng, L))
    if L >= 2:
        k = L // 2
        r = bytearray(dcr.rot(s, k))
        r[L - k - 1:L - k] = other(r[L - k - 1])           # the symbol s[L - 1], next to the wrap point
        seqs.append(bytes(r))
        r = bytearray(dcr.rot(s, k))
        r[L - k:L - k + 1] = other(r[L - k])               # the symbol s[0], on the other side of it
        seqs.append(bytes(r))
    return seqs


def test_edge_lengths(api):
    rng = np.random.default_rng(1)
    seqs = []
    for L in (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33):
        seqs += edge_set(rng, L)
    seqs += [b'', b'']
    order = rng.permutation(len(seqs))
    erep, _, eoffset, st = check_seqs(api, [seqs[int(k)] for k in order])
    assert st['removed'] > 60 and max(eoffset) == 32


@pytest.mark.parametrize('L', [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_chunk_boundary(api, L):
    rng = np.random.default_rng(L)
    s = rand(rng, L)
    seqs = [s]
    for k in (1, CHUNK - 1, CHUNK, L - 1):
        if 0 < k < L:
            r = dcr.rot(s, k)
            seqs += [r, dr.revcomp(r)]
    near = bytearray(dcr.rot(s, 1))                         # one symbol off, at the wrap point (s[L - 1])
    near[L - 2:L - 1] = other(near[L - 2])
    seqs.append(bytes(near))
    erep, _, _, st = check_seqs(api, seqs)
    assert erep[:-1] == [0] * (len(seqs) - 1) and erep[-1] == len(seqs) - 1


def test_periodic_and_low_complexity(api):
    rng = np.random.default_rng(2)
    acgt = b'ACGT' * 50
    unit = rand(rng, 16)
    # the first 16 symbols recur 300 times; the symbols between the occurrences differ, so only the rotation to the last
    # occurrence is the record itself
    rec = b''.join(unit + rand(rng, 5) for _ in range(300))
    last = 299 * 21
    late = bytearray(dcr.rot(rec, last))
    late[-3:-2] = other(late[-3])
    seqs = [b'A' * 40, b'T' * 40, b'A' * 40, acgt] + [dcr.rot(acgt, k) for k in range(4)] + [dr.revcomp(acgt),
            rec, dcr.rot(rec, last), dr.revcomp(dcr.rot(rec, last)), bytes(late), (unit * 400)[:len(rec)], b'AC' * 4, b'CA' * 4]
    erep, estrand, eoffset, st = check_seqs(api, seqs)
    assert erep == [0, 0, 0, 3, 3, 3, 3, 3, 3, 9, 9, 9, 12, 13, 14, 14]
    assert (estrand[1], eoffset[1]) == (1, 0) and eoffset[4:8] == [0, 1, 2, 3] and eoffset[10] == last and eoffset[15] == 1
    assert st['collisions'] == 0


def test_candidate_list_grows_and_takes_many_batches(api):
    """The first 16 symbols recur 1 200 times in a set of 3 records: more candidates than the list's first 4 * 3 + 1 024
    slots, so the candidate pass runs again on a grown list.  Only the rotation to the last occurrence is the record itself:
    the equal candidate has rank 1 199, the 11th batch."""
    rng = np.random.default_rng(5)
    unit = rand(rng, 16)
    rec = b''.join(unit + rand(rng, 5) for _ in range(1200))
    last = 1199 * 21
    assert len(rec) == 25200 and rec.count(unit) >= 1200 > 4 * 3 + 1024
    erep, estrand, eoffset, _ = check_seqs(api, [rec, dcr.rot(rec, last), dr.revcomp(dcr.rot(rec, last))])
    assert (erep, estrand, eoffset) == ([0, 0, 0], [0, 0, 1], [0, 25179, 21])


def test_iupac(api):
    rng = np.random.default_rng(3)
    seqs = []
    for L in (5, 16, 23, 64, 333, 4097):
        s = rand(rng, L, 16)
        k = int(rng.integers(1, L))
        seqs += [s, dcr.rot(s, k), dr.revcomp(dcr.rot(s, k)).lower(), dr.revcomp(s), rand(rng, L, 16)]
    seqs += [b'-' * 20, b'N' * 20, b'-' * 20, b'n' * 20, b'RY' * 10, b'YR' * 10]
    erep, _, _, st = check_seqs(api, seqs)
    assert st['unique'] == 2 * 6 + 3


@pytest.mark.parametrize('bits', [0, 8])
def test_forced_collisions(api, bits):
    rng = np.random.default_rng(10 + bits)
    originals = [rand(rng, L) for L in (9, 40, 700) for _ in range(25)]
    seqs = list(originals)
    while len(seqs) < 200:
        s = originals[int(rng.integers(0, len(originals)))]
        k = int(rng.integers(0, len(s)))
        seqs.append([s, dr.revcomp(s), dcr.rot(s, k), dcr.rot(dr.revcomp(s), k)][int(rng.integers(0, 4))])
    seqs = [seqs[int(k)] for k in rng.permutation(len(seqs))]
    try:
        api.dedup_set_hash_bits(bits)
        _, _, _, st = check_seqs(api, seqs)
        assert st['collisions'] > 0 and st['rounds'] > 1, st
    finally:
        api.dedup_set_hash_bits(128)
    _, _, _, st = check_seqs(api, seqs)
    assert st['collisions'] == 0 and st['rounds'] == 1


def test_one_long_record(api):
    rng = np.random.default_rng(4)
    s = rand(rng, 3_000_000)
    r = dcr.rot(s, 1_000_003)
    rep, strand, offset, st = api.deduplicate([s, r, dr.revcomp(r)], circular=True)
    assert rep.tolist() == [0, 0, 0] and strand.tolist() == [0, 0, 1]
    erep, estrand, eoffset = dcr.run_seqs([s, r, dr.revcomp(r)])
    assert (erep, estrand) == ([0, 0, 0], [0, 0, 1]) and offset.tolist() == eoffset and eoffset[1] == 1_000_003
    assert st['collisions'] == 0 and st['rounds'] == 1


@pytest.mark.parametrize('seed', range(4))
def test_random_sets(api, seed):
    rng = np.random.default_rng(100 + seed)
    n_orig, n = 60, 400
    originals = [rand(rng, int(rng.integers(20, 5001)), 16 if seed % 2 else 4) for _ in range(n_orig)]
    where = sorted(rng.choice(n, n_orig, replace=False).tolist())
    where[0] = 0
    seqs, source, placed = [], [], []
    for i in range(n):
        if i in where:
            seqs.append(originals[len(placed)])
            placed.append(i)
            source.append(i)
            continue
        j = int(rng.integers(0, len(placed)))
        s = originals[j]
        kind, k = int(rng.integers(0, 4)), int(rng.integers(1, len(s)))
        seqs.append([s, dr.revcomp(s), dcr.rot(s, k), dcr.rot(dr.revcomp(s), k)][kind])
        source.append(placed[j])
    erep, _, _, st = check_seqs(api, seqs)
    assert erep == source and st['unique'] == n_orig


@pytest.fixture(scope='module')
def cli_input(tmp_path_factory):
    d = tmp_path_factory.mktemp('circ')
    rng = np.random.default_rng(6)
    g1, g2, g3 = rand(rng, 5000), rand(rng, 777), rand(rng, 30)

    def wrap(s, w=60):
        return b'\n'.join(s[k:k + w] for k in range(0, len(s), w)) + b'\n'
    a = d / 'first.fna'
    a.write_bytes(b'>g1 phage one\n' + wrap(g1) + b'>g2\n' + wrap(g2, 70) + b'>g3 short\n' + g3 + b'\n>e1\n')
    b = d / 'second.fna.gz'
    b.write_bytes(gzip.compress(b'>g1_rot opened elsewhere\n' + wrap(dcr.rot(g1, 1234)) + b'>g2_rc_rot\r\n' + wrap(dr.revcomp(dcr.rot(g2, 500)).lower(), 50)
                                + b'>g3_copy\n' + g3 + b'\n>g3_rc\n' + dr.revcomp(g3) + b'\n>e2\n\n>new\n' + wrap(rand(rng, 777))))
    return [a, b]


@pytest.mark.parametrize('gz', [False, True])
def test_cli_end_to_end(api, cli_input, tmp_path, gz):
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '--circular', '-v', '1',
            *(['--gzip-output', '--gzip-level', '5'] if gz else []))
    assert p.returncode == 0, p.stderr
    assert ' --circular [1 GPU]' in p.stderr
    fasta, dup, (rep, strand, offset) = dcr.run(cli_input, ['A|', 'B|'])
    written = tmp_path / ('nr.fna.gz' if gz else 'nr.fna')
    assert (gzip.decompress(written.read_bytes()) if gz else written.read_bytes()) == fasta
    assert pathlib.Path(f'{written}.duplicates.txt').read_bytes() == dup
    assert dup.splitlines()[:3] == [b'representative\tduplicate\tstrand\toffset', b'A|g1\tB|g1_rot\t+\t1234',
                                    b'A|g2\tB|g2_rc_rot\t-\t%d' % offset[5]]
    assert b'A|g3\tB|g3_rc\t-\t0' in dup and b'A|e1\tB|e2\t+\t0' in dup and len(dup.splitlines()) == 6


def test_without_the_flag_rotations_stay(api, cli_input, tmp_path):
    """Without --circular the output is dedup_restatement.run's, byte for byte, and the rotated copies stay in it; with the
    flag they disappear."""
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '-v', '0')
    assert p.returncode == 0, p.stderr
    fasta, dup, _ = dr.run(cli_input, ['A|', 'B|'])
    assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
    assert dup.startswith(b'representative\tduplicate\tstrand\n') and b'>B|g1_rot ' in fasta and b'>B|g2_rc_rot' in fasta
    circ = tmp_path / 'circ.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', circ, '--add-prefixes', 'A|', 'B|', '--circular', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    kept = circ.read_bytes()
    assert b'g1_rot' not in kept and b'g2_rc_rot' not in kept and b'>A|g1 phage one\n' in kept and b'>B|new\n' in kept
    # the array-level call without the flag is the plain one, and vg_dedup_seqs_ex without options fills the offsets with 0
    seqs = [b'ACGTT', b'GTTAC', b'AACGT']
    rep, strand, st = api.deduplicate(seqs)
    assert rep.tolist() == [0, 1, 0] and strand.tolist() == [0, 0, 1]
    import ctypes as C
    from vclust_amd import _lib
    offsets = np.array([0, 5, 10, 15], dtype=np.int64)
    rep = np.zeros(3, dtype=np.int32)
    strand = np.zeros(3, dtype=np.int8)
    off = np.full(3, -1, dtype=np.int64)
    P = C.POINTER
    for opt in (None, C.byref(_lib.DedupOptions(circular=0))):
        off[:] = -1
        _lib.check(_lib.load().vg_dedup_seqs_ex(b''.join(seqs), offsets.ctypes.data_as(P(C.c_int64)), 3, opt, rep.ctypes.data_as(P(C.c_int32)),
                                                strand.ctypes.data_as(P(C.c_int8)), off.ctypes.data_as(P(C.c_int64)), None))
        assert rep.tolist() == [0, 1, 0] and strand.tolist() == [0, 0, 1] and off.tolist() == [0, 0, 0]
