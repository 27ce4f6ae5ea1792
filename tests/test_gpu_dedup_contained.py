"""Contained mode of the deduplicate stage on the GPU against the sequential restatement
(tests/dedup_contained_restatement.py): representative, strand and offset of every record, on edge lengths and offsets,
chunk boundaries, near misses, chains and ties, low complexity, the full alphabet, flooded candidates, several index
passes, random sets, one long container and the CLI."""
import gzip
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import dedup_contained_restatement as dcn
import dedup_restatement as dr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
SYMBOLS = np.frombuffer(b'ACGTRYSWKMBDHVN-', dtype=np.uint8)
CHUNK = 8 * 2048         # symbols per (candidate, chunk) task: 2 048 words


def run(*args, timeout=600):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


@pytest.fixture
def knobs(api):
    """The two test knobs, restored whatever the test does."""
    yield api
    api.dedup_set_anchor_symbols(16)
    api.dedup_set_index_positions(0)


def rand(rng, L, k=4):
    return SYMBOLS[:k][rng.integers(0, k, L)].tobytes()


def other(ch: int) -> bytes:
    return b'A' if ch != ord('A') else b'C'


def changed(s: bytes, at: int) -> bytes:
    at %= len(s)
    return s[:at] + other(s[at]) + s[at + 1:]


def check_seqs(api, seqs, expected=None):
    rep, strand, offset, st = api.deduplicate(seqs, contained=True)
    erep, estrand, eoffset = expected or dcn.run_seqs(seqs)
    assert rep.tolist() == erep
    assert strand.tolist() == estrand
    assert offset.tolist() == eoffset and offset.dtype == np.int64
    assert st['records'] == len(seqs) and st['unique'] == sum(r == i for i, r in enumerate(erep))
    assert st['removed'] == len(seqs) - st['unique']
    assert st['reverse'] == sum(s for i, s in enumerate(estrand) if erep[i] != i)
    assert st['verified'] <= st['candidates'] <= st['hits'] and st['rounds'] == st['passes']
    return erep, estrand, eoffset, st


LENGTHS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)


def edge_set(rng, size=120):
    """One container and, for every fragment length, the fragments at offsets 0, 1, 7, 8, 9 and flush with its end, forward
    and reverse-complemented."""
    y = rand(rng, size)
    seqs = [y]
    for L in LENGTHS:
        for s in (0, 1, 7, 8, 9, size - L):
            seqs += [y[s:s + L], dr.revcomp(y[s:s + L])]
    return seqs


def test_edge_lengths_and_offsets(api):
    rng = np.random.default_rng(1)
    seqs = edge_set(rng) + edge_set(rng, 97) + [b'', b'']
    seqs = [seqs[int(k)] for k in rng.permutation(len(seqs))]
    erep, estrand, eoffset, st = check_seqs(api, seqs)
    assert st['removed'] >= 2 * 2 * 6 * len(LENGTHS) and sum(estrand) > 50 and {1, 7, 8, 9} <= set(eoffset)


@pytest.mark.parametrize('L', [CHUNK - 1, CHUNK, CHUNK + 1])
def test_chunk_boundary(api, L):
    rng = np.random.default_rng(L)
    y = rand(rng, 3 * CHUNK + 5)
    s = CHUNK - 2051                                         # odd: the container is re-framed, the fragment straddles a chunk
    x = y[s:s + L]
    seqs = [x, dr.revcomp(x), y, changed(x, L - 1), changed(x, CHUNK - 8), dr.revcomp(changed(x, 0)), y[-L:], dr.revcomp(y[:L])]
    erep, estrand, eoffset, st = check_seqs(api, seqs)
    assert erep == [2, 2, 2, 3, 4, 5, 2, 2] and estrand == [0, 1, 0, 0, 0, 0, 0, 1]
    assert eoffset[:2] == [s, len(y) - L - s] and eoffset[6:] == [len(y) - L, len(y) - L]


def test_near_misses_stay(api):
    rng = np.random.default_rng(2)
    y = rand(rng, 400)
    seqs = [y]
    for L in (9, 16, 17, 33, 64, 100):
        for s in (0, 3, 8, 13):
            x = y[s:s + L]
            for at in sorted({0, L - 1, 8, 16} & set(range(L))):    # first, last, behind a word boundary, behind the anchor
                seqs += [changed(x, at), dr.revcomp(changed(x, at))]
    erep, _, _, st = check_seqs(api, seqs)
    # none of them lies in y (a reverse complement joins its forward twin, a shorter one a longer one with the same change)
    assert len(seqs) > 150 and erep[0] == 0 and 0 not in erep[1:]
    assert st['candidates'] > st['verified']


def test_chain_and_ties(api):
    rng = np.random.default_rng(3)
    c = rand(rng, 900)
    b = c[100:700]
    a = b[50:300]
    x = rand(rng, 40)
    c1, c2 = rand(rng, 30) + x + rand(rng, 30), rand(rng, 25) + x + rand(rng, 35)
    longer = rand(rng, 50) + dr.revcomp(x) + rand(rng, 60)
    pal = b'ACGTTGCATGCAACGT'
    assert dr.revcomp(pal) == pal
    seqs = [a, dr.revcomp(b), c, c1, x, c2, a, b'TT' + pal + b'GG', pal, b, dr.revcomp(a)]
    erep, estrand, eoffset, _ = check_seqs(api, seqs)
    assert erep == [2, 2, 2, 3, 3, 5, 2, 7, 7, 2, 2] and estrand == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert eoffset[0] == 150 and eoffset[4] == 30 and eoffset[8] == 2
    # a longer container beats the earlier shorter ones, also on the other strand
    erep, estrand, eoffset, _ = check_seqs(api, seqs + [longer])
    assert (erep[4], estrand[4], eoffset[4]) == (len(seqs), 1, 60)


def test_low_complexity_reports_the_smallest_offset(api):
    seqs = [b'A' * L for L in range(5, 41)] + [b'A' * 3000, b'T' * 17, b'AC' * 300, b'CA' * 20, b'ACA', b'GT' * 7, b'TGT', b'AC' * 300]
    erep, estrand, eoffset, st = check_seqs(api, seqs)
    big, per = 36, 38
    assert erep[:36] == [big] * 36 and set(eoffset[:37]) == {0} and (erep[37], estrand[37]) == (big, 1)
    assert [(erep[k], estrand[k], eoffset[k]) for k in range(39, 44)] == [(per, 0, 1), (per, 0, 0), (per, 1, 0), (per, 1, 1), (per, 0, 0)]
    assert st['candidates'] > 36 * 2900


def test_iupac_and_gap_symbols(api):
    rng = np.random.default_rng(4)
    seqs = []
    for L in (40, 333, 4097):
        y = rand(rng, L, 16)
        for n in (1, 5, 16, 23):
            s = int(rng.integers(0, L - n + 1))
            seqs += [y[s:s + n], dr.revcomp(y[s:s + n]).lower()]
        seqs.append(y)
    seqs += [b'AC-GT--A', b'C-G', b'T--A', b'T--', b'ACNNGT', b'NN', b'CRNG', b'-' * 20, b'-' * 7, b'N' * 7, b'n' * 9, b'RY' * 10, b'YRY']
    check_seqs(api, seqs)


def random_set(rng, n=300, k=4):
    """About 30 % fragments of random earlier or later parents on random strands, some of them fragments of fragments and
    some changed in one symbol."""
    parents = [rand(rng, int(rng.integers(30, 1500)), k) for _ in range(int(n * 0.7))]
    seqs = list(parents)
    while len(seqs) < n:
        p = seqs[int(rng.integers(0, len(seqs)))]            # (a parent or an earlier fragment)
        L = int(rng.integers(1, len(p) + 1))
        s = int(rng.integers(0, len(p) - L + 1))
        x = p[s:s + L]
        if rng.random() < 0.5:
            x = dr.revcomp(x)
        if rng.random() < 0.2:
            x = changed(x, int(rng.integers(0, L)))
        seqs.append(x)
    return [seqs[int(i)] for i in rng.permutation(len(seqs))]


@pytest.fixture(scope='module')
def flood_set():
    seqs = random_set(np.random.default_rng(50), 200)
    return seqs, dcn.run_seqs(seqs)


@pytest.mark.parametrize('anchor', [1, 4])
def test_short_anchors_flood_the_compare(knobs, flood_set, anchor):
    seqs, expected = flood_set
    _, _, _, st16 = check_seqs(knobs, seqs, expected)
    knobs.dedup_set_anchor_symbols(anchor)
    _, _, _, st = check_seqs(knobs, seqs, expected)
    # (records below 16 symbols have short anchors anyway; every longer record now has one too)
    assert st['hits'] > st16['hits'] and st['candidates'] > st16['candidates'] and st['verified'] == st16['verified']
    assert anchor != 1 or st['slices'] > st['passes']        # more hits than one candidate launch takes


def test_several_index_passes(knobs):
    rng = np.random.default_rng(51)
    seqs = random_set(rng, 40)
    total = sum(len(s) for s in seqs)
    assert 15000 < total < 30000
    expected = dcn.run_seqs(seqs)
    _, _, _, st1 = check_seqs(knobs, seqs, expected)
    assert st1['passes'] == 1 and st1['positions'] == total
    knobs.dedup_set_index_positions(1000)
    _, _, _, st = check_seqs(knobs, seqs, expected)
    assert st['passes'] == (total + 999) // 1000 and st['positions'] == total and st['verified'] == st1['verified']


@pytest.mark.parametrize('seed', range(4))
def test_random_sets(api, seed):
    rng = np.random.default_rng(100 + seed)
    seqs = random_set(rng, 300, 16 if seed % 2 else 4)
    erep, _, _, st = check_seqs(api, seqs)
    assert 40 < st['removed'] < 100


def test_one_long_container(api):
    rng = np.random.default_rng(5)
    y = rand(rng, 2_000_000)
    seqs, where = [], []
    for k in range(50):
        L = int(rng.integers(200, 60_000))
        s = int(rng.integers(0, len(y) - L + 1)) if k else len(y) - L
        seqs.append(y[s:s + L] if k % 2 else dr.revcomp(y[s:s + L]))
        where.append((k % 2 == 0, s if k % 2 else len(y) - L - s))
    seqs.insert(25, y)
    rep, strand, offset, st = api.deduplicate(seqs, contained=True)
    assert rep.tolist() == [25] * 51 and st['unique'] == 1 and st['passes'] == 1
    got = [(bool(strand[i]), int(offset[i])) for i in range(51) if i != 25]
    assert got == where


@pytest.fixture(scope='module')
def cli_input(tmp_path_factory):
    d = tmp_path_factory.mktemp('contained')
    rng = np.random.default_rng(6)
    g1, g2, g3 = rand(rng, 5000), rand(rng, 777), rand(rng, 30)

    def wrap(s, w=60):
        return b'\n'.join(s[k:k + w] for k in range(0, len(s), w)) + b'\n'
    a = d / 'first.fna'
    a.write_bytes(b'>g1_frag early fragment\n' + wrap(g1[1003:3000]) + b'>g2\n' + wrap(g2, 70) + b'>g3 short\n' + g3 + b'\n>e1\n')
    b = d / 'second.fna.gz'
    b.write_bytes(gzip.compress(b'>g1 phage one\n' + wrap(g1) + b'>g2_rc_frag\r\n' + wrap(dr.revcomp(g2[100:611]).lower(), 50)
                                + b'>g3_copy\n' + g3 + b'\n>g3_rc\n' + dr.revcomp(g3) + b'\n>e2\n\n>new\n' + wrap(rand(rng, 777))
                                + b'>g1_frag_frag\n' + wrap(dr.revcomp(g1[1500:1600]))))
    return [a, b]


@pytest.mark.parametrize('gz', [False, True])
def test_cli_end_to_end(api, cli_input, tmp_path, gz):
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '--contained', '-v', '1',
            *(['--gzip-output', '--gzip-level', '5'] if gz else []))
    assert p.returncode == 0, p.stderr
    assert ' --contained [1 GPU]' in p.stderr
    fasta, dup, _ = dcn.run(cli_input, ['A|', 'B|'])
    written = tmp_path / ('nr.fna.gz' if gz else 'nr.fna')
    assert (gzip.decompress(written.read_bytes()) if gz else written.read_bytes()) == fasta
    assert pathlib.Path(f'{written}.duplicates.txt').read_bytes() == dup
    assert dup.splitlines() == [b'representative\tduplicate\tstrand\toffset', b'B|g1\tA|g1_frag\t+\t1003', b'A|g2\tB|g2_rc_frag\t-\t166',
                                b'A|g3\tB|g3_copy\t+\t0', b'A|g3\tB|g3_rc\t-\t0', b'A|e1\tB|e2\t+\t0', b'B|g1\tB|g1_frag_frag\t-\t3400']


def test_without_the_flag_fragments_stay(api, cli_input, tmp_path):
    """Without --contained the output is dedup_restatement.run's, byte for byte, and every fragment stays in it; with the
    flag they disappear."""
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', out, '--add-prefixes', 'A|', 'B|', '-v', '0')
    assert p.returncode == 0, p.stderr
    fasta, dup, _ = dr.run(cli_input, ['A|', 'B|'])
    assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
    assert dup.startswith(b'representative\tduplicate\tstrand\n')
    assert b'>A|g1_frag ' in fasta and b'>B|g2_rc_frag' in fasta and b'>B|g1_frag_frag' in fasta
    cont = tmp_path / 'cont.fna'
    p = run('deduplicate', '-i', *cli_input, '-o', cont, '--add-prefixes', 'A|', 'B|', '--contained', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    kept = cont.read_bytes()
    assert b'g1_frag' not in kept and b'g2_rc_frag' not in kept and b'>B|g1 phage one\n' in kept and b'>B|new\n' in kept
    # the array-level call without the flag is the plain one
    seqs = [b'ACGTTGCA', b'CGTTG', b'CAAC']
    rep, strand, st = api.deduplicate(seqs)
    assert rep.tolist() == [0, 1, 2] and strand.tolist() == [0, 0, 0]
    rep, strand, offset, st = api.deduplicate(seqs, contained=True)
    assert rep.tolist() == [0, 0, 0] and strand.tolist() == [0, 0, 1] and offset.tolist() == [0, 1, 2]
