"""New genomes against a database on the GPU: GenomeSet.kmer_shared_new(n_db) must be the all-vs-all result restricted to the pairs
that contain a new genome (test_new2all_cpu.restrict_new) -- of the CPU oracle wherever the oracle is fast, and always of the
library's own all-vs-all kmer_shared on the same GenomeSet.  Pairs compare as a dict (a, b) -> shared; set sizes must be equal for
every new genome and every genome of a returned pair and -1 elsewhere.

Shapes are the smallest at which each index path exists: below 65 536 padded positions (the general radix path), one partition
level (up to 2^21), two levels with 12-byte level-1 records scattered tile by tile, and two levels with 12-byte records scattered
in whole 32 768-position tiles (from 4 x 8 192 x 2 048 positions).  8-byte short records need a larger set than the oracle takes in
a `Case` -- at k = 25 from 134 348 800 padded positions on, see test_geometry_cpu.py -- and have a file of their own,
test_gpu_large_geometry.py.  Families straddle the database / new boundary, so every case has a pair of a new and a database genome and, with two
or more new genomes, a pair of two new ones; both are asserted."""
import numpy as np
import pytest

import oracle_lib as orc
from test_new2all_cpu import restrict_new
from vclust_amd import api, synth

pytestmark = pytest.mark.gpu


def _pairs_dict(pairs):
    return {(int(p['a']), int(p['b'])): int(p['shared']) for p in pairs}


class Case:
    """A genome set with its all-vs-all references, each computed once: the library's own kmer_shared, and the oracle's if asked
    (oracle=True: the single-threaded shared_all; 'mt': shared_all_mt, for sets on which that one would take minutes)."""

    def __init__(self, codes, offsets, names=None, oracle=True):
        self.codes, self.offsets = codes, offsets
        self.gs = api.GenomeSet.from_codes(codes, offsets, names)
        self.n = len(self.gs)
        self.oracle = oracle
        self._ref = {}

    def references(self, k, fraction):
        if (k, fraction) not in self._ref:
            sizes, pairs = self.gs.kmer_shared(k=k, fraction=fraction)
            refs = [([int(x) for x in sizes], _pairs_dict(pairs))]
            assert len(refs[0][1]) == len(pairs)
            if self.oracle:
                run = orc.shared_all_mt if self.oracle == 'mt' else orc.shared_all
                osizes, opairs = run(self.codes, self.offsets, k=k, fraction=fraction)[:2]
                refs.append(([int(x) for x in osizes], opairs))
            self._ref[(k, fraction)] = refs
        return self._ref[(k, fraction)]

    def masked_applies(self, n_db, fraction, subshards):
        """the masked route: a dense single pass with both kinds of genomes, on a set the bucket pipeline takes"""
        return fraction == 1.0 and not subshards and 0 < n_db < self.n and 65536 <= _padded(self.offsets)[0] < (1 << 32)

    def check(self, n_db, k=25, fraction=1.0, min_shared=1, subshards=False):
        """under vg_set_new_path 1 (never the masked route) and 2 (wherever it applies); under 2 the profile says which ran"""
        wants = [restrict_new(sizes, {key: v for key, v in pairs.items() if v >= min_shared}, n_db)
                 for sizes, pairs in self.references(k, fraction)]
        for path in (1, 2):
            api.set_new_path(path)
            api.profile_enable(True)
            api.profile_reset()
            try:
                sizes, pairs = self.gs.kmer_shared_new(n_db, k=k, fraction=fraction, min_shared=min_shared)
                scopes = {e['name'] for e in api.profile_get()}
            finally:
                api.set_new_path(0)
                api.profile_enable(False)
            assert ('kmer_new_mask' in scopes) == (path == 2 and self.masked_applies(n_db, fraction, subshards)), (path, scopes)
            got = _pairs_dict(pairs)
            assert len(got) == len(pairs), 'a pair was returned twice'
            for want_sizes, want_pairs in wants:
                assert got == want_pairs, path
                assert [int(x) for x in sizes] == want_sizes, path
        # the comparison sets are not empty
        if 0 < n_db < self.n:
            assert any(b < n_db for _, b in got), 'no pair of a new and a database genome'
        if self.n - n_db >= 2:
            assert any(b >= n_db for _, b in got), 'no pair of two new genomes'
        if n_db == self.n:
            assert not got and all(int(x) == -1 for x in sizes)
        return got


def _padded(offsets):
    """padded positions of the set as the library lays it out: genomes start at multiples of a power of two of about a sixteenth
    of the mean length (64 .. 4 096), each followed by at least one padding position"""
    lens = np.diff(offsets)
    shift = 6
    while shift < 12 and (1 << (shift + 1)) <= int(lens.sum()) // len(lens) // 16:
        shift += 1
    return int(((lens >> shift) + 1).sum()) << shift, shift


def _member_major(codes, offsets, names, members):
    """family-major order (f0m0 f0m1 .. f1m0 ..) -> member-major (f0m0 f1m0 .. f0m1 f1m1 ..): wherever the set is cut into
    database and new genomes, families lie on both sides"""
    n = len(offsets) - 1
    order = [f * members + m for m in range(members) for f in range(n // members)]
    seqs = [codes[offsets[i]:offsets[i + 1]] for i in order]
    off = np.zeros(n + 1, dtype=np.int64); off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off, [names[i] for i in order]


# ---------------------------------------------------------------- 1. below 65 536 positions: the radix path
@pytest.fixture(scope='module')
def tiny():
    return Case(*_member_major(*synth.make_families(6, 3, length_range=(1500, 4000)), 3))


@pytest.mark.parametrize('where', ['0', '1', 'n/2', 'n-1', 'n'])
def test_radix_path(tiny, where):
    n = tiny.n
    assert n == 18 and _padded(tiny.offsets)[0] < 65536
    tiny.check({'0': 0, '1': 1, 'n/2': n // 2, 'n-1': n - 1, 'n': n}[where])


def test_all_database_is_empty_and_all_new_is_all_vs_all(tiny):
    sizes, pairs = tiny.gs.kmer_shared_new(tiny.n)
    assert len(pairs) == 0 and list(sizes) == [-1] * tiny.n
    sizes, pairs = tiny.gs.kmer_shared_new(0)
    full_sizes, full_pairs = tiny.references(25, 1.0)[0]
    assert [int(x) for x in sizes] == full_sizes and _pairs_dict(pairs) == full_pairs


def test_min_shared_and_writers_take_the_sizes(tiny, tmp_path):
    """min_shared is applied on the device as in kmer_shared; filter_pairs and write_fltr read only the sizes of genomes in pairs:
    the file is the all-vs-all file with the database rows emptied."""
    n_db = tiny.n // 2
    tiny.check(n_db, min_shared=20)
    full_sizes, full_pairs = tiny.gs.kmer_shared(k=25, min_shared=20)
    sizes, pairs = tiny.gs.kmer_shared_new(n_db, min_shared=20)
    assert (sizes[:n_db] == -1).any()
    kept, kept_full = tiny.gs.filter_pairs(sizes, pairs), tiny.gs.filter_pairs(full_sizes, full_pairs)
    assert _pairs_dict(kept) == {key: v for key, v in _pairs_dict(kept_full).items() if key[0] >= n_db} and len(kept)
    tiny.gs.write_fltr(tmp_path / 'new.txt', sizes, pairs)
    tiny.gs.write_fltr(tmp_path / 'all.txt', full_sizes, full_pairs)
    want = (tmp_path / 'all.txt').read_text().splitlines()
    want = want[:1] + [row.split(',')[0] + ',' for row in want[1:1 + n_db]] + want[1 + n_db:]
    assert (tmp_path / 'new.txt').read_text().splitlines() == want
    back = tiny.gs.read_filter(tmp_path / 'new.txt')
    assert {(int(p['a']), int(p['b'])) for p in back} == set(_pairs_dict(kept))


# ---------------------------------------------------------------- 2. one partition level
def test_one_partition_level():
    case = Case(*synth.make_families(10, 4, length=5000, seed=5))
    assert case.n == 40 and 65536 <= _padded(case.offsets)[0] < (1 << 21)
    case.check(case.n - 3)


# ---------------------------------------------------------------- 3. two levels, 12-byte records
@pytest.fixture(scope='module')
def two_levels():
    case = Case(*synth.make_families(24, 5, length=20000, seed=6))
    assert case.n == 120 and case.offsets[-1] > (1 << 21)
    return case


@pytest.mark.parametrize('k', [25, 30])
def test_two_partition_levels(two_levels, k):
    two_levels.check(two_levels.n - 4, k=k)


def test_more_new_genomes_than_database(two_levels):
    """a new set larger than the database saturates the bit field of the masked route: the result must still be exact"""
    two_levels.check(4)


def test_min_shared_on_the_masked_route(two_levels):
    """the sizes of the second pass are those of the database genomes in pairs that reach min_shared"""
    two_levels.check(two_levels.n - 4, min_shared=20)
    two_levels.check(two_levels.n // 2 - 2, min_shared=500)            # (inside a family of five)


# ---------------------------------------------------------------- 4. whole 32 768-position tiles, 12-byte records
def test_tiles_of_32768_positions():
    """1 700 genomes of 40 kb from the bench generator, the last 17 new: 69 632 000 padded positions, super-tiles of four tiles
    scattered as one 32 768-position tile.  At k = 25 the set partitions on 17 bits, 2k - 17 = 33 key bits do not fit one word,
    and the level-1 records stay 12 bytes (short records: test_gpu_large_geometry.py).  Against the library's own all-vs-all
    pass and the multithreaded oracle (7 654 pairs; 2.0 s on an 8-thread machine without a GPU, 0.1 s on the 16 threads of
    the MI355X host for the same genomes in member-major order: test_gpu_large_geometry.py runs those at more key lengths
    and as RANGE shards)."""
    codes, offsets, names = synth.make_families(170, 10, length=40000, seed=3)
    case = Case(codes, offsets, names, oracle='mt')
    assert case.n == 1700 and case.offsets[-1] > 4 * 8192 * 2048
    g = case.gs.kmer_geometry(k=25)
    assert g['P'] == _padded(case.offsets)[0] == 69632000
    assert (g['accepted'], g['levels'], g['tile32k'], g['st_tiles'], g['short_rec'], g['narrow']) == (1, 2, 1, 4, 0, 0)
    case.check(case.n - 17)


def test_row_lists_of_many_genomes():
    """From 65 536 genomes on the SpGEMM takes lists of small and large rows: they must be made of the new rows alone.  33 000
    random genomes of 120 bases, a mutated copy of each, and copies of the last 500 copies; the last 700 genomes are new."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 4, size=(33000, 120), dtype=np.uint8)
    b = a.copy(); b[:, 30] = (b[:, 30] + 1) % 4; b[:, 90] = (b[:, 90] + 2) % 4
    c = b[-500:].copy(); c[:, 60] = (c[:, 60] + 1) % 4
    codes = np.concatenate([a, b, c]).reshape(-1)
    case = Case(codes, np.arange(0, len(codes) + 1, 120, dtype=np.int64), oracle=False)
    assert case.n == 66500 >= 65536
    got = case.check(case.n - 700)
    assert len(got) >= 700
    # Half the set new: all 33 000 database genomes occur in a pair, more than 4 096 and more than a quarter of the database, so
    # the masked route gives the call up after its first pass (its scope has run) and the unmasked route answers.
    got = case.check(33000)
    assert len({b for _, b in got if b < 33000}) == 33000


def test_automatic_route(two_levels):
    """vg_set_new_path(0): the masked route up to 1 % of new padded bases (the measured threshold), the
    unmasked route above it; same result."""
    def scopes_of(n_db):
        api.set_new_path(0)
        api.profile_enable(True)
        api.profile_reset()
        try:
            sizes, pairs = two_levels.gs.kmer_shared_new(n_db)
            return {e['name'] for e in api.profile_get()}, [int(x) for x in sizes], _pairs_dict(pairs)
        finally:
            api.profile_enable(False)
    for n_db, masked in ((two_levels.n - 1, True), (two_levels.n - 4, False)):      # one genome of 120 is 0.8 %, four are 3.3 %
        scopes, sizes, pairs = scopes_of(n_db)
        assert ('kmer_new_mask' in scopes) == masked
        assert (sizes, pairs) == restrict_new(*two_levels.references(25, 1.0)[0], n_db)


# ---------------------------------------------------------------- 5. what must not be lost
N_DB_EDGES = 652


def _edges_input():
    """Database (652 genomes): 600 short genomes around one conserved 60-mer (k-mer runs of several hundred genomes: the 1 024-thread
    bucket variant and k_bucket_big), a few close relatives among them, 50 without the block, one shorter than k, one that
    repeats a segment of its own.  New (12 genomes): one with the conserved block, a copy of a database genome, an all-N genome,
    one that repeats the same segment as the database genome does, relatives of database genomes and of each other.  N runs are
    sprinkled over everything."""
    rng = np.random.default_rng(8)
    core = rng.integers(0, 4, size=60, dtype=np.uint8)
    rep_unit = rng.integers(0, 4, size=90, dtype=np.uint8)

    def rand(lo, hi):
        return rng.integers(0, 4, size=int(rng.integers(lo, hi)), dtype=np.uint8)

    def with_core(flank):
        cut = int(rng.integers(0, len(flank)))
        return np.concatenate([flank[:cut], core, flank[cut:]])

    def mutate(seq, step):
        out = seq.copy(); out[::step] = (out[::step] + 1) % 4
        return out

    db = [with_core(rand(150, 400)) for _ in range(600)]
    for i in range(0, 40, 2):
        db[i + 1] = mutate(db[i], 37)
    db += [rand(300, 900) for _ in range(50)]
    db.append(rand(10, 11))                                                         # shorter than k
    db.append(np.concatenate([rand(200, 300), rep_unit, rand(50, 80), rep_unit, rand(100, 200)]))
    assert len(db) == N_DB_EDGES
    new = [with_core(rand(150, 400)),                                               # the one new genome with the conserved block
           db[605].copy(),                                                          # identical to a database genome
           np.full(200, 4, dtype=np.uint8),                                         # all N
           np.concatenate([rand(100, 200), rep_unit, rep_unit[:50], rep_unit, rand(100, 200)]),
           mutate(db[610], 41), mutate(db[611], 53)]
    new += [mutate(new[4], 47), mutate(new[5], 61), rand(400, 700)]
    new += [mutate(new[-1], 43), mutate(db[3], 59), mutate(new[0][:200], 200)]
    seqs = db + new
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(s) for s in seqs])
    codes = np.concatenate(seqs)
    keep = codes.copy()
    from test_gpu_parity_random import _sprinkle_n
    codes = _sprinkle_n(codes, rng, 60)
    a, b = offsets[N_DB_EDGES], offsets[N_DB_EDGES + 1]
    codes[a:b] = keep[a:b]                                                          # (the new genome with the block keeps it whole)
    a, b = offsets[N_DB_EDGES + 1], offsets[N_DB_EDGES + 2]
    codes[a:b] = codes[offsets[605]:offsets[606]]                                   # (the copy is a copy, N runs included)
    return codes, offsets


@pytest.fixture(scope='module')
def edges():
    return Case(*_edges_input())


def test_nothing_is_lost(edges):
    got = edges.check(N_DB_EDGES)
    n_db = N_DB_EDGES
    with_block = [b for (a, b), s in got.items() if a == n_db]
    assert len(with_block) >= 500, 'the conserved 25-mers of one new genome reach several hundred database genomes'
    assert got[(n_db + 1, 605)] == edges.references(25, 1.0)[0][0][605] > 0            # the copy shares every k-mer of its original
    assert not any(n_db + 2 in key for key in got)                                    # the all-N genome
    assert not any(650 in key for key in got)                                         # the database genome shorter than k
    assert (n_db + 3, 651) in got                                                     # the segment repeated inside both
    sizes, _ = edges.gs.kmer_shared_new(n_db)
    assert sizes[n_db + 2] == 0 and sizes[650] == -1 and sizes[651] > 0


def test_boundary_at_tile_edges(edges):
    """The database / new boundary at the last genome of a 32 768-position tile, at the first of the next, and one further."""
    total, shift = _padded(edges.offsets)
    assert shift == 6 and total > 3 * 32768
    starts = np.concatenate([[0], np.cumsum((np.diff(edges.offsets) // 64 + 1) * 64)])
    for tile in (1, 3):
        first = int(np.searchsorted(starts, tile * 32768))                             # the first genome that starts in the tile
        for n_db in (first - 1, first, first + 1):
            edges.check(n_db)


# ---------------------------------------------------------------- 6. options
def test_fraction(two_levels):
    two_levels.check(two_levels.n - 4, k=17, fraction=0.3)


def test_subshards(two_levels, tiny):
    from vclust_amd import _lib
    lib = _lib.load()
    lib.vg_set_subshards(3)
    try:
        two_levels.check(two_levels.n - 4, subshards=True)
        two_levels.check(two_levels.n - 4, min_shared=20, subshards=True)
        two_levels.check(two_levels.n - 4, k=17, fraction=0.3, subshards=True)
        tiny.check(tiny.n // 2, subshards=True)
        tiny.check(tiny.n, subshards=True)
    finally:
        lib.vg_set_subshards(0)



# ---------------------------------------------------------------- downstream: the align stage of the result
def test_align_rows_of_the_new_pairs(two_levels):
    """The candidates of kmer_shared_new go through filter_pairs, align_tasks and lz_align like any others: every row equals the row
    of the same ordered pair in the align stage of the all-vs-all candidates, and only tasks that name a new genome are made."""
    gs, n_db = two_levels.gs, two_levels.n - 4

    def rows(sizes, pairs):
        cand = gs.filter_pairs(sizes, pairs)
        tasks = gs.align_tasks(cand)
        stats = gs.lz_align(tasks)
        return {(int(t['q']), int(t['r'])): tuple(int(x) for x in s) for t, s in zip(tasks, stats)}
    full = rows(*gs.kmer_shared(k=25, min_shared=20))
    new = rows(*gs.kmer_shared_new(n_db, k=25, min_shared=20))
    assert new == {key: row for key, row in full.items() if max(key) >= n_db}
    assert 0 < len(new) < len(full)
