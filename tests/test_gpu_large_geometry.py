"""The index geometry of large sets -- 32 768-position tiles, 8-byte "short" level-1 records (key bits, position modulo 2^25),
level-2 units that span up to four 2^25-position groups -- held to the CPU oracle count for count: every set size and every shared
count of the all-vs-all pass, of RANGE shards and sub-shards, and of the masked `--db` route (k_new_mask rebuilds positions from the
group base of a super-tile plus 25 low bits).

One dense set at the smallest size with short records at k = 25 (S8: 3 300 genomes of 40 kb, P = 135 168 000, super-tiles of 8
tiles), and the same genomes with the one N of every genome widened to an N run: S12 (super-tiles of 12 tiles: 98 304 positions, no
power of two, so 12-byte records) and S16 (16 tiles, short records, the geometry of the benchmark).  The N run sits at the same base
offset in all three, so their k-mer sets are the same and ONE oracle run on S8 is the reference for all three.  A fourth set, the
first 2 457 genomes of S8 at k = 24, is the one shape whose level-2 unit spans exactly three groups.

Every set asserts its geometry through GenomeSet.kmer_geometry (the rules themselves are pinned in test_geometry_cpu.py), so a
changed threshold fails an assertion here instead of moving the tests onto another geometry."""
import time

import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_new2all import _member_major, _padded, _pairs_dict
from test_new2all_cpu import restrict_new
from vclust_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

FAMILIES, MEMBERS, N_AT = 330, 10, 20000          # member-major: the members of a family lie 330 genomes (13.5 M positions in S8) apart
N_RUN = {'S8': 1, 'S12': 24500, 'S16': 44000}     # length of the N run at base N_AT of every genome
GROUP = 1 << 25
MASKED = {'kmer_new_mask', 'kmer_new_sizes'}


def _widen(codes, offsets, run):
    """every genome with the N at base N_AT widened to `run` Ns (the bases before and behind it unchanged)"""
    if run == 1:
        return codes, offsets
    ns = np.full(run, 4, dtype=np.uint8)
    seqs = [np.concatenate([codes[a:a + N_AT], ns, codes[a + N_AT + 1:b]]) for a, b in zip(offsets[:-1], offsets[1:])]
    off = np.zeros(len(seqs) + 1, dtype=np.int64); off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off


class Big:
    """A set on the device, the start position of every genome as the library lays them out, and the geometry of its dense pass."""

    def __init__(self, codes, offsets, k):
        self.gs = api.GenomeSet.from_codes(codes, offsets)
        self.n, self.k = len(self.gs), k
        total, shift = _padded(offsets)
        self.starts = np.concatenate([[0], np.cumsum(((np.diff(offsets) >> shift) + 1) << shift)])
        self.geo = self.gs.kmer_geometry(k=k)
        assert self.geo['accepted'] == 1 and self.geo['n_passes'] == 1
        assert total == int(self.starts[-1]) == self.geo['P'], 'the layout formula of the tests and the library disagree'
        self.st_pos = self.geo['st_tiles'] * 8192

    def first_at(self, pos):
        """the first genome that starts at or after position pos"""
        return int(np.searchsorted(self.starts[:-1], pos))


def _profiled(call):
    api.profile_enable(True)
    api.profile_reset()
    try:
        sizes, pairs = call()
        scopes = {e['name'] for e in api.profile_get()}
    finally:
        api.profile_enable(False)
    got = _pairs_dict(pairs)
    assert len(got) == len(pairs), 'a pair was returned twice'
    return [int(x) for x in sizes], got, scopes


def _oracle(codes, offsets, k):
    t0 = time.perf_counter()
    sizes, pairs, _, threads = orc.shared_all_mt(codes, offsets, k=k)
    print(f'oracle shared_all_mt: {len(offsets) - 1} genomes, {int(offsets[-1])} bases, k = {k}: {time.perf_counter() - t0:.1f} s on {threads} threads, {len(pairs)} pairs')
    return [int(x) for x in sizes], pairs


# ---------------------------------------------------------------- the sets and their references, each built once
@pytest.fixture(scope='module')
def base():
    """S8 on the host: 330 families of ten 40 kb genomes from the bench generator, member-major, base N_AT of every genome an N."""
    codes, offsets, names = _member_major(*synth.make_families(FAMILIES, MEMBERS, length=40000, seed=3), MEMBERS)
    codes = codes.copy()
    codes[offsets[:-1] + N_AT] = 4
    return codes, offsets


@pytest.fixture(scope='module')
def ref25(base):
    """The one k = 25 reference: the oracle's all-vs-all result on S8, 132.0 Mbp -- the dense set itself, every base valid but one
    per genome; no N runs thin it.  Measured with the thread count the environment gives: 0.4 s on the 16 threads of the MI355X
    host, 4.4 s on an 8-thread machine without a GPU."""
    return _oracle(*base, 25)


def _big(base, name):
    big = Big(*_widen(*base, N_RUN[name]), 25)
    assert big.n == FAMILIES * MEMBERS
    return big


@pytest.fixture(scope='module')
def s8(base):
    big = _big(base, 'S8')
    g = big.geo
    assert g['P'] == 135168000 and (g['short_rec'], g['tile32k'], g['st_tiles'], g['total_bits'], g['n_st']) == (1, 1, 8, 18, 2063)
    assert (g['u_st'], g['g_st']) == (2048, 512)            # two units: four groups, then 15 super-tiles of the fifth group
    assert 4 * GROUP < g['P'] < 4 * GROUP + 1000000
    return big


@pytest.fixture(scope='module')
def s12(base):
    big = _big(base, 'S12')
    g = big.geo
    assert 201326592 <= g['P'] < 268435456 and (g['short_rec'], g['tile32k'], g['st_tiles'], g['narrow']) == (0, 1, 12, 1)
    return big


@pytest.fixture(scope='module')
def s16(base):
    big = _big(base, 'S16')
    g = big.geo
    assert g['P'] >= 268435456 and (g['short_rec'], g['tile32k'], g['st_tiles'], g['total_bits']) == (1, 1, 16, 19)
    assert g['u_st'] == 4 * g['g_st'] == 1024
    return big


def test_the_three_sets_have_the_same_kmers(base):
    """(CPU) the N run replaces one N: no k-mer appears or disappears"""
    codes, offsets = base
    for i in (0, 1234, FAMILIES * MEMBERS - 1):
        one = codes[offsets[i]:offsets[i + 1]]
        wide, _ = _widen(one, np.array([0, len(one)], dtype=np.int64), N_RUN['S16'])
        assert len(wide) == len(one) + N_RUN['S16'] - 1
        assert np.array_equal(orc.kmer_set(one, k=25), orc.kmer_set(wide, k=25))


# ---------------------------------------------------------------- 1. all-vs-all, exact
def _check_all_vs_all(big, ref):
    sizes, got, scopes = _profiled(lambda: big.gs.kmer_shared(k=big.k))
    assert sizes == ref[0]
    assert got == ref[1]
    assert {'kmer_partition', 'kmer_partition2', 'bucket_sort_runs', 'spgemm_rows'} <= scopes
    assert not any('radix' in s or s.startswith('index_') for s in scopes), scopes      # the bucket pipeline, not the general path


@pytest.mark.parametrize('name', ['s8', 's12', 's16'])
def test_all_vs_all(request, ref25, name):
    assert len(ref25[1]) > FAMILIES * MEMBERS * (MEMBERS - 1) // 2, 'no chance pair between unrelated genomes in the reference'
    _check_all_vs_all(request.getfixturevalue(name), ref25)


# ---------------------------------------------------------------- 2. RANGE shards and sub-shards on S8
def test_range_shards_add_up(s8, ref25):
    sizes, pairs = np.zeros(s8.n, dtype=np.int64), {}
    for shard in range(3):
        g = s8.gs.kmer_geometry(k=25, shard=shard, n_shards=3)
        assert g['accepted'] == 1 and g['short_rec'] == 1 and g['n_passes'] == 1
        part_sizes, part, scopes = _profiled(lambda: s8.gs.kmer_shared(k=25, shard=shard, n_shards=3))
        assert not any('radix' in s for s in scopes), scopes
        sizes += np.array(part_sizes)
        for key, v in part.items():
            pairs[key] = pairs.get(key, 0) + v
    assert [int(x) for x in sizes] == ref25[0]
    assert pairs == ref25[1]


def test_subshards(s8, ref25):
    """three RANGE sub-shards: 8-byte level-1 records whose payloads are row numbers"""
    lib = _lib.load()
    lib.vg_set_subshards(3)
    try:
        g = s8.gs.kmer_geometry(k=25)
        assert g['n_passes'] == 3 and g['accepted'] == 1 and g['short_rec'] == 1
        sizes, got, scopes = _profiled(lambda: s8.gs.kmer_shared(k=25))
    finally:
        lib.vg_set_subshards(0)
    assert sizes == ref25[0]
    assert got == ref25[1]


EXTRACTED = {'kmer_count', 'kmer_emit', 'kmer_emit_recompute', 'kmer_extract', 'kmer_multi_mask'}      # scopes of the compact and HASH sources


@pytest.mark.parametrize('n_shards', [2, 8])
def test_range_scatter_half_tiles_and_64k_tiles(s8, ref25, n_shards):
    """The two routes of the RANGE level-1 scatter that three shards do not take.  S8 is the smallest set that has them: 32 768-position
    tiles need super-tiles of four tiles (P >= 2^26), the 65 536-position tile super-tiles of eight (P >= 2^27, S8) and a shard of a
    sixth of the digits or less.

    Eight shards: every pass is the 65 536-position kernel (accepted with more than one shard means RANGE; with 32 768-position
    tiles, B1 = 11 and super-tiles of eight tiles a shard of an eighth of the digits takes two tiles at a time).  Two shards: the 32 768-position kernel, whose list holds 16 384 kept
    k-mers, so a tile that keeps more is taken as two halves.  A genome of S8 occupies 40 960 positions, so every fifth tile lies
    inside one genome and has 32 743 valid positions (one N costs 25); a shard keeps each with probability 1/2 -- 16 371 kept on
    average, standard deviation 90 -- and 0.44 of these 825 tiles exceed the list in either shard.  The set is seeded: the tiles that
    do are the same in every run."""
    sizes, pairs = np.zeros(s8.n, dtype=np.int64), {}
    for shard in range(n_shards):
        g = s8.gs.kmer_geometry(k=25, shard=shard, n_shards=n_shards)
        assert (g['accepted'], g['n_passes'], g['levels'], g['tile32k'], g['short_rec'], g['st_tiles'], g['B1']) == (1, 1, 2, 1, 1, 8, 11)
        part_sizes, part, scopes = _profiled(lambda: s8.gs.kmer_shared(k=25, shard=shard, n_shards=n_shards))
        assert {'kmer_partition', 'kmer_partition2', 'bucket_sort_runs'} <= scopes
        assert not (scopes & EXTRACTED) and not any('radix' in s for s in scopes), scopes      # dense source cut by digit range: RANGE
        sizes += np.array(part_sizes)
        for key, v in part.items():
            pairs[key] = pairs.get(key, 0) + v
    assert [int(x) for x in sizes] == ref25[0]
    assert pairs == ref25[1]


# ---------------------------------------------------------------- 3. new genomes against a database
def _check_new(big, ref, n_db, min_shared=1, paths=(1, 2)):
    """kmer_shared_new(n_db) under every route of `paths` against the restricted oracle result; the profile says which route ran
    (0 = automatic: expected to choose the masked route here)"""
    assert 0 < n_db < big.n
    want_sizes, want = restrict_new(ref[0], {key: v for key, v in ref[1].items() if v >= min_shared}, n_db)
    assert any(b < n_db for _, b in want), 'no pair of a new and a database genome'
    # (the new genomes of a case with at most FAMILIES of them are one member of as many families: related only by chance)
    if big.n - n_db > FAMILIES:
        assert any(b >= n_db for _, b in want), 'no pair of two new genomes'
    for path in paths:
        api.set_new_path(path)
        try:
            sizes, got, scopes = _profiled(lambda: big.gs.kmer_shared_new(n_db, k=big.k, min_shared=min_shared))
        finally:
            api.set_new_path(0)
        assert scopes & MASKED == (set() if path == 1 else MASKED), (path, scopes)
        assert got == want, path
        assert sizes == want_sizes, path


def _n_db_of(big, case):
    g = big.geo
    if case.startswith('first_group'):
        first = big.first_at(GROUP)
    elif case.startswith('last_group'):
        first = big.first_at(((g['P'] - 1) >> 25) << 25)
    elif case.startswith('super_tile'):
        st = (g['n_st'] // 2) | 1                                         # an odd super-tile: not the first of a group
        assert (st * big.st_pos) % GROUP != 0
        first = big.first_at(st * big.st_pos)
    else:
        raise KeyError(case)
    return first + {'-1': -1, '+0': 0, '+1': 1}[case[-2:]]


BOUNDARIES = [where + d for where in ('first_group', 'last_group', 'super_tile') for d in ('-1', '+0', '+1')]


@pytest.mark.parametrize('case', BOUNDARIES)
@pytest.mark.parametrize('name', ['s8', 's16'])
def test_new_at_boundaries(request, ref25, name, case):
    """The database / new boundary at the genome that starts at or behind a 2^25-position group boundary (the first one and the
    last one, where the new part is under 1 % and many workgroups share a bucket) or a super-tile boundary inside a group, at the
    genome before it and the one after it."""
    big = request.getfixturevalue(name)
    assert big.geo['short_rec'] == 1
    n_db = _n_db_of(big, case)
    if case == 'last_group+0':
        assert big.starts[n_db - 1] < ((big.geo['P'] - 1) >> 25) << 25 <= big.starts[n_db]
    if (name, case) == ('s8', 'last_group+0'):
        assert n_db == 3277 and big.geo['P'] - big.starts[n_db] < 0.01 * big.geo['P']
    _check_new(big, ref25, n_db)


@pytest.mark.parametrize('name', ['s8', 's16'])
def test_new_one_per_cent(request, ref25, name):
    """1 % new: the share of the headline measurement; the automatic choice takes the masked route"""
    big = request.getfixturevalue(name)
    _check_new(big, ref25, big.n - 33, paths=(0, 1, 2))


@pytest.mark.parametrize('name', ['s8', 's16'])
def test_new_with_min_shared(request, ref25, name):
    """the second pass restores the sizes of the database genomes whose pairs reach the threshold"""
    big = request.getfixturevalue(name)
    assert sum(v < 20 for v in ref25[1].values()) > 0
    _check_new(big, ref25, big.n - 33, min_shared=20)


@pytest.mark.parametrize('name', ['s8', 's16'])
def test_new_outnumbers_the_database(request, ref25, name):
    """n_db = 4: the LDS bit field saturates; n - 331: the smallest new part that holds two members of one family"""
    big = request.getfixturevalue(name)
    _check_new(big, ref25, 4)
    _check_new(big, ref25, big.n - FAMILIES - 1)


# ---------------------------------------------------------------- 4. a level-2 unit of exactly three position groups
N_THREE = 2457


@pytest.fixture(scope='module')
def three_groups(base):
    """The first 2 457 genomes of S8 at k = 24 (98.3 Mbp, dense, no N runs) with their own oracle run.  Measured: 0.2 s on the 16
    threads of the MI355X host, 2.3 s on an 8-thread machine without a GPU."""
    codes, offsets = base
    offsets = offsets[:N_THREE + 1]
    codes = codes[:offsets[-1]]
    big = Big(codes, offsets, 24)
    g = big.geo
    assert g['P'] == 100638720 and (g['short_rec'], g['st_tiles'], g['n_st'], g['u_st'], g['g_st']) == (1, 4, 3072, 3072, 1024)
    return big, _oracle(codes, offsets, 24)


def test_three_groups_all_vs_all(three_groups):
    _check_all_vs_all(*three_groups)


def test_three_groups_new(three_groups):
    big, ref = three_groups
    _check_new(big, ref, big.n - 25)
