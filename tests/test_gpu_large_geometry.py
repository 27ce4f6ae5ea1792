"""The index geometry of large sets -- 32 768-position tiles, 8-byte "short" level-1 records (key bits, position modulo 2^25),
level-2 units that span up to four 2^25-position groups -- held to the CPU oracle count for count: every set size and every shared
count of the all-vs-all pass, of RANGE shards and sub-shards, and of the masked `--db` route (k_new_mask rebuilds positions from the
group base of a super-tile plus 25 low bits).

One dense set at the smallest size with short records at k = 25 (S8: 3 300 genomes of 40 kb, P = 135 168 000, super-tiles of 8
tiles), and the same genomes with the one N of every genome widened to an N run: S12 (super-tiles of 12 tiles: 98 304 positions, no
power of two, so 12-byte records) and S16 (16 tiles, short records, the geometry of the benchmark).  The N run sits at the same base
offset in all three, so their k-mer sets are the same and ONE oracle run on S8 is the reference for all three.  A fourth set, the
first 2 457 genomes of S8 at k = 24, is the one shape whose level-2 unit spans exactly three groups.

The level-1 kernels are compiled once with k = 25 folded in and once reading k from their arguments, so S8 is also run at k = 21
(short records), 26 and 30 (12-byte records, wide level 2), each against its own oracle run: dense, as RANGE shards and sub-shards
and on the masked route.  T4 (1 700 genomes, P = 69 632 000) is the smallest set with 32 768-position tiles: 12-byte records at
every k, dense and under RANGE; its first 1 639 genomes at k = 24 leave exactly 32 key bits below the digits.  S8 with a few
genomes replaced by homopolymers and tandem repeats is the one set on which a RANGE shard takes a 65 536-position tile as quarters.

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


# The references on S8 at the other key lengths (a GenomeSet does not depend on k: s8 serves them all).  Each measured like ref25.
@pytest.fixture(scope='module')
def ref21(base):
    """k = 21: 31 key bits below the 11 level-1 digits, short records, narrow level 2, k read from the arguments.  17 848 pairs.  0.3 s on the 16 threads
    of the MI355X host, 3.7 s on an 8-thread machine without a GPU."""
    return _oracle(*base, 21)


@pytest.fixture(scope='module')
def ref26(base):
    """k = 26: the first k whose 2k - 11 key bits no longer fit a short record; 12-byte records, wide level 2.  14 850 pairs: the
    family pairs alone.  0.3 s and 4.2 s."""
    return _oracle(*base, 26)


@pytest.fixture(scope='module')
def ref30(base):
    """k = 30: 60 key bits.  14 850 pairs.  0.3 s on the MI355X host."""
    return _oracle(*base, 30)


def _s8_at(k, n_passes=1):
    """the geometry of a pass over S8 at key length k, dense or a RANGE shard: the set's partition (18 bits, super-tiles of eight
    tiles scattered as 32 768-position tiles) with the level-2 and level-1 record formats that k chooses"""
    narrow, short_rec = {21: (1, 1), 25: (1, 1), 26: (0, 0), 30: (0, 0)}[k]
    return dict(accepted=1, n_passes=n_passes, levels=2, P=135168000, total_bits=18, B1=11, st_tiles=8, tile32k=1, narrow=narrow, short_rec=short_rec)


def _assert_geometry(gs, want, **call):
    g = gs.kmer_geometry(**call)
    assert {name: g[name] for name in want} == want, (call, g)


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
def _check_all_vs_all(big, ref, k=None):
    sizes, got, scopes = _profiled(lambda: big.gs.kmer_shared(k=k or big.k))
    assert sizes == ref[0]
    assert got == ref[1]
    assert {'kmer_partition', 'kmer_partition2', 'bucket_sort_runs', 'spgemm_rows'} <= scopes
    assert not any('radix' in s or s.startswith('index_') for s in scopes), scopes      # the bucket pipeline, not the general path


@pytest.mark.parametrize('name', ['s8', 's12', 's16'])
def test_all_vs_all(request, ref25, name):
    assert len(ref25[1]) > FAMILIES * MEMBERS * (MEMBERS - 1) // 2, 'no chance pair between unrelated genomes in the reference'
    _check_all_vs_all(request.getfixturevalue(name), ref25)


@pytest.mark.parametrize('k', [21, 26, 30])
def test_all_vs_all_k_from_the_arguments(request, s8, k):
    """S8 with k read from the arguments: `k_part_count<0,0,false>` and `k_part_scatter_dense<0>` writing short records for the
    narrow level 2 (k = 21) and 12-byte records for the staged wide level 2 (k = 26, the first k without short records, and 30)."""
    ref = request.getfixturevalue(f'ref{k}')
    _assert_geometry(s8.gs, _s8_at(k), k=k)
    if k == 21:
        assert len(ref[1]) > FAMILIES * MEMBERS * (MEMBERS - 1) // 2, 'no chance pair between unrelated genomes in the reference'
    _check_all_vs_all(s8, ref, k)


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
    _check_range_shards(s8, ref25, 25, n_shards, _s8_at(25))


def _check_range_shards(big, ref, k, n_shards, want):
    """every one of n_shards RANGE passes has the geometry `want` and ran on the dense source cut by digit range; set sizes and counts
    summed over the shards are the reference's.  -> the scopes of all passes"""
    sizes, pairs, seen = np.zeros(big.n, dtype=np.int64), {}, set()
    for shard in range(n_shards):
        _assert_geometry(big.gs, want, k=k, shard=shard, n_shards=n_shards)
        part_sizes, part, scopes = _profiled(lambda: big.gs.kmer_shared(k=k, shard=shard, n_shards=n_shards))
        assert {'kmer_partition', 'kmer_partition2', 'bucket_sort_runs'} <= scopes
        assert not (scopes & EXTRACTED) and not any('radix' in s for s in scopes), scopes      # dense source cut by digit range: RANGE
        sizes += np.array(part_sizes)
        for key, v in part.items():
            pairs[key] = pairs.get(key, 0) + v
        seen |= scopes
    assert [int(x) for x in sizes] == ref[0]
    assert pairs == ref[1]
    return seen


@pytest.mark.parametrize('n_shards', [2, 3, 8])
@pytest.mark.parametrize('k', [21, 26])
def test_range_scatter_k_from_the_arguments(request, s8, k, n_shards):
    """`k_part_scatter_range<0,32768>` (two shards: tiles taken as halves; three: whole tiles) and `<0,65536>` (eight), writing short
    records at k = 21 and 12-byte records at k = 26.  Which tile a shard count takes, and that two shards meet tiles of more than
    16 384 kept k-mers, is argued in test_range_scatter_half_tiles_and_64k_tiles; neither argument depends on k (one N costs k positions:
    such a tile has 32 747 valid ones at k = 21 and 32 742 at k = 26)."""
    _check_range_shards(s8, request.getfixturevalue(f'ref{k}'), k, n_shards, _s8_at(k))


def test_subshards_of_long_records(s8, ref26):
    """three RANGE sub-shards at k = 26: 12-byte level-1 records whose payloads are row numbers"""
    lib = _lib.load()
    lib.vg_set_subshards(3)
    try:
        _assert_geometry(s8.gs, _s8_at(26, n_passes=3), k=26)
        sizes, got, scopes = _profiled(lambda: s8.gs.kmer_shared(k=26))
    finally:
        lib.vg_set_subshards(0)
    assert sizes == ref26[0]
    assert got == ref26[1]


# ---------------------------------------------------------------- 3. new genomes against a database
def _check_new(big, ref, n_db, min_shared=1, paths=(1, 2), k=None):
    """kmer_shared_new(n_db) under every route of `paths` against the restricted oracle result; the profile says which route ran
    (0 = automatic: expected to choose the masked route here)"""
    k = k or big.k
    assert 0 < n_db < big.n
    want_sizes, want = restrict_new(ref[0], {key: v for key, v in ref[1].items() if v >= min_shared}, n_db)
    assert any(b < n_db for _, b in want), 'no pair of a new and a database genome'
    # (the new genomes of a case with at most FAMILIES of them are one member of as many families: related only by chance)
    if big.n - n_db > FAMILIES:
        assert any(b >= n_db for _, b in want), 'no pair of two new genomes'
    for path in paths:
        api.set_new_path(path)
        try:
            sizes, got, scopes = _profiled(lambda: big.gs.kmer_shared_new(n_db, k=k, min_shared=min_shared))
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


@pytest.mark.parametrize('name', ['s8', 's12', 's16'])
def test_new_one_per_cent(request, ref25, name):
    """1 % new: the share of the headline measurement; the automatic choice takes the masked route.  On S12 the mask is applied to
    12-byte level-1 records of super-tiles of 98 304 positions (no power of two) ahead of the narrow level 2."""
    big = request.getfixturevalue(name)
    _check_new(big, ref25, big.n - 33, paths=(0, 1, 2))


@pytest.mark.parametrize('k', [21, 26])
def test_new_one_per_cent_k_from_the_arguments(request, s8, k):
    """the masked route with k read from the arguments: over short records (k = 21) and over 12-byte records and the wide level 2 (26)"""
    _assert_geometry(s8.gs, _s8_at(k), k=k)
    _check_new(s8, request.getfixturevalue(f'ref{k}'), s8.n - 33, k=k)


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


# ---------------------------------------------------------------- 5. the smallest set with 32 768-position tiles
T4_FAMILIES, N_T4E = 170, 1639


def _t4_at(k, total_bits=17):
    """12-byte level-1 records at every k (T4 and T4e partition on 17 and 16 bits; no whole number of groups per level-2 unit)"""
    return dict(accepted=1, n_passes=1, levels=2, B1=11, total_bits=total_bits, st_tiles=4, tile32k=1, short_rec=0, narrow=int(2 * k - total_bits <= 32))


@pytest.fixture(scope='module')
def t4_host():
    """T4 on the host: 170 families of ten 40 kb genomes from the bench generator, member-major as S8, no N"""
    codes, offsets, _ = _member_major(*synth.make_families(T4_FAMILIES, MEMBERS, length=40000, seed=3), MEMBERS)
    return codes, offsets


@pytest.fixture(scope='module')
def t4(t4_host):
    """T4 on the device: P = 69 632 000, super-tiles of four tiles -- the least that is scattered as one 32 768-position tile -- and
    its oracle results, one run per k on first use.  Measured per run (7 661 pairs at k = 24, 7 654 at 25, the 7 650 family pairs at 26 and 30):
    0.1 s on the 16 threads of the MI355X host, 1.6 to 2.1 s on an 8-thread machine without a GPU."""
    big = Big(*t4_host, 25)
    assert big.n == T4_FAMILIES * MEMBERS and big.geo['P'] == 69632000 and big.geo['n_st'] == 2125
    refs = {}

    def oracle(k):
        if k not in refs:
            refs[k] = _oracle(*t4_host, k)
            assert len(refs[k][1]) >= T4_FAMILIES * MEMBERS * (MEMBERS - 1) // 2
        return refs[k]
    return big, oracle


@pytest.mark.parametrize('k', [24, 25, 30])
def test_t4_all_vs_all(t4, k):
    """12-byte level-1 records from `k_part_scatter_dense`: k = 25 (`<25>`, then the staged wide level 2 `k_part_scatter<2,2>`),
    k = 24 (`<0>`, then `k_part_scatter2_narrow<false>`: 31 key bits left) and k = 30 (`<0>`, wide)."""
    big, oracle = t4
    _assert_geometry(big.gs, _t4_at(k), k=k)
    assert _t4_at(k)['narrow'] == (k == 24)
    _check_all_vs_all(big, oracle(k), k)


@pytest.mark.parametrize('k', [25, 26])
def test_t4_range_shards(t4, k):
    """three RANGE shards of T4: the 12-byte branch of `k_part_scatter_range<25,32768>` and `<0,32768>` (super-tiles of four tiles
    have no 65 536-position tile)"""
    big, oracle = t4
    assert _t4_at(k)['narrow'] == 0
    _check_range_shards(big, oracle(k), k, 3, _t4_at(k))


def test_t4e_narrowing_shift_of_32_bits(t4_host):
    """T4e, the first 1 639 genomes of T4 (P = 67 133 440: 16 bits), at k = 24: 2k - total_bits = 32, the whole key word of a narrow
    level-2 record is key -- the edge of the narrowing shift, with k read from the arguments.  Its oracle run (7 112 pairs): 0.1 s on the 16 threads of the
    MI355X host, 1.6 s on an 8-thread machine without a GPU."""
    codes, offsets = t4_host
    offsets = offsets[:N_T4E + 1]
    codes = codes[:offsets[-1]]
    big = Big(codes, offsets, 24)
    want = _t4_at(24, total_bits=16)
    assert want['narrow'] == 1 and 2 * 24 - want['total_bits'] == 32
    assert big.geo['P'] == 67133440 and big.geo['n_st'] == 2049
    _assert_geometry(big.gs, want, k=24)
    _check_all_vs_all(big, _oracle(codes, offsets, 24))


# ---------------------------------------------------------------- 6. the quarter-tile arm of the 65 536-position tile
RG_LIST = 16384                                                         # kept k-mers that the list of k_part_scatter_range holds
HOMOPOLYMERS = {1000: 0, 1001: 3, 2500: 1}                              # genome -> its one base; A and T: the same canonical k-mer
TANDEM = (1700, 1701)                                                   # genomes that repeat the same 7-base unit, in another phase
UNIT = (0, 2, 1, 3, 3, 0, 1)                                            # AGCTTAC: no rotation of it is the reverse complement of one
A_RUN = (2002, 6384, 20000)                                             # genome, first base and length of a poly-A run inside it


@pytest.fixture(scope='module')
def low_complexity(base):
    """S8 with five genomes replaced by low-complexity sequence of their own length: three 40 kb homopolymers without the N (every
    position of one carries the same k-mer, hence one level-1 digit, hence one shard) and two tandem repeats of a 7-base unit;
    a sixth genome has 20 kb of its middle replaced by a poly-A run.  P and the geometry stay S8's.  -> (the set, its codes, offsets, oracle(k): one run per k on first use).  Measured per run:
    0.3 s on the 16 threads of the MI355X host, 3.9 s on an 8-thread machine without a GPU."""
    codes, offsets = base
    codes = codes.copy()
    for g, b in HOMOPOLYMERS.items():
        codes[offsets[g]:offsets[g + 1]] = b
    for i, g in enumerate(TANDEM):
        codes[offsets[g]:offsets[g + 1]] = np.resize(np.roll(np.array(UNIT, dtype=np.uint8), 3 * i), int(offsets[g + 1] - offsets[g]))
    g, at, run = A_RUN
    codes[offsets[g] + at:offsets[g] + at + run] = 0
    big = Big(codes, offsets, 25)
    assert big.n == FAMILIES * MEMBERS
    refs = {}

    def oracle(k):
        if k not in refs:
            refs[k] = _oracle(codes, offsets, k)
        return refs[k]
    return big, codes, offsets, oracle


@pytest.mark.parametrize('k', [25, 26])
def test_quarter_tiles(low_complexity, k):
    """Eight RANGE shards take 65 536-position tiles; a tile whose 32 768-position half keeps more than 16 384 k-mers is taken as
    quarters.  Uniform digits never do that to a shard of an eighth; the one k-mer of a homopolymer does, in whichever shard owns its
    digit -- all eight run.  That such a half exists is computed here from the layout and the codes.  k = 25 writes short records
    from there, k = 26 12-byte ones with k read from the arguments.  The some 40 000 occurrences of that k-mer also exceed both LDS
    bucket kernels: `bucket_big` runs.

    The arm between, a tile of more than 16 384 kept k-mers whose halves both fit the list, is what the poly-A run is placed for:
    it straddles the middle of a 65 536-position tile with some 10 000 positions on either side.  The tile keeps all of them in the
    shard of the poly-A k-mer; a half would overflow only if that shard kept more than 6 384 of the half's other 22 768 positions,
    where an eighth (2 846, standard deviation 50) is expected -- the one step here that is an argument, not an assertion."""
    big, codes, offsets, oracle = low_complexity
    _assert_geometry(big.gs, _s8_at(k), k=k)
    for g, b in HOMOPOLYMERS.items():
        seq = codes[offsets[g]:offsets[g + 1]]
        assert (seq == b).all()                                           # no N: every k-mer start of the genome is valid
        first, last = int(big.starts[g]), int(big.starts[g]) + len(seq) - k      # the positions of its k-mer (a k-mer lies at its first base)
        halves = [min(last + 1, h + 32768) - max(first, h) for h in range(first // 32768 * 32768, last + 1, 32768)]
        assert sum(halves) == len(seq) - k + 1 and max(halves) > RG_LIST, 'no half of a 65 536-position tile keeps more of one k-mer than the list holds'
    g, at, run = A_RUN
    first, last = int(big.starts[g]) + at, int(big.starts[g]) + at + run - k
    middle = first // 65536 * 65536 + 32768
    assert (codes[offsets[g] + at:offsets[g] + at + run] == 0).all() and middle - 32768 < first < middle <= last < middle + 32768
    assert last + 1 - first > RG_LIST and max(middle - first, last + 1 - middle) == 10000
    ref = oracle(k)
    a, t = sorted(g for g, b in HOMOPOLYMERS.items() if b in (0, 3))
    assert ref[1][(g, a)] == ref[1][(g, t)] == 1                        # (the run's k-mer is theirs: the same shard)
    assert ref[1][(t, a)] == 1 and ref[0][a] == ref[0][t] == 1          # poly-A and poly-T: one k-mer, the same one
    assert ref[1][(TANDEM[1], TANDEM[0])] == ref[0][TANDEM[0]] == len(UNIT)
    scopes = _check_range_shards(big, ref, k, 8, _s8_at(k))
    assert 'bucket_big' in scopes
