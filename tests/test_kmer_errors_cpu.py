"""The argument errors of the k-mer entries without a GPU: code and full text of vg_last_error() for a null set, k outside 8..31, a
bad shard, a fraction outside (0,1] (NaN included), n_db outside the set, a negative number of positions and a genome index outside
the set.  Every check runs before the device is asked for.  Per entry the order is: null (the entry's own text), k, the shard where
the entry has shards, the fraction; then what only that entry checks.  The texts are the ones the library gave before the checks
were brought together in one place; vg_kmer_set had no fraction check then and has the others' now."""
import math

import pytest

from vclust_amd import _lib, api, synth

EINVAL = -1
K_RANGE = 'k out of range (8..31)'
BAD_SHARD = 'bad shard'
FRACTION = 'fraction must be in (0,1]'
BAD_FRACTIONS = [-1.0, 0.0, 1.5, math.nan]


@pytest.fixture(scope='module')
def gs():
    codes, offsets, names = synth.make_families(4, 3, length=3000, seed=5)
    return api.GenomeSet.from_codes(codes, offsets, names)


def refused(call):
    """-> (code, vg_last_error()) of a call that must be refused"""
    with pytest.raises(_lib.VclustGpuError) as e:
        call()
    return e.value.code, _lib.load().vg_last_error().decode()


# entry -> call(set, k, fraction, shard, n_shards); an entry without shards ignores them
ENTRIES = {
    'vg_kmer_shared': lambda g, k, f, sh, ns: g.kmer_shared(k, f, sh, ns),
    'vg_kmer_shared_new': lambda g, k, f, sh, ns: g.kmer_shared_new(6, k, f),
    'vg_kmer_geometry': lambda g, k, f, sh, ns: g.kmer_geometry(k, f, sh, ns),
    'vg_kmer_set': lambda g, k, f, sh, ns: g.kmer_set(0, k, f),
}
SHARDED = ['vg_kmer_shared', 'vg_kmer_geometry']
NULL_TEXT = {'vg_kmer_shared': 'vg_kmer_shared: null argument', 'vg_kmer_shared_new': 'vg_kmer_shared_new: null argument',
             'vg_kmer_geometry': 'vg_kmer_geometry: null argument', 'vg_kmer_set': 'vg_kmer_set: bad argument'}


def test_twelve_genomes(gs):
    assert len(gs) == 12


@pytest.mark.parametrize('entry', ENTRIES)
def test_null_set_comes_first(entry):
    null = api.GenomeSet(None)
    assert refused(lambda: ENTRIES[entry](null, 25, 1.0, 0, 1)) == (EINVAL, NULL_TEXT[entry])
    assert refused(lambda: ENTRIES[entry](null, 7, -1.0, 3, 2)) == (EINVAL, NULL_TEXT[entry])


@pytest.mark.parametrize('k', [-1, 0, 7, 32, 100])
@pytest.mark.parametrize('entry', ENTRIES)
def test_k_out_of_range(gs, entry, k):
    assert refused(lambda: ENTRIES[entry](gs, k, 1.0, 0, 1)) == (EINVAL, K_RANGE)
    # it comes before the shard and the fraction
    assert refused(lambda: ENTRIES[entry](gs, k, 0.0, 2, 2)) == (EINVAL, K_RANGE)


@pytest.mark.parametrize('k', [7, 32])
def test_k_out_of_range_geometry_at(k):
    assert refused(lambda: api.kmer_geometry_at(1 << 20, k)) == (EINVAL, K_RANGE)
    assert refused(lambda: api.kmer_geometry_at(-1, k)) == (EINVAL, K_RANGE)


@pytest.mark.parametrize('shard,n_shards', [(0, 0), (0, -1), (-1, 2), (2, 2), (5, 1)])
@pytest.mark.parametrize('entry', SHARDED)
def test_bad_shard(gs, entry, shard, n_shards):
    assert refused(lambda: ENTRIES[entry](gs, 25, 1.0, shard, n_shards)) == (EINVAL, BAD_SHARD)
    # it comes before the fraction
    assert refused(lambda: ENTRIES[entry](gs, 25, 0.0, shard, n_shards)) == (EINVAL, BAD_SHARD)


@pytest.mark.parametrize('fraction', BAD_FRACTIONS)
@pytest.mark.parametrize('entry', ENTRIES)
def test_fraction_outside_the_interval(gs, entry, fraction):
    """vg_kmer_set had no such check once: a negative fraction reached the conversion to a 64-bit threshold"""
    assert refused(lambda: ENTRIES[entry](gs, 25, fraction, 0, 1)) == (EINVAL, FRACTION)
    if entry in SHARDED:
        assert refused(lambda: ENTRIES[entry](gs, 8, fraction, 1, 2)) == (EINVAL, FRACTION)


@pytest.mark.parametrize('n_db', [-1, 13, 1 << 20])
def test_n_db_outside_the_set(gs, n_db):
    text = f'vg_kmer_shared_new: n_db = {n_db} is outside 0..12 (the genomes of the set)'
    assert refused(lambda: gs.kmer_shared_new(n_db, 25, 1.0)) == (EINVAL, text)
    # behind k and the fraction
    assert refused(lambda: gs.kmer_shared_new(n_db, 32, 1.0)) == (EINVAL, K_RANGE)
    assert refused(lambda: gs.kmer_shared_new(n_db, 25, 1.5)) == (EINVAL, FRACTION)


def test_negative_number_of_positions():
    assert refused(lambda: api.kmer_geometry_at(-1, 25)) == (EINVAL, 'vg_kmer_geometry_at: negative number of positions')


@pytest.mark.parametrize('idx', [-1, 12, 1000])
def test_kmer_set_index_outside_the_set(gs, idx):
    assert refused(lambda: gs.kmer_set(idx, 25, 1.0)) == (EINVAL, 'vg_kmer_set: bad argument')
    # it is the first check
    assert refused(lambda: gs.kmer_set(idx, 7, 0.0)) == (EINVAL, 'vg_kmer_set: bad argument')
