"""Row pointers that carry a genome id: a k-mer whose only smaller partner is one genome gets the pointer
0xFFFFFFFF - partner instead of 1 + the start of its run, and the SpGEMM counts it without reading the genome list.

Every case compares set sizes and every shared count with the CPU oracle, with the default and -- in a child process: developer
switches are read once per process -- with VG_ROWPTR_INLINE=0 (every pointer a plain one); both must equal the oracle and each
other.  The profile scopes of each run say which kernels wrote and read the pointers.
"""
import functools

import numpy as np
import pytest

import kmer_child as kc
import oracle_lib as orc
from vclust_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


def _concat(parts):
    seqs = [c[o[i]:o[i + 1]] for c, o in parts for i in range(len(o) - 1)]
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.uint8), offsets


def _families(spec, length):
    return _concat([synth.make_families(n, m, length=length, seed=seed)[:2] for n, m, seed in spec])


def _pairs_only():
    """12 families of two 3 kb members: just over the 65 536 positions the bucket pipeline needs; a shared k-mer is a run of two"""
    return _families([(12, 2, 3)], 3000)


def _mixed(length=3000):
    """families of 2, 3 and 5 members: ranks 1, 2 and higher in one bucket"""
    return _families([(6, 2, 5), (4, 3, 6), (3, 5, 7)], length)


def _repeats():
    """A block twice in genome 0 and once in genome 1: the run (g0, g0 repeat, g1), in which g1 has TWO entries in front of it and
    must not inline.  The mirror: a block once in genome 2 and twice in genome 3: (g2, g3, g3 repeat), g3 inlines, its repeat
    writes nothing.  Genome 4 repeats a block three times that genome 5 has once, and genome 6 holds all three blocks."""
    rng = np.random.default_rng(21)
    r = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    b1, b2, b3 = r(700), r(700), r(500)
    seqs = [np.concatenate([r(6000), b1, r(5000), b1, r(6000)]), np.concatenate([r(9000), b1, r(9000)]),
            np.concatenate([r(8000), b2, r(9000)]), np.concatenate([r(5000), b2, r(6000), b2, r(5000)]),
            np.concatenate([r(3000), b3, r(3000), b3, r(3000), b3, r(3000)]), np.concatenate([r(7000), b3, r(7000)]),
            np.concatenate([r(4000), b3, r(4000), b1, r(4000), b2, r(4000)])]
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), offsets


def _mixed_and_repeats():
    return _concat([_mixed(), _repeats()])


def _wide_buckets():
    """the set of test_gpu_configs.test_bucket_pipeline_large_buckets: buckets beyond 1 536 entries, the 1 024-thread variant"""
    return synth.make_families(1, 200, length=40000, seed=5)[:2]


def _big_buckets():
    """the set of test_gpu_configs.test_high_multiplicity_kmers_stay_in_the_own_pipeline: buckets only k_bucket_big takes"""
    from test_gpu_configs import _real_shaped_set
    return _real_shaped_set(6000, 1500, 800, seed=9)[:2]


# The 2^13-slot table hands a row to the dense fallback when more than 7/8 of its slots are used (`s_used > HT_SIZE * 7 / 8`): 7 169
# partners are the smallest count that does.
DENSE_PARTNERS = (1 << 13) * 7 // 8 + 1


def _dense_row():
    """7 169 genomes of 40 bases, and a last genome that is all of them in a row: each of its k-mers inside a block has ONE smaller
    partner (an inline pointer), its partners overflow the 2^11- and the 2^13-slot tables.  Genome 1 also holds genome 0's
    bases, so those k-mers of the last genome have two partners (plain pointers beside the inline ones)."""
    rng = np.random.default_rng(33)
    blocks = rng.integers(0, 4, (DENSE_PARTNERS, 40)).astype(np.uint8)
    seqs = [blocks[0], np.concatenate([blocks[0], blocks[1]])] + [blocks[i] for i in range(2, DENSE_PARTNERS)] + [blocks.reshape(-1)]
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), offsets


def _many_short():
    """66 000 genomes of 60 bases in families of 1, 2, 3 and 4 (a member = its ancestor with one substitution): from 65 536 genomes
    on, rows of at most 8 192 k-mers go to the one-wave workgroups of k_spgemm<9, true>, which count inline pointers where they lie
    and queue the plain ones."""
    rng = np.random.default_rng(41)
    seqs = []
    while len(seqs) < 66000:
        anc = rng.integers(0, 4, 60).astype(np.uint8)
        for m in range(1 + len(seqs) % 4):
            g = anc.copy(); at = int(rng.integers(0, 60)); g[at] = (g[at] + 1 + m % 3) & 3
            seqs.append(g)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(x) for x in seqs])
    return np.concatenate(seqs), offsets


SHAPES = dict(many=_many_short, pairs=_pairs_only, mixed=_mixed, small=lambda: _mixed(1200), repeats=_repeats, both=_mixed_and_repeats,
              wide=_wide_buckets, big=_big_buckets, dense=_dense_row)


@functools.lru_cache(maxsize=None)
def _shape(name):
    codes, offsets = SHAPES[name]()
    codes.setflags(write=False); offsets.setflags(write=False)
    return codes, offsets


@functools.lru_cache(maxsize=None)
def _oracle(name, k, fraction):
    codes, offsets = _shape(name)
    osizes, opairs = orc.shared_all_mt(codes, offsets, k=k, fraction=fraction)[:2]      # (the oracle on all host threads: 1.4 M pairs in the largest set)
    return [int(x) for x in osizes], opairs


def _check(tmp_path, name, calls, env=None, scopes=(), no_scopes=()):
    """The calls on the shape with inline pointers (in this process, or in a child where `env` holds developer switches) and with
    VG_ROWPTR_INLINE=0 (a child): both equal the oracle, so each other; every run launched the `scopes` and none of `no_scopes`."""
    codes, offsets = _shape(name)
    if env:
        on = kc.run(tmp_path, 'on', codes, offsets, calls, env)
    else:
        gs = api.GenomeSet.from_codes(codes, offsets, ['s%d' % i for i in range(len(offsets) - 1)])
        on = [kc.shared_with_scopes(gs, api, _lib.load(), c) for c in calls]
    off = kc.run(tmp_path, 'off', codes, offsets, calls, dict(env or {}, VG_ROWPTR_INLINE='0'))
    for call, a, b in zip(calls, on, off):
        osizes, opairs = _oracle(name, call.get('k', 25), call.get('fraction', 1.0))
        assert len(opairs) > 0
        for what, (sizes, pairs, sc) in (('inline', a), ('plain', b)):
            assert sizes == osizes, (name, call, what)
            assert pairs == opairs, (name, call, what, len(pairs), len(opairs))
            assert all(s in sc for s in scopes) and not any(s in sc for s in no_scopes), (name, call, what, sc)
        assert a[0] == b[0] and a[1] == b[1]


BUCKETS = ('bucket_sort_runs', 'spgemm_rows')
NO_RADIX = ('index_runs', 'radix_sort_pairs')


def test_runs_of_two_only(tmp_path):
    """every pointer is an inline one"""
    codes, offsets = _shape('pairs')
    assert api.GenomeSet.from_codes(codes, offsets).kmer_geometry()['accepted'] == 1
    _check(tmp_path, 'pairs', [dict(k=25)], scopes=BUCKETS, no_scopes=NO_RADIX)


def test_mixed_runs(tmp_path):
    _check(tmp_path, 'mixed', [dict(k=25), dict(k=15)], scopes=BUCKETS, no_scopes=NO_RADIX)


def test_repeats_in_a_run(tmp_path):
    _check(tmp_path, 'repeats', [dict(k=25)], scopes=BUCKETS, no_scopes=NO_RADIX)


def test_writer_wide_buckets(tmp_path):
    _check(tmp_path, 'wide', [dict(k=25)], scopes=BUCKETS + ('bucket_sort_runs_wide',), no_scopes=NO_RADIX + ('bucket_big',))


def test_writer_bucket_big(tmp_path):
    _check(tmp_path, 'big', [dict(k=25)], scopes=BUCKETS + ('bucket_big',), no_scopes=NO_RADIX)


def test_writer_radix_path_by_switch(tmp_path):
    """VG_INDEX_PATH=radix: k_group_runs writes the pointers, repeats included"""
    _check(tmp_path, 'both', [dict(k=25)], env=dict(VG_INDEX_PATH='radix'), scopes=('index_runs', 'spgemm_rows'), no_scopes=('bucket_sort_runs',))


def test_writer_radix_path_by_size(tmp_path):
    """fewer than 65 536 positions: the bucket pipeline declines"""
    assert _shape('small')[1][-1] < 60000
    _check(tmp_path, 'small', [dict(k=25)], scopes=('index_runs', 'spgemm_rows'), no_scopes=('bucket_sort_runs',))


def test_compact_rows_range_and_hash(tmp_path):
    """Row pointers indexed by compact row numbers: the RANGE sub-shard passes of one call, and a HASH pass of a fraction"""
    _check(tmp_path, 'both', [dict(k=25, subshards=3)], scopes=BUCKETS, no_scopes=NO_RADIX)
    _check(tmp_path, 'both', [dict(k=25, fraction=0.5)], scopes=('spgemm_rows',))


def test_compact_reader(tmp_path):
    """k_spgemm<9, true>: the reader of sets of 65 536 genomes and more with short rows"""
    assert len(_shape('many')[1]) - 1 >= 1 << 16
    _check(tmp_path, 'many', [dict(k=25)], scopes=BUCKETS, no_scopes=NO_RADIX)


def test_dense_fallback(tmp_path):
    """k_spgemm_dense reads inline and plain pointers"""
    _check(tmp_path, 'dense', [dict(k=25)], scopes=BUCKETS + ('spgemm_rows_wide', 'spgemm_dense_rows'), no_scopes=NO_RADIX)
