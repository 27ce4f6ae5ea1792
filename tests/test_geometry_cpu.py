"""Which index geometry the prefilter takes, asked on the host (vg_kmer_geometry / vg_kmer_geometry_at: the entry calls the function
the pass calls, so there is one definition of the rules).  The table below pins the thresholds between the geometries: the GPU tests
of the large geometries (test_gpu_large_geometry.py) size their sets by these rules, and a changed threshold must fail HERE instead
of silently moving those tests onto another geometry.  No device is needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vclust_amd import _lib, api, synth

# P (padded positions), k -> st_tiles, total_bits, n_st, u_st, short_rec, 2^25-position groups per level-2 unit (short records only)
TABLE = [
    (69_632_000, 25, 4, 17, 2125, 2125, False, None),          # not narrow: 2k - total_bits = 33 key bits
    (69_632_000, 24, 4, 17, 2125, 2125, False, None),          # narrow, but a unit of 2 125 super-tiles is no whole number of groups
    (67_108_864, 24, 4, 16, 2048, 2048, True, 2),
    (100_663_296, 24, 4, 17, 3072, 3072, True, 3),             # n_st = 3 072 exactly: a unit of three groups
    (134_217_728, 25, 8, 17, 2048, 2048, False, None),         # not narrow
    (134_348_799, 25, 8, 17, 2050, 2048, False, None),         # the last P before total_bits = 18
    (134_348_800, 25, 8, 18, 2050, 2048, True, 4),             # 1 025 x 2^17: the smallest set with short records at k = 25
    (135_168_000, 25, 8, 18, 2063, 2048, True, 4),             # 3 300 genomes x 40 960 (the base set of the GPU tests)
    (201_326_592, 25, 12, 18, 2048, 1365, False, None),        # the st_tiles = 12 band: super-tiles of 98 304 positions, no power of two
    (210_000_000, 25, 12, 18, 2137, 1365, False, None),
    (268_435_455, 25, 12, 18, 2731, 1365, False, None),
    (268_435_456, 25, 16, 18, 2048, 1024, True, 4),          # (2^28 >> 18 = 1 024: still 18 bits)
    (270_000_000, 25, 16, 19, 2060, 1024, True, 4),
    (4_096_000_000, 25, 16, 22, 31250, 1024, True, 4),         # 100 000 genomes x 40 960: the benchmark
]


@pytest.mark.parametrize('P,k,st_tiles,total_bits,n_st,u_st,short_rec,groups', TABLE)
def test_geometry_table(P, k, st_tiles, total_bits, n_st, u_st, short_rec, groups):
    g = api.kmer_geometry_at(P, k)
    assert g['accepted'] == 1 and g['P'] == P and g['n_passes'] == 1
    assert (g['levels'], g['B1'], g['B2']) == (2, 11, total_bits - 11)
    assert (g['st_tiles'], g['total_bits'], g['n_st'], g['u_st']) == (st_tiles, total_bits, n_st, u_st)
    assert g['tile32k'] == 1                                   # every row: whole 32 768-position tiles
    assert g['narrow'] == (2 * k - total_bits <= 32)
    assert bool(g['short_rec']) == short_rec
    if short_rec:
        assert g['g_st'] * st_tiles * 8192 == 1 << 25 and g['u_st'] == groups * g['g_st']
    else:
        assert g['g_st'] == 0


def test_geometry_edges():
    assert api.kmer_geometry_at(65535)['accepted'] == 0                    # the general path: too small, and beyond 32-bit rows
    assert api.kmer_geometry_at(1 << 32)['accepted'] == 0
    one = api.kmer_geometry_at(65536)
    assert (one['accepted'], one['levels'], one['total_bits'], one['short_rec']) == (1, 1, 6, 0)
    assert api.kmer_geometry_at(1 << 21)['levels'] == 1 and api.kmer_geometry_at((1 << 21) + 2048)['levels'] == 2
    for bad in (lambda: api.kmer_geometry_at(100000, k=7), lambda: api.kmer_geometry_at(-1)):
        with pytest.raises(_lib.VclustGpuError) as e:
            bad()
        assert e.value.code == -1


def test_geometry_of_a_set_is_that_of_its_positions():
    """The form that takes a set: P is the set's layout, a dense single pass is the table's geometry, sub-shards and shards are RANGE
    passes (whole buckets of the set's own partition: same digits), a fraction is a compact source."""
    codes, offsets, names = synth.make_families(8, 4, length=5000, seed=5)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    lens = np.diff(offsets)
    P = int(((lens >> 8) + 1).sum()) << 8                                  # mean 5 000 / 16 = 312: genomes start at multiples of 256
    g = gs.kmer_geometry(k=25)
    assert g == api.kmer_geometry_at(P, 25) and g['accepted'] == 1 and g['P'] == P and g['levels'] == 1
    assert gs.kmer_geometry(k=25, fraction=0.5) == {**{name: 0 for name in g}, 'accepted': -1, 'P': P, 'n_passes': 1}
    sharded = gs.kmer_geometry(k=25, shard=1, n_shards=3)
    assert sharded == g                                                    # one level: the shard's buckets are not a geometry field
    lib = _lib.load()
    lib.vg_set_subshards(3)
    try:
        sub = gs.kmer_geometry(k=25)
        assert sub == {**g, 'n_passes': 3}
    finally:
        lib.vg_set_subshards(0)
    with pytest.raises(_lib.VclustGpuError) as e:
        gs.kmer_geometry(shard=2, n_shards=2)
    assert e.value.code == -1


def test_developer_switches_apply():
    """VG_LEVEL1_RECORDS=long and VG_INDEX_PATH=radix are read when the library is loaded: a fresh process."""
    root = str(_lib.PKG_DIR.parent)
    code = ("import sys; sys.path.insert(0, %r); from vclust_amd import api; g = api.kmer_geometry_at(135168000, 25); "
            "print(g['accepted'], g['short_rec'], g['st_tiles'])" % root)

    def run(**env):
        return subprocess.run([sys.executable, '-c', code], env={**os.environ, **env}, stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert run() == ['1', '1', '8']
    assert run(VG_DEV_SWITCHES='1', VG_LEVEL1_RECORDS='long') == ['1', '0', '8']
    assert run(VG_DEV_SWITCHES='1', VG_INDEX_PATH='radix')[0] == '0'
