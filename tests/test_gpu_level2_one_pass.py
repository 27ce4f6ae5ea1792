"""Level 2 of the bucket pipeline in one pass: `k_part_scatter2_narrow<., true>` gives every final bucket a
fixed number of record slots and counts as it writes -- no `k_part_count2`, no `k_scan_units`, no unit table -- and falls back to
the counted level 2 when a bucket outgrows its slots.

Every case runs in child processes (developer switches and VG_HOST_TRACE are read once per process), with VG_LEVEL2=onepass and
VG_LEVEL2=counted, and compares set sizes and every shared count with each other and with the CPU oracle.  The host marks of a child
(`[vg host] level2: ...` on stderr) say which level 2 ran.  The sets are the smallest that reach the kernels, from the makers of
test_gpu_large_geometry.py: S (328 families of ten 40 kb genomes, P = 134 348 800: the smallest k = 25 set with short level-1 records
and two levels) and T4 at k = 24 (12-byte level-1 records into the narrow scatter); their geometry is asserted through kmer_geometry.
"""
import json
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import kmer_child as kc
import oracle_lib as orc

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
MEMBERS = 10
BK_MAXBIN = 768                     # vg_prefilter.hip: a k-mer in more entries of one bucket than this leaves the LDS bucket kernels
ONE_PASS = re.compile(r'level2: one pass \(largest bucket (\d+) of (\d+) slots\)')
OVERFLOWED = 'level2: one pass overflowed, counted'


# ---------------------------------------------------------------- children
def _marks(stderr):
    return [line for line in stderr.splitlines() if line.startswith('[vg host]')]


def _start(program, args, env):
    p = subprocess.run([sys.executable, str(program)] + [str(a) for a in args], env=dict(os.environ, VG_DEV_SWITCHES='1', VG_HOST_TRACE='1', **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
    return _marks(p.stderr)


class Job:
    """A set and one kmer_shared call, written once for all the children that run it (tests/kmer_child.py is the child's program)."""

    def __init__(self, job_dir, name, codes, offsets, call):
        self.dir, self.name, self.runs = pathlib.Path(job_dir), name, 0
        self.fin = self.dir / f'{name}.job.npz'
        np.savez(self.fin, codes=codes, offsets=offsets, calls=np.array(json.dumps([call])))

    def run(self, **env):
        """-> (set sizes, pairs as a dict, host marks) of the call in a fresh process with these developer switches"""
        self.runs += 1
        fout = self.dir / f'{self.name}.{self.runs}.out.npz'
        marks = _start(ROOT / 'tests' / 'kmer_child.py', [self.fin, fout], env)
        d = np.load(fout)
        return d['sizes_0'].tolist(), {(int(a), int(b)): int(c) for a, b, c in d['pairs_0'].tolist()}, marks


def _which(marks):
    """'one pass', 'overflowed' or 'counted' (no mark of the one-pass form at all), and the (largest bucket, slots) of a one-pass run"""
    text = '\n'.join(marks)
    assert 'buckets: level 2 done' in text, marks
    m = ONE_PASS.search(text)
    if m:
        assert OVERFLOWED not in text
        return 'one pass', (int(m.group(1)), int(m.group(2)))
    return ('overflowed' if OVERFLOWED in text else 'counted'), None


# ---------------------------------------------------------------- the sets, each with one oracle run
def _families(n_families):
    from test_gpu_new2all import _member_major
    from vclust_amd import synth
    codes, offsets, _ = _member_major(*synth.make_families(n_families, MEMBERS, length=40000, seed=3), MEMBERS)
    return codes, offsets


def _oracle(codes, offsets, k):
    sizes, pairs = orc.shared_all_mt(codes, offsets, k=k)[:2]
    return [int(x) for x in sizes], pairs


def _geometry(codes, offsets, **call):
    """kmer_geometry of the call, with the slots of its level 2 (kmer_level2_slots) as 'level2_slots'"""
    from vclust_amd import api
    gs = api.GenomeSet.from_codes(codes, offsets)
    return dict(gs.kmer_geometry(**call), level2_slots=gs.kmer_level2_slots(**call))


class Set:
    def __init__(self, tmp, name, codes, offsets, k):
        self.codes, self.offsets, self.k = codes, offsets, k
        self.geo = _geometry(codes, offsets, k=k)
        self.job = Job(tmp, name, codes, offsets, dict(k=k))
        self.ref = _oracle(codes, offsets, k)
        self.results = {}

    def run(self, level2, **env):
        """the all-vs-all call under VG_LEVEL2=level2 (+ env): one child per distinct environment"""
        key = (level2,) + tuple(sorted(env.items()))
        if key not in self.results:
            self.results[key] = self.job.run(VG_LEVEL2=level2, **env)
        return self.results[key]


@pytest.fixture(scope='module')
def short_set(tmp_path_factory):
    """S: 3 280 genomes, k = 25, 8-byte level-1 records, 2^11 x 2^7 final buckets of 512 records on average"""
    s = Set(tmp_path_factory.mktemp('short'), 's', *_families(328), 25)
    g = s.geo
    assert (g['accepted'], g['n_passes'], g['levels'], g['P'], g['short_rec'], g['narrow'], g['B1'], g['B2']) == (1, 1, 2, 134348800, 1, 1, 11, 7)
    return s


@pytest.fixture(scope='module')
def long_set(tmp_path_factory):
    """T4 at k = 24: 12-byte level-1 records (super-tiles of four tiles), 31 key bits left: `k_part_scatter2_narrow<false>`"""
    s = Set(tmp_path_factory.mktemp('long'), 't4', *_families(170), 24)
    g = s.geo
    assert (g['accepted'], g['n_passes'], g['levels'], g['P'], g['short_rec'], g['narrow'], g['B1'], g['B2']) == (1, 1, 2, 69632000, 0, 1, 11, 6)
    return s


def _capacity(g):
    """the slots of a final bucket as DESIGN.md section 3 states them: m + 7 sqrt(m), rounded up to 8 records"""
    m = g['P'] / 2.0 ** g['total_bits']
    return (int(np.ceil(m + 7.0 * np.sqrt(m))) + 7) // 8 * 8


def _check_both_forms(s):
    assert s.geo['level2_slots'] == _capacity(s.geo) > 0
    one, counted = s.run('onepass'), s.run('counted')
    assert len(s.ref[1]) > 0
    for what, (sizes, pairs, marks) in (('onepass', one), ('counted', counted)):
        assert sizes == s.ref[0], what
        assert pairs == s.ref[1], (what, len(pairs), len(s.ref[1]))
    which, (largest, slots) = _which(one[2])
    print(f'one pass: largest final bucket {largest} of {slots} slots')
    assert which == 'one pass' and slots == s.geo['level2_slots'] and 0 < largest <= slots
    assert _which(counted[2])[0] == 'counted'


# ---------------------------------------------------------------- the two record forms
def test_short_records(short_set):
    """`k_part_scatter2_narrow<true, true>`: no bucket of S outgrows its slots; sizes and pairs are the counted form's and the oracle's"""
    _check_both_forms(short_set)


def test_long_level1_records(long_set):
    """`k_part_scatter2_narrow<false, true>`"""
    _check_both_forms(long_set)


def test_row_pointers_without_inlining(short_set):
    """the one-pass layout moves records only: gen[] and the row pointers are numbered by boff[] with inlining on and off"""
    sizes, pairs, marks = short_set.run('onepass', VG_ROWPTR_INLINE='0')
    assert _which(marks)[0] == 'one pass'
    assert sizes == short_set.ref[0] and pairs == short_set.ref[1]
    assert (sizes, pairs) == short_set.run('onepass')[:2]


# ---------------------------------------------------------------- overflow
def test_overflow_falls_back_to_the_counted_form(short_set, tmp_path):
    """One 25-mer planted in more genomes than a final bucket has slots -- its records alone outgrow the bucket, whatever else the
    bucket holds -- and in fewer than BK_MAXBIN, so that the bucket still goes through the LDS bucket kernels."""
    slots = short_set.geo['level2_slots']
    assert slots + 8 < BK_MAXBIN, 'no room between the slots of a bucket and BK_MAXBIN at this geometry'
    n_planted = (slots + BK_MAXBIN) // 2
    assert slots < n_planted < BK_MAXBIN
    codes, offsets = short_set.codes.copy(), short_set.offsets
    kmer = np.random.default_rng(7).integers(0, 4, 25).astype(np.uint8)
    for g in range(n_planted):                                  # member-major: genomes 0 .. 327 are one member of every family, and so on
        codes[offsets[g] + 1000:offsets[g] + 1025] = kmer
    g = _geometry(codes, offsets, k=25)
    assert g == short_set.geo
    ref = _oracle(codes, offsets, 25)
    assert all(ref[1][(b, a)] >= 1 for a in (0, 1) for b in (n_planted - 2, n_planted - 1))
    sizes, pairs, marks = Job(tmp_path, 'planted', codes, offsets, dict(k=25)).run(VG_LEVEL2='onepass')
    assert _which(marks)[0] == 'overflowed', marks
    assert sizes == ref[0]
    assert pairs == ref[1]


def test_bucket_at_capacity_and_one_over(short_set):
    """The slots set through the developer switch to the largest final bucket of S: one pass, that bucket full to the last slot.
    One slot fewer: the counted form runs.  Both give the counted form's result."""
    counted = short_set.run('counted')
    which, (largest, _) = _which(short_set.run('onepass')[2])
    assert which == 'one pass'
    full = short_set.run(f'onepass:{largest}')
    assert _which(full[2]) == ('one pass', (largest, largest))
    over = short_set.run(f'onepass:{largest - 1}')
    assert _which(over[2])[0] == 'overflowed'
    assert full[:2] == counted[:2] and over[:2] == counted[:2]


# ---------------------------------------------------------------- the decision
def test_range_shard_and_masked_route_keep_the_counted_form(short_set, tmp_path):
    """A RANGE shard and the masked `--db` route of the same set under VG_LEVEL2=onepass: the geometry says counted, no mark of the
    one-pass form appears, and the results are the oracle's."""
    from test_new2all_cpu import restrict_new
    s = short_set
    g = _geometry(s.codes, s.offsets, k=25, shard=1, n_shards=3)
    assert (g['accepted'], g['levels'], g['level2_slots']) == (1, 2, 0)
    sizes, pairs = np.zeros(len(s.offsets) - 1, dtype=np.int64), {}
    for shard in range(3):
        part_sizes, part, marks = Job(tmp_path, f'range{shard}', s.codes, s.offsets, dict(k=25, shard=shard, n_shards=3)).run(VG_LEVEL2='onepass')
        assert _which(marks)[0] == 'counted'
        sizes += np.array(part_sizes)
        for key, v in part.items():
            pairs[key] = pairs.get(key, 0) + v
    assert [int(x) for x in sizes] == s.ref[0] and pairs == s.ref[1]
    # the masked route: this module is the child's program
    n_db = len(s.offsets) - 1 - 33
    fout = tmp_path / 'new.out.npz'
    marks = _start(__file__, [s.job.fin, fout, n_db], dict(VG_LEVEL2='onepass'))
    assert any('buckets: enter' in m for m in marks) and not any('level2: one pass' in m for m in marks), marks
    d = np.load(fout)
    assert 'kmer_new_mask' in json.loads(str(d['scopes']))
    want_sizes, want = restrict_new(s.ref[0], s.ref[1], n_db)
    assert d['sizes'].tolist() == want_sizes
    assert {(int(a), int(b)): int(c) for a, b, c in d['pairs'].tolist()} == want


def _new_child_main(fin, fout, n_db):
    """kmer_shared_new(n_db) on the masked route, on the set of a job file -> sizes, pairs, profile scopes"""
    sys.path.insert(0, str(ROOT))
    from vclust_amd import api
    d = np.load(fin)
    gs = api.GenomeSet.from_codes(d['codes'], d['offsets'])
    api.set_new_path(2)
    api.profile_enable(True); api.profile_reset()
    sizes, pairs = gs.kmer_shared_new(n_db, k=25)
    scopes = sorted(e['name'] for e in api.profile_get())
    out = np.asarray([(a, b, c) for (a, b), c in sorted(kc.pairs_dict(pairs).items())], dtype=np.int64).reshape(-1, 3)
    np.savez(fout, sizes=np.asarray(sizes, dtype=np.int64), pairs=out, scopes=np.array(json.dumps(scopes)))


if __name__ == '__main__':
    _new_child_main(sys.argv[1], sys.argv[2], int(sys.argv[3]))
