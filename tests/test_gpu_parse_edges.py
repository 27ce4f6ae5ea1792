"""HIP rows against the CPU oracle on pairs built to reach the edges of the FAST parse kernels: the wave-uniform
extension round (taken only when all 2 048 positions lie inside the query and the strand of the match) and the
branch-free window rule ((aw, am) = (15, 7)).
  * extensions that end exactly at, one before and one after a 2 048-position round boundary (forward, and backward
    from an event behind a stretch of literals);
  * extensions that run into the query end, the reference end, and the forward / reverse-complement strand boundary;
  * windows holding exactly am and am + 1 mismatches, straddling a 32-base chunk boundary;
  * buckets whose candidates all need verification (tandem repeats: one msl-mer, many entries with the query's tag).
Every ordered pair of the set is parsed in separate processes (developer switches are read once per process): the
one-wave FAST kernel, the four-wave one, the one that also writes regions, the general kernel and the general kernel
that writes regions.  The region-writing variants hand their regions back: every task's regions equal orc.lz_regions as
an ordered list (lz_checks.assert_rows_and_regions).
The four-wave kernel splits a query among its waves only from qlen - mal >= 8 192 on, i.e. from 8 203 bases: of this set
only three sequences reach that -- `ref` (13 001 bases), the tandem repeat `rep` and its mutated copy (9 200 bases
each); on every other query wave 0 parses alone, so
`fast_segments` checks these edges in the four-wave kernel's code, not the hand-over between segments.  The hand-over has
its own inputs and its own file: test_gpu_parse_handover.py."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import lz_checks as lc
import oracle_lib as orc

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _mutate_at(s, positions):
    s = s.copy()
    for p in positions:
        s[p] = (s[p] + 1) % 4
    return s


def _revcomp(s):
    return (3 - s)[::-1].copy()


def _edge_set():
    rng = np.random.default_rng(20261015)
    seqs = []
    ref = _rand(rng, 13001)
    seqs.append(ref)
    # forward extension ending at, one before and one after round boundaries (a dense block of 9 mismatches stops it)
    for k in (1, 2, 3):
        for d in (-1, 0, 1):
            e = 2048 * k + d
            seqs.append(_mutate_at(ref[:e + 700], range(e, e + 17, 2)))
    # backward extension across round boundaries: literals, then a long approximate stretch whose left end sits near a
    # boundary, reached from an event found to its right
    for k in (1, 2):
        for d in (-1, 0, 1):
            ln = 2048 * k + d
            body = _mutate_at(ref[3000:3000 + ln + 400], range(50, ln, 97))
            seqs.append(np.concatenate([_rand(rng, 300), body]))
    # the query end, the reference end and the strand boundary
    for m in (2047, 2048, 2049, 4096, 5003):
        seqs.append(ref[:m].copy())                                   # the query ends inside a round
        seqs.append(np.concatenate([_rand(rng, 211), ref[-m:]]))      # the match runs into the reference end
    rc = _revcomp(ref)
    for m in (2047, 2048, 2049, 3000):
        seqs.append(np.concatenate([ref[-m:], rc[:m]]))               # forward end, then the reverse-complement start
        seqs.append(rc[:m + 500].copy())                              # reverse-complement strand from its start
        seqs.append(np.concatenate([_rand(rng, 97), rc[-m:]]))        # into the end of RR
    # exactly am (7) and am + 1 (8) mismatches in one 15-base window, straddling a 32-base chunk boundary
    for n_mm in (7, 8):
        for c in (32, 64, 2048 - 32, 2048, 2080):
            for off in (-14, -9, -7, -1, 0):
                lo = c + off
                pos = list(range(lo, lo + 15))[:n_mm] if n_mm == 8 else list(range(lo, lo + 15, 2))
                seqs.append(_mutate_at(ref[:c + 900], pos))
    # tandem repeats: every bucket entry of the unit's msl-mers carries the query's tag
    unit = _rand(rng, 23)
    rep = np.tile(unit, 400)
    seqs.append(rep)
    seqs.append(_mutate_at(rep, range(5, len(rep), 61)))
    seqs.append(np.concatenate([_rand(rng, 500), np.tile(unit, 150), ref[:3000]]))
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), offsets


RUN = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from vclust_amd import api
d = np.load(sys.argv[1]); codes, offsets = d['codes'], d['offsets']
gs = api.GenomeSet.from_codes(codes, offsets, ['s%%d' %% i for i in range(len(offsets) - 1)])
tasks = np.array([(q, r) for q in range(len(offsets) - 1) for r in range(len(offsets) - 1) if q != r], dtype=api.TASK_DTYPE)
if sys.argv[3] == 'regions':
    stats, regions = gs.lz_align(tasks, want_regions=True)
else:
    stats = gs.lz_align(tasks)
    np.savez(sys.argv[2], tasks=tasks, stats=stats)
if sys.argv[3] == 'regions':
    np.savez(sys.argv[2], tasks=tasks, stats=stats, regions=regions)
""" % str(ROOT)


@pytest.fixture(scope='module')
def edge_set(tmp_path_factory):
    codes, offsets = _edge_set()
    d = tmp_path_factory.mktemp('edges')
    f = d / 'set.npz'
    np.savez(f, codes=codes, offsets=offsets)
    n = len(offsets) - 1
    tasks = np.array([(q, r) for q in range(n) for r in range(n) if q != r], dtype=[('q', '<u4'), ('r', '<u4')])
    cache = lc.oracle_of(orc, codes, offsets, tasks)              # (q, r) -> (row, regions)
    ref = {k: v[0] for k, v in cache.items()}
    return f, ref, (codes, offsets, cache)


@pytest.mark.parametrize('variant,env,mode', [
    ('fast_one_wave', dict(VG_LZ_SEGMENTS='1'), 'stats'),
    ('fast_segments', dict(VG_LZ_SEGMENTS='4'), 'stats'),
    ('fast_regions', {}, 'regions'),
    ('general', dict(VG_LZ_KERNEL='general', VG_LZ_SEGMENTS='1'), 'stats'),
    ('general_regions', dict(VG_LZ_KERNEL='general'), 'regions'),
])
def test_edge_pairs_match_the_oracle(edge_set, tmp_path, variant, env, mode):
    f, ref, (codes, offsets, cache) = edge_set
    out = tmp_path / f'{variant}.npz'
    p = subprocess.run([sys.executable, '-c', RUN, str(f), str(out), mode], env=dict(os.environ, VG_DEV_SWITCHES='1', **env),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = np.load(out)
    bad = []
    for t, s in zip(d['tasks'], d['stats']):
        got = (int(s['n_match']), int(s['aln_len']), int(s['n_regions']))
        if got != ref[(int(t['q']), int(t['r']))]:
            bad.append((int(t['q']), int(t['r']), ref[(int(t['q']), int(t['r']))], got))
    assert not bad, (len(bad), bad[:5])
    if mode == 'regions':
        lc.assert_rows_and_regions(orc, codes, offsets, d['tasks'], d['stats'], d['regions'], cache=cache, what=variant)
    # the set does reach long extensions: some rows cover more than two rounds of 2 048
    assert int(d['stats']['n_match'].max()) > 4096
