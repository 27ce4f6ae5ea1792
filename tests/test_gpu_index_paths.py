"""Every index-build path of the LZ align stage at both sides of every class limit: rows AND regions against the CPU
oracle (orc.lz_pair_stat, orc.lz_regions), and the index itself (vg_lz_index_dump) against RR restated in numpy (lz_checks.check_index).

The plan (lz_plan_references, vclust_amd/csrc/vg_align.hip) picks the build by n_rr = 2 L + 1: six register builds, mid,
lds, global; pos_bits and tag_bits follow from n_rr and (mal, msl).  LIMIT_LENGTHS are the last length of one class and
the first of the next one, for every limit; TINY are the lengths around msl, mal and reg.  Per length L (default_rng(L)):
a random reference R, `ends(R)` (both ends of both strands of R between random stretches), `mut(R)` (4 % substitutions,
aligned in both directions, so it is a reference of the class too); for a tiny L the query 50 random | R | 50 random.

Each run is ONE child process (developer switches are read once per process; a GPU fault ends the child, not the
suite): it aligns every task with regions, dumps the indexes, and the parent holds them to the oracle.  What keeps the
file from passing vacuously is asserted on the ORACLE's output and on the predicted plan (see _vacuity).

"""
import functools

import numpy as np
import pytest

import lz_checks as lc
import oracle_lib as orc
from vclust_amd import api

pytestmark = pytest.mark.gpu

LIMIT_LENGTHS = sorted({2048 * c - d for c in (4, 8, 12, 16, 20, 24) for d in (129, 128)}
                       | {131071, 131072, 262143, 262144, 1048575, 1048576})
NARROW_LENGTHS = [(1 << 23) - 1, 1 << 23]

WIDE = dict(mal=14, msl=7, mrd=60, mqd=70, reg=50, aw=25, am=12, ar=4)
LONG_31_12 = dict(mal=31, msl=12)
LONG_9_8 = dict(mal=9, msl=8)
SHORT = dict(mal=8, msl=4, reg=10)


def _tiny_lengths(lz):
    p = {**lc.DEFAULT_LZ, **(lz or {})}
    return sorted({1, p['msl'] - 1, p['msl'], p['mal'] - 1, p['mal'], p['reg'] - 1, p['reg'], 64})


class LzSet:
    """genomes, tasks and who is who: per length a dict(L, tiny, R, mut, ends / qry, RN: genome ids)"""

    def __init__(self, lengths, tiny, with_n=False, n_dump_only=False, extra_refs=()):
        seqs, tasks, self.cases = [], [], []

        def add(s):
            seqs.append(s)
            return len(seqs) - 1
        for L in lengths:
            rng = np.random.default_rng(L)
            R = lc.rand_seq(rng, L)
            E = lc.ends_query(rng, R)
            M = lc.mutated(rng, R)
            c = dict(L=L, tiny=False)
            if with_n:
                c['R'], c['mut'], c['ends'] = add(lc.with_n_runs(R)), add(lc.with_n_runs(M)), add(E)
            else:
                c['R'], c['mut'], c['ends'] = add(R), add(M), add(E)
            tasks += [(c['mut'], c['R']), (c['R'], c['mut']), (c['ends'], c['R'])]
            if n_dump_only:
                c['RN'] = add(lc.with_n_runs(R))              # no task names it: its index is dumped
            if L in extra_refs:                               # one more reference of the class (the batch-cut run)
                c['mut2'] = add(lc.mutated(rng, R))
                tasks += [(c['R'], c['mut2']), (c['mut2'], c['R'])]
            self.cases.append(c)
        for L in tiny:
            rng = np.random.default_rng(L)
            R = lc.rand_seq(rng, L)
            c = dict(L=L, tiny=True)
            c['R'], c['qry'] = add(R), add(lc.flanked(rng, R))
            tasks.append((c['qry'], c['R']))
            self.cases.append(c)
        self.codes, self.offsets = lc.pack(seqs)
        self.tasks = np.array(tasks, dtype=api.TASK_DTYPE)
        self.oracle = {}                                      # (q, r) -> (row, regions): shared by the runs of this set

    def seq(self, gi):
        return self.codes[self.offsets[gi]:self.offsets[gi + 1]]

    def references(self):
        return sorted({int(t['r']) for t in self.tasks})


@functools.lru_cache(maxsize=None)
def _set(name):
    if name == 'default':
        return LzSet(LIMIT_LENGTHS, _tiny_lengths(None))
    if name == 'default_n':
        return LzSet(LIMIT_LENGTHS, [], with_n=True)
    if name == 'budget':
        return LzSet(LIMIT_LENGTHS, _tiny_lengths(None), extra_refs=(1048575, 1048576))
    if name == 'wide':
        return LzSet(LIMIT_LENGTHS, _tiny_lengths(WIDE), n_dump_only=True)
    if name == 'long_31_12':
        return LzSet([L for L in LIMIT_LENGTHS if L <= 262144], _tiny_lengths(LONG_31_12), n_dump_only=True)
    if name == 'long_9_8':
        return LzSet([L for L in LIMIT_LENGTHS if L <= 262144], _tiny_lengths(LONG_9_8), n_dump_only=True)
    if name == 'short':
        return LzSet([L for L in LIMIT_LENGTHS if L <= 49024], _tiny_lengths(SHORT), n_dump_only=True)
    if name == 'narrow':
        return LzSet(NARROW_LENGTHS, [])
    raise KeyError(name)


def _vacuity(S, lz, four_ends):
    """Conditions on the ORACLE's regions (they hold whatever the GPU does)."""
    p = {**lc.DEFAULT_LZ, **(lz or {})}
    ref = lc.oracle_of(orc, S.codes, S.offsets, S.tasks, lz, S.oracle)
    seen_tiny = set()
    for c in S.cases:
        L = c['L']
        if c['tiny']:
            row, regs = ref[(c['qry'], c['R'])]
            if lz is None:
                # below reg nothing is kept; from reg on the one region of L matches
                assert row == ((L, L, 1) if L >= p['reg'] else (0, 0, 0)), (L, row)
            seen_tiny.add(len(regs) > 0)
            continue
        regs = ref[(c['ends'], c['R'])][1]
        if four_ends:
            assert 0 in regs['rstart'] and L - 1 in regs['rend'] and L + 1 in regs['rstart'] and 2 * L in regs['rend'], (L, regs)
        for key in ((c['mut'], c['R']), (c['R'], c['mut'])):
            regs = ref[key][1]
            assert len(regs) and int((regs['qend'] - regs['qstart'] + 1).max()) > L // 2, (L, key)
    if lz is None and any(c['tiny'] for c in S.cases):
        assert seen_tiny == {False, True}
    return ref


def _check_plans(S, plans, lz, lds_build=False):
    """every genome whose plan was reported chose the predicted build path, pos_bits and tag_bits"""
    bad = [(gi, len(S.seq(gi)), got, lc.predicted_plan(len(S.seq(gi)), lz, lds_build)) for gi, got in plans.items()
           if got != lc.predicted_plan(len(S.seq(gi)), lz, lds_build)]
    assert not bad, bad[:5]
    return {got[0] for got in plans.values()}, {got[2] for got in plans.values()}


def _check_dumps(S, dumps, lz, what):
    n = 0
    for gi, d in dumps.items():
        n += lc.check_index(S.seq(gi), d, lz, what=f'{what}: genome {gi}, L = {len(S.seq(gi))}')
    return n


def _run(S, tmp_path, name, lz=None, env=None, want_regions=True, dump=(), plan_of=(), budget=0):
    out = lc.run_child(tmp_path, name, S.codes, S.offsets, S.tasks, lz=lz, env=env, want_regions=want_regions, dump=dump,
                       plan_of=plan_of, budget=budget)
    lc.assert_rows_and_regions(orc, S.codes, S.offsets, S.tasks, out['stats'], out['regions'], lz=lz, cache=S.oracle, what=name)
    return out


def _all_refs_and_n(S):
    return S.references() + [c['RN'] for c in S.cases if 'RN' in c]


def test_fast_parse_every_build_path(tmp_path):
    """Default parameters, no N: the FAST parse kernel over the six register builds, mid, lds and global."""
    S = _set('default')
    _vacuity(S, None, four_ends=True)
    refs = S.references()
    out = _run(S, tmp_path, 'fast', dump=[c['R'] for c in S.cases], plan_of=refs)
    paths, tags = _check_plans(S, out['plans'], None)
    assert paths == set(range(9)) and tags == {8}, (paths, tags)
    # both sides of every limit chose different builds
    by_len = {len(S.seq(gi)): p[0] for gi, p in out['plans'].items()}
    for a, b in zip(LIMIT_LENGTHS[0::2], LIMIT_LENGTHS[1::2]):
        assert by_len[a] != by_len[b] or (a, b) == (131071, 131072), (a, b, by_len[a], by_len[b])       # (131 072: pos_bits 18 | 19 only)
    assert _check_dumps(S, out['dumps'], None, 'fast') > 0


def test_lds_build_for_every_length(tmp_path):
    """VG_LZ_BUILD=lds: the scratch-based LDS build also where the register and mid builds would run."""
    S = _set('default')
    _vacuity(S, None, four_ends=True)
    out = _run(S, tmp_path, 'lds', env=dict(VG_LZ_BUILD='lds'), dump=[c['R'] for c in S.cases], plan_of=S.references())
    paths, tags = _check_plans(S, out['plans'], None, lds_build=True)
    assert paths == {lc.PATH_LDS, lc.PATH_GLOBAL} and tags == {8}
    assert _check_dumps(S, out['dumps'], None, 'lds') > 0


def test_general_parse_kernel(tmp_path):
    """The general kernel at default parameters: one wave per pair (rows and regions), then four waves (rows: segments
    emit no regions)."""
    S = _set('default')
    _vacuity(S, None, four_ends=True)
    _run(S, tmp_path, 'general_1', env=dict(VG_LZ_KERNEL='general', VG_LZ_SEGMENTS='1'))
    # (reached only if the first child ended well and matched)
    _run(S, tmp_path, 'general_4', env=dict(VG_LZ_KERNEL='general', VG_LZ_SEGMENTS='4'), want_regions=False)


def test_n_runs_in_reference_and_query(tmp_path):
    """N over bases 0..4, across L / 2 and over the last 10 bases of every R and mut(R): default parameters."""
    S = _set('default_n')
    _vacuity(S, None, four_ends=False)           # (the ends of R are N here)
    out = _run(S, tmp_path, 'n_runs', dump=[c['R'] for c in S.cases], plan_of=S.references())
    paths, tags = _check_plans(S, out['plans'], None)
    assert paths == set(range(9)) and tags == {8}
    assert _check_dumps(S, out['dumps'], None, 'n_runs') > 0


def test_wide_tags_narrowed_by_position_bits(tmp_path):
    """mal 14 / msl 7 asks for 14 tag bits; from 131 072 bases on pos_bits > 18 leaves 13, 12, 11, 10 (13 and 11: odd)."""
    S = _set('wide')
    _vacuity(S, WIDE, four_ends=True)
    out = _run(S, tmp_path, 'wide', lz=WIDE, dump=[c['R'] for c in S.cases] + [c['RN'] for c in S.cases if 'RN' in c],
               plan_of=S.references())
    paths, tags = _check_plans(S, out['plans'], WIDE)
    assert paths == set(range(9)) and tags == {14, 13, 12, 11, 10}, (paths, tags)
    assert [out['plans'][c['R']][2] for c in S.cases if c['L'] == 131072] == [13]
    assert _check_dumps(S, out['dumps'], WIDE, 'wide') > 0


@pytest.mark.parametrize('name,lz,four_ends,tag', [('long_31_12', LONG_31_12, True, {14, 13, 12}), ('long_9_8', LONG_9_8, False, {2})])
def test_long_seeds_global_build(tmp_path, name, lz, four_ends, tag):
    """msl > 7: every reference takes the global build, whatever its length."""
    S = _set(name)
    _vacuity(S, lz, four_ends=four_ends)
    full = [c['R'] for c in S.cases] + [c['RN'] for c in S.cases if 'RN' in c]
    if lz['msl'] == 12:                          # (a 4^12-word table per dump: three lengths, one of them with N, and the tiny ones)
        full = [c['R'] for c in S.cases if c['tiny'] or c['L'] in (8063, 262144)] + [c['RN'] for c in S.cases if c['L'] == 8064]
    out = _run(S, tmp_path, name, lz=lz, dump=full, plan_of=_all_refs_and_n(S))
    paths, tags = _check_plans(S, out['plans'], lz)
    assert paths == {lc.PATH_GLOBAL} and tags == tag, (paths, tags)
    assert _check_dumps(S, out['dumps'], lz, name) > 0


def test_short_seeds_register_builds(tmp_path):
    """mal 8 / msl 4 / reg 10 on the six register classes and the first mid length (49 024): 256 long buckets, 8 tag bits."""
    S = _set('short')
    _vacuity(S, SHORT, four_ends=False)          # (short seeds find chance matches first: the four ends are not promised)
    out = _run(S, tmp_path, 'short', lz=SHORT, dump=[c['R'] for c in S.cases] + [c['RN'] for c in S.cases if 'RN' in c],
               plan_of=S.references())
    paths, tags = _check_plans(S, out['plans'], SHORT)
    assert paths == set(range(7)) and tags == {8}, (paths, tags)
    assert _check_dumps(S, out['dumps'], SHORT, 'short') > 0


def _ref_need(L, msl=7):
    """lz_ref_need restated: bytes of one reference's share of the index pools"""
    n_rr = 2 * L + 1
    chunks = (n_rr + 128 + 31) // 32 + 2
    return chunks * 12 + (4 ** msl + n_rr) * 4


def test_batches_cut_inside_the_set(tmp_path):
    """The smallest index budget the library takes: the references of the set need more, so the pools are reused by
    several batches (offsets of a later batch start at zero again)."""
    S = _set('budget')
    budget = (64 << 20) + 1
    needs = [_ref_need(len(S.seq(gi))) for gi in S.references()]
    assert sum(needs) > budget > max(needs)       # at least two batches, and every reference fits one
    _vacuity(S, None, four_ends=True)
    _run(S, tmp_path, 'budget', budget=budget)


def test_narrow_tags_at_the_defaults(tmp_path):
    """2^23 - 1 and 2^23 bases: a genome >= 2^22 sends the call to the general kernel; pos_bits 24 | 25 leaves 8 | 7 tag
    bits at the default parameters (7: three and a half bases)."""
    S = _set('narrow')
    _vacuity(S, None, four_ends=True)
    out = _run(S, tmp_path, 'narrow', dump=[c['R'] for c in S.cases], plan_of=S.references())
    paths, tags = _check_plans(S, out['plans'], None)
    assert paths == {lc.PATH_GLOBAL} and tags == {8, 7}, (paths, tags)
    assert _check_dumps(S, out['dumps'], None, 'narrow') > 0
