"""The register builds' trips of four positions (build_ref_reg, vclust_amd/csrc/vg_align.hip): a trip whose four positions
are valid in every lane of its wave runs without a test per position, every other trip -- at the separator, at the end of
RR, at an N -- takes the general path, and the slot pass reuses that decision.  So the inputs put the separator (RR
position L) and the end of RR (2 L + 1) at every offset inside a trip and on the 32-base chunk boundaries, and single Ns
and N runs at the places where the two paths meet; N-free and N-carrying references alternate inside every launch.

Per parameter set ONE child process (lz_checks.run_child): it aligns every task with regions and dumps the index of every
reference; the parent holds rows and regions to the CPU oracle, every index to lz_checks.check_index and every plan to
lz_checks.predicted_plan.  What keeps the file from passing vacuously is asserted on the inputs, on the oracle's output
and on the predicted plans (_inputs_cover), not on the device.

Lengths: in the two smallest register classes (4 and 8 trips) L mod 32 in {0, 1, 2, 3, 30, 31} -- every residue of
L mod 4, and L mod 32 in {0, 1, 31} --, one length inside each of the other four classes (all below 49 kb).  Every length
comes as R (N-free) and RN (R with one of N_PLACEMENTS), each with a 4 % mutated copy aligned in both directions, so the
copies are references of the class too.

Parameters: the defaults, WIDE (mal 14 / msl 7: 14 tag bits), SHORT (mal 8 / msl 4) and TIGHT (mal 8 / msl 7: 2 tag bits).
Zero tag bits need mal == msl, and the parameter check admits mal >= 8 only while the register builds take msl <= 7:
no register build ever runs without tag bits, and TIGHT is the nearest set that is admitted.  MSL_5 and MSL_6 are the
seed lengths between SHORT and the defaults, with 8 and 14 tag bits.
"""
import numpy as np
import pytest

import lz_checks as lc
import oracle_lib as orc
from vclust_amd import api

pytestmark = pytest.mark.gpu

WIDE = dict(mal=14, msl=7, mrd=60, mqd=70, reg=50, aw=25, am=12, ar=4)
SHORT = dict(mal=8, msl=4, reg=10)
TIGHT = dict(mal=8, msl=7)
MSL_5 = dict(mal=9, msl=5, reg=12)
MSL_6 = dict(mal=13, msl=6)

RESIDUES = (0, 1, 2, 3, 30, 31)
SMALL_BASES = (2976, 12000)            # multiples of 32 inside the classes of 4 trips (L <= 8 063) and 8 trips (L <= 16 255)
OTHER_LENGTHS = (20011, 28005, 36002, 45003)          # 12, 16, 20 and 24 trips


def _single(at):
    return lambda L: [at(L)]


# name -> the N positions of a reference of L bases
N_PLACEMENTS = {
    'first': _single(lambda L: 0),
    'last_of_trip': _single(lambda L: 3),
    'first_of_trip': _single(lambda L: 4),
    'end_minus_8': _single(lambda L: L - 8),
    'end_minus_7': _single(lambda L: L - 7),
    'last': _single(lambda L: L - 1),
    'run_over_trip': lambda L: list(range(1018, 1023)),          # across 1 020: a multiple of 4 that is none of 32
    'run_over_chunk': lambda L: list(range(2044, 2052)),         # across 2 048: a multiple of 32
}


def _with_n(s, where):
    s = s.copy()
    s[np.asarray(where)] = 4
    return s


class TripSet:
    """genomes, tasks and per reference length a dict(L, R, RN, placement, mut, mutN: genome ids)"""

    def __init__(self):
        seqs, tasks, self.cases = [], [], []
        names = list(N_PLACEMENTS)

        def add(s):
            seqs.append(s)
            return len(seqs) - 1
        lengths = [b + r for b in SMALL_BASES for r in RESIDUES] + list(OTHER_LENGTHS)
        for k, L in enumerate(lengths):
            rng = np.random.default_rng(L)
            R = lc.rand_seq(rng, L)
            name = names[k % len(names)]
            RN = _with_n(R, N_PLACEMENTS[name](L))
            c = dict(L=L, placement=name)
            # N-free and N-carrying references alternate in genome order, which is the order of a launch's list
            c['R'], c['RN'] = add(R), add(RN)
            c['mut'], c['mutN'] = add(lc.mutated(rng, R)), add(_with_n(lc.mutated(rng, R), N_PLACEMENTS[name](L)))
            tasks += [(c['mut'], c['R']), (c['R'], c['mut']), (c['mutN'], c['RN']), (c['RN'], c['mutN'])]
            self.cases.append(c)
        self.codes, self.offsets = lc.pack(seqs)
        self.tasks = np.array(tasks, dtype=api.TASK_DTYPE)
        self.oracle = {}

    def seq(self, gi):
        return self.codes[self.offsets[gi]:self.offsets[gi + 1]]

    def references(self):
        return sorted({int(t['r']) for t in self.tasks})


def _inputs_cover(S, lz):
    """Conditions on the inputs, the predicted plans and the ORACLE's regions (they hold whatever the GPU does)."""
    refs = S.references()
    assert 56 <= len(refs) <= 80 and max(len(S.seq(g)) for g in refs) <= 49000
    has_n = {g: bool((S.seq(g) > 3).any()) for g in refs}
    by_class = {}
    for g in refs:
        by_class.setdefault(lc.predicted_plan(len(S.seq(g)), lz)[0], set()).add(has_n[g])
    assert by_class == {path: {False, True} for path in range(6)}, by_class        # every class, both kinds in each
    # N-free and N-carrying references alternate in the order the launches list them
    assert all(has_n[a] != has_n[b] for a, b in zip(refs[0::2], refs[1::2]))
    for path in (4, 5):                                                             # the two smallest classes
        Ls = {len(S.seq(g)) for g in refs if lc.predicted_plan(len(S.seq(g)), lz)[0] == path}
        assert {L % 4 for L in Ls} == {0, 1, 2, 3} and {0, 1, 31} <= {L % 32 for L in Ls}, (path, sorted(Ls))
    # every placement is used, lies where its name says and leaves the other bases alone
    assert {c['placement'] for c in S.cases} == set(N_PLACEMENTS)
    for c in S.cases:
        at = np.flatnonzero(S.seq(c['RN']) > 3)
        assert at.tolist() == sorted(N_PLACEMENTS[c['placement']](c['L'])) and not (S.seq(c['R']) > 3).any()
    runs = {c['placement']: N_PLACEMENTS[c['placement']](c['L']) for c in S.cases}
    assert any(p % 4 == 0 and p % 32 != 0 for p in runs['run_over_trip'][1:]) and any(p % 32 == 0 for p in runs['run_over_chunk'][1:])
    ref = lc.oracle_of(orc, S.codes, S.offsets, S.tasks, lz, S.oracle)
    for t in S.tasks:                                                               # every task aligns: rows and regions say something
        assert len(ref[(int(t['q']), int(t['r']))][1]) > 0, (int(t['q']), int(t['r']))
    return ref


@pytest.mark.parametrize('name,lz,tag_bits', [('default', None, 8), ('wide', WIDE, 14), ('short', SHORT, 8), ('tight', TIGHT, 2),
                                              ('msl_5', MSL_5, 8), ('msl_6', MSL_6, 14)])
def test_trips_at_separator_end_and_n(tmp_path, name, lz, tag_bits):
    S = TripSet()
    _inputs_cover(S, lz)
    refs = S.references()
    out = lc.run_child(tmp_path, name, S.codes, S.offsets, S.tasks, lz=lz, dump=refs, plan_of=refs)
    lc.assert_rows_and_regions(orc, S.codes, S.offsets, S.tasks, out['stats'], out['regions'], lz=lz, cache=S.oracle, what=name)
    bad = [(g, len(S.seq(g)), got, lc.predicted_plan(len(S.seq(g)), lz)) for g, got in out['plans'].items()
           if got != lc.predicted_plan(len(S.seq(g)), lz)]
    assert not bad, bad[:5]
    assert {p[0] for p in out['plans'].values()} == set(range(6)) and {p[2] for p in out['plans'].values()} == {tag_bits}
    assert sorted(out['dumps']) == refs
    n = 0
    for g, d in out['dumps'].items():
        n += lc.check_index(S.seq(g), d, lz, what=f'{name}: genome {g}, L = {len(S.seq(g))}')
    assert n > 0
