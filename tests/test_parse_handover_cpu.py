"""The rule the four-wave LZ parse rests on, checked on the CPU oracle alone (no GPU): a wave that starts at w * seg_len
with an empty state and the parse that came from the left are THE SAME PARSE from the first event (i, j) both place once
both open regions span >= reg.  For a query Q, a reference R, E = the oracle's events of the whole parse and F_w = those
of the parse from w * seg_len (oracle_lib.lz_events), handover_lib asserts

  (a) behind every event that two of these parses share with span_ok in both, their event lists are identical in (i, j);
  (b) the differences of the virtual sums VM, VA, VN stay constant mod 2^32 from there to the end (and the rows the two
      parses end with differ by the same constants);
  (c) the kernel's scheme restated in plain Python -- segment geometry, logs of 250 events, lookup by cursor in the log of
      segment min(3, ev_i // seg_len), hand-over at the first common span_ok event, the final sums -- gives
      orc.lz_pair_stat(Q, R), whether the event that crosses the end of a segment is logged (wide probe), is not (narrow
      probe), or is when the kernel's probe widths (64, 32 after an event) reach it.

Everything is integer equality.  Inputs: the pairs built to reach the arms of the hand-over (handover_lib.adversarial_set:
the ones test_gpu_parse_handover.py runs on the GPU, whose conditions are checked here too), families of ragged lengths
at four divergences, with N runs, and under three non-default parameter sets."""
import numpy as np
import pytest

import handover_lib as hl
import oracle_lib as orc
from vclust_amd import synth

# non-default parameter sets of test_gpu_parity_random.py::test_non_default_lz_parameters: mqd above mrd; reg = 1 (every
# region is kept, every event has span_ok); short anchors and seeds; the first is the one the GPU test runs
PARAMETER_SETS = [
    dict(mal=14, msl=7, mrd=60, mqd=70, reg=50, aw=25, am=12, ar=4),
    dict(mal=16, msl=5, mrd=10, mqd=5, reg=1, aw=3, am=0, ar=3),
    dict(mal=9, msl=6, mrd=20, mqd=30, reg=20, aw=10, am=4, ar=2),
]
GPU_PARAMETERS = PARAMETER_SETS[0]

TALLY = dict(pairs=0, split_pairs=0, pair_waves=0, couples=0, chains=0)


def _check(Q, R, lz, what):
    F, couples, chains = hl.check_pair(Q, R, lz, what)
    split = hl.geometry(len(Q), hl.params(lz)['mal'])[1]
    TALLY['pairs'] += 1
    TALLY['split_pairs'] += int(split)
    TALLY['pair_waves'] += (hl.WAVES - 1) if split else 0        # (pair, wave w >= 1): F_w against E and against the other waves
    TALLY['couples'] += couples
    TALLY['chains'] += len(chains)
    return F, chains


@pytest.mark.parametrize('form', ['fast', 'n', 'parameters'])
def test_adversarial_pairs_obey_the_rule_and_reach_every_arm(form):
    lz = GPU_PARAMETERS if form == 'parameters' else None
    seqs, cases = hl.adversarial_set(lz, with_n=(form == 'n'))
    F_of = {}
    for c in cases:
        F_of[c['name']], _ = _check(seqs[c['q']], seqs[c['r']], lz, (form, c['name']))
        _check(seqs[c['r']], seqs[c['q']], lz, (form, c['name'], 'reference and query swapped'))
    arms = hl.arms_reached(seqs, cases, lz, F_of)
    missing = [a for a in hl.ARMS + ((hl.ARM_N,) if form == 'n' else ()) if not arms[a]]
    assert not missing, (form, 'no pair meets the condition of', missing)


@pytest.mark.parametrize('form', ['fast', 'parameters'])
@pytest.mark.parametrize('side', ['looker_ok', 'owner_ok'])
def test_each_side_of_the_span_ok_condition_is_needed(form, side):
    """the restated chain WITHOUT the span_ok test of the looking wave, or of the owner of the log, leaves the oracle's row on
    a pair of the set: these pairs can tell a kernel that forgets either"""
    lz = GPU_PARAMETERS if form == 'parameters' else None
    seqs, cases = hl.adversarial_set(lz)
    wrong = []
    for c in cases:
        Q, R = seqs[c['q']], seqs[c['r']]
        if hl.chain(len(Q), hl.parses(Q, R, lz), lz, **{side: False})['row'] != orc.lz_pair_stat(Q, R, lz):
            wrong.append(c['name'])
    assert wrong, (form, side, 'a hand-over at an event where one region does not span reg yet went unnoticed')


@pytest.mark.parametrize('form', ['fast', 'parameters'])
def test_a_lookup_that_misses_records_delays_the_hand_over_and_nothing_else(form):
    """Shorter logs (down to none) and a cursor that is not reset between segments skip records of the owner; by (a) and
    (b) every later common event serves as well, so the row stays the oracle's.  (That is why no row can tell such a
    kernel from the right one: these arms cost time, not results.)"""
    lz = GPU_PARAMETERS if form == 'parameters' else None
    seqs, cases = hl.adversarial_set(lz)
    moved = 0
    for c in cases:
        Q, R = seqs[c['q']], seqs[c['r']]
        F = hl.parses(Q, R, lz)
        row = orc.lz_pair_stat(Q, R, lz)
        full = hl.chain(len(Q), F, lz)
        for kw in (dict(cap=0), dict(cap=1), dict(cap=200), dict(reset_cursor=False), dict(cap=200, reset_cursor=False)):
            got = hl.chain(len(Q), F, lz, **kw)
            assert got['row'] == row, (form, c['name'], kw, got['row'], row)
            moved += got['sync'] != full['sync']
    assert moved > 10, 'the variants never changed a hand-over: the set does not exercise them'


def _family_pairs(codes, offsets, n_families, members, lz, what, max_pairs=None):
    n = 0
    for f in range(n_families):
        for a in range(members):
            for b in range(members):
                if a != b and (max_pairs is None or n < max_pairs):
                    q, r = f * members + a, f * members + b
                    _check(codes[offsets[q]:offsets[q + 1]], codes[offsets[r]:offsets[r + 1]], lz, (what, q, r))
                    n += 1
    return n


@pytest.mark.parametrize('p_hi', [0.05, 0.1, 0.2, 0.3])
def test_ragged_families(p_hi):
    codes, offsets, _ = synth.make_families(10, 3, seed=int(p_hi * 100), length_range=(8150, 40000), p_hi=p_hi)
    assert _family_pairs(codes, offsets, 10, 3, None, ('families', p_hi)) == 60


def test_ragged_families_with_n_runs():
    rng = np.random.default_rng(7)
    codes, offsets, _ = synth.make_families(6, 3, seed=7, length_range=(8150, 40000), p_hi=0.2)
    codes = codes.copy()
    for _ in range(60):
        p = int(rng.integers(0, len(codes) - 60))
        codes[p:p + int(rng.integers(1, 50))] = 4
    _family_pairs(codes, offsets, 6, 3, None, 'families with N')


@pytest.mark.parametrize('lz', PARAMETER_SETS, ids=lambda lz: 'mal%d_reg%d_mqd%d' % (lz['mal'], lz['reg'], lz['mqd']))
def test_non_default_parameters(lz):
    codes, offsets, _ = synth.make_families(5, 3, seed=11, length_range=(8150, 30000), p_hi=0.25)
    _family_pairs(codes, offsets, 5, 3, lz, ('parameters', lz['mal']))


def test_unrelated_and_repetitive_queries():
    """nothing to hand over (unrelated), and buckets full of candidates (a tandem repeat, mutated)"""
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 4, 12000).astype(np.uint8), rng.integers(0, 4, 9000).astype(np.uint8)
    rep = np.tile(rng.integers(0, 4, 37).astype(np.uint8), 300)
    rep2 = rep.copy()
    rep2[rng.random(len(rep2)) < 0.03] = 1
    dup = np.concatenate([a[:5000], a[2000:7000], a[:3000]])
    for what, (Q, R) in dict(unrelated=(a, b), repeat=(rep2, rep), repeat_back=(rep, rep2), duplicated=(dup, a), duplicated_back=(a, dup)).items():
        _check(Q, R, None, what)


def test_start_zero_is_the_ordinary_parse_and_the_sums_are_the_regions():
    rng = np.random.default_rng(3)
    R = rng.integers(0, 4, 9000).astype(np.uint8)
    Q = R.copy()
    Q[rng.random(len(Q)) < 0.05] = 2
    for b in range(150, len(Q) - 20, 150):          # ten mismatches in a row end the approximate extension: an event behind each
        Q[b:b + 10] = (R[b:b + 10] + 1) % 4
    ev, row = orc.lz_events(Q, R, 0, with_row=True)
    regs = orc.lz_regions(Q, R)
    assert row == orc.lz_pair_stat(Q, R) == (int(regs['n_match'].sum()), int((regs['qend'] - regs['qstart'] + 1).sum()), len(regs))
    assert len(ev) > 20 and np.all(np.diff(ev['ev_i']) > 0) and np.all(ev['ev_end'] > ev['ev_i'])
    # VN counts the regions kept so far: it ends at the row's, or one below while the last region is still open
    assert int(ev['VN'][-1]) in (row[2], row[2] - 1) and np.all(np.diff(ev['VN'].astype(np.int64)) >= 0)
    # a later start sees nothing in front of it
    ev2 = orc.lz_events(Q, R, 4000)
    assert len(ev2) and int(ev2['ev_i'][0]) >= 4000


def test_tally():
    """(runs last in this file) the sizes the checks above ran on; printed with -s"""
    print('pairs %(pairs)d, of them split %(split_pairs)d; (pair, wave) combinations %(pair_waves)d; couples of parses with a '
          'common event (a, b) %(couples)d; restated chains (c) %(chains)d' % TALLY)
    if TALLY['pairs'] > 100:          # the whole file ran
        assert TALLY['split_pairs'] > 100 and TALLY['couples'] > 300 and TALLY['chains'] == 3 * TALLY['pairs'], TALLY
