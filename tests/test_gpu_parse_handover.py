"""The hand-over between the segments of the four-wave LZ parse (k_lz_parse_seg_fast / k_lz_parse_seg, lz_parse_body<4, ...>)
against the CPU oracle, on pairs built to reach each of its arms (handover_lib.adversarial_set).

One small set is loaded with api.GenomeSet.from_codes and aligned with gs.lz_align(tasks) -- the product's default: far
fewer than 32 768 tasks, so four waves per pair without any developer switch -- and again with want_regions=True, the
one-wave parse.  Every row of both calls equals orc.lz_pair_stat; the regions go through lz_checks.assert_rows_and_regions.
Three forms:

  fast        no N, default parameters: k_lz_parse_seg_fast;
  n           one more genome that holds N (a run across a segment boundary of its query): the whole call takes
              k_lz_parse_seg;
  parameters  mal 14, msl 7, mrd 60, mqd 70, reg 50, aw 25, am 12, ar 4: k_lz_parse_seg, and lim and seg_len move
              (the set is built for the parameters: breaks, islands and gaps follow am, mal, mqd and reg).

The profile scopes do not tell the parse kernels apart (all run under "lz_parse"), so every form runs a second time in a
child process with VG_DEV_SWITCHES=1 VG_LZ_SEGMENTS=4 (and VG_LZ_KERNEL=general for the two general forms), which names the
kernel whatever the task count.

BEFORE the GPU is asked anything, every arm is proved reached from the oracle's events (handover_lib.arms_reached; E = the
events of the whole parse, F_w = of the parse wave w starts, `chain` = the kernel's scheme restated):

  split threshold          queries of mal + 8191, mal + 8192, mal + 8193 bases: no split, seg_len 2048, seg_len 2112 with a
                           short last segment
  immediate hand-over      the first event of E inside segment w is a common span_ok event, for w = 1, 2, 3
  refused by span_ok       E and F_w share >= 20 events inside segment w before their first common span_ok event
  ... of the owner alone   one of the shared events has span_ok in E and not in F_w (the owner meets a region too late to
                           keep it: handing over there would lose the region)
  ... of the looking wave  one of them has span_ok in F_w and not in E (E's region cannot reach back into the region it kept
  alone                    just before, F_w's can; E drops it, F_w keeps it: handing over there would add a region)
  late hand-over           the first common span_ok event has index 20 .. 200 in F_w, inside segment w
  log cap                  it has index >= 252 in F_w and lies inside segment w, and F_w has >= 252 events that start before
                           (w + 1) * seg_len: the wave goes on into segment w + 1
  a wave is skipped        the chain visits wave 0, then a wave >= 2 (under every probe width)
  empty log                some F_w has no event that starts inside its own segment
  no hand-over at all      the chain ends at wave 0, and E has events in the last segment
  boundary                 E has an event with ev_i == w * seg_len, an exact match of more than seg_len bases across one
                           boundary and one of more than 2 * seg_len bases across two
  strands                  consecutive span_ok events of E change strand at a boundary, within 64 bases in front of one and
                           within 64 bases behind one
  N (form n)               an N run lies across a segment boundary of a split query
"""
import functools

import numpy as np
import pytest

import handover_lib as hl
import lz_checks as lc
import oracle_lib as orc
from vclust_amd import api

pytestmark = pytest.mark.gpu

PARAMETERS = dict(mal=14, msl=7, mrd=60, mqd=70, reg=50, aw=25, am=12, ar=4)
FORMS = {
    'fast': dict(lz=None, with_n=False, env=dict(VG_LZ_SEGMENTS='4')),
    'n': dict(lz=None, with_n=True, env=dict(VG_LZ_SEGMENTS='4', VG_LZ_KERNEL='general')),
    'parameters': dict(lz=PARAMETERS, with_n=False, env=dict(VG_LZ_SEGMENTS='4', VG_LZ_KERNEL='general')),
}


@functools.lru_cache(maxsize=None)
def _form(name):
    """the set of a form, its tasks (every pair in both directions) and the oracle's verdict on the arms -- no GPU here"""
    f = FORMS[name]
    seqs, cases = hl.adversarial_set(f['lz'], f['with_n'])
    codes, offsets = lc.pack(seqs)
    tasks = np.array([(c['q'], c['r']) for c in cases] + [(c['r'], c['q']) for c in cases], dtype=api.TASK_DTYPE)
    arms = hl.arms_reached(seqs, cases, f['lz'])
    cache = {}
    lc.oracle_of(orc, codes, offsets, tasks, f['lz'], cache)
    return codes, offsets, tasks, arms, cache, seqs


def _assert_arms(name):
    codes, offsets, tasks, arms, cache, seqs = _form(name)
    wanted = hl.ARMS + ((hl.ARM_N,) if FORMS[name]['with_n'] else ())
    missing = [a for a in wanted if not arms[a]]
    assert not missing, (name, 'no pair of the set meets the condition of', missing)
    if FORMS[name]['with_n']:
        assert any(np.any(s > 3) for s in seqs)
    else:
        assert not np.any(codes > 3)
    # the split queries are the small ones the arms need
    assert max(len(s) for s in seqs) <= 100000 and len(tasks) <= 40


def _assert_rows(name, tasks, stats, cache, what):
    assert len(stats) == len(tasks)
    bad = []
    for t, s in zip(tasks, stats):
        key = (int(t['q']), int(t['r']))
        got = (int(s['n_match']), int(s['aln_len']), int(s['n_regions']))
        if got != cache[key][0]:
            bad.append((key, cache[key][0], got))
    assert not bad, (name, what, len(bad), bad[:5])


@pytest.mark.parametrize('name', list(FORMS))
def test_default_call_matches_the_oracle(name):
    """gs.lz_align(tasks): four waves by the task count alone; and the one-wave parse that writes regions"""
    _assert_arms(name)
    codes, offsets, tasks, arms, cache, seqs = _form(name)
    lz = FORMS[name]['lz']
    gs = api.GenomeSet.from_codes(codes, offsets)
    stats = gs.lz_align(tasks, lz=lz)
    _assert_rows(name, tasks, stats, cache, 'four waves')
    stats1, regions = gs.lz_align(tasks, lz=lz, want_regions=True)
    _assert_rows(name, tasks, stats1, cache, 'one wave, regions')
    lc.assert_rows_and_regions(orc, codes, offsets, tasks, stats1, regions, lz=lz, cache=cache, what=name)


@pytest.mark.parametrize('name', list(FORMS))
def test_named_kernel_matches_the_oracle(name, tmp_path):
    """the same set in a child process whose switches name the four-wave kernel of the form"""
    _assert_arms(name)
    codes, offsets, tasks, arms, cache, seqs = _form(name)
    out = lc.run_child(tmp_path, name, codes, offsets, tasks, lz=FORMS[name]['lz'], env=FORMS[name]['env'], want_regions=False, timeout=120)
    _assert_rows(name, tasks, out['stats'], cache, FORMS[name]['env'])
