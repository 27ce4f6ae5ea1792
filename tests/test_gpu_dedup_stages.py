"""The launch structure of a deduplicate call per mode, read from the profile table (one entry per scope name, `launches` =
how often the scope was opened): which stages run, how often per round, pass and slice, and which never run in a mode.
The counts are equalities against the stats the call returns; where a count is not a function of the stats, the constant
is the one the commit before the host-side reshaping showed for that input.  Results are held to the restatements."""
import numpy as np
import pytest

import dedup_circular_restatement as dcr
import dedup_contained_restatement as dcn
import dedup_restatement as dr
import dedup_trepeat_restatement as dtr
from test_gpu_dedup_contained import changed, rand, random_set

pytestmark = pytest.mark.gpu

LENGTHS = (33, 16390)        # below one word-aligned window; two verify chunks of 2 048 words and 6 symbols
PLAIN_ONLY = {'dedup_hash', 'dedup_verify'}
CIRCULAR_ONLY = {'dedup_chash', 'dedup_ccand', 'dedup_cverify'}
REPEAT_ONLY = {'dedup_trepeat', 'dedup_trim'}


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


@pytest.fixture
def knobs(api):
    yield api
    api.dedup_set_hash_bits(128)
    api.dedup_set_anchor_symbols(16)
    api.dedup_set_index_positions(0)


def profiled(api, call):
    """-> (what call() returns, {scope name: launches})"""
    api.profile_enable(True)
    api.profile_reset()
    try:
        out = call()
        scopes = {e['name']: e['launches'] for e in api.profile_get()}
    finally:
        api.profile_enable(False)
    print(scopes, out[-1] if isinstance(out, tuple) else '')
    return out, scopes


def plain_set():
    """40 records of two lengths: per length 8 originals, 4 copies (one in lower case), 3 reverse complements and 5 near
    misses (first, last and a middle symbol changed, one of them reverse-complemented), shuffled."""
    rng = np.random.default_rng(7)
    seqs = []
    for L in LENGTHS:
        o = [rand(rng, L) for _ in range(8)]
        seqs += o + [o[0], o[1], o[1].lower(), o[7]] + [dr.revcomp(o[0]), dr.revcomp(o[2]), dr.revcomp(o[3])]
        seqs += [changed(o[0], 0), changed(o[0], L - 1), changed(o[4], L // 2), dr.revcomp(changed(o[5], 9)), changed(o[6], L - 9)]
    return [seqs[int(k)] for k in rng.permutation(len(seqs))]


def circular_set(overlap=False):
    """plain_set() and, per length, three rotations and two rotated reverse complements of its records; overlap: half of all
    records get the first 0, 21, 55 or 127 symbols again at their end (the shorter ones at most a third of their length)."""
    rng = np.random.default_rng(8)
    seqs = plain_set()
    for L in LENGTHS:
        own = [s for s in seqs if len(s) == L]
        for k in range(5):
            s = own[int(rng.integers(0, len(own)))]
            r = dcr.rot(s, int(rng.integers(1, L)))
            seqs.append(dr.revcomp(r) if k >= 3 else r)
    seqs = [seqs[int(k)] for k in rng.permutation(len(seqs))]
    if overlap:
        seqs = [s + s[:min((0, 21, 55, 127)[i % 4], len(s) // 3)] if i % 2 else s for i, s in enumerate(seqs)]
    return seqs


def passes_set():
    """the 40 records of test_gpu_dedup_contained.test_several_index_passes"""
    return random_set(np.random.default_rng(51), 40)


def flood_set():
    """the 200 records of test_gpu_dedup_contained's flood_set fixture"""
    return random_set(np.random.default_rng(50), 200)


@pytest.fixture(scope='module')
def plain_case():
    seqs = plain_set()
    return seqs, dr.run_seqs(seqs)


@pytest.fixture(scope='module')
def circular_case():
    seqs = circular_set()
    return seqs, dcr.run_seqs(seqs)


@pytest.fixture(scope='module')
def repeat_case():
    seqs = circular_set(overlap=True)
    return seqs, dtr.run_seqs(seqs, 20)


def check_rounds(scopes, st, mode_only):
    """what the plain and the circular mode share: one hash, one key and one sort stage, then per round the runs and the
    labels, and a compaction between two rounds"""
    rounds = st['rounds']
    assert scopes['dedup_keys'] == 1 and scopes['dedup_sort'] == 1
    assert scopes['dedup_runs'] == scopes['dedup_labels'] == rounds >= 1
    assert scopes.get('dedup_compact', 0) == rounds - 1 and ('dedup_compact' in scopes) == (rounds > 1)
    assert not [name for name in scopes if name.startswith('dedupc_')]
    assert not (set(scopes) & ((PLAIN_ONLY | CIRCULAR_ONLY | REPEAT_ONLY) - mode_only))


# dedup_verify opens only in a round with a member to compare: a function of the input, not of the stats.  The counts are
# the parent commit's for plain_set(): one round at 128 bits; at 0 bits every record of a length is one run, 13 rounds peel
# the groups off and the last one finds heads only.
VERIFY_128, VERIFY_0 = 1, 12


@pytest.mark.parametrize('bits', [128, 0])
def test_plain_stages(knobs, plain_case, bits):
    seqs, (erep, estrand) = plain_case
    knobs.dedup_set_hash_bits(bits)
    (rep, strand, st), scopes = profiled(knobs, lambda: knobs.deduplicate(seqs))
    assert rep.tolist() == erep and strand.tolist() == estrand
    assert scopes['dedup_hash'] == 1
    check_rounds(scopes, st, PLAIN_ONLY)
    assert 1 <= scopes['dedup_verify'] <= st['rounds']
    assert scopes['dedup_verify'] == (VERIFY_0 if bits == 0 else VERIFY_128)
    assert (st['rounds'] > 1 and st['collisions'] > 0) if bits == 0 else (st['rounds'] == 1 and st['collisions'] == 0)


# as above for circular_set(): dedup_cverify opens only in a round with a candidate offset (parent commit's counts)
CVERIFY_128, CVERIFY_0 = 1, 10


@pytest.mark.parametrize('bits', [128, 0])
def test_circular_stages(knobs, circular_case, bits):
    seqs, (erep, estrand, eoffset) = circular_case
    knobs.dedup_set_hash_bits(bits)
    (rep, strand, offset, st), scopes = profiled(knobs, lambda: knobs.deduplicate(seqs, circular=True))
    assert rep.tolist() == erep and strand.tolist() == estrand and offset.tolist() == eoffset
    assert scopes['dedup_chash'] == 1
    check_rounds(scopes, st, CIRCULAR_ONLY)
    assert scopes['dedup_ccand'] == st['rounds']
    assert scopes['dedup_cverify'] <= st['rounds']
    assert scopes['dedup_cverify'] == (CVERIFY_0 if bits == 0 else CVERIFY_128)
    assert st['rounds'] > 1 if bits == 0 else st['rounds'] == 1


def test_circular_all_unique_compares_nothing(api):
    rng = np.random.default_rng(9)
    seqs = [rand(rng, L) for L in LENGTHS for _ in range(6)]
    (rep, strand, offset, st), scopes = profiled(api, lambda: api.deduplicate(seqs, circular=True))
    assert rep.tolist() == list(range(len(seqs))) and st['rounds'] == 1
    check_rounds(scopes, st, CIRCULAR_ONLY)
    assert scopes['dedup_chash'] == scopes['dedup_ccand'] == 1 and 'dedup_cverify' not in scopes


def test_terminal_repeat_stages(api, repeat_case):
    seqs, (erep, estrand, eoffset, erepeat) = repeat_case
    (rep, strand, offset, st), scopes = profiled(api, lambda: api.deduplicate(seqs, circular=True, terminal_repeat=20))
    assert rep.tolist() == erep and strand.tolist() == estrand and offset.tolist() == eoffset and st['repeat'].tolist() == erepeat
    assert st['with_repeat'] >= len(seqs) // 4 and st['removed'] > 10
    assert scopes['dedup_chash'] == 1 and scopes['dedup_trepeat'] == 1 and scopes['dedup_trim'] == 1
    check_rounds(scopes, st, CIRCULAR_ONLY | REPEAT_ONLY)
    assert scopes['dedup_ccand'] == st['rounds'] and scopes['dedup_cverify'] == CVERIFY_128 <= st['rounds']     # (the parent commit's, again)
    # the pass alone: its two scopes and nothing else, and the same repeats
    repeat, scopes = profiled(api, lambda: api.terminal_repeats(seqs, 20))
    assert scopes == {'dedup_trepeat': 1, 'dedup_trim': 1}
    assert repeat.tolist() == st['repeat'].tolist() == erepeat


# dedupc_verify and dedupc_pick open once per slice with a candidate (parent commit's counts for the two inputs)
CONTAINED_VERIFY = {'passes': 8, 'flood': 13}


@pytest.mark.parametrize('which', ['passes', 'flood'])
def test_contained_stages(knobs, which):
    seqs = passes_set() if which == 'passes' else flood_set()
    if which == 'passes':
        knobs.dedup_set_index_positions(1000)
    else:
        knobs.dedup_set_anchor_symbols(1)
    (rep, strand, offset, st), scopes = profiled(knobs, lambda: knobs.deduplicate(seqs, contained=True))
    assert (rep.tolist(), strand.tolist(), offset.tolist()) == dcn.run_seqs(seqs)
    assert st['passes'] == (sum(map(len, seqs)) + 999) // 1000 if which == 'passes' else st['slices'] > st['passes'] == 1
    assert scopes['dedupc_windows'] == scopes['dedupc_sort'] == st['passes']
    assert scopes['dedupc_lookup'] == st['passes'] + st['slices']
    assert scopes['dedupc_verify'] == scopes['dedupc_pick'] == CONTAINED_VERIFY[which] <= st['slices']
    assert set(scopes) == {'dedupc_windows', 'dedupc_sort', 'dedupc_lookup', 'dedupc_verify', 'dedupc_pick'}


def test_empty_input_opens_no_scope(api):
    calls = {'plain': lambda: api.deduplicate([]), 'circular': lambda: api.deduplicate([], circular=True),
             'repeat': lambda: api.deduplicate([], circular=True, terminal_repeat=20), 'contained': lambda: api.deduplicate([], contained=True)}
    for mode, call in calls.items():
        out, scopes = profiled(api, call)
        assert scopes == {}, mode
        assert all(len(a) == 0 for a in out[:-1]), mode
        assert all(v == 0 for k, v in out[-1].items() if k != 'repeat'), (mode, out[-1])
    repeat, scopes = profiled(api, lambda: api.terminal_repeats([], 20))
    assert scopes == {} and len(repeat) == 0
