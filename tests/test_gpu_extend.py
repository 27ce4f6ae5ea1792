"""vg_genomes_extend / vg_genomes_truncate / vg_genomes_reserve on the GPU: a subset that was extended and truncated in place is, to
every kernel, the set that from_codes makes of the same genomes in the same order -- the bases read back, the align order, the shared
k-mer counts at two key lengths and every integer of the LZ parse -- after every step of a sequence of calls, whatever the set held
before (its caches and the bases behind its end included), and the parent set is left as it was.  Two parents, as in
test_gpu_subset.py: the 12 golden genomes plus short synthetic ones (blocks of 1 024 bases; four of the golden ones take part), and the synthetic ones alone (blocks of 64
bases, so that lengths 64 and 1 024 fill their blocks and the padding takes a block of its own)."""
import numpy as np
import pytest

import oracle_lib as orc
from vclust_amd import api

pytestmark = pytest.mark.gpu

SYNTH_LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
N_BIG = 4          # golden genomes that take part in the sequences (all 12 are in the parent: they set its block size)


def _synthetic():
    """-> list of (name, codes): the lengths above without a single A (the 1 024 is the head of the 4 097, so that two of them share
    k-mers) -- whatever lies behind a genome that ends the set after a truncate held C, G or T before -- then one genome of N alone,
    one with N as its first base and one with N as its last base"""
    rng = np.random.default_rng(11)
    long = rng.integers(1, 4, 4097).astype(np.uint8)
    out = []
    for ln in SYNTH_LENGTHS:
        out.append((f's{ln}', long.copy() if ln == 4097 else long[:ln].copy() if ln == 1024 else rng.integers(1, 4, ln).astype(np.uint8)))
    out.append(('all_n', np.full(65, 4, dtype=np.uint8)))
    first = rng.integers(1, 4, 127).astype(np.uint8); first[0] = 4
    last = long[1000:1064].copy(); last[-1] = 4
    return out + [('n_first', first), ('n_last', last)]


def _block(genomes):
    """the block size the loader chooses for these genomes (vg_choose_align_shift: about a 16th of the mean length, 64 .. 4 096)"""
    mean = sum(len(c) for _, c in genomes) // len(genomes)
    shift = 6
    while shift < 12 and (1 << (shift + 1)) <= mean // 16:
        shift += 1
    return 1 << shift


def _set(genomes):
    offsets = np.zeros(len(genomes) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(c) for _, c in genomes])
    codes = np.concatenate([c for _, c in genomes]) if genomes else np.zeros(0, dtype=np.uint8)
    return api.GenomeSet.from_codes(codes, offsets, [n for n, _ in genomes])


def _shared(gs, k):
    sizes, pairs = gs.kmer_shared(k=k)
    return list(map(int, sizes)), sorted((int(p['a']), int(p['b']), int(p['shared'])) for p in pairs)


@pytest.fixture(scope='module')
def parents(golden_dir):
    """{name: (genomes, resident set, its shared counts before anything was taken from it)}; the references (from_codes of a list of
    genomes) are made once per list and shared"""
    api.set_device(0)
    codes, offsets, names = orc.read_fasta_codes(golden_dir / 'multifasta.fna')
    golden = [(names[i], codes[offsets[i]:offsets[i + 1]].copy()) for i in range(len(names))]
    out = {}
    for key, genomes, block in (('golden+synthetic', golden + _synthetic(), 1024), ('synthetic', _synthetic(), 64)):
        assert _block(genomes) == block
        gs = _set(genomes)
        gs.to_device()
        out[key] = (genomes, gs, {k: _shared(gs, k) for k in (15, 25)})
    return out


_references = {}


def _check(parent, genomes, sub, ids, what):
    """sub against from_codes of genomes[ids], in that order"""
    key = (parent, tuple(ids))
    if key not in _references:
        ref = _set([genomes[i] for i in ids])
        tasks = np.array([(q, r) for q in range(len(ids)) for r in range(len(ids)) if q != r], dtype=api.TASK_DTYPE)
        _references[key] = (ref, ref.names(), list(ref.lengths()), list(ref.align_order()), {k: _shared(ref, k) for k in (15, 25)}, tasks,
                            ref.lz_align(tasks).tolist() if len(tasks) else [])
    ref, names, lengths, order, shared, tasks, parse = _references[key]
    assert len(sub) == len(ids), what
    assert sub.names() == names and list(sub.lengths()) == lengths, what
    for i in range(len(ids)):
        assert np.array_equal(sub.codes(i), np.minimum(genomes[ids[i]][1], 4)), (what, i)
    assert list(sub.align_order()) == order, what
    for k in (15, 25):
        assert _shared(sub, k) == shared[k], (what, k)
    # every ordered pair, every integer of the parse: the golden genomes, the all-N genome, the N at either end, the head of another
    if len(tasks):
        got = sub.lz_align(tasks)
        assert got.tolist() == parse, what
        return int(got['n_match'].sum())
    return 0


def _names(genomes):
    return {name: i for i, (name, _) in enumerate(genomes)}


def _big(genomes):
    return [i for i, (name, _) in enumerate(genomes) if not name.startswith(('s', 'all_n', 'n_'))][:N_BIG]


def _steps(genomes, sequence):
    """sequence name -> list of (call, argument, the ids the set holds afterwards); ids by name, so both parents take the same lists"""
    at = _names(genomes)
    pick = lambda *names: [at[n] for n in names]                                  # noqa: E731
    big = _big(genomes)
    a, b, c = pick('s4097', 's1', 's64'), pick('all_n', 's1023', 's1024'), pick('n_last', 's65', 'n_first', 's1025', 's63')
    if sequence == 'onto an empty subset':
        return [('subset', [], []), ('extend', big + a + c, big + a + c)]
    if sequence == 'twice':
        return [('subset', a, a), ('extend', big[:2] + b, a + big[:2] + b), ('extend', c + big[2:], a + big[:2] + b + c + big[2:])]
    if sequence == 'outgrows the capacity':
        small = pick('s1')                                                        # one block: everything after it is many times that
        return [('subset', small, small), ('extend', pick('s63'), small + pick('s63')),
                ('extend', big + pick('s4097', 's1024', 'all_n'), small + pick('s63') + big + pick('s4097', 's1024', 'all_n'))]
    if sequence == 'reserved':
        small = pick('s1')
        rest = big + pick('s4097', 's1024', 'all_n', 's63')
        return [('subset', small, small), ('reserve', rest, small), ('extend', rest[:-1], small + rest[:-1]), ('extend', rest[-1:], small + rest)]
    if sequence == 'truncate to the middle':
        # the genome that ends the set after each truncate: s64 fills its block of 64 bases (the padding takes a block of its own), s1024
        # fills its blocks in both parents, s1023 fills none; directly behind each of them lay a genome without a single A
        head = big[:1] + pick('s1024', 's64')
        first = head + pick('s4097', 's63', 's1025') + big[1:2]
        second = head[:-1] + pick('all_n', 's1023', 's65') + big[2:3]
        return [('subset', first, first), ('truncate', len(head), head), ('extend', pick('n_first', 's65'), head + pick('n_first', 's65')),
                ('truncate', len(head) - 1, head[:-1]), ('extend', second[len(head) - 1:], second),
                ('truncate', len(head) + 1, second[:len(head) + 1])]
    if sequence == 'truncate to nothing':
        return [('subset', a + big[:1], a + big[:1]), ('truncate', 0, []), ('extend', b + big[1:2], b + big[1:2]),
                ('truncate', len(b + big[1:2]), b + big[1:2])]
    raise KeyError(sequence)


SEQUENCES = ['onto an empty subset', 'twice', 'outgrows the capacity', 'reserved', 'truncate to the middle', 'truncate to nothing']


@pytest.mark.parametrize('sequence', SEQUENCES)
@pytest.mark.parametrize('parent', ['golden+synthetic', 'synthetic'])
def test_after_every_step_the_set_equals_the_set_made_from_the_same_codes(parents, parent, sequence):
    genomes, gs, before = parents[parent]
    sub, matched = None, 0
    for step, (call, arg, ids) in enumerate(_steps(genomes, sequence)):
        if call == 'subset':
            sub = gs.subset(arg)
        elif call == 'extend':
            sub.extend(gs, arg)
        elif call == 'truncate':
            sub.truncate(arg)
        else:
            sub.reserve(sum(len(genomes[i][1]) for i in arg), len(arg))
        matched += _check(parent, genomes, sub, ids, (parent, sequence, step, call))
    if parent == 'golden+synthetic':
        assert matched > 0                                            # the parse found something to compare
    # the parent is what it was
    for k in (15, 25):
        assert _shared(gs, k) == before[k]


def test_an_extend_is_one_profiled_gather_of_the_appended_genomes(parents):
    """one gather per extend, in the scope `derep_extend`, and its bytes are those of the appended genomes alone: the resident prefix is
    neither read nor copied"""
    genomes, gs, _ = parents['golden+synthetic']
    at = _names(genomes)
    big = _big(genomes)
    sub = gs.subset([at['s1']])
    sub.reserve(sum(len(genomes[i][1]) for i in big), len(big))
    api.profile_enable(True)
    api.profile_reset()
    try:
        for i in big:
            sub.extend(gs, [i])
        prof = {p['name']: p for p in api.profile_get()}
    finally:
        api.profile_enable(False)
    # read and written once, 2 bits of code and 1 of mask per base
    assert prof['derep_extend']['launches'] == len(big) and 'derep_subset' not in prof
    block = _block(genomes)
    appended = sum((len(genomes[i][1]) // block + 1) * block for i in big)
    assert prof['derep_extend']['bytes'] == 2 * (appended // 4 + appended // 8)
    _check('golden+synthetic', genomes, sub, [at['s1']] + big, 'reserved, one by one')


def test_errors_that_need_a_subset(parents):
    genomes, gs, _ = parents['golden+synthetic']
    _, other, _ = parents['synthetic']
    sub = gs.subset([5, 3])
    with pytest.raises(api._lib.VclustGpuError) as e:
        sub.extend(gs, [1, 3])
    assert e.value.code == -1 and 'ids[1] = 3 is in the set already' in str(e.value)
    with pytest.raises(api._lib.VclustGpuError) as e:
        sub.extend(gs, [1, 1])
    assert e.value.code == -1 and 'ids[1] = 1 is listed twice' in str(e.value)
    with pytest.raises(api._lib.VclustGpuError) as e:
        sub.extend(gs, [len(genomes)])
    assert e.value.code == -1 and 'outside 0..' in str(e.value)
    with pytest.raises(api._lib.VclustGpuError) as e:
        sub.extend(other, [0])
    assert e.value.code == -1 and 'not gathered from this parent' in str(e.value)
    with pytest.raises(api._lib.VclustGpuError) as e:
        sub.truncate(3)
    assert e.value.code == -1 and 'n_keep = 3' in str(e.value)
    with pytest.raises(api._lib.VclustGpuError) as e:
        gs.truncate(1)                                                # a loaded set, resident or not
    assert e.value.code == -1 and 'vg_genomes_subset' in str(e.value)
    # none of them changed the set; a dropped genome may come back; a subset of a subset extends from the subset
    _check('golden+synthetic', genomes, sub, [5, 3], 'after the errors')
    sub.truncate(1)
    sub.extend(gs, [3, 0])
    _check('golden+synthetic', genomes, sub, [5, 3, 0], 'dropped and appended again')
    inner = sub.subset([2])
    inner.extend(sub, [0])
    assert inner.names() == [genomes[0][0], genomes[5][0]]
    assert np.array_equal(inner.codes(1), np.minimum(genomes[5][1], 4))
