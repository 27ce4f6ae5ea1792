"""Parity of the HIP product path with the CPU oracle (and, through it, the reference goldens).

All tests call through the C ABI of libvclust_gpu.so; integers must be bit-exact.
"""
import filecmp
import pathlib
import sys

import numpy as np
import pytest

import lz_checks as lc
import oracle_lib as orc
from vclust_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def example(golden_dir):
    codes, offsets, names = orc.read_fasta_codes(golden_dir / 'multifasta.fna')
    gs = api.GenomeSet.load([golden_dir / 'multifasta.fna'], multisample=True)
    return codes, offsets, names, gs


def _pairs_dict(pairs):
    return {(int(p['a']), int(p['b'])): int(p['shared']) for p in pairs}


def test_ingest_matches_oracle_reader(example):
    codes, offsets, names, gs = example
    assert gs.names() == names
    assert list(gs.lengths()) == list(np.diff(offsets))


def test_kmer_sets_example(example):
    codes, offsets, names, gs = example
    for idx in (0, 5, 11):
        mine = gs.kmer_set(idx, 25)
        ref = orc.kmer_set(codes[offsets[idx]:offsets[idx + 1]], 25)
        assert np.array_equal(mine, ref)


@pytest.mark.parametrize('k,fraction', [(25, 0.5), (21, 0.3)])
def test_kmer_sets_fraction_example(example, k, fraction):
    """vg_kmer_set with a fraction: the compact extraction (scan, count, emit) followed by both sorts.  The oracle's set at these
    fractions is a non-empty proper subset of the full one."""
    codes, offsets, names, gs = example
    for idx in (0, 5, 11):
        seq = codes[offsets[idx]:offsets[idx + 1]]
        ref = orc.kmer_set(seq, k, fraction)
        assert 0 < len(ref) < len(orc.kmer_set(seq, k))
        assert np.array_equal(gs.kmer_set(idx, k, fraction), ref)


@pytest.mark.parametrize('k', [12, 28, 29, 30, 31])
def test_kmer_sets_from_bit_planes(example, k):
    """The kernels read k-mers off the bit planes and keep (hi plane : lo plane) of the smaller strand as the key; what
    leaves through vg_kmer_set is the oracle's number again (2-bit codes, first base most significant).  k = 29 is the
    last k whose four windows come out of one funnel shift per plane, 30 and 31 take one per position."""
    codes, offsets, names, gs = example
    for idx in (1, 7):
        mine = gs.kmer_set(idx, k)
        ref = orc.kmer_set(codes[offsets[idx]:offsets[idx + 1]], k)
        assert np.array_equal(mine, ref), k
    sizes, pairs = gs.kmer_shared(k=k)
    osizes, opairs = orc.shared_all(codes, offsets, k=k)
    assert list(sizes) == list(osizes) and _pairs_dict(pairs) == opairs


@pytest.mark.parametrize('k', [25, 20, 30, 15])
def test_kmer_shared_example(example, k):
    codes, offsets, names, gs = example
    sizes, pairs = gs.kmer_shared(k=k)
    osizes, opairs = orc.shared_all(codes, offsets, k=k)
    assert list(sizes) == list(osizes)
    assert _pairs_dict(pairs) == opairs


@pytest.mark.parametrize('n_shards', [3, 8])       # 8: the sparse emit pass (few k-mers kept per wave)
def test_kmer_shared_shards_add_up(example, n_shards):
    codes, offsets, names, gs = example
    osizes, opairs = orc.shared_all(codes, offsets, k=25)
    tot_sizes = np.zeros(len(gs), dtype=np.int64)
    tot = {}
    for s in range(n_shards):
        sizes, pairs = gs.kmer_shared(k=25, shard=s, n_shards=n_shards)
        tot_sizes += sizes
        for key, v in _pairs_dict(pairs).items():
            tot[key] = tot.get(key, 0) + v
    assert list(tot_sizes) == list(osizes)
    assert tot == opairs


def test_kmer_shared_subshard_loop(example):
    """Sets too large for one pass are processed as sub-shards of the k-mer range inside one call:
    forced here on the small example (sizes and counts must not change), alone and under an outer shard."""
    from vclust_amd import _lib
    lib = _lib.load()
    codes, offsets, names, gs = example
    osizes, opairs = orc.shared_all(codes, offsets, k=25)
    lib.vg_set_subshards(3)
    try:
        sizes, pairs = gs.kmer_shared(k=25, min_shared=20)
        assert list(sizes) == list(osizes)
        assert _pairs_dict(pairs) == {k: v for k, v in opairs.items() if v >= 20}
        tot_sizes = np.zeros(len(gs), dtype=np.int64); tot = {}
        for s in range(2):
            sz, pr = gs.kmer_shared(k=25, shard=s, n_shards=2)
            tot_sizes += sz
            for key, v in _pairs_dict(pr).items():
                tot[key] = tot.get(key, 0) + v
        assert list(tot_sizes) == list(osizes) and tot == opairs
    finally:
        lib.vg_set_subshards(0)


def test_kmer_fraction(example):
    codes, offsets, names, gs = example
    sizes, pairs = gs.kmer_shared(k=25, fraction=0.2)
    osizes, opairs = orc.shared_all(codes, offsets, k=25, fraction=0.2)
    assert list(sizes) == list(osizes)
    assert _pairs_dict(pairs) == opairs


def test_prefilter_file_is_golden(tmp_path, golden_dir):
    out = tmp_path / 'fltr.txt'
    api.prefilter([golden_dir / 'multifasta.fna'], out, is_multifasta=True)
    assert filecmp.cmp(out, golden_dir / 'output' / 'fltr.txt', shallow=False)
    out2 = tmp_path / 'fltr_gz.txt'
    api.prefilter([golden_dir / 'multifasta.fna.gz'], out2, is_multifasta=True)
    assert filecmp.cmp(out2, golden_dir / 'output' / 'fltr.txt', shallow=False)


def test_lz_example_all_pairs(example):
    codes, offsets, names, gs = example
    tasks = gs.align_tasks(gs.read_filter(None))
    assert len(tasks) == 132
    stats = gs.lz_align(tasks)
    bad = []
    for t, s in zip(tasks, stats):
        q, r = int(t['q']), int(t['r'])
        ref = orc.lz_pair_stat(codes[offsets[q]:offsets[q + 1]], codes[offsets[r]:offsets[r + 1]])
        if ref != (int(s['n_match']), int(s['aln_len']), int(s['n_regions'])):
            bad.append((names[q], names[r], ref, tuple(int(x) for x in s)))
    assert not bad, bad[:10]


def test_align_files_equal_oracle(tmp_path, golden_dir):
    mine = tmp_path / 'ani.tsv'
    aln = tmp_path / 'ani.aln.tsv'
    api.align([golden_dir / 'multifasta.fna'], mine, is_multifasta=True, columns=api.ALIGN_FIELDS[:11], out_aln=aln)
    ref = tmp_path / 'ref.tsv'
    ref_aln = tmp_path / 'ref.aln.tsv'
    orc.run_cli('align', '-o', ref, '--out-aln', ref_aln, golden_dir / 'multifasta.fna')
    assert filecmp.cmp(mine, ref, shallow=False)
    assert filecmp.cmp(tmp_path / 'ani.ids.tsv', golden_dir / 'output' / 'ani.ids.tsv', shallow=False)
    assert sorted(open(aln).read().splitlines()) == sorted(open(ref_aln).read().splitlines())


def test_hip_output_against_reference_goldens(tmp_path, golden_dir):
    """The HIP path against the reference's own files (example/output/ani.tsv:1-133, ani.aln.tsv:1-5694,
    ani.ids.tsv), not against the oracle -- STRICT identity: ani.tsv and ani.ids.tsv byte-identical, the
    alignment table equal as a multiset of lines (5 693 regions; the reference's block order follows its
    thread completion)."""
    mine = tmp_path / 'ani.tsv'; aln = tmp_path / 'ani.aln.tsv'
    api.align([golden_dir / 'multifasta.fna'], mine, is_multifasta=True, columns=api.ALIGN_FIELDS[:11], out_aln=aln)
    assert filecmp.cmp(tmp_path / 'ani.ids.tsv', golden_dir / 'output' / 'ani.ids.tsv', shallow=False)
    assert filecmp.cmp(mine, golden_dir / 'output' / 'ani.tsv', shallow=False)
    g = (golden_dir / 'output' / 'ani.aln.tsv').read_text().splitlines(); m = aln.read_text().splitlines()
    assert g[0] == m[0] and len(g) == len(m) == 5694
    assert sorted(g[1:]) == sorted(m[1:])
    # the step after the path: Clusty's golden output follows from the files the HIP path wrote
    from test_oracle_golden import single_linkage_partition, golden_partition
    assert single_linkage_partition(mine, tmp_path / 'ani.ids.tsv') == golden_partition(golden_dir)


@pytest.fixture(scope='module')
def small_synth():
    codes, offsets, names = synth.make_families(6, 4, length=6000, seed=7)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    return codes, offsets, names, gs


def test_synth_prefilter(small_synth):
    codes, offsets, names, gs = small_synth
    sizes, pairs = gs.kmer_shared(k=25)
    osizes, opairs = orc.shared_all(codes, offsets, k=25)
    assert list(sizes) == list(osizes)
    assert _pairs_dict(pairs) == opairs


def test_synth_lz(small_synth):
    codes, offsets, names, gs = small_synth
    tasks = gs.align_tasks(synth.family_pairs(6, 4))
    stats = gs.lz_align(tasks)
    for t, s in zip(tasks, stats):
        q, r = int(t['q']), int(t['r'])
        ref = orc.lz_pair_stat(codes[offsets[q]:offsets[q + 1]], codes[offsets[r]:offsets[r + 1]])
        assert ref == (int(s['n_match']), int(s['aln_len']), int(s['n_regions'])), (names[q], names[r])


def test_lz_with_n_and_edges():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, size=3000, dtype=np.uint8)
    b = a.copy()
    b[rng.random(3000) < 0.05] = 0
    b[500:520] = 4                      # run of N in the reference copy
    c = a[1000:2200].copy()
    c[100] = 4
    tiny = a[:8].copy()                 # shorter than mal
    empty_like = np.full(40, 4, dtype=np.uint8)
    seqs = [a, b, c, tiny, empty_like]
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    codes = np.concatenate(seqs)
    gs = api.GenomeSet.from_codes(codes, offsets)
    tasks = gs.align_tasks(gs.read_filter(None))
    stats = gs.lz_align(tasks)
    for t, s in zip(tasks, stats):
        q, r = int(t['q']), int(t['r'])
        ref = orc.lz_pair_stat(seqs[q], seqs[r])
        assert ref == (int(s['n_match']), int(s['aln_len']), int(s['n_regions'])), (q, r)


def test_messy_fasta_bases_equal_oracle_reader(tmp_path):
    """Same file as tests/test_abi_host.py::test_ingest_messy_fasta: the packed bases (seen through the
    k-mer sets at a small k) equal the oracle reader's, plain and gzip."""
    import gzip
    from test_abi_host import MESSY
    p = tmp_path / 'messy.fna'; p.write_bytes(MESSY)
    pz = tmp_path / 'messy.fna.gz'; pz.write_bytes(gzip.compress(MESSY))
    codes, offsets, names = orc.read_fasta_codes(p)
    for path in (p, pz):
        gs = api.GenomeSet.load([path], multisample=True)
        for i in range(len(gs)):
            assert list(gs.kmer_set(i, 8)) == list(orc.kmer_set(codes[offsets[i]:offsets[i + 1]], 8)), names[i]


def test_degenerate_genome_sets():
    """One genome; genomes shorter than k / mal; an all-N genome; an empty genome; identical genomes."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 4, size=3000, dtype=np.uint8)
    one = api.GenomeSet.from_codes(a, np.array([0, 3000], dtype=np.int64))
    sizes, pairs = one.kmer_shared(k=25)
    assert list(sizes) == list(orc.shared_all(a, np.array([0, 3000]), k=25)[0]) and len(pairs) == 0
    assert len(one.align_tasks(pairs)) == 0 and len(one.lz_align(one.align_tasks(pairs))) == 0
    seqs = [a, a.copy(), a[:20].copy(), np.full(100, 4, dtype=np.uint8), np.zeros(0, dtype=np.uint8),
            rng.integers(0, 4, size=2500, dtype=np.uint8), a[::-1].copy()]
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(s) for s in seqs])
    codes = np.concatenate(seqs)
    gs = api.GenomeSet.from_codes(codes, offsets)
    for k in (25, 12):
        sizes, pairs = gs.kmer_shared(k=k)
        osizes, opairs = orc.shared_all(codes, offsets, k=k)
        assert list(sizes) == list(osizes) and _pairs_dict(pairs) == opairs
    tasks = gs.align_tasks(gs.read_filter(None))           # all-vs-all, including the empty and the N genome
    stats = gs.lz_align(tasks)
    for t, s in zip(tasks, stats):
        q, r = int(t['q']), int(t['r'])
        assert orc.lz_pair_stat(seqs[q], seqs[r]) == (int(s['n_match']), int(s['aln_len']), int(s['n_regions'])), (q, r)
    ident = [s for t, s in zip(tasks, stats) if {int(t['q']), int(t['r'])} == {0, 1}]
    assert all(int(s['n_match']) == 3000 and int(s['aln_len']) == 3000 and int(s['n_regions']) == 1 for s in ident)


def test_index_budget_batches_do_not_change_results():
    """vg_set_index_budget: with the smallest budget (64 MiB) the ~100 MB of indexes of 160 x 40 kb
    references are built in several batches (several build + parse launches); rows and regions equal the
    single-batch run."""
    from vclust_amd import _lib
    lib = _lib.load()
    codes, offsets, names = synth.make_families(16, 10, length=40000, seed=9)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    tasks = gs.align_tasks(synth.family_pairs(16, 10))
    ref_stats, ref_regions = gs.lz_align(tasks, want_regions=True)
    lib.vg_set_index_budget((64 << 20) + 1)
    try:
        stats, regions = gs.lz_align(tasks, want_regions=True)
        stats2 = gs.lz_align(tasks)
    finally:
        lib.vg_set_index_budget(24 << 30)
    assert np.array_equal(stats, ref_stats) and np.array_equal(stats2, ref_stats)
    key = lambda r: tuple(int(x) for x in r)
    assert sorted(map(key, regions)) == sorted(map(key, ref_regions))


@pytest.mark.parametrize('families,batches', [(16, 1), (20, 2)])
def test_index_budget_batches_with_every_regions_path(tmp_path, families, batches):
    """Several batches crossed with each --out-aln path: under the 64 MiB budget, a child process each (developer switches
    are read once) for the one-parse path, a first arena far too small (every batch repeats itself), the two-pass checker
    (its arena and offsets in a later batch) and the general kernel.  Rows equal those of a child with the default budget,
    regions equal them as sorted tuples, and the four budgeted children return the same region array.  16 families are the
    set of the budget test above: 160 references x 415.6 kB (lz_ref_need) = 63.4 MiB, ONE batch under that budget; 20
    families (79 MiB) are what it cuts in two."""
    codes, offsets, names = synth.make_families(families, 10, length=40000, seed=9)
    n_rr = 2 * np.diff(offsets) + 1
    need = int((((n_rr + 128 + 31) // 32 + 2) * 12 + (4 ** 7 + n_rr) * 4).sum())         # lz_ref_need restated, every genome a reference
    budget = (64 << 20) + 1
    assert (batches - 1) * budget < need <= batches * budget and (batches == 1 or need < 1.5 * budget)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    tasks = gs.align_tasks(synth.family_pairs(families, 10))
    from vclust_amd import _lib
    _lib.load().vg_set_index_budget(budget)                  # what the library itself plans: one index build per batch
    api.profile_enable(True); api.profile_reset()
    try:
        gs.lz_align(tasks)
        builds = {e['name']: e['launches'] for e in api.profile_get()}.get('lz_build_index')
    finally:
        api.profile_enable(False)
        _lib.load().vg_set_index_budget(24 << 30)
    assert builds == batches
    base = lc.run_child(tmp_path, 'base', codes, offsets, tasks)
    key = lambda r: tuple(int(x) for x in r)
    base_regions = sorted(map(key, base['regions']))
    assert len(base_regions) == int(base['stats']['n_regions'].sum()) > 0
    out = {name: lc.run_child(tmp_path, name, codes, offsets, tasks, env=env, budget=budget)
           for name, env in (('one_parse', {}), ('tiny_arena', dict(VG_LZ_ARENA='64')), ('two_pass', dict(VG_LZ_REGIONS='two-pass')),
                             ('general', dict(VG_LZ_KERNEL='general')))}
    for name, o in out.items():
        assert np.array_equal(o['stats'], base['stats']), name
        assert sorted(map(key, o['regions'])) == base_regions, name
        assert np.array_equal(o['regions'], out['one_parse']['regions']), name


@pytest.mark.parametrize('mode', ['malloc'])
def test_allocator_cycles_1_to_64_gib(mode):
    """The device allocator (hipMalloc blocks): three rounds of 1 + 4 + 17 + 64 GiB blocks -- a size that is not a
    multiple of 2 MiB among them -- written and read back at both ends, released and returned to the driver, in a
    process of its own."""
    import os
    import subprocess
    import pathlib
    import sys
    ROOT = pathlib.Path(__file__).resolve().parent.parent
    code = ('import ctypes as C, sys\n'
            'sys.path.insert(0, %r)\n'
            'from vclust_amd import _lib\n'
            'lib = _lib.load()\n'
            'sizes = (C.c_int64 * 4)(1 << 30, 4 << 30, (17 << 30) + (3 << 20), 64 << 30)\n'
            'rc = lib.vg_alloc_selftest(sizes, 4, 3)\n'
            'assert rc == 0, lib.vg_last_error()\n'
            'print("ok")\n') % str(ROOT)
    p = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, VG_ALLOC_TRACE='1'),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith('ok'), p.stderr[-3000:]
    assert ' hipMalloc of ' in p.stderr


def test_prepared_indexes_do_not_change_the_rows():
    """vg_lz_prepare queues the reference indexes of the candidate pairs ahead of vg_lz_align: taken over when the task
    list names the same references (ONE index build in the profile), dropped otherwise; rows identical in every case,
    and a plan may be pending when the set is freed."""
    codes, offsets, names = synth.make_families(30, 6, length=20000, seed=17)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    pairs = synth.family_pairs(30, 6)
    tasks = gs.align_tasks(pairs)
    ref = gs.lz_align(tasks)
    api.profile_enable(True); api.profile_reset()
    gs.lz_prepare(pairs)
    got = gs.lz_align(tasks)
    builds = {e['name']: e['launches'] for e in api.profile_get()}.get('lz_build_index')
    api.profile_enable(False)
    assert np.array_equal(got, ref) and builds == 1
    gs.lz_prepare(pairs[:10])                                   # other references: the plan is dropped
    assert np.array_equal(gs.lz_align(tasks), ref)
    gs.lz_prepare(pairs)
    sub = gs.align_tasks(pairs[5:40])
    want = {(int(t['q']), int(t['r'])): tuple(int(x) for x in s) for t, s in zip(tasks, ref)}
    assert all(want[(int(t['q']), int(t['r']))] == tuple(int(x) for x in s) for t, s in zip(sub, gs.lz_align(sub)))
    gs.lz_prepare(pairs, lz=dict(mal=12))                        # other parameters: dropped
    assert np.array_equal(gs.lz_align(tasks), ref)
    gs.lz_prepare(pairs)
    del gs                                                      # a pending plan goes with its set
    gs2 = api.GenomeSet.from_codes(codes, offsets, names)
    assert np.array_equal(gs2.lz_align(tasks), ref)


def test_plan_survives_calls_with_different_task_lists():
    """The plan of a call is kept (host side) for the next call on the same references and depends on the references only:
    calls with different task lists over the same references, with and without regions and after vg_lz_prepare, return the
    rows of the first call, and the regions of a fresh set."""
    codes, offsets, names = synth.make_families(30, 6, length=20000, seed=17)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    pairs = synth.family_pairs(30, 6)
    tasks = gs.align_tasks(pairs)
    sub = tasks[np.arange(len(tasks)) % 3 != 2]
    assert np.array_equal(np.unique(sub['r']), np.unique(tasks['r']))          # the same references, so the same plan
    want = {(int(t['q']), int(t['r'])): tuple(int(x) for x in s) for t, s in zip(tasks, gs.lz_align(tasks))}
    same = lambda tk, st: len(st) == len(tk) and all(want[(int(t['q']), int(t['r']))] == tuple(int(x) for x in s) for t, s in zip(tk, st))
    assert same(sub, gs.lz_align(sub))
    stats, regions = gs.lz_align(tasks, want_regions=True)
    assert same(tasks, stats)
    api.profile_enable(True); api.profile_reset()
    try:
        gs.lz_prepare(pairs)
        prepared = gs.lz_align(sub)
        builds = {e['name']: e['launches'] for e in api.profile_get()}.get('lz_build_index')
    finally:
        api.profile_enable(False)
    assert same(sub, prepared) and builds == 1
    fresh_stats, fresh_regions = api.GenomeSet.from_codes(codes, offsets, names).lz_align(tasks, want_regions=True)
    assert np.array_equal(stats, fresh_stats) and np.array_equal(regions, fresh_regions) and len(regions) > 0


def test_accuracy_against_known_truth():
    """The reference's own acceptance criterion (/root/reference test.py:456-477: tANI within 0.007 of the simulated truth,
    example/README.txt:4-11) on pairs whose truth is EXACT: ancestor / member pairs of 40 kb with substitutions only (truth =
    fraction of equal positions), 24 pairs in the phage range of SURVEY 8(d) (0.5 ... 12 % substitutions), 9 moderately diverged
    (15 ... 20 %) and 9 far diverged (22 ... 30 %), through vg_lz_align -- at the fitted constants of the restatement and with each
    of the three thin constants (held by one to three events of the reference's 12-genome example) at its
    alternative value (vg_set_lz_fit).  Up to 20 % the criterion holds whatever the thin constants are; beyond, the parse loses
    coverage (never over-estimates).  The table goes to gpurun_out/ (committed as profiles/r06_accuracy_vs_truth.md)."""
    sys.path.insert(0, str(ROOT / 'tools'))
    import accuracy_vs_truth as acc
    res, pairs = acc.table(use_oracle=False)
    for (label, band), (mx, mean, n, lo, hi) in res.items():
        if band != 'far diverged':
            assert mx < acc.TOLERANCE, (label, band, mx)
        else:
            assert mean <= 0.0 and mx > acc.TOLERANCE, (label, band, mx, mean)      # coverage is lost, identity never invented
    # the fitted constants on the HIP path = the CPU restatement, to the integer
    codes, offsets, names, prs = acc.make_set()
    assert acc.tani_hip(codes, offsets, names, prs[:6], {}) == acc.tani_oracle(codes, offsets, names, prs[:6], {})
    # where the thin constants CAN act (full mutation model): they change rows, and tANI by far less than the criterion
    sens = acc.knob_sensitivity()
    assert any(v[0] > 0 for d in sens.values() for v in d.values()), 'no thin constant changed a single row: the sensitivity sets exercise nothing'
    assert all(v[2] < acc.TOLERANCE for d in sens.values() for v in d.values()), sens
    out = ROOT / 'gpurun_out'
    try:
        out.mkdir(exist_ok=True)
        (out / 'r06_accuracy_vs_truth.md').write_text(acc.markdown(res, False, sens))
    except OSError:
        pass
