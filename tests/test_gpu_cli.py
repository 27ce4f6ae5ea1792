"""The reference's black-box CLI tests for the hot path (test.py:336-588), run against the
drop-in front-end on a real GPU."""
import pathlib
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
EX = ROOT / 'tests' / 'golden' / 'example'
FASTA_DIR, FASTA_FILE, FASTAGZ_FILE = EX / 'fna', EX / 'multifasta.fna', EX / 'multifasta.fna.gz'


def run(*args, capture=True):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE if capture else None,
                          stderr=subprocess.PIPE if capture else None, text=True)


def parse_fltr(path):
    with open(path) as fh:
        vids = fh.readline().strip().rstrip(',').split(',')[1:]
        idx2vid = {i: v.rstrip('.fna') for i, v in enumerate(vids, start=1)}
        res = {}
        for line in fh:
            cols = line.rstrip().rstrip(',').split(',')
            v1 = cols[0].rstrip('.fna')
            for f in cols[1:]:
                i, ani = f.split(':')
                res[(v1, idx2vid[int(i)])] = float(ani); res[(idx2vid[int(i)], v1)] = float(ani)
    return res


@pytest.mark.parametrize('inp,params', [(FASTA_DIR, []), (FASTA_FILE, []), (FASTA_FILE, ['--batch-size', '4']), (FASTAGZ_FILE, [])])
def test_prefilter_default(tmp_path, inp, params):
    out = tmp_path / 'filter.txt'
    p = run('prefilter', '-i', inp, '-o', out, '-v', '0', *params)
    assert p.returncode == 0 and not p.stderr
    r = parse_fltr(out)
    assert r[('NC_010807.alt1', 'NC_010807')] == 0.99848
    assert r[('NC_010807.alt2', 'NC_010807.alt3')] == 0.992238
    assert r[('NC_025457', 'NC_025457.alt1')] == 0.990832
    assert r[('NC_010807.alt1', 'NC_010807.alt3')] == 0.996723
    assert r[('NC_025457.alt2', 'NC_025457.alt1')] == 0.94527
    assert r[('NC_002486', 'NC_002486.alt')] == 0.999979
    assert len(r) == 26


@pytest.mark.parametrize('params', [['--kmers-fraction', '0.2'], ['--max-seqs', '2'], ['-k', '20']])
def test_prefilter_params(tmp_path, params):
    out = tmp_path / 'filter.txt'
    p = run('prefilter', '-i', FASTA_FILE, '-o', out, '-v', '0', *params)
    assert p.returncode == 0 and not p.stderr and out.stat().st_size


def test_prefilter_verbose(tmp_path):
    p = run('prefilter', '-i', FASTA_FILE, '-o', tmp_path / 'f.txt')
    assert p.returncode == 0 and all(w in p.stderr for w in ['Running', 'Completed', 'INFO'])


@pytest.mark.parametrize('inp', [FASTA_DIR, FASTA_FILE, FASTAGZ_FILE])
def test_align_default(tmp_path, inp):
    out = tmp_path / 'ani.tsv'
    p = run('align', '-i', inp, '-o', out, capture=False)
    assert p.returncode == 0 and out.stat().st_size
    truth = {('NC_010807', 'NC_010807.alt1'): 0.99753, ('NC_010807', 'NC_010807.alt2'): 0.98985,
             ('NC_010807', 'NC_010807.alt3'): 0.98384, ('NC_005091', 'NC_005091.alt1'): 0.97161,
             ('NC_005091', 'NC_005091.alt2'): 0.96707, ('NC_025457', 'NC_025457.alt1'): 0.80607,
             ('NC_025457', 'NC_025457.alt2'): 0.75921, ('NC_002486', 'NC_002486.alt'): 1.00000}
    pairs = {}
    with open(out) as fh:
        next(fh)
        for line in fh:
            c = line.split()
            pairs[(c[2].rstrip('.fna'), c[3].rstrip('.fna'))] = float(c[4])
    for k, t in truth.items():
        assert abs(pairs[k] - t) < 0.007
    assert (tmp_path / 'ani.ids.tsv').exists()


@pytest.mark.parametrize('fmt', ['standard', 'lite', 'complete'])
def test_align_outfmt(tmp_path, fmt):
    sys.path.insert(0, str(ROOT))
    import vclust
    out = tmp_path / 'ani.tsv'
    assert run('align', '-i', FASTA_FILE, '-o', out, '--outfmt', fmt).returncode == 0
    assert open(out).readline().split() == vclust.ALIGN_OUTFMT[fmt]


@pytest.mark.parametrize('inp', [FASTA_DIR, FASTA_FILE])
def test_align_alignments(tmp_path, inp):
    out, aln = tmp_path / 'ani.tsv', tmp_path / 'ani.aln.tsv'
    assert run('align', '-i', inp, '-o', out, '--out-aln', aln).returncode == 0
    with open(aln) as fh:
        assert len(fh.readline().split()) == 10
        assert fh.readlines()


def test_align_verbose(tmp_path):
    p = run('align', '-i', FASTA_FILE, '-o', tmp_path / 'ani.tsv')
    assert p.returncode == 0 and all(w in p.stderr for w in ['Running', 'Completed', 'INFO'])


@pytest.mark.parametrize('inp,params', [(FASTA_DIR, []), (FASTA_FILE, []), (FASTA_FILE, ['--batch-size', '4'])])
def test_workflow_prefilter_align(tmp_path, inp, params):
    flt, ani = tmp_path / 'filter.txt', tmp_path / 'ani.tsv'
    assert run('prefilter', '-i', inp, '-o', flt, *params).returncode == 0 and flt.stat().st_size
    assert run('align', '-i', inp, '-o', ani, '--filter', flt).returncode == 0
    assert sum(1 for _ in open(ani)) == 27        # header + 13 pairs x 2 directions


def test_workflow_equals_oracle_files(tmp_path):
    """Whole-file identity with the CPU oracle through both CLIs (prefilter -> align --filter)."""
    sys.path.insert(0, str(ROOT / 'tests'))
    import filecmp
    import oracle_lib as orc
    flt, ani = tmp_path / 'f.txt', tmp_path / 'a.tsv'
    assert run('prefilter', '-i', FASTA_FILE, '-o', flt, '-v', '0').returncode == 0
    assert run('align', '-i', FASTA_FILE, '-o', ani, '--filter', flt, '--outfmt', 'complete', '-v', '0').returncode == 0
    oflt, oani = tmp_path / 'of.txt', tmp_path / 'oa.tsv'
    orc.run_cli('prefilter', '-o', oflt, FASTA_FILE)
    orc.run_cli('align', '-o', oani, '--filter', oflt, '0', '--outfmt', 'complete', FASTA_FILE)
    assert filecmp.cmp(flt, oflt, shallow=False) and filecmp.cmp(ani, oani, shallow=False)


def test_workflow_with_n_runs_and_several_upload_stretches(tmp_path):
    """The whole-stage calls upload the packed genomes stretch by stretch (128 M bases) while they pack; the N mask
    travels only for stretches that hold an N, the other stretches' masks are written on the device from the lengths.
    A 150 Mbp multi-FASTA (two stretches) with N runs in a few genomes of the second one, plain and bgzip-compressed:
    both files of both formats equal the CPU oracle's."""
    sys.path.insert(0, str(ROOT / 'tests'))
    import filecmp
    import numpy as np
    import oracle_lib as orc
    from test_abi_host import _bgzf
    from vclust_amd import synth
    codes, offsets, names = synth.make_families(375, 4, length=100000, seed=21)       # 1 500 genomes x 100 kb
    codes = np.array(codes, copy=True)
    for gi in (1400, 1401, 1403, 1460):                                                # N runs inside related genomes
        o = int(offsets[gi]); codes[o + 5000:o + 5400] = 4; codes[o + 60000:o + 60003] = 4
    fa = tmp_path / 'g.fna'
    synth.write_fasta(str(fa), codes, offsets, names)
    bg = tmp_path / 'g.fna.gz'
    bg.write_bytes(_bgzf(fa.read_bytes()))
    oflt, oani = tmp_path / 'of.txt', tmp_path / 'oa.tsv'
    orc.run_cli('prefilter', '-o', oflt, fa)
    orc.run_cli('align', '-o', oani, '--filter', oflt, '0', '--outfmt', 'complete', fa)
    for inp in (fa, bg):
        flt, ani = tmp_path / 'f.txt', tmp_path / 'a.tsv'
        assert run('prefilter', '-i', inp, '-o', flt, '-v', '0').returncode == 0
        assert run('align', '-i', inp, '-o', ani, '--filter', flt, '--outfmt', 'complete', '-v', '0').returncode == 0
        assert filecmp.cmp(flt, oflt, shallow=False) and filecmp.cmp(ani, oani, shallow=False), inp.name
    assert sum(1 for _ in open(oani)) > 2 * 375 * 5


def test_kernel_variants_write_the_same_files(tmp_path):
    """The specialised kernels against the general ones they replace, through the CLI on a 7 000-genome set (280 M
    positions: 18 partition bits) without N and with the default parameters, so that the default run takes
    k_lz_parse_fast, the register index build, the 8-byte level-1 records, the 32 768-position tiles and the narrow
    level-2 scatter: switching each of them off must not change a byte."""
    import filecmp
    import os
    sys.path.insert(0, str(ROOT))
    from vclust_amd import synth
    codes, offsets, names = synth.make_families(700, 10, length=40000, seed=31)
    fa = tmp_path / 'set.fna'
    synth.write_fasta(fa, codes, offsets, names)

    def go(tag, **env):
        flt, ani = tmp_path / f'{tag}.flt', tmp_path / f'{tag}.tsv'
        e = dict(os.environ, VG_DEV_SWITCHES='1', **env)          # (developer switches are honoured only beside this one)
        for args in (('prefilter', '-i', fa, '-o', flt, '-v', '0'), ('align', '-i', fa, '-o', ani, '--filter', flt, '--outfmt', 'complete', '-v', '0')):
            p = subprocess.run([sys.executable, str(VCLUST), *map(str, args)], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert p.returncode == 0, p.stderr[-2000:]
        return flt, ani

    base = go('default')
    assert sum(1 for _ in open(base[1])) > 50000
    for tag, env in (('general_parse', dict(VG_LZ_KERNEL='general')), ('lds_build', dict(VG_LZ_BUILD='lds')),
                     ('long_records', dict(VG_LEVEL1_RECORDS='long')), ('staged', dict(VG_DENSE_SCATTER='staged', VG_LEVEL2_SCATTER='staged')),
                     ('radix', dict(VG_INDEX_PATH='radix')),
                     # the cold CLI's bounded footprint at a budget that bites here: eight RANGE sub-shards of the prefilter
                     # (k_part_scatter_range; then the all-positions scatter it replaces), many small index batches
                     ('subshards', dict(VG_WORKSPACE_GB='0.6')), ('subshards_dense', dict(VG_WORKSPACE_GB='1.5', VG_RANGE_SCATTER='dense')),
                     ('index_batches', dict(VG_ONESHOT_INDEX_GB='0.25'))):
        other = go(tag, **env)
        assert filecmp.cmp(base[0], other[0], shallow=False) and filecmp.cmp(base[1], other[1], shallow=False), tag


def test_cold_cli_calls_keep_a_bounded_device_footprint(tmp_path):
    """The two whole-stage calls of the CLI touch ~10 GB of device memory whatever one pass over the set would take
    (a cold process may wait 25-32 ms per GiB for memory the driver has not wiped yet: DESIGN.md section 3).  30 000 x 40 kb
    genomes: one prefilter pass would hold 20 GB of records and row pointers, one index batch 12 GB; the allocator trace
    of both processes stays below 12 GB (live + cached), the prefilter runs as sub-shards, and the files equal those of
    the unbounded run."""
    import filecmp
    import os
    import re
    sys.path.insert(0, str(ROOT))
    from vclust_amd import synth
    codes, offsets, names, _ = synth.make_workload('phage-100k', 3000)
    fa = tmp_path / 'set.fna'
    synth.write_fasta(fa, codes, offsets, names)

    def go(tag, **env):
        flt, ani = tmp_path / f'{tag}.flt', tmp_path / f'{tag}.tsv'
        e = dict(os.environ, VG_ALLOC_TRACE='1', VG_HOST_TRACE='1', **env)
        peak, marks = [], []
        for args in (('prefilter', '-i', fa, '-o', flt, '-v', '0'), ('align', '-i', fa, '-o', ani, '--filter', flt, '-v', '0')):
            p = subprocess.run([sys.executable, str(VCLUST), *map(str, args)], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert p.returncode == 0, p.stderr[-2000:]
            gb = [float(a) + float(b) for a, b in re.findall(r'new block [0-9.]+ MB (?:at \S+ )?\(live ([0-9.]+) GB, cached ([0-9.]+) GB\)', p.stderr)]
            peak.append(max(gb)); marks.append(p.stderr)
        return flt, ani, peak, marks
    flt, ani, peak, marks = go('bounded')
    assert peak[0] < 10.0 and peak[1] < 8.0, peak
    assert marks[0].count('buckets: enter') >= 2            # the prefilter ran as sub-shards
    flt2, ani2, peak2, _ = go('one_pass', VG_WORKSPACE_GB='1000', VG_ONESHOT_INDEX_GB='64')
    assert peak2[0] > 15.0 and peak2[1] > 10.0, peak2
    assert filecmp.cmp(flt, flt2, shallow=False) and filecmp.cmp(ani, ani2, shallow=False)


def test_weak_seed_rule_is_exercised_and_switchable(tmp_path):
    """R3's weak-seed margin (`lit > 3 * seed`: the anchor needs msl - 1 instead of msl more symbols) rests on one event
    of the reference's example (profiles/r04_lz_fit_leave_one_out.md).  On strongly diverged synthetic families the branch
    decides several regions: the product equals the oracle with the rule on (default) AND with it switched off
    (VG_LZ_WEAK_SEED=0 is read by both), and the two settings give different tables -- so the branch is really taken."""
    import filecmp
    import os
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / 'tests'))
    import oracle_lib as orc
    from vclust_amd import synth
    codes, offsets, names = synth.make_families(2, 6, length=20000, seed=5, p_lo=0.15, p_hi=0.30)
    fa = tmp_path / 'div.fna'
    synth.write_fasta(fa, codes, offsets, names)
    out = {}
    for tag, extra in (('on', {}), ('off', dict(VG_LZ_WEAK_SEED='0', VG_DEV_SWITCHES='1'))):      # (the product honours the variable only beside VG_DEV_SWITCHES)
        e = dict(os.environ, **extra)
        ani, aln, oani, oaln = (tmp_path / f'{tag}.{x}' for x in ('tsv', 'aln', 'o.tsv', 'o.aln'))
        p = subprocess.run([sys.executable, str(VCLUST), 'align', '-i', str(fa), '-o', str(ani), '--out-aln', str(aln), '--outfmt', 'complete', '-v', '0'],
                           env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        orc.run_cli('align', '-o', oani, '--out-aln', oaln, '--outfmt', 'complete', fa, env=e)
        assert filecmp.cmp(ani, oani, shallow=False), tag
        assert sorted(open(aln).read().splitlines()) == sorted(open(oaln).read().splitlines()), tag
        out[tag] = sorted(open(aln).read().splitlines())
    assert out['on'] != out['off']


@pytest.mark.parametrize('knob,alt', [('anchor_margin', 7), ('anchor_margin', 5), ('seed_choice', 1), ('weak_seed_ratio', 0)])
def test_thin_fit_constants_are_parameters(knob, alt):
    """The constants of the LZ restatement that <= 3 events of the reference's example decide are parameters of the product
    (vg_set_lz_fit) and of the checker (the same developer variables), not literals: with the alternative value the HIP rows
    still equal the oracle's on every ordered pair of strongly diverged families, and the table differs from the default
    one -- the branch is exercised both ways."""
    import os
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / 'tests'))
    import numpy as np
    import oracle_lib as orc
    from vclust_amd import api, synth
    env_name = dict(anchor_margin='VG_LZ_ANCHOR_MARGIN', seed_choice='VG_LZ_SEED_CHOICE', weak_seed_ratio='VG_LZ_WEAK_SEED')[knob]
    codes, offsets, names = synth.make_families(4, 8, length=24000, seed=7, p_lo=0.12, p_hi=0.30)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    cand = gs.read_filter(None)
    fam = np.arange(len(gs)) // 8
    tasks = gs.align_tasks(cand[fam[cand['a']] == fam[cand['b']]])
    tables = {}
    try:
        for tag, val in (('default', None), ('alt', alt)):
            api.set_lz_fit(**({knob: val} if val is not None else {}))
            if val is None: os.environ.pop(env_name, None)
            else: os.environ[env_name] = str(val)
            stats = gs.lz_align(tasks)
            for t, st in zip(tasks, stats):
                q, r = int(t['q']), int(t['r'])
                assert orc.lz_pair_stat(codes[offsets[q]:offsets[q + 1]], codes[offsets[r]:offsets[r + 1]]) == tuple(int(x) for x in st), (tag, q, r)
            tables[tag] = stats.copy()
    finally:
        api.set_lz_fit(); os.environ.pop(env_name, None)
    assert len(tasks) == 4 * 56 and not np.array_equal(tables['default'], tables['alt'])


def _torchrun(nproc, *cmd):
    import os
    import socket
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VCLUST_DIST_BACKEND='gloo')      # two ranks share the one GPU of the test box
    return subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={nproc}',
                           '--master-addr', '127.0.0.1', '--master-port', str(port), *map(str, cmd)],
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_two_ranks_write_the_same_files(tmp_path):
    """One process per rank (here both on the single GPU, gathers over gloo): the sharded prefilter
    and align produce byte-identical files to the single-process run."""
    import filecmp
    f1, a1, l1 = tmp_path / 'f1.txt', tmp_path / 'a1.tsv', tmp_path / 'l1.tsv'
    assert run('prefilter', '-i', FASTA_FILE, '-o', f1, '-v', '0').returncode == 0
    assert run('align', '-i', FASTA_FILE, '-o', a1, '--out-aln', l1, '-v', '0').returncode == 0
    f2, a2, l2 = tmp_path / 'f2.txt', tmp_path / 'a2.tsv', tmp_path / 'l2.tsv'
    p = _torchrun(2, VCLUST, 'prefilter', '-i', FASTA_FILE, '-o', f2, '-v', '0')
    assert p.returncode == 0, p.stderr[-2000:]
    p = _torchrun(2, VCLUST, 'align', '-i', FASTA_FILE, '-o', a2, '--out-aln', l2, '-v', '0')
    assert p.returncode == 0, p.stderr[-2000:]
    assert filecmp.cmp(f1, f2, shallow=False)
    assert filecmp.cmp(a1, a2, shallow=False)
    assert sorted(open(l1).read().splitlines()) == sorted(open(l2).read().splitlines())
    # without --out-aln the ranks start from the candidate pairs (vg_lz_align_pairs_sharded), with and without a filter
    a3, a4 = tmp_path / 'a3.tsv', tmp_path / 'a4.tsv'
    p = _torchrun(2, VCLUST, 'align', '-i', FASTA_FILE, '-o', a3, '-v', '0')
    assert p.returncode == 0, p.stderr[-2000:]
    assert filecmp.cmp(a1, a3, shallow=False)
    assert run('align', '-i', FASTA_FILE, '-o', a4, '--filter', f1, '-v', '0').returncode == 0
    p = _torchrun(2, VCLUST, 'align', '-i', FASTA_FILE, '-o', tmp_path / 'a5.tsv', '--filter', f2, '-v', '0')
    assert p.returncode == 0, p.stderr[-2000:]
    assert filecmp.cmp(a4, tmp_path / 'a5.tsv', shallow=False)


def test_two_ranks_align_from_pairs(tmp_path):
    """vg_lz_align_pairs_sharded on two ranks (both on the single GPU, gathers over gloo): every rank receives the canonical
    task list and exactly the rows of the single-process vg_align_tasks + vg_lz_align."""
    script = tmp_path / 'two_rank_pairs.py'
    script.write_text("""
import sys
sys.path.insert(0, %r)
import numpy as np
from vclust_amd import api, synth, distributed as D
dist, dev = D.init_process_group()
api.set_device(0)
comm = D.make_comm(dist, dev)
codes, offsets, names = synth.make_families(40, 5, length=9000, seed=21)
gs = api.GenomeSet.from_codes(codes, offsets, names)
sizes, pairs = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20)
cand = gs.filter_pairs(sizes, pairs)
tasks, stats = D.align_pairs(gs, cand, comm)
ref_tasks = gs.align_tasks(cand)
assert len(cand) > 300 and np.array_equal(tasks, ref_tasks), (len(cand), len(tasks), len(ref_tasks))
ref = gs.lz_align(ref_tasks)
assert np.array_equal(stats, ref), int((stats != ref).sum())
print('pairs ok rank', dist.get_rank(), flush=True)
comm.close(); dist.destroy_process_group()
""" % str(ROOT))
    p = _torchrun(2, script)
    assert p.returncode == 0 and p.stdout.count('pairs ok rank') == 2, (p.stdout[-500:], p.stderr[:3000])


@pytest.mark.parametrize('nproc', [2, 3])
def test_ranks_exchange_kept_masks(tmp_path, nproc):
    """vg_kmer_shared_sharded on a set with two partition levels (4.5 M bases): every rank scans 1/world of the bases and the
    kept masks + level-1 counts travel (here: the all-to-all emulated over the callback communicator's all-gather, ranks
    sharing the one GPU).  Every rank receives the sizes and pairs of the single-process pass."""
    script = tmp_path / 'mask_exchange.py'
    script.write_text("""
import sys
sys.path.insert(0, %r)
import numpy as np
from vclust_amd import api, synth, distributed as D
dist, dev = D.init_process_group()
api.set_device(0)
comm = D.make_comm(dist, dev)
codes, offsets, names = synth.make_families(100, 5, length=9000, seed=31)
gs = api.GenomeSet.from_codes(codes, offsets, names)
api.profile_enable(True); api.profile_reset()
sizes, pairs = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20)
scopes = {e['name'] for e in api.profile_get()}
api.profile_enable(False)
s0, p0 = gs.kmer_shared(k=25, min_shared=20)
p0 = np.sort(p0, order=['a', 'b'])
assert 'kmer_slice_scan' in scopes, scopes
assert np.array_equal(sizes, s0) and np.array_equal(pairs, p0) and len(p0) > 500, (len(pairs), len(p0))
print('masks ok rank', dist.get_rank(), flush=True)
comm.close(); dist.destroy_process_group()
""" % str(ROOT))
    p = _torchrun(nproc, script)
    assert p.returncode == 0 and p.stdout.count('masks ok rank') == nproc, (p.stdout[-500:], p.stderr[:3000])


def test_four_processes_write_the_files_of_one(tmp_path):
    """World 4 as FOUR REAL PROCESSES (sharing the one GPU of the test box, exchanges over gloo through the callback
    communicator): configs[1] -- phage-1k, 1 000 x 40 kb -- through `torchrun ... vclust.py prefilter` / `align --filter` =
    vg_prefilter_sharded / vg_align_sharded.  The prefilter takes the sliced scan (every rank scans a quarter of the bases, the
    kept masks and level-1 counts travel in the all-to-all, nominations / union / counts in all-gathers), the align stage
    deals the references into four ranges and gathers rows (and, with --out-aln, regions).  Four ranks, because at most six
    processes may hold one GPU at once: the ranks, this test process and the tear-down of a one-process command
    (test_sliced_scan_equals_the_replicated_scan takes world 8 in one process).  fltr.txt, ani.tsv and the
    ids file must be the bytes one process writes; the alignment table the same multiset of lines."""
    import filecmp
    sys.path.insert(0, str(ROOT))
    from vclust_amd import synth
    codes, offsets, names, _ = synth.make_workload('phage-1k')
    fa = tmp_path / 'phage1k.fna'
    synth.write_fasta(fa, codes, offsets, names)
    f1, a1, l1 = tmp_path / 'f1.txt', tmp_path / 'a1.tsv', tmp_path / 'l1.tsv'
    assert run('prefilter', '-i', fa, '-o', f1, '-v', '0').returncode == 0
    assert run('align', '-i', fa, '-o', a1, '--filter', f1, '--out-aln', l1, '-v', '0').returncode == 0
    f4, a4, l4, b4 = tmp_path / 'f4.txt', tmp_path / 'a4.tsv', tmp_path / 'l4.tsv', tmp_path / 'b4.tsv'
    p = _torchrun(4, VCLUST, 'prefilter', '-i', fa, '-o', f4, '-v', '0')
    assert p.returncode == 0, p.stderr[-3000:]
    assert filecmp.cmp(f1, f4, shallow=False)
    p = _torchrun(4, VCLUST, 'align', '-i', fa, '-o', a4, '--filter', f4, '--out-aln', l4, '-v', '0')
    assert p.returncode == 0, p.stderr[-3000:]
    assert filecmp.cmp(a1, a4, shallow=False) and filecmp.cmp(str(a1)[:-4] + '.ids.tsv', str(a4)[:-4] + '.ids.tsv', shallow=False)
    assert sum(1 for _ in open(a4)) == 9001
    assert sorted(open(l1).read().splitlines()) == sorted(open(l4).read().splitlines())
    # without --out-aln the ranks start from the candidate pairs (vg_lz_align_pairs_sharded)
    p = _torchrun(4, VCLUST, 'align', '-i', fa, '-o', b4, '--filter', f4, '-v', '0')
    assert p.returncode == 0, p.stderr[-3000:]
    assert filecmp.cmp(a1, b4, shallow=False)


def test_ranks_that_plan_differently_are_stopped_before_the_exchange(tmp_path):
    """How a rank cuts its shard (sliced scan or not, RANGE or HASH shards) follows from PROCESS-LOCAL knobs (vg_set_subshards,
    VG_INDEX_PATH).  Two ranks on a set that takes the sliced scan; rank 1 forces sub-shards, which switches ITS
    sliced scan off: without the agreement in front of the exchange rank 0 would wait inside the all-to-all for a peer that
    never comes.  Both ranks must return the same error, naming the cause, and the communicator must still work afterwards."""
    script = tmp_path / 'plan_mismatch.py'
    script.write_text("""
import sys
sys.path.insert(0, %r)
import numpy as np
from vclust_amd import api, synth, distributed as D, _lib
dist, dev = D.init_process_group()
api.set_device(0)
comm = D.make_comm(dist, dev)
lib = _lib.load()
codes, offsets, names = synth.make_families(100, 5, length=9000, seed=31)
gs = api.GenomeSet.from_codes(codes, offsets, names)
if dist.get_rank() == 1:
    lib.vg_set_subshards(2)
try:
    D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20); raise SystemExit('ranks with different plans went on')
except _lib.VclustGpuError as e:
    assert 'plan the prefilter shard differently' in str(e), str(e)
lib.vg_set_subshards(0)
sizes, pairs = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20)
s0, p0 = gs.kmer_shared(k=25, min_shared=20)
assert np.array_equal(sizes, s0) and np.array_equal(pairs, np.sort(p0, order=['a', 'b'])) and len(p0) > 500
print('mismatch ok rank', dist.get_rank(), flush=True)
comm.close(); dist.destroy_process_group()
""" % str(ROOT))
    p = _torchrun(2, script)
    assert p.returncode == 0 and p.stdout.count('mismatch ok rank') == 2, (p.stdout[-500:], p.stderr[-3000:])


def test_two_ranks_align_from_many_pairs(tmp_path):
    """vg_lz_align_pairs_sharded with more than 2^17 candidate pairs (80 families of 60 short genomes): the listing of a
    rank's tasks and their positions in the owners' lists runs on several host threads; every rank must still receive
    exactly the rows of the single-process vg_align_tasks + vg_lz_align, in the canonical order."""
    script = tmp_path / 'two_rank_many_pairs.py'
    script.write_text("""
import sys
sys.path.insert(0, %r)
import numpy as np
from vclust_amd import api, synth, distributed as D
dist, dev = D.init_process_group()
api.set_device(0)
comm = D.make_comm(dist, dev)
codes, offsets, names = synth.make_families(80, 60, length=3000, seed=29, p_lo=0.005, p_hi=0.05)
gs = api.GenomeSet.from_codes(codes, offsets, names)
sizes, pairs = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20)        # (sorted: the same list on every rank)
cand = gs.filter_pairs(sizes, pairs)
assert len(cand) > (1 << 17), len(cand)
tasks, stats = D.align_pairs(gs, cand, comm)
ref_tasks = gs.align_tasks(cand)
assert np.array_equal(tasks, ref_tasks)
ref = gs.lz_align(ref_tasks)
assert np.array_equal(stats, ref), int((stats != ref).sum())
# ranks that pass differently ordered lists are told so, all of them (the rows could not be placed)
from vclust_amd import _lib
try:
    D.align_pairs(gs, cand[::-1] if dist.get_rank() == 1 else cand, comm); raise SystemExit('a different pair order went unnoticed')
except _lib.VclustGpuError as e:
    assert 'different candidate pair lists' in str(e), str(e)
print('many pairs ok rank', dist.get_rank(), len(cand), flush=True)
comm.close(); dist.destroy_process_group()
""" % str(ROOT))
    p = _torchrun(2, script)
    assert p.returncode == 0 and p.stdout.count('many pairs ok rank') == 2, (p.stdout[-500:], p.stderr[-3000:])


def test_rccl_failure_falls_back_to_the_callback_communicator(tmp_path):
    """Two ranks on the ONE GPU of the test box ask for the built-in RCCL communicator: RCCL refuses a device twice, every
    rank agrees on the failure before any further collective, and all fall back to the callback communicator -- the
    run completes with the right rows instead of leaving a rank inside a collective."""
    script = tmp_path / 'two_rank_rccl.py'
    script.write_text("""
import sys
sys.path.insert(0, %r)
import numpy as np
from vclust_amd import api, synth, distributed as D
dist, dev = D.init_process_group()
api.set_device(0)
comm = D.make_comm(dist, dev, kind='rccl')
codes, offsets, names = synth.make_families(12, 4, length=6000, seed=22)
gs = api.GenomeSet.from_codes(codes, offsets, names)
sizes, pairs = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20)
s0, p0 = gs.kmer_shared(k=25, min_shared=20)
assert np.array_equal(sizes, s0) and len(pairs) == len(p0)
print('fallback ok rank', dist.get_rank(), flush=True)
comm.close(); dist.destroy_process_group()
""" % str(ROOT))
    import os
    import socket
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VCLUST_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    p = subprocess.run(['timeout', '150', sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.count('fallback ok rank') == 2, (p.stdout[-500:], p.stderr[:3000])
    assert 'falling back to the callback communicator' in p.stderr


def test_bench_two_ranks_smoke():
    p = _torchrun(2, ROOT / 'bench.py', '--gpus', '2', '--steps', '1', '--warmup', '1', '--workload', 'phage-1k', '--count', '6',
                  '--no-cpu-baseline', '--no-cli-wall')
    assert p.returncode == 0, p.stderr[-2000:]
    import json
    line = [l for l in p.stdout.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 2 and d['config']['pairs_per_step'] == 6 * 45 and d['value'] > 0 and d['scaling'] == 'strong'


def test_bench_plain_run_and_full(tmp_path):
    """One GPU, six families: a plain run prints the headline line with every leg of --full null; --full adds the CLI,
    --out-aln and CPU-baseline legs and the set's sha256 (the other workloads belong to the default set only)."""
    import json
    from vclust_amd import synth

    def line(*extra):
        p = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', '1', '--steps', '1', '--warmup', '1',
                            '--workload', 'phage-1k', '--count', '6', *extra], cwd=tmp_path,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])

    plain = line()
    assert plain['n_gpus'] == 1 and plain['config']['pairs_per_step'] == 6 * 45 and plain['value'] > 0 and plain['ms_per_step'] > 0
    assert plain['full'] is False and plain['roofline'] is not None
    assert all(plain[k] is None for k in ('cli_wall', 'out_aln', 'other_workloads', 'cpu_baseline')) and plain['config']['sha256'] is None
    assert 'vs_cpu_baseline' not in plain
    full = line('--full', '--cpu-reps', '1')
    assert full['full'] is True and full['config']['pairs_per_step'] == 6 * 45 and full['value'] > 0
    assert full['cli_wall']['cli_rows_equal_step'] is True and full['cli_wall']['rows'] > 0
    assert full['out_aln']['regions'] > 0 and 'error' not in full['out_aln']
    assert full['cpu_baseline']['value'] > 0 and full['vs_cpu_baseline']['device_resident'] > 0
    assert full['other_workloads'] is None
    codes, offsets, _, _ = synth.make_workload('phage-1k', 6)
    assert full['config']['sha256'] == synth.sha256(codes, offsets)


def test_rccl_two_ranks_when_two_gpus_are_visible():
    """The built-in RCCL communicator with two ranks on two GPUs (skipped on a one-GPU box; runs unattended
    wherever the suite sees >= 2 devices): sharded results equal the single-process ones on every rank."""
    from vclust_amd import api
    if api.device_count() < 2:
        pytest.skip('needs two visible HIP devices')
    import os
    import socket
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), str(ROOT / 'tools' / 'rccl_one_rank.py')], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0 and 'rccl ok: world 2' in p.stdout, (p.stdout[-500:], p.stderr[-1500:])


def test_rccl_collectives_one_rank():
    """The sharded C-ABI entry points through the built-in RCCL communicator (ncclCommInitRank / ncclAllGather
    of the real librccl) with world size 1 (the test box has one GPU) and VG_DIST_FORCE=1, so that every exchange
    really runs ncclAllGather (nranks = 1) and every merge kernel runs: results equal the plain calls."""
    p = subprocess.run([sys.executable, str(ROOT / 'tools' / 'rccl_one_rank.py')], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert p.returncode == 0 and 'rccl ok: world 1' in p.stdout, (p.stdout[-500:], p.stderr[-1500:])


def test_forced_exchanges_with_a_callback_communicator():
    """VG_DIST_FORCE=1 with a one-rank callback communicator (the all-gather copies send to recv): the nomination /
    union / count-sum protocol of vg_kmer_shared_sharded and the row / region gathers of vg_lz_align_sharded run in
    this process and reproduce the plain calls, for min_shared = 1 and above."""
    code = r"""
import os, sys, ctypes as C
os.environ['VG_DIST_FORCE'] = '1'
sys.path.insert(0, %r)
import numpy as np
from vclust_amd import api, synth, _lib, distributed as D
lib = _lib.load()
calls = []
def ag(ctx, send, recv, nbytes, on_device):
    calls.append((int(nbytes), int(on_device)))
    if on_device:
        tmp = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        _lib.hip_copy(tmp.ctypes.data, send, nbytes, to_host=True); _lib.hip_copy(recv, tmp.ctypes.data, nbytes, to_host=False)
    else:
        C.memmove(recv, send, int(nbytes))
    return 0
cb = _lib.ALLGATHER_FN(ag)
h = C.c_void_p(); _lib.check(lib.vg_comm_create(0, 1, C.cast(cb, C.c_void_p), None, C.byref(h)))
comm = D.Comm(h, lib, keep=cb)
codes, offsets, names = synth.make_families(8, 5, length=7000, seed=12)
gs = api.GenomeSet.from_codes(codes, offsets, names)
for ms in (1, 20, 200):
    s0, p0 = gs.kmer_shared(k=25, min_shared=ms); s1, p1 = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=ms)
    o0 = np.lexsort((p0['b'], p0['a'])); o1 = np.lexsort((p1['b'], p1['a']))
    assert np.array_equal(s0, s1) and np.array_equal(p0[o0], p1[o1]), ms
assert any(d for _, d in calls)                      # device-to-device exchanges happened
# the shard's own sub-shard loop (sets beyond 2^32 positions per rank) under the same protocol: partial lists of the
# sub-shards summed in HBM, then nominated / counted as one list
lib.vg_set_subshards(3)
try:
    for ms in (1, 20):
        s0, p0 = gs.kmer_shared(k=25, min_shared=ms); s1, p1 = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=ms)
        o0 = np.lexsort((p0['b'], p0['a'])); o1 = np.lexsort((p1['b'], p1['a']))
        assert np.array_equal(s0, s1) and np.array_equal(p0[o0], p1[o1]), ('sub-shards', ms)
        assert np.array_equal(p0, p0[o0])               # the summed list comes back in (a, b) order
finally:
    lib.vg_set_subshards(0)
s1, p1 = D.prefilter_counts(gs, comm, 25, 1.0, min_shared=20)
tasks = gs.align_tasks(gs.filter_pairs(s1, p1))
st0, rg0 = gs.lz_align(tasks, want_regions=True); st1, rg1 = D.align_rows(gs, tasks, comm, None, True)
assert np.array_equal(st0, st1) and np.array_equal(rg0, rg1)
# the align stage from the candidate PAIRS (tasks listed per rank in pair order, canonical list on a helper thread)
t2, st2 = D.align_pairs(gs, gs.filter_pairs(s1, p1), comm)
assert np.array_equal(t2, tasks) and np.array_equal(st2, st0)
print('forced ok', len(calls))
""" % str(ROOT)
    p = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0 and 'forced ok' in p.stdout, (p.stdout[-500:], p.stderr[-1500:])
