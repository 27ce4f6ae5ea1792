"""Shared checks of the LZ align stage against the CPU oracle and against a plain restatement of the reference index
-- TEST INFRASTRUCTURE ONLY (not a conftest, no fixtures: the test modules import it).

  * assert_rows_and_regions: every task of a gs.lz_align(..., want_regions=True) call against orc.lz_pair_stat (rows) and
    orc.lz_regions (the task's regions as an ordered list of 5-tuples);
  * predicted_plan / check_index: the build path, pos_bits and tag_bits the plan must choose for a reference length, and
    the dumped index (GenomeSet.lz_index_dump) against RR restated in numpy;
  * run as a program (`python tests/lz_checks.py job.npz out.npz`) it is the child process of the tests whose run needs
    developer switches (read once per process): it aligns, dumps the indexes asked for and hands the arrays back.
"""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent

DEFAULT_LZ = dict(mal=11, msl=7, mrd=40, mqd=40, reg=35, aw=15, am=7, ar=3)

# ---- the constants of the plan, restated (vclust_amd/csrc/vg_align.hip)
REG_MAX_RR = 4 * 1024 * 24 - 256      # `constexpr int REG_MAX_RR = 4 * 1024 * REG_IT - 256` (REG_IT = 24)
MID_MAX_RR = 1 << 19                  # `constexpr int MID_MAX_RR = 1 << 19`
LDS_MAX_RR = 1 << 21                  # lz_plan_references: `small = n_rr <= (1 << 21) && p->msl <= 7`
PATH_MID, PATH_LDS, PATH_GLOBAL = 6, 7, 8


def predicted_plan(L, lz=None, lds_build=False):
    """(path, pos_bits, tag_bits) of a reference of L bases: lz_plan_references restated.  path 0..5 = the register build
    of 24, 20, 16, 12, 8, 4 trips (`trips = (n_rr + 256 + 4095) / 4096`, a reference takes the smallest that holds it),
    6 mid, 7 lds, 8 global; lds_build: VG_LZ_BUILD=lds (no register and no mid build)."""
    p = {**DEFAULT_LZ, **(lz or {})}
    n_rr = 2 * L + 1
    pos_bits = 1 if n_rr <= 2 else int(n_rr - 1).bit_length()          # the smallest pb >= 1 with 2^pb >= n_rr
    tag_bits = max(0, min(2 * (p['mal'] - p['msl']), 14, 32 - pos_bits))
    small = n_rr <= LDS_MAX_RR and p['msl'] <= 7
    if small and n_rr <= REG_MAX_RR and not lds_build:
        trips = (n_rr + 256 + 4095) // 4096
        path = 0 if trips > 20 else 1 if trips > 16 else 2 if trips > 12 else 3 if trips > 8 else 4 if trips > 4 else 5
    elif small and n_rr <= MID_MAX_RR and not lds_build:
        path = PATH_MID
    elif small:
        path = PATH_LDS
    else:
        path = PATH_GLOBAL
    return path, pos_bits, tag_bits


# ---- inputs
def rand_seq(rng, n):
    return rng.integers(0, 4, int(n)).astype(np.uint8)


def revcomp(s):
    return (3 - s)[::-1].copy()


def ends_query(rng, R):
    """R[:w] | 200 random | R[-w:] | 200 random | rc(R)[:w] | 200 random | rc(R)[-w:], w = min(3000, L // 3)"""
    w = min(3000, len(R) // 3)
    rc = revcomp(R)
    return np.concatenate([R[:w], rand_seq(rng, 200), R[len(R) - w:], rand_seq(rng, 200), rc[:w], rand_seq(rng, 200), rc[len(R) - w:]])


def mutated(rng, R, rate=0.04):
    s = R.copy()
    at = np.flatnonzero(rng.random(len(R)) < rate)
    s[at] = (s[at] + rng.integers(1, 4, len(at)).astype(np.uint8)) % 4
    return s


def with_n_runs(s):
    """N (code 4) over bases 0..4, over 7 bases across L / 2 and over the last 10 bases"""
    s = s.copy()
    L = len(s)
    s[:5] = 4
    s[L // 2 - 3:L // 2 + 4] = 4
    s[L - 10:] = 4
    return s


def flanked(rng, R):
    return np.concatenate([rand_seq(rng, 50), R, rand_seq(rng, 50)])


def pack(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)).astype(np.uint8), offsets


# ---- rows and regions of a call against the oracle
def oracle_of(orc, codes, offsets, tasks, lz=None, cache=None):
    """{(q, r): (row, regions)} of every task, from the oracle; `cache` (a dict) keeps them between runs of one set"""
    out = cache if cache is not None else {}
    for t in tasks:
        key = (int(t['q']), int(t['r']))
        if key not in out:
            q = codes[offsets[key[0]]:offsets[key[0] + 1]]
            r = codes[offsets[key[1]]:offsets[key[1] + 1]]
            out[key] = (orc.lz_pair_stat(q, r, lz), orc.lz_regions(q, r, lz))
    return out


def _tuples(a):
    return list(zip(a['qstart'].tolist(), a['qend'].tolist(), a['rstart'].tolist(), a['rend'].tolist(), a['n_match'].tolist()))


def one_run_per_task(region_task, n_regions):
    """A task's regions are contiguous in the output: the task ids form exactly one run per task that has regions (the
    number of run starts equals the number of tasks with n_regions > 0)"""
    tk = np.asarray(region_task)
    runs = (1 + int(np.count_nonzero(tk[1:] != tk[:-1]))) if len(tk) else 0
    return runs == int(np.count_nonzero(np.asarray(n_regions) > 0))


def assert_rows_and_regions(orc, codes, offsets, tasks, stats, regions, lz=None, cache=None, what=''):
    """Every task: its row equals orc.lz_pair_stat, and (regions is not None) its regions equal orc.lz_regions as an
    ordered list of (qstart, qend, rstart, rend, n_match).  No task is sampled away; every region belongs to a task."""
    ref = oracle_of(orc, codes, offsets, tasks, lz, cache)
    assert len(stats) == len(tasks), (what, len(stats), len(tasks))
    by_task = None
    if regions is not None:
        assert len(regions) == 0 or int(regions['task'].max()) < len(tasks), (what, 'a region names no task')
        assert one_run_per_task(regions['task'], stats['n_regions']), (what, "a task's regions are not contiguous in the output")
        order = np.argsort(regions['task'], kind='stable')          # (a no-op after the line above: kept so that a failure names tasks)
        sorted_regions = regions[order]
        first = np.searchsorted(sorted_regions['task'], np.arange(len(tasks) + 1))
        by_task = (sorted_regions, first)
    bad_rows, bad_regions = [], []
    for i, (t, s) in enumerate(zip(tasks, stats)):
        key = (int(t['q']), int(t['r']))
        row, regs = ref[key]
        got = (int(s['n_match']), int(s['aln_len']), int(s['n_regions']))
        if got != row:
            bad_rows.append((key, row, got))
        if by_task is not None:
            mine = _tuples(by_task[0][by_task[1][i]:by_task[1][i + 1]])
            want = _tuples(regs)
            if mine != want:
                k = next((j for j, (a, b) in enumerate(zip(mine, want)) if a != b), min(len(mine), len(want)))
                bad_regions.append((key, len(want), len(mine), k, want[k:k + 2], mine[k:k + 2]))
    assert not bad_rows, (what, len(bad_rows), bad_rows[:5])
    assert not bad_regions, (what, len(bad_regions), bad_regions[:3])
    return ref


# ---- the index against RR restated in numpy
def check_index(seq, dump, lz=None, what=''):
    """The dumped index of the reference `seq` (codes 0..3, > 3 = N) against the contract of DESIGN.md section 3 and of
    ref_desc, read off the plain global build (k_index_pass) and restated WITHOUT decoding bucket numbers or tag values:

      RR = fwd | separator | rc (n_rr = 2 L + 1 symbols; the separator and every N are masked);
      admission: position p has an entry iff p + msl <= n_rr and none of RR[p .. p + msl - 1] is masked (k_index_pass:
        `p + msl <= rd.n_rr && (m & ((1 << msl) - 1)) == 0`) -- so the msl-mer lies in one strand and holds no N;
      entry = p | tag << pos_bits, every admitted p exactly once; bucket_end is non-decreasing and ends at n_entries;
      one bucket = one msl-mer: all its positions spell the same msl symbols, two non-empty buckets different ones;
      order inside a bucket: NONE is promised.  k_index_pass places entries by atomicAdd, and the parse (scan4 in
        lz_parse_body) walks the whole bucket and breaks ties on the position itself ("ties -> smallest position"), so
        only the SET of a bucket is asserted;
      tag (tag_of): the bits of the tag_bits / 2 bases behind the msl-mer; for an odd tag_bits the low plane keeps one bit
        more (`tl = (tag_bits + 1) >> 1, th = tag_bits >> 1`): of the last base only bit 0 of its code survives (A / G
        against C / T).  The planes are zero where RR is masked and behind RR (rr_chunk_planes: `lo & ~mask`), so a tag
        window that runs into an N, the separator or past the end of RR reads code 0 (A) there.  Asserted as: within a
        bucket two entries have equal tags iff these keys are equal.
    """
    p = {**DEFAULT_LZ, **(lz or {})}
    msl = p['msl']
    L = len(seq)
    n_rr = 2 * L + 1
    bucket_end = np.asarray(dump['bucket_end']).astype(np.int64)
    entries = np.asarray(dump['entries'])
    pos_bits, tag_bits = int(dump['pos_bits']), int(dump['tag_bits'])
    assert len(bucket_end) == 4 ** msl, what
    fwd = np.asarray(seq, dtype=np.uint8)
    masked = np.ones(n_rr + 64, dtype=bool)                  # the separator and everything behind RR
    sym = np.zeros(n_rr + 64, dtype=np.int64)                # code 0 where masked
    masked[:L] = fwd > 3
    masked[L + 1:n_rr] = (fwd > 3)[::-1]
    sym[:L] = np.where(fwd > 3, 0, fwd)
    sym[L + 1:n_rr] = np.where(fwd > 3, 0, 3 - fwd.astype(np.int64))[::-1]
    # admission
    cm = np.concatenate([[0], np.cumsum(masked)])
    ps = np.arange(n_rr)
    admitted = ps[(ps + msl <= n_rr) & (cm[np.minimum(ps + msl, n_rr + 64)] - cm[ps] == 0)]
    assert len(entries) == len(admitted), (what, 'entries', len(entries), 'admitted positions', len(admitted))
    assert np.all(np.diff(bucket_end) >= 0), (what, 'bucket_end decreases')
    assert int(bucket_end[-1]) == len(entries), (what, int(bucket_end[-1]), len(entries))
    if len(entries) == 0:
        return 0
    pos = (entries & np.uint32((1 << pos_bits) - 1)).astype(np.int64)
    tag = (entries >> np.uint32(pos_bits)).astype(np.int64) if pos_bits < 32 else np.zeros(len(entries), np.int64)
    assert np.array_equal(np.sort(pos), admitted), (what, 'the indexed positions are not exactly the admitted ones, each once')
    assert int(tag.max()) < (1 << tag_bits), (what, 'a tag needs more than tag_bits bits', int(tag.max()), tag_bits)
    # one bucket = one msl-mer
    mer = np.zeros(n_rr, dtype=np.int64)
    for j in range(msl):
        mer = mer * 4 + sym[j:j + n_rr]
    bucket = np.searchsorted(bucket_end, np.arange(len(entries)), side='right')      # bucket of every entry slot
    em = mer[pos]
    pairs = np.unique(bucket.astype(np.int64) * (1 << 24) + em)       # (bucket, msl-mer) couples; both < 4^12 = 2^24
    assert len(np.unique(pairs >> 24)) == len(pairs), (what, 'a bucket holds two different msl-mers')
    assert len(np.unique(pairs & ((1 << 24) - 1))) == len(pairs), (what, 'one msl-mer lies in two buckets')
    # tags
    tl, th = (tag_bits + 1) >> 1, tag_bits >> 1
    key = np.zeros(n_rr, dtype=np.int64)
    for j in range(tl):
        s = sym[msl + j:msl + j + n_rr]
        key = key * 4 + (s if j < th else (s & 1))
    ek = key[pos]
    b64 = bucket.astype(np.int64)                                      # (key, tag < 2^14)
    n_bk = len(np.unique(b64 * (1 << 14) + ek))
    n_bt = len(np.unique(b64 * (1 << 14) + tag))
    n_bkt = len(np.unique((b64 * (1 << 14) + ek) * (1 << 14) + tag))
    assert n_bk == n_bt == n_bkt, (what, 'within a bucket, equal tags <=> equal bases behind the msl-mer fails',
                                   dict(keys=n_bk, tags=n_bt, key_tag_pairs=n_bkt, tag_bits=tag_bits))
    return len(entries)


# ---- the child process
def run_child(job_dir, name, codes, offsets, tasks, lz=None, env=None, want_regions=True, dump=(), plan_of=(), budget=0, timeout=600):
    """One child process (developer switches are read once per process): align `tasks`, dump the indexes of the genomes
    `dump` and report (path, pos_bits, tag_bits) of the genomes `plan_of` -> dict(stats, regions or None,
    dumps {genome: dict}, plans {genome: (path, pos_bits, tag_bits)}).  Asserts the child's return code."""
    job_dir = pathlib.Path(job_dir)
    fin, fout = job_dir / f'{name}.job.npz', job_dir / f'{name}.out.npz'
    dump = list(dump)
    every = dump + [g for g in plan_of if g not in set(dump)]
    np.savez(fin, codes=codes, offsets=offsets, tasks=tasks, dump=np.asarray(every, dtype=np.int64), n_full=len(dump),
             spec=np.array(json.dumps(dict(lz=lz or {}, want_regions=bool(want_regions), budget=int(budget)))))
    full_env = dict(os.environ)
    if env:
        full_env.update(VG_DEV_SWITCHES='1', **env)
    p = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), str(fin), str(fout)], env=full_env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, (name, p.returncode, p.stderr[-2000:])
    d = np.load(fout)
    dumps, plans = {}, {}
    for i, gi in enumerate(d['dump'].tolist()):
        pos_bits, tag_bits, path = (int(x) for x in d['plan'][i])
        plans[gi] = (path, pos_bits, tag_bits)
        if i < len(dump):
            dumps[gi] = dict(bucket_end=d[f'bucket_end_{i}'], entries=d[f'entries_{i}'], pos_bits=pos_bits, tag_bits=tag_bits, path=path)
    return dict(stats=d['stats'], regions=d['regions'] if 'regions' in d.files else None, dumps=dumps, plans=plans)


def _child_main(fin, fout):
    sys.path.insert(0, str(ROOT))
    from vclust_amd import _lib, api
    d = np.load(fin)
    spec = json.loads(str(d['spec']))
    codes, offsets, tasks = d['codes'], d['offsets'], d['tasks'].astype(api.TASK_DTYPE)
    lz = spec['lz'] or None
    gs = api.GenomeSet.from_codes(codes, offsets, ['s%d' % i for i in range(len(offsets) - 1)])
    out = {}
    if spec['budget']:
        _lib.load().vg_set_index_budget(int(spec['budget']))
    try:
        if len(tasks) and spec['want_regions']:
            out['stats'], out['regions'] = gs.lz_align(tasks, lz=lz, want_regions=True)
        elif len(tasks):
            out['stats'] = gs.lz_align(tasks, lz=lz)
        else:
            out['stats'] = np.zeros(0, dtype=api.STAT_DTYPE)
    finally:
        if spec['budget']:
            _lib.load().vg_set_index_budget(24 << 30)         # the library's default
    plan = np.zeros((len(d['dump']), 3), dtype=np.int64)
    for i, gi in enumerate(d['dump'].tolist()):
        x = gs.lz_index_dump(gi, lz=lz)
        plan[i] = (x['pos_bits'], x['tag_bits'], x['path'])
        if i < int(d['n_full']):
            out[f'bucket_end_{i}'] = np.array(x['bucket_end'])
            out[f'entries_{i}'] = np.array(x['entries'])
    np.savez(fout, dump=d['dump'], plan=plan, **out)


if __name__ == '__main__':
    _child_main(sys.argv[1], sys.argv[2])
