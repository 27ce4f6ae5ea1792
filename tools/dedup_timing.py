"""Timing of the deduplicate stage (vg_deduplicate / vg_dedup_seqs): CLI wall time on a redundant FASTA file, the
array-level call, the per-kernel profile table and the hash kernel's bandwidth.

  python tools/dedup_timing.py [--records 100000] [--length 40000] [--circular [--terminal-repeat 20] | --contained] [--repeat 5]
                               [--json out.json]

Input: `records` records of length-1000 .. length+1000 random bases (single-line sequences); 10 % of them are copies of
an earlier original record, a third each exact, reverse-complement and lower-case.  make_redundant() is also the input
of the `slow` test in tests/test_gpu_dedup.py.

--circular: the copies are additionally rotated at random (circular genomes opened elsewhere), and every leg runs twice on
that input, in the plain mode (which then finds only the copies rotated by 0) and in circular mode; the result carries
both and their ratios.

--circular --terminal-repeat M: every copy additionally ends with a copy of its first 0, 55 or 127 symbols (the overlap an
assembler leaves on a circular contig), and a third run of every leg takes terminal repeats of at least M symbols off first
(`trepeat_` keys: the groups dedup_trepeat and dedup_trim beside dedup_chash, the repeat counters, and the ratios to the
circular mode of the same run and input, which finds only the copies without an overlap).

--contained: 30 % of the records are replaced by fragments (a tenth of the length up to all of it, either strand) of earlier
original records, and every leg runs in the plain mode (which keeps every fragment) and in contained mode; the result
carries both, the contained mode's counters (index passes, anchor hits and candidates per record) and the ratios.

--repeat N: the in-process legs run N + 1 times; the first run is discarded and the medians are reported.
"""
import argparse
import ctypes as C
import json
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from vclust_amd import _lib, api  # noqa: E402

BASES = np.frombuffer(b'ACGT', dtype=np.uint8)
HBM_PEAK = 8e12          # bytes/s, MI355X


def original(seed, j, length):
    rng = np.random.default_rng([seed, j])
    n = int(length + rng.integers(-1000, 1001))
    return BASES[rng.integers(0, 4, n, dtype=np.uint8)].tobytes()


def make_redundant(path, records, length, seed=7, copy_fraction=0.1, rotate=False, fragment_fraction=0.0, overlaps=None):
    """Writes the FASTA file; -> dict(records, copies, reverse, source, kind): source[i] = the original record that record i
    copies, kind[i] = 0 exact, 1 reverse complement, 2 lower case.  rotate: every copy is also rotated by a random number
    of symbols (draws of their own: the file without rotation does not depend on the option).  fragment_fraction: that share
    of the records (never record 0) is replaced by a fragment of an earlier original record, a tenth of its length up to all
    of it, on either strand (draws of their own again); fragment_source[i] = that original.  overlaps: every copy also ends
    with a copy of its first k symbols, k drawn from that list (draws of their own); overlap[i] = k."""
    rng = np.random.default_rng(seed)
    rot_rng = np.random.default_rng([seed, 1 << 40])
    frag_rng = np.random.default_rng([seed, 2 << 40])
    over_rng = np.random.default_rng([seed, 3 << 40])
    is_copy = rng.random(records) < copy_fraction
    is_copy[0] = False
    kind = rng.integers(0, 3, records)             # 0 exact, 1 reverse complement, 2 lower case
    is_frag = frag_rng.random(records) < fragment_fraction
    is_frag[0] = False
    is_copy &= ~is_frag
    comp = bytes.maketrans(b'ACGT', b'TGCA')
    originals = np.flatnonzero(~is_copy & ~is_frag)
    source, fragment_source, overlap = {}, {}, {}
    with open(path, 'wb') as f:
        for i in range(records):
            if is_frag[i]:
                j = int(originals[frag_rng.integers(0, int(np.searchsorted(originals, i)))])
                s = original(seed, j, length)
                n = int(frag_rng.integers(len(s) // 10, len(s) + 1))
                at = int(frag_rng.integers(0, len(s) - n + 1))
                s = s[at:at + n]
                if frag_rng.random() < 0.5:
                    s = s.translate(comp)[::-1]
                fragment_source[i] = j
            elif is_copy[i]:
                k = int(np.searchsorted(originals, i))          # originals before i
                j = int(originals[rng.integers(0, k)])
                s = original(seed, j, length)
                s = s if kind[i] == 0 else s.translate(comp)[::-1] if kind[i] == 1 else s.lower()
                if rotate:
                    k = int(rot_rng.integers(0, len(s)))
                    s = s[k:] + s[:k]
                if overlaps:
                    overlap[i] = int(over_rng.choice(overlaps))
                    s = s + s[:overlap[i]]
                source[i] = j
            else:
                s = original(seed, i, length)
            f.write(b'>r%d copy=%d\n' % (i, source.get(i, fragment_source.get(i, -1))) + s + b'\n')
    return dict(records=records, copies=int(is_copy.sum()), reverse=int((is_copy & (kind == 1)).sum()), source=source,
                kind={i: int(kind[i]) for i in source}, fragments=int(is_frag.sum()), fragment_source=fragment_source, overlap=overlap)


def kernels():
    return {k['name']: round(k['total_ms'], 3) for k in api.profile_get() if k['name'].startswith('dedup')}


def mode_flags(mode, m):
    """the CLI options of a leg's mode ('', 'circular', 'contained', 'trepeat')"""
    return ['--circular', '--terminal-repeat', str(m)] if mode == 'trepeat' else ['--' + mode] if mode else []


def mode_keywords(mode, m):
    return dict(circular=True, terminal_repeat=m) if mode == 'trepeat' else {mode: True} if mode else {}


def cli_leg(fna, d, threads, mode, m=0):
    """The CLI in a fresh process: context creation, ingest, kernels, writer."""
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, str(ROOT / 'vclust.py'), 'deduplicate', '-i', str(fna), '-o', str(pathlib.Path(d) / 'nr.fna'),
                        '-t', str(threads), '-v', '1'] + mode_flags(mode, m),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
    res = dict(cli_wall_s=round(time.perf_counter() - t0, 2), cli_rc=p.returncode,
               cli_summary=[ln for ln in p.stderr.splitlines() if 'vg_deduplicate:' in ln])
    if p.returncode != 0:
        print(p.stderr, file=sys.stderr)
    for name in ('nr.fna', 'nr.fna.duplicates.txt'):
        (pathlib.Path(d) / name).unlink(missing_ok=True)
    return res


def median_of(runs):
    """Median wall time and per-group kernel times of the runs after the first (all of them when there is only one)."""
    runs = runs[1:] or runs
    names = sorted({k for _, kern in runs for k in kern})
    return (round(float(np.median([w for w, _ in runs])), 3),
            {k: round(float(np.median([kern.get(k, 0.0) for _, kern in runs])), 3) for k in names})


def stage_leg(fna, d, threads, mode, repeat, m=0):
    """The whole stage in this process (context warm): profile table of one call."""
    runs = []
    for _ in range(repeat + 1):
        api.profile_reset()
        t0 = time.perf_counter()
        api.deduplicate_files([fna], pathlib.Path(d) / 'nr2.fna', pathlib.Path(d) / 'nr2.dup', num_threads=threads,
                              **mode_keywords(mode, m))
        runs.append((time.perf_counter() - t0, kernels()))
        (pathlib.Path(d) / 'nr2.fna').unlink()
    wall, kern = median_of(runs)
    return dict(stage_wall_s=wall, stage_kernels_ms=kern)


def seqs_leg(buf, offsets, n, mode, repeat, m=0):
    """The array-level call (one buffer, no FASTA parse, no writer)."""
    rep = np.zeros(n, dtype=np.int32)
    strand = np.zeros(n, dtype=np.int8)
    off = np.zeros(n, dtype=np.int64)
    st = _lib.DedupStats()
    cst = _lib.DedupContainedStats()
    rst = _lib.DedupRepeatStats()
    tr = np.zeros(n, dtype=np.int64)
    opt = _lib.DedupOptions(circular=int(mode == 'circular'))
    P = C.POINTER
    lib = _lib.load()
    runs = []
    for _ in range(repeat + 1):
        api.profile_reset()
        t0 = time.perf_counter()
        if mode == 'contained':
            _lib.check(lib.vg_dedup_seqs_contained(buf.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(P(C.c_int64)), n,
                                                   rep.ctypes.data_as(P(C.c_int32)), strand.ctypes.data_as(P(C.c_int8)),
                                                   off.ctypes.data_as(P(C.c_int64)), C.byref(st), C.byref(cst)))
        elif mode == 'trepeat':
            _lib.check(lib.vg_dedup_seqs_circular_tr(buf.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(P(C.c_int64)), n, m,
                                                     rep.ctypes.data_as(P(C.c_int32)), strand.ctypes.data_as(P(C.c_int8)),
                                                     off.ctypes.data_as(P(C.c_int64)), tr.ctypes.data_as(P(C.c_int64)), C.byref(st),
                                                     C.byref(rst)))
        else:
            _lib.check(lib.vg_dedup_seqs_ex(buf.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(P(C.c_int64)), n, C.byref(opt),
                                            rep.ctypes.data_as(P(C.c_int32)), strand.ctypes.data_as(P(C.c_int8)),
                                            off.ctypes.data_as(P(C.c_int64)), C.byref(st)))
        runs.append((time.perf_counter() - t0, kernels()))
    wall, kern = median_of(runs)
    res = dict(seqs_wall_s=wall, seqs_kernels_ms=kern, seqs_stats={k: getattr(st, k) for k, _ in _lib.DedupStats._fields_})
    if mode == 'contained':
        res['seqs_contained_stats'] = {k: getattr(cst, k) for k, _ in _lib.DedupContainedStats._fields_}
        res['hits_per_record'] = round(cst.hits / n, 2)
        res['candidates_per_record'] = round(cst.candidates / n, 2)
    if mode == 'trepeat':
        res['seqs_repeat_stats'] = {k: getattr(rst, k) for k, _ in _lib.DedupRepeatStats._fields_}
        res['candidates_per_record'] = round(rst.candidates / n, 3)
        res['repeats'] = tr.copy()
    return res, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=100000)
    ap.add_argument('--length', type=int, default=40000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--circular', action='store_true', help='rotate the copies at random; time the plain and the circular mode on that input')
    ap.add_argument('--terminal-repeat', type=int, default=0, metavar='M',
                    help='with --circular: give every copy an overlap of 0, 55 or 127 symbols; time the circular mode with and without '
                         '--terminal-repeat M on that input')
    ap.add_argument('--contained', action='store_true',
                    help='replace 30 %% of the records by fragments of others; time the plain and the contained mode on that input')
    ap.add_argument('--repeat', type=int, default=1, help='timed runs of the in-process legs after one discarded run; medians are reported')
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    if a.circular and a.contained:
        ap.error('--circular and --contained are two inputs: one run each')
    if a.terminal_repeat and not a.circular:
        ap.error('--terminal-repeat needs --circular')
    res = {}
    m = a.terminal_repeat
    extra = 'circular' if a.circular else 'contained' if a.contained else ''
    modes = (['', extra] if extra else ['']) + (['trepeat'] if m else [])
    with tempfile.TemporaryDirectory() as d:
        fna = pathlib.Path(d) / 'in.fna'
        t0 = time.perf_counter()
        exp = make_redundant(fna, a.records, a.length, rotate=a.circular, fragment_fraction=0.3 if a.contained else 0.0,
                             overlaps=[0, 55, 127] if m else None)
        res['generate_s'] = round(time.perf_counter() - t0, 1)
        res['input_mb'] = round(fna.stat().st_size / 2**20, 1)
        res['expected'] = dict(records=exp['records'], removed=exp['copies'], reverse=exp['reverse'], fragments=exp['fragments'])
        for mode in modes:
            res.update({(mode and mode + '_') + k: v for k, v in cli_leg(fna, d, a.threads, mode, m).items()})
        api.set_device(0)
        api.profile_enable(True)
        api.deduplicate(['ACGT', 'ACGT'])
        api.deduplicate(['ACGT', 'CGTA'], circular=True)
        api.deduplicate(['ACGT', 'CGT'], contained=True)
        api.deduplicate(['ACGTAC', 'CGTA'], circular=True, terminal_repeat=2)
        for mode in modes:
            res.update({(mode and mode + '_') + k: v for k, v in stage_leg(fna, d, a.threads, mode, a.repeat, m).items()})
        # the sequences back to back
        text = fna.read_bytes()
        arr = np.frombuffer(text, dtype=np.uint8)
        nl = np.flatnonzero(arr == ord('\n'))              # (two lines per record: header, sequence)
        seq_beg, seq_end = nl[0::2] + 1, nl[1::2]
        n = len(seq_beg)
        lens = seq_end - seq_beg
        buf = np.empty(int(lens.sum()), dtype=np.uint8)
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lens)
        for i in range(n):
            buf[offsets[i]:offsets[i + 1]] = arr[seq_beg[i]:seq_end[i]]
        del text, arr
        symbols = int(lens.sum())
        res['symbols'] = symbols
        for mode in modes:
            pre = mode and mode + '_'
            leg, rep = seqs_leg(buf, offsets, n, mode, a.repeat, m)
            repeats = leg.pop('repeats', None)
            res.update({pre + k: v for k, v in leg.items()})
            hash_ms = leg['seqs_kernels_ms'].get('dedup_chash' if mode in ('circular', 'trepeat') else 'dedup_hash')
            if hash_ms:
                bw = 0.5 * symbols / (hash_ms * 1e-3)
                res[pre + 'hash_TBps'] = round(bw / 1e12, 3)
                res[pre + 'hash_fraction_of_hbm_peak'] = round(bw / HBM_PEAK, 3)
            if mode == 'trepeat':
                res[pre + 'sources_match'] = all(int(rep[i]) == j for i, j in exp['source'].items())
                res[pre + 'repeats_match'] = all(int(repeats[i]) == exp['overlap'].get(i, 0) for i in range(n))
            elif (mode == 'circular' and not m) or not a.circular:   # (the plain mode does not find the rotated copies, the circular mode not those with an overlap)
                res[pre + 'sources_match'] = all(int(rep[i]) == j for i, j in exp['source'].items())
            if mode == 'contained':
                res[pre + 'fragment_sources_match'] = all(int(rep[i]) == j for i, j in exp['fragment_source'].items())
        if m:
            res['trepeat_over_circular'] = {k: round(res['trepeat_' + k] / res['circular_' + k], 2)
                                            for k in ('cli_wall_s', 'stage_wall_s', 'seqs_wall_s')}
        if extra:
            res[extra + '_over_plain'] = {k: round(res[extra + '_' + k] / res[k], 2) for k in ('cli_wall_s', 'stage_wall_s', 'seqs_wall_s')}
    print(json.dumps(res, indent=1))
    if a.json:
        a.json.write_text(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
