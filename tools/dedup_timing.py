"""Timing of the deduplicate stage (vg_deduplicate / vg_dedup_seqs): CLI wall time on a redundant FASTA file, the
array-level call, the per-kernel profile table and the hash kernel's bandwidth.

  python tools/dedup_timing.py [--records 100000] [--length 40000] [--circular] [--json out.json]

Input: `records` records of length-1000 .. length+1000 random bases (single-line sequences); 10 % of them are copies of
an earlier original record, a third each exact, reverse-complement and lower-case.  make_redundant() is also the input
of the `slow` test in tests/test_gpu_dedup.py.

--circular: the copies are additionally rotated at random (circular genomes opened elsewhere), and every leg runs twice on
that input, in the plain mode (which then finds only the copies rotated by 0) and in circular mode; the result carries
both and their ratios.
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


def make_redundant(path, records, length, seed=7, copy_fraction=0.1, rotate=False):
    """Writes the FASTA file; -> dict(records, copies, reverse, source, kind): source[i] = the original record that record i
    copies, kind[i] = 0 exact, 1 reverse complement, 2 lower case.  rotate: every copy is also rotated by a random number
    of symbols (draws of their own: the file without rotation does not depend on the option)."""
    rng = np.random.default_rng(seed)
    rot_rng = np.random.default_rng([seed, 1 << 40])
    is_copy = rng.random(records) < copy_fraction
    is_copy[0] = False
    kind = rng.integers(0, 3, records)             # 0 exact, 1 reverse complement, 2 lower case
    comp = bytes.maketrans(b'ACGT', b'TGCA')
    originals = np.flatnonzero(~is_copy)
    source = {}
    with open(path, 'wb') as f:
        for i in range(records):
            if is_copy[i]:
                k = int(np.searchsorted(originals, i))          # originals before i
                j = int(originals[rng.integers(0, k)])
                s = original(seed, j, length)
                s = s if kind[i] == 0 else s.translate(comp)[::-1] if kind[i] == 1 else s.lower()
                if rotate:
                    k = int(rot_rng.integers(0, len(s)))
                    s = s[k:] + s[:k]
                source[i] = j
            else:
                s = original(seed, i, length)
            f.write(b'>r%d copy=%d\n' % (i, source.get(i, -1)) + s + b'\n')
    return dict(records=records, copies=int(is_copy.sum()), reverse=int((is_copy & (kind == 1)).sum()), source=source,
                kind={i: int(kind[i]) for i in source})


def kernels():
    return {k['name']: round(k['total_ms'], 3) for k in api.profile_get() if k['name'].startswith('dedup_')}


def cli_leg(fna, d, threads, circular):
    """The CLI in a fresh process: context creation, ingest, kernels, writer."""
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, str(ROOT / 'vclust.py'), 'deduplicate', '-i', str(fna), '-o', str(pathlib.Path(d) / 'nr.fna'),
                        '-t', str(threads), '-v', '1'] + (['--circular'] if circular else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
    res = dict(cli_wall_s=round(time.perf_counter() - t0, 2), cli_rc=p.returncode,
               cli_summary=[ln for ln in p.stderr.splitlines() if 'vg_deduplicate:' in ln])
    if p.returncode != 0:
        print(p.stderr, file=sys.stderr)
    for name in ('nr.fna', 'nr.fna.duplicates.txt'):
        (pathlib.Path(d) / name).unlink(missing_ok=True)
    return res


def stage_leg(fna, d, threads, circular):
    """The whole stage in this process (context warm): profile table of one call."""
    api.profile_reset()
    t0 = time.perf_counter()
    api.deduplicate_files([fna], pathlib.Path(d) / 'nr2.fna', pathlib.Path(d) / 'nr2.dup', num_threads=threads, circular=circular)
    res = dict(stage_wall_s=round(time.perf_counter() - t0, 3), stage_kernels_ms=kernels())
    (pathlib.Path(d) / 'nr2.fna').unlink()
    return res


def seqs_leg(buf, offsets, n, circular):
    """The array-level call (one buffer, no FASTA parse, no writer)."""
    rep = np.zeros(n, dtype=np.int32)
    strand = np.zeros(n, dtype=np.int8)
    off = np.zeros(n, dtype=np.int64)
    st = _lib.DedupStats()
    opt = _lib.DedupOptions(circular=int(circular))
    P = C.POINTER
    api.profile_reset()
    t0 = time.perf_counter()
    _lib.check(_lib.load().vg_dedup_seqs_ex(buf.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(P(C.c_int64)), n, C.byref(opt),
                                            rep.ctypes.data_as(P(C.c_int32)), strand.ctypes.data_as(P(C.c_int8)),
                                            off.ctypes.data_as(P(C.c_int64)), C.byref(st)))
    res = dict(seqs_wall_s=round(time.perf_counter() - t0, 3), seqs_kernels_ms=kernels(),
               seqs_stats={k: getattr(st, k) for k, _ in _lib.DedupStats._fields_})
    return res, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=100000)
    ap.add_argument('--length', type=int, default=40000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--circular', action='store_true', help='rotate the copies at random; time the plain and the circular mode on that input')
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    res = {}
    modes = [('', False), ('circular_', True)] if a.circular else [('', False)]
    with tempfile.TemporaryDirectory() as d:
        fna = pathlib.Path(d) / 'in.fna'
        t0 = time.perf_counter()
        exp = make_redundant(fna, a.records, a.length, rotate=a.circular)
        res['generate_s'] = round(time.perf_counter() - t0, 1)
        res['input_mb'] = round(fna.stat().st_size / 2**20, 1)
        res['expected'] = dict(records=exp['records'], removed=exp['copies'], reverse=exp['reverse'])
        for pre, circ in modes:
            res.update({pre + k: v for k, v in cli_leg(fna, d, a.threads, circ).items()})
        api.set_device(0)
        api.profile_enable(True)
        api.deduplicate(['ACGT', 'ACGT'])
        api.deduplicate(['ACGT', 'CGTA'], circular=True)
        for pre, circ in modes:
            res.update({pre + k: v for k, v in stage_leg(fna, d, a.threads, circ).items()})
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
        for pre, circ in modes:
            leg, rep = seqs_leg(buf, offsets, n, circ)
            res.update({pre + k: v for k, v in leg.items()})
            hash_ms = leg['seqs_kernels_ms'].get('dedup_chash' if circ else 'dedup_hash')
            if hash_ms:
                bw = 0.5 * symbols / (hash_ms * 1e-3)
                res[pre + 'hash_TBps'] = round(bw / 1e12, 3)
                res[pre + 'hash_fraction_of_hbm_peak'] = round(bw / HBM_PEAK, 3)
            if circ or not a.circular:          # (the plain mode does not find the rotated copies)
                res[pre + 'sources_match'] = all(int(rep[i]) == j for i, j in exp['source'].items())
        if a.circular:
            res['circular_over_plain'] = {k: round(res['circular_' + k] / res[k], 2) for k in ('cli_wall_s', 'stage_wall_s', 'seqs_wall_s')}
    print(json.dumps(res, indent=1))
    if a.json:
        a.json.write_text(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
