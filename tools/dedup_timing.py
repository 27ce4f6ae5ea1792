"""Timing of the deduplicate stage (vg_deduplicate / vg_dedup_seqs): CLI wall time on a redundant FASTA file, the
array-level call, the per-kernel profile table and the hash kernel's bandwidth.

  python tools/dedup_timing.py [--records 100000] [--length 40000] [--json out.json]

Input: `records` records of length-1000 .. length+1000 random bases (single-line sequences); 10 % of them are copies of
an earlier original record, a third each exact, reverse-complement and lower-case.  make_redundant() is also the input
of the `slow` test in tests/test_gpu_dedup.py.
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


def make_redundant(path, records, length, seed=7, copy_fraction=0.1):
    """Writes the FASTA file; -> dict(records, copies, reverse, source, kind): source[i] = the original record that record i
    copies, kind[i] = 0 exact, 1 reverse complement, 2 lower case."""
    rng = np.random.default_rng(seed)
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
                source[i] = j
            else:
                s = original(seed, i, length)
            f.write(b'>r%d copy=%d\n' % (i, source.get(i, -1)) + s + b'\n')
    return dict(records=records, copies=int(is_copy.sum()), reverse=int((is_copy & (kind == 1)).sum()), source=source,
                kind={i: int(kind[i]) for i in source})


def kernels():
    return {k['name']: round(k['total_ms'], 3) for k in api.profile_get() if k['name'].startswith('dedup_')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--records', type=int, default=100000)
    ap.add_argument('--length', type=int, default=40000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    res = {}
    with tempfile.TemporaryDirectory() as d:
        fna = pathlib.Path(d) / 'in.fna'
        t0 = time.perf_counter()
        exp = make_redundant(fna, a.records, a.length)
        res['generate_s'] = round(time.perf_counter() - t0, 1)
        res['input_mb'] = round(fna.stat().st_size / 2**20, 1)
        # the CLI, a fresh process: context creation, ingest, kernels, writer
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, str(ROOT / 'vclust.py'), 'deduplicate', '-i', str(fna), '-o', str(pathlib.Path(d) / 'nr.fna'),
                            '-t', str(a.threads), '-v', '1'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
        res['cli_wall_s'] = round(time.perf_counter() - t0, 2)
        res['cli_rc'] = p.returncode
        res['cli_summary'] = [ln for ln in p.stderr.splitlines() if 'vg_deduplicate:' in ln]
        if p.returncode != 0:
            print(p.stderr, file=sys.stderr)
        for name in ('nr.fna', 'nr.fna.duplicates.txt'):
            (pathlib.Path(d) / name).unlink(missing_ok=True)
        res['expected'] = dict(records=exp['records'], removed=exp['copies'], reverse=exp['reverse'])
        # the whole stage in this process (context warm): profile table of one call
        api.set_device(0)
        api.profile_enable(True)
        api.deduplicate(['ACGT', 'ACGT'])
        api.profile_reset()
        t0 = time.perf_counter()
        api.deduplicate_files([fna], pathlib.Path(d) / 'nr2.fna', pathlib.Path(d) / 'nr2.dup', num_threads=a.threads)
        res['stage_wall_s'] = round(time.perf_counter() - t0, 3)
        res['stage_kernels_ms'] = kernels()
        (pathlib.Path(d) / 'nr2.fna').unlink()
        # the array-level call on the same sequences (one buffer, no FASTA parse, no writer)
        text = fna.read_bytes()
        arr = np.frombuffer(text, dtype=np.uint8)
        nl = np.flatnonzero(arr == ord('\n'))              # (two lines per record: header, sequence)
        seq_beg, seq_end = nl[0::2] + 1, nl[1::2]
        n = len(seq_beg)
        # the sequences back to back
        lens = seq_end - seq_beg
        buf = np.empty(int(lens.sum()), dtype=np.uint8)
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lens)
        for i in range(n):
            buf[offsets[i]:offsets[i + 1]] = arr[seq_beg[i]:seq_end[i]]
        del text, arr
        rep = np.zeros(n, dtype=np.int32)
        strand = np.zeros(n, dtype=np.int8)
        st = _lib.DedupStats()
        P = C.POINTER
        api.profile_reset()
        t0 = time.perf_counter()
        _lib.check(_lib.load().vg_dedup_seqs(buf.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(P(C.c_int64)), n,
                                             rep.ctypes.data_as(P(C.c_int32)), strand.ctypes.data_as(P(C.c_int8)), C.byref(st)))
        res['seqs_wall_s'] = round(time.perf_counter() - t0, 3)
        res['seqs_kernels_ms'] = kern = kernels()
        res['seqs_stats'] = {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}
        symbols = int(lens.sum())
        res['symbols'] = symbols
        if kern.get('dedup_hash'):
            bw = 0.5 * symbols / (kern['dedup_hash'] * 1e-3)
            res['hash_TBps'] = round(bw / 1e12, 3)
            res['hash_fraction_of_hbm_peak'] = round(bw / HBM_PEAK, 3)
        ok = all(int(rep[i]) == j for i, j in exp['source'].items())
        res['sources_match'] = ok
    print(json.dumps(res, indent=1))
    if a.json:
        a.json.write_text(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
