"""Timing of dereplicate (GenomeSet.dereplicate_set) beside the three-step path it stands for, array level,
in one process.

  python tools/derep_timing.py [--families 200] [--members 500] [--length 40000] [--p-lo 0.001] [--p-hi 0.03] [--batches 1024 4096 16384] [--runs 3]
                               [--tani 0.95] [--json profiles/derep_timing_<workload>.json]

The set is vclust_amd.synth.make_families with many members per family: a redundant set, the case dereplicate is for.
  three-step   kmer_shared -> filter_pairs -> align_tasks -> lz_align -> cluster_graph('cd-hit') on the rows with tani >= the
               threshold (tani from the integers, in numpy: the file route's last printed digit is not reproduced here, so the two
               results are compared and the comparison is reported, not asserted)
  dereplicate  dereplicate_set, once per batch size
Protocol: every path is run once and discarded, then `--runs` times with the profile scopes on; reported are the median and the range
of the wall time, the profile scopes of the median run, the pairs aligned on both sides, the batches and the share of `derep_subset`.
Beside it, as a sanity figure only: one subset of the whole set (the gather kernel) against a device-to-device copy of the same
bytes (hipMemcpy, wall time).  One JSON line on stdout; --json also writes it to a file."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
K, MIN_KMERS, MIN_IDENT = 25, 20, 0.7


def timed(api, fn):
    api.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    return out, round(wall, 2), {e['name']: round(e['total_ms'], 3) for e in api.profile_get()}


def measure(api, fn, runs):
    """one run discarded, `runs` timed -> (result of the last run, dict(median_ms, min_ms, max_ms, scopes of the median run))"""
    fn()
    got = [timed(api, fn) for _ in range(runs)]
    walls = [g[1] for g in got]
    med = sorted(range(runs), key=lambda i: walls[i])[runs // 2]
    return got[-1][0], dict(median_ms=statistics.median(walls), min_ms=min(walls), max_ms=max(walls), scopes=got[med][2])


def three_step(api, np, gs, lengths, rank, tani):
    sizes, pairs = gs.kmer_shared(k=K, min_shared=MIN_KMERS)
    cand = gs.filter_pairs(sizes, pairs, k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT)
    tasks = gs.align_tasks(cand)
    stats = gs.lz_align(tasks)
    q, r = tasks['q'].astype(np.int64), tasks['r'].astype(np.int64)
    both = stats['n_match'].astype(np.int64)
    both = both + both.reshape(-1, 2)[:, ::-1].reshape(-1)            # the task and its reverse are neighbours
    w = both / (lengths[q] + lengths[r])
    keep = w >= tani
    label, rep, _ = api.cluster_graph(len(lengths), rank[q[keep]], rank[r[keep]], w[keep], 'cd-hit')
    return rep, len(cand)


def subset_against_copy(api, gs, runs):
    """the gather of the whole set against a device-to-device copy of the bytes it reads (2-bit codes + mask), hipMemcpy through ctypes"""
    ids = list(range(len(gs)))
    gs.subset(ids)
    times, moved = [], 0
    for _ in range(runs):
        api.profile_reset()
        gs.subset(ids)
        e = {p['name']: p for p in api.profile_get()}['derep_subset']
        times.append(e['total_ms'])
        moved = e['bytes']
    out = dict(bytes_read_and_written=moved, derep_subset_ms=[round(t, 3) for t in times])
    try:
        import ctypes as C
        hip = C.CDLL('libamdhip64.so')
        n = int(moved // 2)
        a, b = C.c_void_p(), C.c_void_p()
        if hip.hipMalloc(C.byref(a), C.c_size_t(n)) or hip.hipMalloc(C.byref(b), C.c_size_t(n)):
            raise RuntimeError('hipMalloc failed')
        copies = []
        for i in range(runs + 1):           # (the first one discarded; wall time of copy + synchronise, so it includes the launch)
            t0 = time.perf_counter()
            if hip.hipMemcpy(b, a, C.c_size_t(n), 3) or hip.hipDeviceSynchronize():       # 3 = hipMemcpyDeviceToDevice
                raise RuntimeError('hipMemcpy failed')
            if i:
                copies.append(round((time.perf_counter() - t0) * 1e3, 3))
        hip.hipFree(a)
        hip.hipFree(b)
        out['device_copy_ms'] = copies
    except Exception as e:      # noqa: BLE001
        out['device_copy_ms'] = f'not measured: {e}'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--families', type=int, default=200)
    ap.add_argument('--members', type=int, default=500)
    ap.add_argument('--length', type=int, default=40000)
    ap.add_argument('--p-lo', type=float, default=0.001, help='lowest mutation rate of a member')
    ap.add_argument('--p-hi', type=float, default=0.03, help='highest; 0.03 makes most members join at tani 0.95, 0.12 almost none')
    ap.add_argument('--batches', type=int, nargs='+', default=[1024, 4096, 16384])
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--tani', type=float, default=0.95)
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    import numpy as np
    from vclust_amd import api, synth
    api.set_device(0)
    codes, offsets, names = synth.make_families(a.families, a.members, length=a.length, seed=3, p_lo=a.p_lo, p_hi=a.p_hi)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    gs.to_device()
    n = len(gs)
    lengths = gs.lengths()
    order = gs.align_order()
    rank = np.empty(n, dtype=np.int64); rank[order] = np.arange(n)
    api.profile_enable(True)
    out = dict(workload=f'families-{a.families}x{a.members}x{a.length}-p{a.p_hi:g}', genomes=n, bases=int(offsets[-1]), tani=a.tani, runs=a.runs,
               protocol='one run discarded, then the timed runs; median and range of the wall time, scopes of the median run')
    (rep3, n_cand), t3 = measure(api, lambda: three_step(api, np, gs, lengths, rank, a.tani), a.runs)
    out['three_step'] = dict(pairs_aligned=int(n_cand), representatives=int((rep3 == np.arange(n)).sum()), **t3)
    out['dereplicate'] = {}
    for batch in a.batches:
        (label, rep, st), t = measure(api, lambda: gs.dereplicate_set(batch_genomes=batch, k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT, tani=a.tani), a.runs)
        sub = t['scopes'].get('derep_subset', 0.0)
        out['dereplicate'][str(batch)] = dict(**st, same_representatives_as_three_step=bool((rep == rep3).all()), derep_subset_ms=sub,
                                              derep_subset_share=round(sub / t['median_ms'], 4), worst_case_pair_list_bytes=12 * batch * (batch - 1) // 2, **t)
    out['subset_against_copy'] = subset_against_copy(api, gs, a.runs)
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        a.json.write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
