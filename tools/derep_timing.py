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
bytes (hipMemcpy, wall time).  One JSON line on stdout; --json also writes it to a file.

  python tools/derep_timing.py --update 0.01 [--route-from <checkout of the parent commit, built>] [the options above]

measures `dereplicate --db --prior` instead (dereplicate_set with prior_rep, DESIGN.md section 13, "Update"): the last `--update` share
of the genomes in input order are new (--split stride: every so-manyth genome instead), the prior is the plain run on the rest.  Beside it the route the command replaces, at the
array level: kmer_shared_new -> filter_pairs -> align_tasks -> lz_align of every kept pair -> cluster_update_graph('cd-hit').  That
route uses nothing this tool's own checkout adds, so with --route-from it runs in a fresh process on the library of ANOTHER checkout
(the parent commit's, built there): the comparison is then against the code before the change, not against the code under test.
Reported beside the times: the scopes `derep_extend` and `derep_subset`, the pairs aligned on both routes, and the bytes of the
working set [R | largest batch] (2 bits of code and 1 of mask per padded base), once and with a second copy of R."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
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


def update_route(api, np, gs, n_db, lengths, rank, prior, tani):
    """the three calls `dereplicate --db --prior` replaces: every kept pair that contains a new genome is aligned"""
    sizes, pairs = gs.kmer_shared_new(n_db, k=K, min_shared=MIN_KMERS)
    cand = gs.filter_pairs(sizes, pairs, k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT)
    tasks = gs.align_tasks(cand)
    stats = gs.lz_align(tasks)
    q, r = tasks['q'].astype(np.int64), tasks['r'].astype(np.int64)
    both = stats['n_match'].astype(np.int64)
    both = both + both.reshape(-1, 2)[:, ::-1].reshape(-1)
    w = both / (lengths[q] + lengths[r])
    keep = w >= tani
    label, rep, _ = api.cluster_update_graph(len(lengths), rank[q[keep]], rank[r[keep]], w[keep], prior, 'cd-hit')
    return rep, len(cand)


def update_main(a, root):
    """--update: the update under test, or (--route-only, in a process of its own) the three-call route on the library under `root`"""
    import subprocess
    import tempfile
    sys.path.insert(0, str(root))
    import numpy as np
    from vclust_amd import api, synth
    api.set_device(0)
    codes, offsets, names = synth.make_families(a.families, a.members, length=a.length, seed=3, p_lo=a.p_lo, p_hi=a.p_hi)
    n = len(names)
    n_db = n - max(1, int(round(n * a.update)))
    if a.split == 'stride':
        # the new genomes spread over the input order (every n / n_new-th genome), moved behind the others: members of the database's families
        step = n // (n - n_db)
        new = set(range(step - 1, n, step)[:n - n_db])
        ids = [i for i in range(n) if i not in new] + sorted(new)
        seqs = [codes[offsets[i]:offsets[i + 1]] for i in ids]
        names = [names[i] for i in ids]
        offsets = np.zeros(n + 1, dtype=np.int64); offsets[1:] = np.cumsum([len(x) for x in seqs])
        codes = np.concatenate(seqs)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    gs.to_device()
    lengths = gs.lengths()
    order = gs.align_order()
    rank = np.empty(n, dtype=np.int64); rank[order] = np.arange(n)
    api.profile_enable(True)
    if a.route_only:
        prior = np.load(a.prior)
        (rep, n_cand), t = measure(api, lambda: update_route(api, np, gs, n_db, lengths, rank, prior, a.tani), a.runs)
        np.save(a.prior, rep)
        print(json.dumps(dict(pairs_aligned=int(n_cand), library=str(root), **t)), flush=True)
        return
    # the prior: the plain run on the database genomes alone, its representatives as ranks of the combined set
    db = api.GenomeSet.from_codes(codes[:offsets[n_db]], offsets[:n_db + 1], names[:n_db])
    db.to_device()
    _, db_rep, db_st = db.dereplicate_set(batch_genomes=a.batches[0], k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT, tani=a.tani)
    db_order = db.align_order()
    db.close()
    prior = np.full(n, -1, dtype=np.int32)
    prior[rank[db_order]] = rank[db_order[db_rep]]
    out = dict(workload=f'families-{a.families}x{a.members}x{a.length}-p{a.p_hi:g}-update{a.update:g}-{a.split}', genomes=n, new_genomes=n - n_db, bases=int(offsets[-1]),
               tani=a.tani, runs=a.runs, prior_representatives=int(db_st['representatives']),
               protocol='one run discarded, then the timed runs; median and range of the wall time, scopes of the median run')
    with tempfile.TemporaryDirectory() as tmp:
        prior_file = pathlib.Path(tmp) / 'prior.npy'
        np.save(prior_file, prior)
        cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), '--update', str(a.update), '--route-only', '--prior', str(prior_file),
               '--package-root', str(a.route_from or ROOT), '--families', str(a.families), '--members', str(a.members), '--length', str(a.length),
               '--p-lo', str(a.p_lo), '--p-hi', str(a.p_hi), '--runs', str(a.runs), '--tani', str(a.tani), '--split', a.split]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        out['three_call_route'] = json.loads(p.stdout.strip().split('\n')[-1])
        rep3 = np.load(prior_file)
    out['three_call_route']['library_is_the_parent_checkout'] = a.route_from is not None
    pad = lambda ids: int(sum((int(lengths[i]) // 64 + 1) * 64 for i in ids))      # noqa: E731  (at least: blocks of 64 bases)
    out['update'] = {}
    for batch in a.batches:
        (label, rep, st), t = measure(api, lambda: gs.dereplicate_set(batch_genomes=batch, k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT, tani=a.tani,
                                                                     n_db=n_db, prior_rep=prior), a.runs)
        reps = order[np.flatnonzero(rep == np.arange(n))]
        news = order[np.flatnonzero(prior < 0)]
        largest = max(pad(news[b0:b0 + batch]) for b0 in range(0, len(news), batch))
        one = (pad(reps) + largest) * 3 // 8
        out['update'][str(batch)] = dict(**st, same_representatives_as_the_route=bool((rep == rep3).all()),
                                         derep_extend_ms=t['scopes'].get('derep_extend', 0.0), derep_subset_ms=t['scopes'].get('derep_subset', 0.0),
                                         working_set_bytes=dict(one_copy_of_R=one, two_copies_of_R=one + pad(reps) * 3 // 8,
                                                                how='computed from the lengths, 3 bits per padded base; not read from the allocator'), **t)
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        a.json.write_text(json.dumps(out, indent=1) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--update', type=float, help='measure the update: this share of the genomes, the last in input order, are new')
    ap.add_argument('--route-from', type=pathlib.Path, help='--update: a built checkout whose library runs the three-call route (default: this one)')
    ap.add_argument('--split', choices=['tail', 'stride'], default='tail',
                    help='--update: which genomes are new -- the last ones of the input order (with family sets: whole families, unrelated to the '
                         'database) or every so-manyth genome (members of the database\'s families)')
    ap.add_argument('--route-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--prior', type=pathlib.Path, help=argparse.SUPPRESS)
    ap.add_argument('--package-root', type=pathlib.Path, help=argparse.SUPPRESS)
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
    if a.update is not None:
        return update_main(a, (a.package_root or ROOT).resolve())
    sys.path.insert(0, str(ROOT))
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
