"""Timing of the cluster stage (vg_cluster / vg_cluster_graph), per algorithm: host parse, GPU time per kernel (profile
table), rounds, objects finished by the tail sweep, end-to-end wall time.

  python tools/cluster_timing.py [--sizes 100000 1000000] [--ani ani.tsv --ids ani.ids.tsv] [--metric tani --min 0.95] [--linkage]
  python tools/cluster_timing.py --complete [--sizes 100000] [--clique-chain 200]
  python tools/cluster_timing.py --average [--sizes 100000] [--floor 0.8]
  python tools/cluster_timing.py --update [--sizes 100000] [--new-fraction 0.01]
  python tools/cluster_timing.py --stats [--sizes 100000 1000000]
  python tools/cluster_timing.py --mcl [--sizes 100000] [--rows-per-object 9 90]

Synthetic graphs: families of 20-200 objects in index order, ~50 rows per object (both directions, ~25 distinct
neighbours), weights 0.80-1.00 inside families and a few weak rows between them.  With --ani, the file is also clustered
through the whole-stage call (parse + GPU + write) for each algorithm.  --linkage: the single-linkage merge table
(vg_cluster_linkage_graph) on the same synthetic graphs instead of the four algorithms, with `single` timed on the same graph
in the same process as the yardstick.  --complete: the complete-linkage merge table (vg_cluster_complete_linkage_graph) with
`single` and the single-linkage table as yardsticks, all three on the same graph in the same process, each run once and
discarded and then timed three times (the median is printed).  The graph is the synthetic one with every family made a full
clique (the 50-rows-per-object families are no cliques and would merge almost nothing); the row prints the two profile groups
`cluster_complete_best` / `cluster_complete_contract`, the rounds and the records of the cluster graph after each contraction
(read from the library's VG_HOST_TRACE lines, which this mode switches on).  --clique-chain N adds the known worst case: one
clique of N objects whose weights force one merge per round, with the time per round.  --average: the average-linkage merge
table (vg_cluster_average_linkage_graph, floor --floor) on the clique-family graph beside the complete-linkage table, both in the
same process, each run once and discarded and then timed three times; the row prints the two profile groups
`cluster_average_best` / `cluster_average_contract`, the rounds and the ratio of GPU time to `complete`.  --update: the update of a
prior clustering (vg_cluster_update_graph) on the synthetic family graph with the last --new-fraction of the objects new: the
prior is the plain run on the rows among the other objects, the update gets the rows with a new end (what `align --db` writes),
and the plain run on the whole graph (vg_cluster_graph) is the yardstick, in the same process; each is run once and discarded and
then timed three times.  The row also says whether the update's labels equal the plain run's (properties P1 and P2).  --stats: the
cluster report (vg_cluster_stats_graph) on the synthetic family graph, of the `cd-hit` labelling and of the labelling with every
object in one cluster, beside the `single` run in the same process; each is run once and discarded and then timed three times, and
the row prints the three profile groups `cluster_stats_rows` / `cluster_stats_reduce` / `cluster_stats_nearest`.  --mcl: Markov
clustering (vg_cluster_mcl_graph, default parameters) on the synthetic family graph at --rows-per-object rows per object (9: about
4.5 edges per object, the shape of the benchmark's pair set; 90: ten times denser), beside `single` in the same process; each is run
once and discarded and then timed three times, and the row prints all three wall times, the `cluster_mcl_*` and graph-build
(`cluster_edges_*`, `cluster_csr`) profile groups of the median run with their spread over the three, the iterations and the
LDS / spill row split.
"""
import argparse
import json
import os
import pathlib
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vclust_amd import api  # noqa: E402

ALGOS = ('single', 'cd-hit', 'uclust', 'set-cover')


def family_graph(n, per_object=50, seed=0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 201, n // 20 + 2)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    starts = starts[starts < n]
    fam_start = np.repeat(starts, np.diff(np.concatenate([starts, [n]])))
    fam_size = np.repeat(np.diff(np.concatenate([starts, [n]])), np.diff(np.concatenate([starts, [n]])))
    rows = n * per_object // 2
    q = rng.integers(0, n, rows)
    r = fam_start[q] + rng.integers(0, 1 << 30, rows) % fam_size[q]
    w = rng.uniform(0.8, 1.0, rows).round(4)
    weak = rng.random(rows) < 0.02
    r[weak] = rng.integers(0, n, weak.sum())
    w[weak] = 0.5
    q = np.concatenate([q, r]); r = np.concatenate([r, q[:rows]]); w = np.concatenate([w, w])
    return q.astype(np.uint32), r.astype(np.uint32), w


def clique_family_graph(n, seed=0):
    """the families of family_graph (20-200 objects in index order), every pair inside one a row of weight 0.80-1.00"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 201, n // 20 + 2)
    q, r, start = [], [], 0
    for size in sizes:
        size = min(int(size), n - start)
        if size <= 0:
            break
        a, b = np.triu_indices(size, 1)
        q.append(a + start); r.append(b + start)
        start += size
    q, r = np.concatenate(q), np.concatenate(r)
    return q.astype(np.uint32), r.astype(np.uint32), rng.uniform(0.8, 1.0, len(q)).round(4)


def clique_chain(n):
    """one clique with w(i, j) = 1 - max(i, j) / (4 n): object k joins {0 .. k-1} in round k, one merge per round"""
    q, r = np.triu_indices(n, 1)
    return q.astype(np.uint32), r.astype(np.uint32), 1.0 - np.maximum(q, r) / (4.0 * n)


def records_per_round(fn):
    """run fn with the library's host trace on stderr captured -> its result, [records after each contraction]"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(keep, 2); os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors='replace')
    return out, [int(x) for x in re.findall(r'complete round \d+: \d+ merges, (\d+) records', text)][1:]


def median_of_three(fn):
    """discard one run, then the run of median wall time of three -> (result, wall ms, kernel groups)"""
    fn()
    runs = sorted((timed(fn) for _ in range(3)), key=lambda x: x[1])
    return runs[1]


def complete_row(name, n, q, r, w):
    (lab, rep, st), wall1, kern1 = median_of_three(lambda: api.cluster_graph(n, q, r, w, 'single'))
    (_, lst), wall2, kern2 = median_of_three(lambda: api.cluster_linkage(n, q, r, w))
    (table, cst), wall, kern = median_of_three(lambda: api.cluster_complete_linkage_graph(n, q, r, w))
    _, records = records_per_round(lambda: api.cluster_complete_linkage_graph(n, q, r, w))
    gpu, rounds = sum(kern.values()), max(cst['rounds'], 1)
    per_round = (kern.get('cluster_complete_best', 0) + kern.get('cluster_complete_contract', 0)) / rounds
    return dict(input=f'{name} n={n} rows={len(q)}', algorithm='complete', wall_ms=round(wall, 2), gpu_ms=round(gpu, 2), kernels=kern,
                best_ms=kern.get('cluster_complete_best', 0), contract_ms=kern.get('cluster_complete_contract', 0),
                gpu_ms_per_round=round(per_round, 4), wall_ms_per_round=round(wall / rounds, 4), records_after_contraction=records,
                single_wall_ms=round(wall1, 2), single_gpu_ms=round(sum(kern1.values()), 2),
                linkage_wall_ms=round(wall2, 2), linkage_gpu_ms=round(sum(kern2.values()), 2), linkage_rounds=lst['rounds'],
                gpu_ratio_to_single=round(gpu / max(sum(kern1.values()), 1e-9), 2),
                gpu_ratio_to_linkage=round(gpu / max(sum(kern2.values()), 1e-9), 2), **cst)


def average_row(name, n, q, r, w, floor):
    (_, cst), wall1, kern1 = median_of_three(lambda: api.cluster_complete_linkage_graph(n, q, r, w))
    (table, ast), wall, kern = median_of_three(lambda: api.cluster_average_linkage_graph(n, q, r, w, floor))
    gpu, gpu1, rounds = sum(kern.values()), sum(kern1.values()), max(ast['rounds'], 1)
    return dict(input=f'{name} n={n} rows={len(q)}', algorithm='average', floor=floor, wall_ms=round(wall, 2), gpu_ms=round(gpu, 2),
                kernels=kern, best_ms=kern.get('cluster_average_best', 0), contract_ms=kern.get('cluster_average_contract', 0),
                gpu_ms_per_round=round(gpu / rounds, 4), complete_wall_ms=round(wall1, 2), complete_gpu_ms=round(gpu1, 2),
                complete_rounds=cst['rounds'], complete_merges=cst['n_merges'], gpu_ratio_to_complete=round(gpu / max(gpu1, 1e-9), 2), **ast)


def update_rows(n, q, r, w, new_fraction):
    n_prior = n - max(1, int(round(n * new_fraction)))
    inside = (q < n_prior) & (r < n_prior)
    nq, nr, nw = (np.ascontiguousarray(x[~inside]) for x in (q, r, w))          # the rows with a new end
    res = []
    for algo in ('single', 'cd-hit', 'uclust'):
        _, prep, _ = api.cluster_graph(n_prior, q[inside], r[inside], w[inside], algo)
        prior = np.concatenate([prep, np.full(n - n_prior, -1, np.int32)])
        (plab, prep_full, pst), pwall, pkern = median_of_three(lambda: api.cluster_graph(n, q, r, w, algo))
        (lab, rep, st), wall, kern = median_of_three(lambda: api.cluster_update_graph(n, nq, nr, nw, prior, algo))
        res.append(dict(input=f'synthetic n={n} rows={len(q)}, last {n - n_prior} objects new ({len(nq)} rows)', algorithm=algo,
                        wall_ms=round(wall, 2), gpu_ms=round(sum(kern.values()), 2), kernels=kern,
                        plain_wall_ms=round(pwall, 2), plain_gpu_ms=round(sum(pkern.values()), 2), plain_rounds=pst['rounds'],
                        plain_sweep_objects=pst['sweep_objects'], plain_edges=pst['n_edges'],
                        equals_plain=bool((lab == plab).all() and (rep == prep_full).all()), **st))
    return res


def stats_rows(n, q, r, w):
    """the cluster report of the `cd-hit` labelling (many clusters; `single` is one component on this graph), and of the labelling
    that puts every object into one cluster (the hot record of the reduce pass), beside the `single` run itself"""
    (lab, rep, st), wall1, kern1 = median_of_three(lambda: api.cluster_graph(n, q, r, w, 'single'))
    res = []
    for name, label in (('cd-hit', api.cluster_graph(n, q, r, w, 'cd-hit')[0]), ('one cluster', np.zeros(n, np.int32))):
        k = int(label.max()) + 1
        (rec, own, oth_max, oth), wall, kern = median_of_three(lambda: api.cluster_stats_graph(n, q, r, w, label, k))
        groups = {g: kern.get(f'cluster_stats_{g}', 0) for g in ('rows', 'reduce', 'nearest')}
        res.append(dict(input=f'synthetic n={n} rows={len(q)}', algorithm='stats', labelling=name, clusters=k, wall_ms=round(wall, 2),
                        gpu_ms=round(sum(kern.values()), 2), kernels=kern, **{f'{g}_ms': v for g, v in groups.items()},
                        single_wall_ms=round(wall1, 2), single_gpu_ms=round(sum(kern1.values()), 2), edges=st['n_edges'],
                        linked=int(rec['linked'].sum()), external=int(rec['external'].sum()) // 2, misfits=int(rec['misfits'].sum())))
        assert res[-1]['linked'] + res[-1]['external'] == st['n_edges'] and int(rec['size'].sum()) == n, res[-1]
    return res


def mcl_row(n, q, r, w, rows_per_object):
    (lab1, _, st1), wall1, kern1 = median_of_three(lambda: api.cluster_graph(n, q, r, w, 'single'))
    api.cluster_mcl_graph(n, q, r, w)
    runs = sorted((timed(lambda: api.cluster_mcl_graph(n, q, r, w)) for _ in range(3)), key=lambda x: x[1])
    (lab, rep, st), wall, kern = runs[1]
    spread = {k: [round(min(x[2].get(k, 0) for x in runs), 3), round(max(x[2].get(k, 0) for x in runs), 3)] for k in kern}
    mcl = {k: v for k, v in kern.items() if k.startswith('cluster_mcl_')}
    build = {k: v for k, v in kern.items() if k.startswith('cluster_edges_') or k == 'cluster_csr'}
    return dict(input=f'synthetic n={n} rows={len(q)} ({rows_per_object} per object)', algorithm='mcl', wall_ms=round(wall, 2),
                wall_ms_all=[round(x[1], 2) for x in runs], gpu_ms=round(sum(kern.values()), 2), mcl_ms=round(sum(mcl.values()), 2),
                build_ms=round(sum(build.values()), 2), kernels=kern, kernels_min_max=spread,
                mcl_ms_per_iteration=round(sum(mcl.values()) / max(st['iterations'], 1), 3), clusters=int(lab.max()) + 1,
                single_clusters=int(lab1.max()) + 1, single_wall_ms=round(wall1, 2), single_gpu_ms=round(sum(kern1.values()), 2), **st)


def timed(fn):
    api.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    kern = {k['name']: round(k['total_ms'], 3) for k in api.profile_get() if k['name'].startswith('cluster_')}
    return out, wall, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[100000, 1000000])
    ap.add_argument('--ani', type=pathlib.Path)
    ap.add_argument('--ids', type=pathlib.Path)
    ap.add_argument('--metric', default='tani')
    ap.add_argument('--min', type=float, default=0.95)
    ap.add_argument('--linkage', action='store_true')
    ap.add_argument('--complete', action='store_true')
    ap.add_argument('--clique-chain', type=int, default=0, metavar='N')
    ap.add_argument('--average', action='store_true')
    ap.add_argument('--floor', type=float, default=0.8)
    ap.add_argument('--update', action='store_true')
    ap.add_argument('--new-fraction', type=float, default=0.01)
    ap.add_argument('--stats', action='store_true')
    ap.add_argument('--mcl', action='store_true')
    ap.add_argument('--rows-per-object', type=int, nargs='*', default=[9, 90])
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    if a.complete:
        os.environ['VG_HOST_TRACE'] = '1'      # (read once, at the library's first trace point; only records_per_round shows it)
    api.set_device(0)
    api.profile_enable(True)
    api.cluster_graph(2, [0], [1], [1.0])          # context, code object
    res = []
    if a.linkage:
        api.cluster_linkage(2, [0], [1], [1.0])
    if a.complete:
        silent = lambda fn: records_per_round(fn)[0]            # noqa: E731  (the trace lines of the timed runs are dropped)
        silent(lambda: api.cluster_complete_linkage_graph(2, [0], [1], [1.0]))
        silent(lambda: api.cluster_linkage(2, [0], [1], [1.0]))
        graphs = [('synthetic clique families', n, *clique_family_graph(n)) for n in a.sizes]
        if a.clique_chain:
            graphs.append(('one clique, one merge per round', a.clique_chain, *clique_chain(a.clique_chain)))
        for name, n, q, r, w in graphs:
            row = silent(lambda: complete_row(name, n, q, r, w))
            print(json.dumps(row), flush=True)
            res.append(row)
        a.sizes = []
    if a.average:
        api.cluster_complete_linkage_graph(2, [0], [1], [1.0])
        api.cluster_average_linkage_graph(2, [0], [1], [1.0])
        for n in a.sizes:
            row = average_row('synthetic clique families', n, *clique_family_graph(n), a.floor)
            print(json.dumps(row), flush=True)
            res.append(row)
        a.sizes = []
    if a.update:
        api.cluster_update_graph(2, [0], [1], [1.0], [0, -1])
        for n in a.sizes:
            for row in update_rows(n, *family_graph(n), a.new_fraction):
                print(json.dumps(row), flush=True)
                res.append(row)
        a.sizes = []
    if a.stats:
        api.cluster_stats_graph(2, [0], [1], [1.0], [0, 0])
        for n in a.sizes:
            for row in stats_rows(n, *family_graph(n)):
                print(json.dumps(row), flush=True)
                res.append(row)
        a.sizes = []
    if a.mcl:
        api.cluster_mcl_graph(2, [0], [1], [1.0])
        for n in a.sizes:
            for per_object in a.rows_per_object:
                row = mcl_row(n, *family_graph(n, per_object), per_object)
                print(json.dumps(row), flush=True)
                res.append(row)
        a.sizes = []
    for n in a.sizes:
        q, r, w = family_graph(n)
        if a.linkage:
            (lab, rep, st), wall1, kern1 = timed(lambda: api.cluster_graph(n, q, r, w, 'single'))
            (table, lst), wall, kern = timed(lambda: api.cluster_linkage(n, q, r, w))
            row = dict(input=f'synthetic n={n} rows={len(q)}', algorithm='linkage', wall_ms=round(wall, 2), gpu_ms=round(sum(kern.values()), 2),
                       kernels=kern, single_wall_ms=round(wall1, 2), single_gpu_ms=round(sum(kern1.values()), 2), single_kernels=kern1,
                       gpu_ratio_to_single=round(sum(kern.values()) / max(sum(kern1.values()), 1e-9), 2),
                       components=int(lab.max()) + 1, **lst)
            assert lst['n_merges'] == n - row['components'], row
            print(json.dumps(row), flush=True)
            res.append(row)
            continue
        for algo in ALGOS:
            (lab, rep, st), wall, kern = timed(lambda: api.cluster_graph(n, q, r, w, algo))
            row = dict(input=f'synthetic n={n} rows={len(q)}', algorithm=algo, wall_ms=round(wall, 2), gpu_ms=round(sum(kern.values()), 2),
                       kernels=kern, clusters=int(lab.max()) + 1, **st)
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.ani:
        with tempfile.TemporaryDirectory() as d:
            for algo in ALGOS:
                out = pathlib.Path(d) / 'c.tsv'
                _, wall, kern = timed(lambda: api.cluster(a.ani, a.ids, out, algorithm=algo, metric=a.metric, **{a.metric: a.min}))
                # host_ms: everything but the kernels -- parse of both files, uploads, downloads, the writer
                row = dict(input=str(a.ani), size_mb=round(a.ani.stat().st_size / 2**20, 1), algorithm=algo, wall_ms=round(wall, 2),
                           gpu_ms=round(sum(kern.values()), 2), host_ms=round(wall - sum(kern.values()), 2), kernels=kern)
                print(json.dumps(row), flush=True)
                res.append(row)
    if a.json:
        a.json.write_text(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
