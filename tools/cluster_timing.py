"""Timing of the cluster stage (vg_cluster / vg_cluster_graph), per algorithm: host parse, GPU time per kernel (profile
table), rounds, objects finished by the tail sweep, end-to-end wall time.

  python tools/cluster_timing.py [--sizes 100000 1000000] [--ani ani.tsv --ids ani.ids.tsv] [--metric tani --min 0.95] [--linkage]

Synthetic graphs: families of 20-200 objects in index order, ~50 rows per object (both directions, ~25 distinct
neighbours), weights 0.80-1.00 inside families and a few weak rows between them.  With --ani, the file is also clustered
through the whole-stage call (parse + GPU + write) for each algorithm.  --linkage: the single-linkage merge table
(vg_cluster_linkage_graph) on the same synthetic graphs instead of the four algorithms, with `single` timed on the same graph
in the same process as the yardstick.
"""
import argparse
import json
import pathlib
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
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    api.set_device(0)
    api.profile_enable(True)
    api.cluster_graph(2, [0], [1], [1.0])          # context, code object
    res = []
    if a.linkage:
        api.cluster_linkage(2, [0], [1], [1.0])
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
