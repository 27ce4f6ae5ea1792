"""Timing of the mosaic painting (vg_paint_rows): wall time, GPU time per profile scope and the run counts, with
the coverage map's time on the same rows beside it.

  python tools/paint_timing.py [--objects 100000] [--rows-per-object 100] [--hot-rows 1000000] [--json out.json]

The two synthetic inputs of tools/cover_timing.py (families, and families plus --hot-rows rows on one object of length 1 000 000), every
row with an n_match of 70-100 % of its span.  One run is discarded, three are timed: a row prints the median wall time of
paint_rows (upload, device, download of the records, segments and donor records) with the minimum and maximum, the `paint_*` profile
scopes of the median run and the run counts, then the same for cover_rows, measured in the same process on the same rows."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from cover_timing import family_rows, with_hot_object  # noqa: E402
from vclust_amd import api  # noqa: E402


def timed(fn, prefix):
    api.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    return out, wall, {k['name']: round(k['total_ms'], 3) for k in api.profile_get() if k['name'].startswith(prefix)}


def median_of_three(call, prefix):
    call()
    runs = sorted((timed(call, prefix) for _ in range(3)), key=lambda x: x[1])
    out, wall, scopes = runs[1]
    return out, dict(wall_ms=round(wall, 2), wall_min_ms=round(runs[0][1], 2), wall_max_ms=round(runs[2][1], 2), gpu_ms=round(sum(scopes.values()), 2),
                     scopes=scopes)


def row(name, case, seed=2):
    lengths, label, q, r, qstart, qend = case
    q, r, qstart, qend = q.astype(np.uint32), r.astype(np.uint32), qstart.astype(np.int32), qend.astype(np.int32)
    label = label.astype(np.int32)
    span = (qend - qstart + 1).astype(np.int64)
    n_match = (span * np.random.default_rng(seed).integers(700, 1001, len(span)) // 1000).astype(np.int32)
    (records, segments, donors, run), paint = median_of_three(lambda: api.paint_rows(lengths, q, r, qstart, qend, n_match, label=label), 'paint_')
    _, cover = median_of_three(lambda: api.cover_rows(lengths, q, r, qstart, qend, label=label), 'cover_')
    return dict(input=f'{name} n={len(lengths)} rows={len(q)}', **paint, painted_frac=round(float(records['painted'].sum() / records['len'].sum()), 4),
                max_donors=int(records['donors'].max()), **run, cover=cover)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=100000)
    ap.add_argument('--rows-per-object', type=int, default=100)
    ap.add_argument('--hot-rows', type=int, default=1000000)
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    api.set_device(0)
    api.profile_enable(True)
    api.paint_rows([4, 4], [0], [1], [0], [3], [3])     # context, code object
    api.cover_rows([4, 4], [0], [1], [0], [3])
    case = family_rows(a.objects, a.rows_per_object)
    res = [row('families', case)]
    print(json.dumps(res[-1]), flush=True)
    if a.hot_rows:
        res.append(row(f'families + hot object ({a.hot_rows} rows)', with_hot_object(case, a.hot_rows)))
        print(json.dumps(res[-1]), flush=True)
    if a.json:
        a.json.write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
