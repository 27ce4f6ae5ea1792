"""Timing of the coverage map (vg_cover_rows): wall time, GPU time per profile scope and the run counts.

  python tools/cover_timing.py [--objects 100000] [--rows-per-object 100] [--hot-rows 1000000] [--json out.json]

Synthetic families: objects in families of 20-200 in index order (the family is the group), lengths 20 000-100 000, every object the
query of --rows-per-object rows to about 25 partners of its family (four rows per partner, 200-2 000 positions each, anywhere on the
query, so rows of a pair overlap now and then).  One run is discarded, three are timed: the row prints the median wall time of
cover_rows (upload, device, download of the records and segments) with the minimum and maximum, the `cover_*` profile scopes of the
median run and the run counts.  The second row repeats the run with --hot-rows more rows on one object of length 1 000 000 from 300
partners (0 = leave it out)."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vclust_amd import api  # noqa: E402


def family_rows(n, per_object, seed=0):
    """-> (lengths, label, q, r, qstart, qend)"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 201, n // 20 + 2)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    starts = starts[starts < n]
    bounds = np.concatenate([starts, [n]])
    label = np.repeat(np.arange(len(starts)), np.diff(bounds))
    fam_start, fam_size = np.repeat(starts, np.diff(bounds)), np.repeat(np.diff(bounds), np.diff(bounds))
    lengths = rng.integers(20000, 100001, n)
    q = np.repeat(np.arange(n), per_object)
    # about per_object / 4 partners per object: a window of the family behind the object
    r = fam_start[q] + (q - fam_start[q] + 1 + rng.integers(0, max(1, per_object // 4), len(q))) % fam_size[q]
    span = rng.integers(200, 2001, len(q))
    qstart = (rng.random(len(q)) * (lengths[q] - span)).astype(np.int64)
    return lengths, label, q, r, qstart, qstart + span - 1


def with_hot_object(case, rows, seed=1):
    lengths, label, q, r, qstart, qend = case
    rng = np.random.default_rng(seed)
    lengths = lengths.copy()
    lengths[0] = 1000000
    span = rng.integers(200, 2001, rows)
    s = (rng.random(rows) * (lengths[0] - span)).astype(np.int64)
    return (lengths, label, np.concatenate([q, np.zeros(rows, np.int64)]), np.concatenate([r, rng.integers(1, 301, rows)]),
            np.concatenate([qstart, s]), np.concatenate([qend, s + span - 1]))


def timed(fn):
    api.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    return out, wall, {k['name']: round(k['total_ms'], 3) for k in api.profile_get() if k['name'].startswith('cover_')}


def row(name, case):
    lengths, label, q, r, qstart, qend = case
    q, r, qstart, qend = q.astype(np.uint32), r.astype(np.uint32), qstart.astype(np.int32), qend.astype(np.int32)
    label = label.astype(np.int32)
    call = lambda: api.cover_rows(lengths, q, r, qstart, qend, label=label)      # noqa: E731
    call()
    runs = sorted((timed(call) for _ in range(3)), key=lambda x: x[1])
    (records, segments, run), wall, scopes = runs[1]
    return dict(input=f'{name} n={len(lengths)} rows={len(q)}', wall_ms=round(wall, 2), wall_min_ms=round(runs[0][1], 2), wall_max_ms=round(runs[2][1], 2),
                gpu_ms=round(sum(scopes.values()), 2), scopes=scopes, max_depth=int(records['max_depth'].max()),
                covered_frac=round(float(records['covered'].sum() / records['len'].sum()), 4), **run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=100000)
    ap.add_argument('--rows-per-object', type=int, default=100)
    ap.add_argument('--hot-rows', type=int, default=1000000)
    ap.add_argument('--json', type=pathlib.Path)
    a = ap.parse_args()
    api.set_device(0)
    api.profile_enable(True)
    api.cover_rows([4, 4], [0], [1], [0], [3])          # context, code object
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
