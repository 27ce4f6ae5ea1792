"""Plain-Python sequential restatement of the average-linkage (UPGMA) merge table and its cuts ("Merge
table: average linkage"): the checker of vg_cluster_average_linkage_graph, vg_cluster_average_levels_graph and of vg_cluster /
vg_cluster_linkage with algorithm average.  It stands on cluster_restatement (rows, edges, labels) and linkage_restatement (table,
the bytes of both files).

A weight w (in [0, 1]) is the integer u = round(Fraction(w) * 2**32), ties to even.  S(A, B) is the sum of u over the edges between
two clusters, P(A, B) = |A| * |B|, sim(A, B) = Fraction(S, P << 32): a pair of objects without an edge adds 0 to S and 1 to P, and
two clusters without any edge between them are no candidate.  A candidate has the key (-sim, c, d), c < d the cluster ids (minimum
members).  From singletons, the candidate of smallest key merges, until none is left or the smallest has sim < floor, which is
S < F * P with F the quantised floor.  The cut at level t joins the merges with S >= T * P, T the quantised level.  Everything is
exact; it is sequential and quadratic, which is fine at test sizes."""
from fractions import Fraction

import cluster_restatement as cr
import linkage_restatement as lr


def quantum(w):
    return round(Fraction(w) * 2**32)


def similarity(s, p):
    """the double nearest to the exact quotient"""
    return float(Fraction(s, p << 32))


def merges(n, e, floor=0.0):
    """-> [(c, d, S, P)] of the merges in merge order; e = cr.edges(rows)"""
    f = quantum(floor)
    size = [1] * n
    total = {pair: quantum(w) for pair, w in e.items()}             # (c, d), c < d -> S
    key = {pair: (-Fraction(s), *pair) for pair, s in total.items()}
    out = []
    while key:
        _, c, d = min(key.values())
        s, p = total[(c, d)], size[c] * size[d]
        if s < f * p:
            break
        out.append((c, d, s, p))
        size[c] += size[d]
        joined = {}
        for (x, y), v in total.items():                             # d's records move to c; the pair's own record goes
            if (x, y) != (c, d):
                x, y = (c if x == d else x), (c if y == d else y)
                pair = (min(x, y), max(x, y))
                joined[pair] = joined.get(pair, 0) + v
        for pair in [k for k in key if c in k or d in k]:
            del key[pair]
        total = joined
        for (x, y), v in total.items():
            if x == c or y == c:
                key[(x, y)] = (-Fraction(v, size[x] * size[y]), x, y)
    return out


def table(n, m):
    """-> [(node_a, node_b, similarity, size, object_a, object_b)], one row per merge"""
    return lr.table(n, [(c, d, similarity(s, p)) for c, d, s, p in m])


def cut(n, m, level):
    """cluster id (minimum member) of every object after the merges with sim >= level, compared exactly"""
    t = quantum(level) if level > 0 else 0
    return lr.cut(n, [(c, d, 1) for c, d, s, p in m if s >= t * p], 0)


def linkage(n, rows, floor=0.0):
    return table(n, merges(n, cr.edges(rows), floor))


def cluster_ids(n, rows, floor=0.0, level=0.0):
    return cut(n, merges(n, cr.edges(rows), floor), level)


def levels(n, rows, lv, floor=0.0):
    """-> [(label, representative)] per level, in the order given"""
    m = merges(n, cr.edges(rows), floor)
    return [cr.labels(cut(n, m, t)) for t in lv]


def run(ani_path, ids_path, metric='tani', lv=(), num_alns=0, representatives=False, **mins):
    """-> (the bytes of clusters.tsv with one column per level, the bytes of the linkage file) for these files and options; the
    floor is the minimum of the metric"""
    ids = cr.read_ids(ids_path)
    n = len(ids)
    m = merges(n, cr.edges(cr.read_rows(ani_path, n, metric, num_alns, **mins)), mins.get(metric, 0.0))
    columns = [cr.labels(cut(n, m, 0.0))] + [cr.labels(cut(n, m, t)) for t in lv]
    return lr.clusters_tsv(ids, metric, list(lv), columns, representatives), lr.linkage_tsv(table(n, m))


def random_graph(rng, n, rows, weights):
    """rows (q, r, w) between random objects (self rows, duplicates and reverse rows included), weights drawn from `weights`"""
    import numpy as np
    return (rng.integers(0, n, rows).astype(np.uint32), rng.integers(0, n, rows).astype(np.uint32),
            rng.choice(np.asarray(weights, dtype=np.float64), rows))
