"""Plain-Python sequential restatement of the complete-linkage merge table and its cuts ("Merge table:
complete linkage"): the checker of vg_cluster_complete_linkage_graph, vg_cluster_complete_levels_graph, vg_cluster_linkage with
algorithm complete and the `complete` algorithm of vg_cluster_graph.  It stands on cluster_restatement (rows, edges, labels) and
linkage_restatement (table, cut, the bytes of both files).

Edge {a, b} (a < b) of weight w has the key (-w, a, b), with -0.0 read as +0.0; a pair without an edge has the key +infinity.
K(A, B) of two clusters is the LARGEST key over all pairs a in A, b in B.  From singletons, the two clusters of smallest finite K
merge until no finite K is left; the merge record is that worst edge (a, b, w).  Objects are nodes 0 .. n-1, merge k creates
node n + k; the cut at level t joins the merges with w >= t; a cluster id is its minimum member."""
import heapq

import cluster_restatement as cr
import linkage_restatement as lr


def merges(n, e):
    """-> [(a, b, w)] of the merges in merge order; e = cr.edges(rows)"""
    near = [dict() for _ in range(n)]               # near[c][d] = K(c, d) as (-w, a, b), finite ones only; clusters by minimum member
    heap = []
    for (a, b), w in e.items():
        near[a][b] = near[b][a] = (-(w + 0.0), a, b)
        heap.append((near[a][b], a, b))
    heapq.heapify(heap)
    out = []
    while heap:
        k, c, d = heapq.heappop(heap)               # c < d
        if near[c].get(d) != k:
            continue                                # a pair that has merged, or lost a constituent pair, since
        out.append((k[1], k[2], e[(k[1], k[2])] + 0.0))
        del near[c][d], near[d][c]
        kept = {}
        for x in set(near[c]) | set(near[d]):
            kc, kd = near[c].get(x), near[d].get(x)
            near[x].pop(c, None)
            near[x].pop(d, None)
            if kc is not None and kd is not None:   # every pair present: the worst of the two; else K is infinite from now on
                kept[x] = max(kc, kd)
        near[c], near[d] = kept, {}
        for x, kx in kept.items():
            near[x][c] = kx
            heapq.heappush(heap, (kx, min(c, x), max(c, x)))
    return out


def linkage(n, rows):
    return lr.table(n, merges(n, cr.edges(rows)))


def cluster_ids(n, rows, level=float('-inf')):
    """cluster id (minimum member) of every object at `level` (default: after every merge)"""
    return lr.cut(n, merges(n, cr.edges(rows)), level)


def levels(n, rows, lv):
    """-> [(label, representative)] per level, in the order given"""
    m = merges(n, cr.edges(rows))
    return [cr.labels(lr.cut(n, m, t)) for t in lv]


def run(ani_path, ids_path, metric='tani', lv=(), num_alns=0, representatives=False, **mins):
    """-> (the bytes of clusters.tsv with one column per level, the bytes of the linkage file) for these files and options"""
    ids = cr.read_ids(ids_path)
    n = len(ids)
    m = merges(n, cr.edges(cr.read_rows(ani_path, n, metric, num_alns, **mins)))
    columns = [cr.labels(lr.cut(n, m, float('-inf')))] + [cr.labels(lr.cut(n, m, t)) for t in lv]
    return lr.clusters_tsv(ids, metric, list(lv), columns, representatives), lr.linkage_tsv(lr.table(n, m))


def planted_cliques(rng, n, max_size, weight, noise_rows, noise_weight):
    """Rows (q, r, w) of a graph of cliques of 2 .. max_size consecutive objects, every pair inside one an edge of weight
    weight(rng, count), plus noise_rows rows between random objects of weight noise_weight(rng, count).  numpy arrays."""
    import numpy as np
    q, r, start = [], [], 0
    while start < n:
        size = min(int(rng.integers(2, max_size + 1)), n - start)
        a, b = np.triu_indices(size, 1)
        q.append(a + start)
        r.append(b + start)
        start += size
    q, r = np.concatenate(q), np.concatenate(r)
    w = weight(rng, len(q))
    nq, nr = rng.integers(0, n, noise_rows), rng.integers(0, n, noise_rows)
    return (np.concatenate([q, nq]).astype(np.uint32), np.concatenate([r, nr]).astype(np.uint32),
            np.concatenate([w, noise_weight(rng, noise_rows)]).astype(np.float64))
