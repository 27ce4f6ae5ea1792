"""Plain-Python restatement of Markov clustering as this project defines it ("Markov clustering"): the checker
of vg_cluster_mcl and vg_cluster_mcl_graph.  Every matrix entry is an integer in units of 2^-30, every sum an integer sum, so the
result does not depend on the order in which anything is added: the library is held to this bit for bit.

Rows, filters, edges, labels and the clusters.tsv writer are those of cluster_restatement."""
import math

import cluster_restatement as cr

ONE = 1 << 30
DEFAULTS = dict(inflation=2.0, prune=1e-4, max_row=128, chaos_eps=1e-3, max_iterations=100)


def quantise(w):
    """llrint(w * 2^32): the product is exact, round() and llrint both round ties to even"""
    return int(round(math.ldexp(w, 32)))


def normalise(x):
    """{j: floor(x_j * ONE / sum)}, entries that become 0 dropped"""
    s = sum(x.values())
    return {j: v * ONE // s for j, v in x.items() if v * ONE // s > 0}


def power(y, a):
    """y^(a/2) in units of 2^-30, every step floored"""
    t = math.isqrt(y << 30) if a & 1 else ONE
    for _ in range(a >> 1):
        t = (t * y) >> 30
    return t


def prune(p, cut, max_row):
    """entries >= cut (the largest, if none passes), then the max_row largest by (value descending, column ascending)"""
    kept = {j: v for j, v in p.items() if v >= cut}
    if not kept:
        j = min(p, key=lambda j: (-p[j], j))
        kept = {j: p[j]}
    if len(kept) > max_row:
        kept = {j: kept[j] for j in sorted(kept, key=lambda j: (-kept[j], j))[:max_row]}
    return kept


def start(n, e):
    """the start matrix: quantised weights, a loop as heavy as the row's heaviest edge (ONE without edges), normalised, not pruned"""
    adj = cr.adjacency(n, e)
    m = []
    for i in range(n):
        x = {j: quantise(w) for j, w in adj[i].items()}
        x[i] = max(x.values(), default=0) or ONE          # (weights that all quantise to 0 leave nothing to normalise by: as without edges)
        m.append(normalise(x))
    return m


def step(m, a, cut, max_row):
    """one iteration -> (the next matrix, its chaos)"""
    nxt, chaos = [], 0
    for i, row in enumerate(m):
        acc = {}
        for k, p in row.items():
            for j, q in m[k].items():
                acc[j] = acc.get(j, 0) + p * q
        x = {}
        for j, v in acc.items():
            t = power(v >> 30, a)
            if t:
                x[j] = t
        if not x:
            x = {i: ONE}
        p = normalise(prune(normalise(x), cut, max_row))
        nxt.append(p)
        chaos = max(chaos, max(p.values()) - (sum(v * v for v in p.values()) >> 30))
    return nxt, chaos


def check_params(inflation, prune, max_row, chaos_eps, max_iterations):
    a = int(round(2 * inflation))
    if not (1.5 <= inflation <= 6 and abs(2 * inflation - a) < 1e-9):
        raise ValueError('inflation')
    if not 0 <= prune <= 0.1:
        raise ValueError('prune')
    if not 2 <= max_row <= 4096:
        raise ValueError('max_row')
    if not 0 <= chaos_eps < 1:
        raise ValueError('chaos_eps')
    if not 1 <= max_iterations <= 1000:
        raise ValueError('max_iterations')
    return a, int(math.floor(prune * ONE)), int(math.floor(chaos_eps * ONE))


def trace(n, e, **params):
    """-> [dict(matrix, iterations, converged, chaos)]: the iterate after every iteration up to the stop (entry t - 1 is what
    max_iterations = t gives, the last entry what any larger limit gives); with no objects, the one empty iterate"""
    p = {**DEFAULTS, **params}
    a, cut, eps = check_params(**p)
    m, out = start(n, e), []
    if not n:
        return [dict(matrix=m, iterations=0, converged=0, chaos=0)]
    while len(out) < p['max_iterations']:
        m, chaos = step(m, a, cut, p['max_row'])
        out.append(dict(matrix=m, iterations=len(out) + 1, converged=int(chaos <= eps), chaos=chaos))
        if chaos <= eps:
            break
    return out


def iterate(n, e, **params):
    """-> dict(matrix, iterations, converged, chaos): the iterate at the stop"""
    return trace(n, e, **params)[-1]


def components(n, m):
    """cluster ids: the connected components of {i, j : m_ij > 0, i != j}, each named by its minimum member"""
    f = {}
    for i, row in enumerate(m):
        for j in row:
            if i != j:
                f[(min(i, j), max(i, j))] = 1.0
    return cr.single(n, cr.adjacency(n, f))


def mcl(n, e, **params):
    """-> (cluster ids, iterations, converged, matrix)"""
    r = iterate(n, e, **params)
    return components(n, r['matrix']), r['iterations'], r['converged'], r['matrix']


def csr(m):
    """the matrix as (offsets, columns, values), columns ascending per row"""
    off, col, val = [0], [], []
    for row in m:
        for j in sorted(row):
            col.append(j)
            val.append(row[j])
        off.append(len(col))
    return off, col, val


def run(ani_path, ids_path, metric='tani', num_alns=0, representatives=False, mcl_params=None, **mins):
    """the bytes of clusters.tsv for these files and options"""
    ids = cr.read_ids(ids_path)
    rows = cr.read_rows(ani_path, len(ids), metric, num_alns, **mins)
    label, rep = cr.labels(mcl(len(ids), cr.edges(rows), **(mcl_params or {}))[0])
    return cr.clusters_tsv(ids, label, rep, representatives)
