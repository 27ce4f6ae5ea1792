"""Plain-Python sequential restatement of the cluster stage's contract: the checker of vg_cluster and
vg_cluster_graph.  It lives beside the tests because oracle/ is frozen.

Objects are the rows of the ids file; a row of ani.tsv passes when every minimum > 0 holds (column >= value), num_alns <=
max when that is > 0, and qidx != ridx; it gives the undirected edge {qidx, ridx} with the metric as weight (max over
duplicates).  The four algorithms visit objects in index order; labels number multi-member clusters by earliest member,
then singletons in object order; --out-repr prints the id of the cluster's earliest member."""
import heapq

FILTERS = ('tani', 'gani', 'ani', 'qcov', 'rcov', 'len_ratio')


class RowError(ValueError):
    pass


def read_ids(ids_path):
    lines = open(ids_path).read().split('\n')
    return [ln.split('\t')[0] for ln in lines[1:] if ln]


def read_rows(ani_path, n_objects, metric='tani', num_alns=0, **mins):
    """-> list of (q, r, w) of the passing rows; RowError('<path>:<line>: ...') on a missing column, an index outside the ids
    file or a malformed number."""
    lines = open(ani_path).read().split('\n')
    head = lines[0].split('\t')

    def col(name):
        if name not in head:
            raise RowError(f'{ani_path}:1: missing column {name}')
        return head.index(name)
    qc, rc, mc = col('qidx'), col('ridx'), col(metric)
    active = [(col(f), v) for f, v in ((f, mins.get(f, 0)) for f in FILTERS) if v > 0]
    nc = col('num_alns') if num_alns > 0 else None
    out = []
    for ln, line in enumerate(lines[1:], start=2):
        if not line:
            continue
        f = line.split('\t')
        try:
            q, r = int(f[qc]), int(f[rc])
            w = float(f[mc])
            vals = [float(f[c]) for c, _ in active]
            na = float(f[nc]) if nc is not None else None
        except (ValueError, IndexError) as e:
            raise RowError(f'{ani_path}:{ln}: malformed row ({e})')
        if not (0 <= q < n_objects and 0 <= r < n_objects):
            raise RowError(f'{ani_path}:{ln}: index outside the ids file')
        if q == r or any(v < m for v, (_, m) in zip(vals, active)) or (na is not None and na > num_alns):
            continue
        out.append((q, r, w))
    return out


def edges(rows):
    """{(a, b): w} with a < b: self rows dropped, duplicates and reverse rows merged to the maximum weight."""
    e = {}
    for q, r, w in rows:
        if q == r:
            continue
        k = (min(q, r), max(q, r))
        e[k] = max(e.get(k, w), w)
    return e


def adjacency(n, e):
    adj = [dict() for _ in range(n)]
    for (a, b), w in e.items():
        adj[a][b] = w
        adj[b][a] = w
    return adj


def single(n, adj):
    """connected components; cluster id = minimum member"""
    cid = [-1] * n
    for s in range(n):
        if cid[s] >= 0:
            continue
        cid[s] = s
        stack = [s]
        while stack:
            x = stack.pop()
            for y in adj[x]:
                if cid[y] < 0:
                    cid[y] = s
                    stack.append(y)
    return cid


def greedy(n, adj, uclust):
    """cd-hit: join the earliest representative linked to the object; uclust: the one of highest weight (ties: earliest)"""
    rep = [-1] * n
    for i in range(n):
        best = None
        for j, w in adj[i].items():
            if j < i and rep[j] == j:
                key = (-w, j) if uclust else (j,)
                if best is None or key < best[0]:
                    best = (key, j)
        rep[i] = best[1] if best else i
    return rep


def set_cover(n, adj):
    """greedy set cover: repeatedly the unassigned object with the most unassigned neighbours (ties: earliest) becomes a
    representative; it and its unassigned neighbours form its cluster"""
    asg = [-1] * n
    cnt = [len(a) for a in adj]
    heap = [(-cnt[i], i) for i in range(n)]
    heapq.heapify(heap)
    while heap:
        c, p = heapq.heappop(heap)
        if asg[p] >= 0:
            continue
        if -c != cnt[p]:
            heapq.heappush(heap, (-cnt[p], p))
            continue
        new = [p] + [j for j in adj[p] if asg[j] < 0]
        for x in new:
            asg[x] = p
        for x in new:
            for y in adj[x]:
                if asg[y] < 0:
                    cnt[y] -= 1
    return asg


def cluster_ids(n, e, algorithm):
    adj = adjacency(n, e)
    if algorithm == 'single':
        return single(n, adj)
    if algorithm in ('cd-hit', 'uclust'):
        return greedy(n, adj, algorithm == 'uclust')
    if algorithm == 'set-cover':
        return set_cover(n, adj)
    raise ValueError(algorithm)


def labels(cid):
    """-> (label, representative): representative = the cluster's earliest member; multi-member clusters numbered by it,
    then singletons in object order"""
    n = len(cid)
    first, size = {}, {}
    for i, c in enumerate(cid):
        first.setdefault(c, i)
        size[c] = size.get(c, 0) + 1
    rep = [first[c] for c in cid]
    multi = sorted(first[c] for c in first if size[c] >= 2)
    num = {h: k for k, h in enumerate(multi)}
    k = len(multi)
    for i in range(n):
        if rep[i] == i and size[cid[i]] == 1:
            num[i] = k
            k += 1
    return [num[r] for r in rep], rep


def cluster_graph(n, rows, algorithm):
    return labels(cluster_ids(n, edges(rows), algorithm))


def clusters_tsv(ids, label, rep, representatives=False):
    body = ''.join(f'{x}\t{ids[rep[i]] if representatives else label[i]}\n' for i, x in enumerate(ids))
    return ('object\tcluster\n' + body).encode()


def run(ani_path, ids_path, algorithm='single', metric='tani', num_alns=0, representatives=False, **mins):
    """the bytes of clusters.tsv for these files and options"""
    ids = read_ids(ids_path)
    label, rep = cluster_graph(len(ids), read_rows(ani_path, len(ids), metric, num_alns, **mins), algorithm)
    return clusters_tsv(ids, label, rep, representatives)
