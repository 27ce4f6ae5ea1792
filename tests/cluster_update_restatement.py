"""Plain-Python sequential restatement of the update of a prior clustering ("Update of a prior
clustering"): the checker of vg_cluster_update and vg_cluster_update_graph, on the shared rules of cluster_restatement.

prior_rep[i] is -1 for a new object, else the index of the representative of i's prior cluster.  The visit order is the prior
objects in index order, then the new ones in index order.  Rows are filtered and merged as ever, and an edge between two prior
objects is dropped.  cd-hit / uclust: prior clusters and their representatives are frozen; a new object joins the earliest
(cd-hit) or heaviest (uclust; ties: earliest) representative before it in visit order that it has an edge to, else founds a
cluster.  single: the components of the prior partition plus the kept edges; the representative is the earliest member."""
import cluster_restatement as cr

ALGORITHMS = ('single', 'cd-hit', 'uclust')


class PriorError(ValueError):
    pass


def read_prior(prior_path, ids, is_repr=False):
    """-> prior_rep; PriorError('<path>:<line>: ...') on a bad header, a malformed line, a name that is not in the ids file or
    listed twice, and (is_repr) a representative that is no object of the file or not its own representative."""
    index = {x: i for i, x in enumerate(ids)}
    lines = open(prior_path).read().split('\n')
    if lines[0].rstrip('\r') != 'object\tcluster':
        raise PriorError(f'{prior_path}:1: malformed header')
    entries, seen = [], set()
    for ln, line in enumerate(lines[1:], start=2):
        line = line.rstrip('\r')
        if not line:
            continue
        f = line.split('\t')
        if len(f) != 2 or not f[0] or not f[1]:
            raise PriorError(f'{prior_path}:{ln}: malformed line')
        if f[0] not in index:
            raise PriorError(f'{prior_path}:{ln}: object {f[0]} is not in the ids file')
        if f[0] in seen:
            raise PriorError(f'{prior_path}:{ln}: object {f[0]} is listed twice')
        seen.add(f[0])
        entries.append((index[f[0]], ln, f[1]))
    prior_rep = [-1] * len(ids)
    if is_repr:
        for obj, ln, value in entries:
            if value not in seen:
                raise PriorError(f'{prior_path}:{ln}: representative {value} is not an object of this file')
            prior_rep[obj] = index[value]
        for obj, ln, value in entries:
            if prior_rep[prior_rep[obj]] != prior_rep[obj]:
                raise PriorError(f'{prior_path}:{ln}: representative {value} is not its own representative')
        return prior_rep
    first = {}
    for obj, ln, value in entries:
        if not (value.isascii() and value.isdigit()):
            raise PriorError(f'{prior_path}:{ln}: malformed cluster number {value}')
        first[int(value)] = min(first.get(int(value), obj), obj)
    for obj, ln, value in entries:
        prior_rep[obj] = first[int(value)]
    return prior_rep


def visit_rank(prior_rep):
    order = [i for i, p in enumerate(prior_rep) if p >= 0] + [i for i, p in enumerate(prior_rep) if p < 0]
    rank = [0] * len(prior_rep)
    for v, i in enumerate(order):
        rank[i] = v
    return rank


def kept_edges(rows, prior_rep):
    """the edges of the rows without those between two prior objects"""
    return {(a, b): w for (a, b), w in cr.edges(rows).items() if prior_rep[a] < 0 or prior_rep[b] < 0}


def frozen_greedy(n, adj, prior_rep, uclust):
    rank = visit_rank(prior_rep)
    rep = list(prior_rep)
    for i in range(n):                      # (the new objects in index order: their visit order)
        if prior_rep[i] >= 0:
            continue
        best = None
        for j, w in adj[i].items():
            if rank[j] < rank[i] and rep[j] == j:
                key = (-w, rank[j]) if uclust else (rank[j],)
                if best is None or key < best[0]:
                    best = (key, j)
        rep[i] = best[1] if best else i
    return rep


def union_single(n, e, prior_rep):
    """components of the prior partition plus the edges: every prior member is tied to its representative"""
    tied = dict(e)
    for i, p in enumerate(prior_rep):
        if p >= 0 and p != i:
            tied[(min(i, p), max(i, p))] = 1.0
    return cr.single(n, cr.adjacency(n, tied))


def update_graph(n, rows, prior_rep, algorithm):
    """-> (label, representative, stats): label numbers the final partition by earliest member (the rule of cr.labels);
    representative is the frozen or founding representative (single: the earliest member)"""
    assert all(p == -1 or (0 <= p < n and prior_rep[p] == p) for p in prior_rep)
    e = kept_edges(rows, prior_rep)
    new = [i for i in range(n) if prior_rep[i] < 0]
    stats = dict(n_edges=len(e), n_prior=n - len(new), n_new=len(new), joined_prior=0, joined_new=0, founded=0, prior_merged=0)
    if algorithm == 'single':
        cid = union_single(n, e, prior_rep)
        with_prior = {cid[i] for i in range(n) if prior_rep[i] >= 0}
        stats['founded'] = sum(cid[i] not in with_prior for i in new)
        stats['joined_prior'] = len(new) - stats['founded']
        stats['prior_merged'] = len({p for p in prior_rep if p >= 0}) - len(with_prior)
        label, rep = cr.labels(cid)
        return label, rep, stats
    if algorithm not in ('cd-hit', 'uclust'):
        raise ValueError(algorithm)
    rep = frozen_greedy(n, cr.adjacency(n, e), prior_rep, algorithm == 'uclust')
    for i in new:
        stats['founded' if rep[i] == i else 'joined_prior' if prior_rep[rep[i]] >= 0 else 'joined_new'] += 1
    return cr.labels(rep)[0], rep, stats


def prior_of(cid, members):
    """the prior_rep of a run restricted to `members`: cid[i] (a member) for them, -1 for the others"""
    inside = set(members)
    return [c if i in inside else -1 for i, c in enumerate(cid)]


def run(ani_path, ids_path, prior_path, algorithm='single', metric='tani', num_alns=0, representatives=False, prior_repr=False, **mins):
    """the bytes of clusters.tsv for these files and options"""
    ids = cr.read_ids(ids_path)
    prior_rep = read_prior(prior_path, ids, prior_repr)
    label, rep, _ = update_graph(len(ids), cr.read_rows(ani_path, len(ids), metric, num_alns, **mins), prior_rep, algorithm)
    return cr.clusters_tsv(ids, label, rep, representatives)
