"""Plain-Python sequential restatement of the single-linkage merge table and its cuts ("Merge table"):
the checker of vg_cluster_linkage_graph, vg_cluster_levels_graph and vg_cluster_linkage.  It stands on cluster_restatement
(rows, edges, labels, the bytes of clusters.tsv).

Edge {a, b} (a < b) of weight w has the key (-w, a, b), with -0.0 read as +0.0: a strict total order.  Kruskal over the edges
in key order; an edge whose ends lie in different clusters is a merge.  Objects are nodes 0 .. n-1, merge k creates node
n + k.  The cut at level t joins the merges with w >= t; a cluster id is its minimum member."""
import cluster_restatement as cr


class _Sets:
    """union-find; the root of a set is its minimum member"""

    def __init__(self, n):
        self.up = list(range(n))

    def find(self, x):
        while self.up[x] != x:
            self.up[x] = self.up[self.up[x]]
            x = self.up[x]
        return x

    def join(self, a, b):
        a, b = sorted((self.find(a), self.find(b)))
        self.up[b] = a
        return a


def forest(n, e):
    """-> [(a, b, w)] of the merges in key order; e = cr.edges(rows)"""
    sets = _Sets(n)
    out = []
    for (a, b), w in sorted(e.items(), key=lambda kv: (-(kv[1] + 0.0), kv[0][0], kv[0][1])):
        if sets.find(a) != sets.find(b):
            sets.join(a, b)
            out.append((a, b, w + 0.0))
    return out


def table(n, merges):
    """-> [(node_a, node_b, similarity, size, object_a, object_b)], one row per merge"""
    sets = _Sets(n)
    node, size = list(range(n)), [1] * n
    rows = []
    for k, (a, b, w) in enumerate(merges):
        ra, rb = sets.find(a), sets.find(b)
        assert ra != rb
        na, nb = sorted((node[ra], node[rb]))
        sz = size[ra] + size[rb]
        root = sets.join(ra, rb)
        node[root], size[root] = n + k, sz
        rows.append((na, nb, w, sz, a, b))
    return rows


def cut(n, merges, level):
    """-> cluster id (minimum member) of every object after the merges with w >= level"""
    sets = _Sets(n)
    for a, b, w in merges:
        if w >= level:
            sets.join(a, b)
    return [sets.find(i) for i in range(n)]


def linkage(n, rows):
    return table(n, forest(n, cr.edges(rows)))


def levels(n, rows, lv):
    """-> [(label, representative)] per level, in the order given"""
    merges = forest(n, cr.edges(rows))
    return [cr.labels(cut(n, merges, t)) for t in lv]


def linkage_tsv(tab):
    body = ''.join('%d\t%d\t%.6g\t%d\t%d\t%d\n' % row for row in tab)
    return ('node_a\tnode_b\tsimilarity\tsize\tobject_a\tobject_b\n' + body).encode()


def clusters_tsv(ids, metric, lv, columns, representatives=False):
    """columns[0] = (label, rep) of the cut at the floor, columns[1 + k] that of level lv[k]"""
    head = 'object\tcluster' + ''.join('\t%s_%g' % (metric, t) for t in lv) + '\n'
    body = ''.join(x + ''.join('\t' + (ids[rep[i]] if representatives else str(label[i])) for label, rep in columns) + '\n'
                   for i, x in enumerate(ids))
    return (head + body).encode()


def run(ani_path, ids_path, metric='tani', lv=(), num_alns=0, representatives=False, **mins):
    """-> (the bytes of clusters.tsv with one column per level, the bytes of the linkage file) for these files and options"""
    ids = cr.read_ids(ids_path)
    n = len(ids)
    merges = forest(n, cr.edges(cr.read_rows(ani_path, n, metric, num_alns, **mins)))
    columns = [cr.labels(cut(n, merges, float('-inf')))] + [cr.labels(cut(n, merges, t)) for t in lv]
    return clusters_tsv(ids, metric, list(lv), columns, representatives), linkage_tsv(table(n, merges))
