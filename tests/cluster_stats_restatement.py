"""Plain-Python sequential restatement of the cluster report ("Cluster report"): the checker of
vg_cluster_stats_graph, vg_cluster_stats_file and `cluster --out-stats`.  `int` and `fractions.Fraction` only: no float takes part in
any figure before the one conversion to the printed double.  It lives beside the tests because oracle/ is frozen.

The graph is that of cluster_restatement (self rows dropped, duplicate and reverse rows merged to the maximum); a weight w in [0, 1]
is the integer u = round-half-even(w * 2^32).  label[i] in [0, n_clusters) is any partition of the objects."""
from fractions import Fraction

import cluster_restatement as cr

FIELDS = ('size', 'rep', 'pairs', 'linked', 'sum', 'min', 'external', 'nearest', 'nearest_max', 'nearest_sum', 'misfits')
COLUMNS = ('column', 'cluster', 'size', 'representative', 'pairs', 'linked', 'min_{m}', 'mean_linked', 'mean_all', 'external', 'nearest',
           'nearest_{m}', 'nearest_mean', 'misfits')


class ClustersError(ValueError):
    pass


def quanta(w):
    if not (w == w and 0 <= w <= 1):
        raise ValueError(f'weight {w} outside [0, 1]')
    return round(Fraction(w) * 2 ** 32)


def stats_graph(n, rows, label, n_clusters):
    """-> (records: list of dicts with FIELDS, own_max[n], other_max[n], other[n])"""
    for x in label:
        if not 0 <= x < n_clusters:
            raise ValueError(f'label {x} outside 0..{n_clusters - 1}')
    e = {k: quanta(w) for k, w in cr.edges(rows).items()}
    rec = [dict(size=0, rep=-1, pairs=0, linked=0, sum=0, min=None, external=0, nearest=-1, nearest_max=0, nearest_sum=0, misfits=0)
           for _ in range(n_clusters)]
    for i in range(n):
        c = rec[label[i]]
        c['size'] += 1
        if c['rep'] < 0:
            c['rep'] = i
    between = [dict() for _ in range(n_clusters)]       # between[c][d] = [largest u, sum of u] over the edges between c and d
    own_max, other_max, other = [0] * n, [0] * n, [-1] * n
    for (a, b), u in sorted(e.items()):
        ca, cb = label[a], label[b]
        if ca == cb:
            c = rec[ca]
            c['linked'] += 1
            c['sum'] += u
            c['min'] = u if c['min'] is None else min(c['min'], u)
            own_max[a], own_max[b] = max(own_max[a], u), max(own_max[b], u)
            continue
        for x, cx, cy in ((a, ca, cb), (b, cb, ca)):
            rec[cx]['external'] += 1
            t = between[cx].setdefault(cy, [0, 0])
            t[0] = max(t[0], u)
            t[1] += u
            if other[x] < 0 or (u, -cy) > (other_max[x], -other[x]):        # the largest u; ties: the smallest label
                other_max[x], other[x] = u, cy
    for k, c in enumerate(rec):
        c['pairs'] = c['size'] * (c['size'] - 1) // 2
        c['min'] = c['min'] or 0
        if between[k]:
            d = min(between[k], key=lambda d: (-between[k][d][0], d))
            c['nearest'], c['nearest_max'], c['nearest_sum'] = d, between[k][d][0], between[k][d][1]
    for i in range(n):
        rec[label[i]]['misfits'] += other_max[i] > own_max[i]
    return rec, own_max, other_max, other


# ---------------------------------------------------------------- clusters.tsv
def read_clusters(path, ids, is_repr=False):
    """-> (names, label, text): the headers of the label columns; label[c][i] = the cluster of object i in column c, clusters numbered
    0.. by their earliest member; text[c][k] = the label of cluster k as the file writes it.  ClustersError('<path>:<line>: ...')."""
    data = open(path, newline='').read()
    if not data:
        raise ClustersError(f'{path}:1: empty file (no header)')
    lines = data.split('\n')
    if lines[-1] == '':
        lines.pop()
    lines = [ln[:-1] if ln.endswith('\r') else ln for ln in lines]
    head = lines[0].split('\t')
    if len(head) < 2 or head[0] != 'object' or '' in head:
        raise ClustersError(f'{path}:1: malformed header')
    names, nc = head[1:], len(head) - 1
    index = {x: i for i, x in enumerate(ids)}
    line_of, value = {}, {}
    for no, ln in enumerate(lines[1:], start=2):
        if not ln:
            continue
        f = ln.split('\t')
        if len(f) != nc + 1 or '' in f:
            raise ClustersError(f'{path}:{no}: malformed line')
        if f[0] not in index:
            raise ClustersError(f"{path}:{no}: object '{f[0]}' is not in the ids file")
        i = index[f[0]]
        if i in line_of:
            raise ClustersError(f"{path}:{no}: object '{f[0]}' is listed twice")
        line_of[i], value[i] = no, f[1:]
        if not is_repr:
            for v in f[1:]:
                if not (v.isascii() and v.isdigit() and int(v) < 2 ** 31):
                    raise ClustersError(f"{path}:{no}: malformed cluster number '{v}'")
    for i, x in enumerate(ids):
        if i not in line_of:
            raise ClustersError(f"{path}:{len(lines)}: object '{x}' of the ids file is missing")
    if is_repr:
        for i in range(len(ids)):
            for c, v in enumerate(value[i]):
                if v not in index:
                    raise ClustersError(f"{path}:{line_of[i]}: representative '{v}' is not in the ids file")
                if value[index[v]][c] != v:
                    raise ClustersError(f"{path}:{line_of[i]}: representative '{v}' is not a member of its cluster")
    label, text = [], []
    for c in range(nc):
        seen, lab, txt = {}, [], []
        for i in range(len(ids)):
            v = value[i][c]
            key = v if is_repr else int(v)
            if key not in seen:
                seen[key] = len(txt)
                txt.append(v)
            lab.append(seen[key])
        label.append(lab)
        text.append(txt)
    return names, label, text


# ---------------------------------------------------------------- the report
def quotient(s, p):
    """the printed form of s / (p * 2^32): the double nearest the exact value, %.6g; `-` without a denominator"""
    if p is None or p == 0:
        return '-'
    return '%.6g' % float(Fraction(s, p * 2 ** 32))


def report(ids, rows, names, label, text, metric='tani'):
    """the bytes of the report file"""
    out = ['\t'.join(COLUMNS).replace('{m}', metric)]
    for c, name in enumerate(names):
        rec = stats_graph(len(ids), rows, label[c], len(text[c]))[0]
        for k in sorted((k for k in range(len(rec)) if rec[k]['size']), key=lambda k: rec[k]['rep']):
            r = rec[k]
            near = r['nearest'] >= 0
            out.append('\t'.join(str(x) for x in (
                name, text[c][k], r['size'], ids[r['rep']], r['pairs'], r['linked'],
                quotient(r['min'], 1 if r['linked'] else None), quotient(r['sum'], r['linked']), quotient(r['sum'], r['pairs']),
                r['external'], text[c][r['nearest']] if near else '-', quotient(r['nearest_max'], 1 if near else None),
                quotient(r['nearest_sum'], r['size'] * rec[r['nearest']]['size'] if near else None), r['misfits'])))
    return ('\n'.join(out) + '\n').encode()


def run(ani_path, ids_path, clusters_path, is_repr=False, metric='tani', num_alns=0, **mins):
    """the bytes of the report for these files and options"""
    ids = cr.read_ids(ids_path)
    rows = cr.read_rows(ani_path, len(ids), metric, num_alns, **mins)
    names, label, text = read_clusters(clusters_path, ids, is_repr)
    return report(ids, rows, names, label, text, metric)
