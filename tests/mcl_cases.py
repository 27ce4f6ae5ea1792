"""The graphs the Markov-clustering tests share (tests/test_mcl_cpu.py checks them against the restatement alone, tests/test_gpu_mcl.py
holds the library to it on them): (name, n_objects, rows [(q, r, w)], parameters) per case, small enough for seconds.
table_size_cases() are the graphs at the constants of the expansion (the 4 096-slot table, its 3/4 limit, the spill batch), with
predict(), which reads off the restatement's matrices what the table does with each row."""
import random

SMALLEST = 2.0 ** -32           # one quantum of the weights


def bridged_cliques():
    """two 6-cliques of 0.9 joined by one row of 0.71: two clusters, where single linkage sees one"""
    rows = [(c + x, c + y, 0.9) for c in (0, 6) for x in range(6) for y in range(x + 1, 6)]
    return 12, rows + [(5, 6, 0.71)]


def widths():
    """hubs of 0, 1, 63, 64, 65, 255, 256 and 257 neighbours among objects of degree 2 (a ring of leaves, each hub on leaves of its own)"""
    degrees = (0, 1, 63, 64, 65, 255, 256, 257)
    n_leaves = sum(degrees)
    rows = [(len(degrees) + k, len(degrees) + (k + 1) % n_leaves, 0.75 + 0.2 * ((k * 7) % 11) / 11) for k in range(n_leaves)]
    leaf = len(degrees)
    for hub, d in enumerate(degrees):
        rows += [(hub, leaf + k, 0.8 + 0.15 * ((k * 5) % 13) / 13) for k in range(d)]
        leaf += d
    return len(degrees) + n_leaves, rows


def hub(distinct, degree=20):
    """a hub of `degree` leaves, more than max_row = 8: with equal weights the selection goes by column alone"""
    return degree + 1, [(0, k, 0.9 - (0.01 * k if distinct else 0)) for k in range(1, degree + 1)]


def random_graph(n, seed):
    rng = random.Random(seed)
    rows = []
    for _ in range(rng.randrange(n, 4 * n + 1)):
        rows.append((rng.randrange(n), rng.randrange(n), rng.choice([0.7, 0.8, 0.95, 1.0, rng.random() * 0.3 + 0.7])))
    return n, rows


def planted(cliques=20, size=8):
    """cliques of 0.95 joined in a ring by one row of 0.7 each"""
    rows = []
    for c in range(cliques):
        rows += [(c * size + x, c * size + y, 0.95) for x in range(size) for y in range(x + 1, size)]
        rows.append((c * size + size - 1, ((c + 1) % cliques) * size, 0.7))
    return cliques * size, rows


def path(n=100):
    return n, [(k, k + 1, 0.9) for k in range(n - 1)]


def definition_edges():
    return [('one object', 1, [], {}),
            ('no rows', 5, [], {}),
            ('self rows only', 4, [(0, 0, 0.9), (2, 2, 1.0), (3, 3, 0.5)], {}),
            ('duplicate and reverse rows', 4, [(0, 1, 0.8), (1, 0, 0.9), (0, 1, 0.7), (2, 3, 0.75), (3, 2, 0.75), (1, 2, 0.71), (1, 1, 1.0)], {}),
            ('one edge', 3, [(2, 0, 0.85)], {}),
            ('weights 1.0 and one quantum', 6, [(0, 1, 1.0), (1, 2, SMALLEST), (2, 3, 1.0), (3, 4, SMALLEST), (4, 5, 1.0), (0, 5, 1.0)], {}),
            ('weights that quantise to 0', 4, [(0, 1, 0.0), (1, 2, 2.0 ** -40), (2, 3, 0.9)], {})]


RANDOM_SIZES = (2, 3, 17, 65, 130, 300)
RANDOM_PARAMS = ((1.5, 4), (2.0, 16), (3.5, 64))


def random_cases():
    """every size under every inflation; max_row goes round with the size so that each value meets each inflation"""
    out = []
    for si, n in enumerate(RANDOM_SIZES):
        for pi, (inflation, _) in enumerate(RANDOM_PARAMS):
            max_row = RANDOM_PARAMS[(pi + si) % 3][1]
            out.append((f'random n={n} inflation={inflation} max_row={max_row}', *random_graph(n, 100 * n + pi),
                        dict(inflation=inflation, max_row=max_row)))
    return out


def crown(leaves_of_the_first_spoke=82, spokes=37, leaves=82, n=4400):
    """a hub joined to `spokes` spokes that form a clique, every spoke with private leaves, then objects without rows up to n.
    Hub and spokes name each other, so each of these 38 rows has every connected object as a candidate column:
    1 + 37 + 37 * 82 = 3 072, three quarters of the 4 096-slot table to the column; one more leaf makes it 3 073."""
    rows = [(0, s, 0.9) for s in range(1, spokes + 1)]
    rows += [(s, t, 0.8 + 0.1 * ((s * t) % 7) / 7) for s in range(1, spokes + 1) for t in range(s + 1, spokes + 1)]
    leaf = spokes + 1
    for s in range(1, spokes + 1):
        for k in range(leaves_of_the_first_spoke if s == 1 else leaves):
            rows.append((s, leaf, 0.7 + 0.25 * ((leaf * 7) % 13) / 13))
            leaf += 1
    assert leaf <= n
    return n, rows


def two_cliques(size=72, n=4400):
    """every row names `size` rows of `size` entries: a bound of 5 184 over 72 distinct columns"""
    return n, [(c + x, c + y, 0.9 - 0.002 * ((x + y) % 5)) for c in (0, size) for x in range(size) for y in range(x + 1, size)]


def star(roots, mids, leaves, w_mid=0.7, w_leaf=1.0):
    """two-level stars: `mids` objects on every root (weight w_mid), `leaves` objects on every one of those (weight w_leaf); the
    roots are not joined.  With the lighter inner weight a root's row keeps candidates among the leaves after the first iteration,
    so that max_row cuts it."""
    rows, nxt = [], roots
    for a in range(roots):
        for _ in range(mids):
            rows.append((a, nxt, w_mid))
            nxt += 1
    for m in range(roots, roots + roots * mids):
        for _ in range(leaves):
            rows.append((m, nxt, w_leaf))
            nxt += 1
    return nxt, rows


def predict(start, trace, iterations, slots, row=None):
    """What the expansion does with the table, from the restatement's matrices alone: per matrix that is expanded (the start matrix,
    then every iterate but the last) dict(tried, distinct, spilled, records).  A row's candidate bound is the sum of nnz over the
    rows it names; with min(bound, n) > slots the row is `tried` in the table, and it spills iff its distinct candidate columns
    exceed 3/4 of the slots (they are counted for tried rows only; `distinct` is that count for `row`, None if it is not tried);
    a spilled row costs its bound in records."""
    out = []
    for m in [start] + [t['matrix'] for t in trace[:iterations - 1]]:
        n, nnz = len(m), [len(x) for x in m]
        fig = dict(tried=0, distinct=None, spilled=0, records=0)
        for i, named in enumerate(m):
            bound = sum(nnz[k] for k in named)
            if min(bound, n) <= slots:
                continue
            fig['tried'] += 1
            distinct = len(set().union(*(m[k] for k in named)))
            if i == row:
                fig['distinct'] = distinct
            if distinct > slots - slots // 4:
                fig['spilled'] += 1
                fig['records'] += bound
        out.append(fig)
    return out


def table_size_cases():
    """(name, n, rows, parameters, slots, expected) at the sizes where the constants of the expansion bite.  They are not part of
    all_cases(), which is re-run at 64 slots and at four iteration limits.  expected = dict(row, figures, widest): figures[t] is
    what predict() must say of the expansion of iteration t + 1 (a key left out is not asserted, but the list has one entry per
    iteration of the run), widest the widest row of the last matrix -- see reaches_its_path.  The default table has 4 096 slots:
    3 072 distinct columns stay in it, 3 073 spill.  The restatement's trace on one CPU core: a crown 0.5 to 0.7 s, the cliques
    0.1 s, the 1 x 64 x 64 star 2.3 s (0.3 s for its one iteration at max_row 2 048), the 2 x 70 x 70 star 7 s and 0.6 s of
    predict() -- the one long case, because the reference does the same 5 x 10^7 products."""
    one, wide = dict(max_iterations=1), dict(max_row=1024, prune=0.0, max_iterations=1)
    stays = [dict(tried=38, distinct=3072, spilled=0, records=0)]
    spills = [dict(tried=38, distinct=3073, spilled=38)]
    hub_spills = dict(tried=1, distinct=4161, spilled=1, records=4289)          # 65 + 64 * 66 products
    n_star, star_rows = star(1, 64, 64)
    n_two, two_rows = star(2, 70, 70)
    return [('crown of 3072 columns', *crown(82), one, 4096, dict(row=0, figures=stays)),
            ('crown of 3073 columns', *crown(83), one, 4096, dict(row=0, figures=spills)),
            # the select over 3 072 candidates in LDS, and over 3 073 in the global segment of the spill path
            ('crown of 3072 columns, max_row 1024', *crown(82), wide, 4096, dict(row=0, figures=stays, widest=1024)),
            ('crown of 3073 columns, max_row 1024', *crown(83), wide, 4096, dict(row=0, figures=spills, widest=1024)),
            ('two cliques of 72', *two_cliques(), one, 4096, dict(row=0, figures=[dict(tried=144, distinct=72, spilled=0, records=0)])),
            ('star 1 x 64 x 64', n_star, star_rows, {}, 4096,
             dict(row=0, figures=[hub_spills, dict(tried=4161, spilled=1), dict(tried=0, spilled=0)])),
            ('star 1 x 64 x 64, max_row 2048', n_star, star_rows, dict(max_row=2048, prune=0.0, max_iterations=1), 4096,
             dict(row=0, figures=[hub_spills], widest=2048)),
            # more records in one iteration than the 2^25 = 33 554 432 the spill path sorts at once
            ('star 2 x 70 x 70 at 64 slots', n_two, two_rows, {}, 64,
             dict(row=0, figures=[dict(spilled=n_two), dict(spilled=n_two, records=52076144), dict(tried=0)]))]


def reaches_its_path(case, start, trace):
    """asserts, from the restatement's matrices alone, that a case of table_size_cases() does what it is there for -> predict()'s
    figures of the whole run"""
    name, n, rows, params, slots, expected = case
    figures = predict(start, trace, len(trace), slots, row=expected['row'])
    assert len(figures) == len(expected['figures']), (name, len(figures))
    for t, (got, want) in enumerate(zip(figures, expected['figures'])):
        assert {k: got[k] for k in want} == want, (name, t, got)
    if 'widest' in expected:
        assert max(len(row) for row in trace[-1]['matrix']) == expected['widest'], name
    return figures


def all_cases():
    return (definition_edges()
            + [('bridged cliques', *bridged_cliques(), {}), ('widths', *widths(), {}),
               ('hub of equal weights', *hub(False), dict(max_row=8)), ('hub of distinct weights', *hub(True), dict(max_row=8)),
               ('planted partition', *planted(), {})]
            + random_cases())
