"""The graphs the Markov-clustering tests share (tests/test_mcl_cpu.py checks them against the restatement alone, tests/test_gpu_mcl.py
holds the library to it on them): (name, n_objects, rows [(q, r, w)], parameters) per case, small enough for seconds."""
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


def all_cases():
    return (definition_edges()
            + [('bridged cliques', *bridged_cliques(), {}), ('widths', *widths(), {}),
               ('hub of equal weights', *hub(False), dict(max_row=8)), ('hub of distinct weights', *hub(True), dict(max_row=8)),
               ('planted partition', *planted(), {})]
            + random_cases())
