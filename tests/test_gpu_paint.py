"""The mosaic painting on the MI355X (vg_paint_rows, vg_paint_file, `python -m vclust_amd.paint`) against the
sequential restatement (tests/paint_restatement.py): every field of every record, every segment, every donor record and every run
count is an integer and must be equal, and the three files must equal the restatement's text byte for byte.  Every test first
asserts, from the reference, that its input reaches the path it names."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_stats_restatement as cs
import paint_restatement as pr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


@pytest.fixture(scope='module')
def golden(golden_dir):
    out = golden_dir / 'output'
    ids, lengths = pr.read_ids(out / 'ani.ids.tsv')
    rows = pr.read_aln(out / 'ani.aln.tsv', ids, lengths)
    names, label, text = cs.read_clusters(out / 'clusters.tsv', ids)
    plain = pr.paint(lengths, rows)
    grouped = pr.paint(lengths, rows, label[0], len(text[0]))
    return dict(out=out, ids=ids, lengths=lengths, rows=rows, label=label[0], text=text[0], plain=plain, grouped=grouped)


def library(api, lengths, rows, label=None, n_groups=None):
    cols = [np.array([t[k] for t in rows], dtype=np.int64) for k in range(5)]
    return api.paint_rows(lengths, *cols, label=label, n_groups=n_groups)


def equal(got, want):
    records, segments, donors, run = got
    w_records, w_segments, w_donors, w_run = want
    assert run == w_run
    for f in pr.FIELDS:
        assert records[f].tolist() == [x[f] for x in w_records], f
    assert [tuple(t) for t in segments.tolist()] == w_segments
    assert [tuple(t) for t in donors.tolist()] == w_donors


def check(api, lengths, rows, label=None, n_groups=None, want=None):
    """the library's records, segments, donor records and run counts equal the restatement's; -> the library's raw bytes"""
    got = library(api, lengths, rows, label, n_groups)
    equal(got, want if want is not None else pr.paint(lengths, rows, label, n_groups))
    return got[0].tobytes() + got[1].tobytes() + got[2].tobytes()


# ---------------------------------------------------------------- level edges
LEVEL_TOP = 12


def level_edges_input():
    """Objects 0 and 1: unit rows with n_match 0 from partner 2 on every position (so every position is a breakpoint and a row of
    m positions covers m elementary segments), and over them rows of 2^k - 1, 2^k and 2^k + 1 positions for k = 0..12 at the offsets
    0, 1 and 2^(k-1), from partners 3..7.  On object 0 the identity rises along that list, on object 1 it falls: what decides a
    position is then the raise at a row's left end, the one at its right end, or what came down from the level above.  Object 2 has
    the same unit rows and one row of each of those sizes apart from all the others: it wins its whole extent, so each of its
    positions must receive the row's priority from one of the two raises through every level below the row's."""
    L = 2 ** LEVEL_TOP + 1 + 2 ** (LEVEL_TOP - 1) + 3
    shapes = []
    for k in range(LEVEL_TOP + 1):
        for m in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            for off in (0, 1, 2 ** k // 2):
                if m >= 1 and (m, off) not in shapes:
                    shapes.append((m, off))
    rows = []
    for obj in (0, 1):
        rows += [(obj, 2, x, x, 0) for x in range(L)]
        for idx, (m, off) in enumerate(shapes):
            step = idx + 1 if obj == 0 else len(shapes) - idx
            rows.append((obj, 3 + idx % 5, off, off + m - 1, max(1, m * step // (len(shapes) + 1))))
    pos = 1
    for idx, m in enumerate(sorted({m for m, _ in shapes})):
        rows.append((2, 3 + idx % 5, pos, pos + m - 1, m - m // 3))
        pos += m + 1
    rows += [(2, 1, x, x, 0) for x in range(pos)]
    return [L, L, pos, 5, 5, 5, 5, 5], rows, shapes


def test_level_edges(api):
    lengths, rows, shapes = level_edges_input()
    want = pr.paint(lengths, rows)
    assert want[3]['levels'] == LEVEL_TOP + 1 and want[3]['breakpoints'] == sum(lengths[:3]) + 3 + 5 * 2
    assert {(m.bit_length() - 1) for m, _ in shapes} == set(range(LEVEL_TOP + 1))
    for obj in (0, 1):                                   # several of the overlapping rows win somewhere, not one row alone
        assert len({(t[4], t[5]) for t in want[1] if t[0] == obj and t[3] >= 3}) >= 3
    alone = [(t[2] - t[1] + 1, t[5] - t[4] + 1) for t in want[1] if t[0] == 2 and t[3] >= 3]
    assert sorted(alone) == [(m, m) for m in sorted({m for m, _ in shapes})]           # each row of object 2 is one segment of its whole extent
    check(api, lengths, rows, want=want)


# ---------------------------------------------------------------- object boundaries at every tile offset
TILE_OBJECTS = 307


def boundaries_input():
    """Object k (k = 1..m) has k rows from k distinct partners with random identities (the shape of the coverage map's tile test: the
    object boundary falls at every offset of a 1 024-element tile in the rows, the breakpoints and the segments), then a long poor
    row that ends on its last position, and a perfect row that starts on its first."""
    m = TILE_OBJECTS
    rng = np.random.default_rng(25)
    lengths = [int(x) for x in rng.integers(30, 90, m + 1)]
    rows = []
    for k in range(1, m + 1):
        partners = [p for p in rng.permutation(m + 1).tolist() if p != k][:k]
        for p in partners:
            s = int(rng.integers(0, lengths[k]))
            e = min(lengths[k] - 1, s + int(rng.integers(0, 12)))
            rows.append((k, p, s, e, int(rng.integers(0, e - s + 2))))
        rows.append((k, (k + 1) % (m + 1), 1, lengths[k] - 1, 1))
        rows.append((k, (k + 2) % (m + 1), 0, 2, 3))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return lengths, rows, [int(x) for x in rng.integers(0, 3, m + 1)], 3


def test_object_boundaries(api):
    lengths, rows, label, n_groups = boundaries_input()
    want = pr.paint(lengths, rows, label, n_groups)
    assert len(rows) >= 4 * 1024 * 4 and want[3]['breakpoints'] >= 4 * 1024 and want[3]['segments'] >= 2 * 1024
    last = {t[0]: t for t in want[1]}                    # the last segment of every object, and the first of the next
    first = {}
    for t in want[1]:
        first.setdefault(t[0], t)
    for k in range(1, TILE_OBJECTS):
        assert last[k][2] == lengths[k] - 1 and last[k][3] >= 0                       # painted up to its last position ...
        nxt = first[k + 1]                                                              # ... and the next starts with a perfect row of its own
        assert nxt[1] == 0 and nxt[4] == 0 and nxt[6] == nxt[5] + 1
    check(api, lengths, rows, label, n_groups, want=want)


# ---------------------------------------------------------------- ties and nesting
def ties_input():
    lengths = [60, 60, 60, 60, 9, 9, 9]
    rows = [(0, 4, 0, 9, 5), (0, 5, 5, 24, 10),                      # I equal (1/2): the longer span wins 5..9
            (1, 5, 0, 9, 5), (1, 4, 5, 14, 5), (1, 6, 8, 17, 5),      # I and span equal: the smaller partner wins the overlaps
            (2, 4, 10, 19, 7), (2, 4, 5, 14, 7), (2, 4, 12, 21, 7),   # ... and the partner: the smaller qstart
            (3, 4, 0, 29, 20), (3, 4, 0, 29, 20), (3, 4, 0, 29, 20), (3, 5, 10, 19, 9), (3, 5, 10, 19, 9),      # repeated rows
            (3, 6, 40, 40, 1), (3, 6, 40, 40, 1), (3, 3, 0, 59, 60)]  # ... of one position, and a perfect self row
    return lengths, rows


def nesting_input():
    lengths = [100, 100, 100, 5, 5, 5]
    rows = [(0, 3, 10, 89, 40), (0, 4, 30, 49, 19),                                        # a better row inside a worse one
            (1, 3, 0, 99, 50), (1, 4, 20, 79, 45), (1, 5, 40, 59, 19), (1, 4, 45, 50, 6),  # three deep, and a fourth on top
            (2, 3, 0, 9, 5), (2, 4, 10, 19, 5), (2, 3, 20, 29, 5), (2, 3, 30, 39, 6), (2, 5, 99, 99, 0)]   # rows that touch; n_match 0
    return lengths, rows


def test_ties(api):
    lengths, rows = ties_input()
    want = pr.paint(lengths, rows)
    seg = want[1]
    assert [t[1:4] for t in seg if t[0] == 0] == [(0, 4, 4), (5, 24, 5), (25, 59, -1)]
    assert [t[1:4] for t in seg if t[0] == 1] == [(0, 4, 5), (5, 14, 4), (15, 17, 6), (18, 59, -1)]
    assert [t[1:5] for t in seg if t[0] == 2] == [(0, 4, -1, -1), (5, 14, 4, 5), (15, 19, 4, 10), (20, 21, 4, 12), (22, 59, -1, -1)]
    assert [t[1:4] for t in seg if t[0] == 3] == [(0, 9, 4), (10, 19, 5), (20, 29, 4), (30, 39, -1), (40, 40, 6), (41, 59, -1)]
    check(api, lengths, rows, want=want)
    check(api, lengths, rows + rows[::-1])               # every row repeated


def test_nesting(api):
    lengths, rows = nesting_input()
    want = pr.paint(lengths, rows)
    seg = want[1]
    assert [t[1:5] for t in seg if t[0] == 0] == [(0, 9, -1, -1), (10, 29, 3, 10), (30, 49, 4, 30), (50, 89, 3, 10), (90, 99, -1, -1)]
    assert [t[1:5] for t in seg if t[0] == 1] == [(0, 19, 3, 0), (20, 39, 4, 20), (40, 44, 5, 40), (45, 50, 4, 45), (51, 59, 5, 40), (60, 79, 4, 20), (80, 99, 3, 0)]
    assert want[0][1]['switches'] == 6 and want[0][1]['donors'] == 3 and want[0][1]['segments'] == 7
    assert [t[1:4] for t in seg if t[0] == 2] == [(0, 9, 3), (10, 19, 4), (20, 29, 3), (30, 39, 3), (40, 98, -1), (99, 99, 5)]
    assert want[0][2]['switches'] == 2 and want[0][0]['switches'] == 2
    check(api, lengths, rows, want=want)


# ---------------------------------------------------------------- a hot object
def hot_object_input():
    rng = np.random.default_rng(26)
    n = 1001
    lengths = [40000] + [int(x) for x in rng.integers(1, 50, n - 1)]
    rows = []
    for k in range(4096):                                # one row in eight is long and poor, the others are short and good
        s = int(rng.integers(0, 40000))
        e = min(39999, s + int(rng.integers(0, 3000 if k % 8 == 0 else 30)))
        span = e - s + 1
        rows.append((0, int(rng.integers(1, 301)), s, e, int(rng.integers(span // 4, span // 2 + 1) if k % 8 == 0 else rng.integers(span - span // 4, span + 1))))
    for k in range(1, n):
        s = int(rng.integers(0, lengths[k]))
        e = int(rng.integers(s, lengths[k]))
        rows.append((k, int(rng.integers(0, n)), s, e, int(rng.integers(0, e - s + 2))))
    return lengths, rows, [int(x) for x in rng.integers(0, 4, n)], 4


def test_hot_object(api):
    """One object with 4 096 rows from 300 partners (several workgroups of rows, breakpoints and segments in one object, rows of many
    levels) beside 1 000 objects with one row each."""
    lengths, rows, label, n_groups = hot_object_input()
    want = pr.paint(lengths, rows, label, n_groups)
    assert want[0][0]['segments'] > 2 * 1024 and want[0][0]['donors'] > 100 and want[3]['levels'] >= 10
    check(api, lengths, rows, label, n_groups, want=want)


# ---------------------------------------------------------------- groups
GROUPS_LABEL, GROUPS_SPARSE_LABEL = [0, 1, 0, 2, 1, 2, 1, 0, 2], [5, 1, 5, 7, 1, 7, 1, 5, 7]


def groups_input():
    rng = np.random.default_rng(27)
    n = 9
    lengths = [int(x) for x in rng.integers(20, 60, n)]
    rows = []
    for q in range(n):
        for r in range(n):
            for _ in range(2):
                s = int(rng.integers(0, lengths[q]))
                e = int(rng.integers(s, lengths[q]))
                rows.append((q, r, s, e, int(rng.integers(0, e - s + 2))))
    return lengths, rows


def test_groups(api):
    lengths, rows = groups_input()
    n = len(lengths)
    plain = check(api, lengths, rows)                                      # no labels
    assert plain == check(api, lengths, rows, [0] * n, 1)
    records = library(api, lengths, rows)[0]
    assert records['painted_in'].tolist() == records['painted'].tolist() and not records['painted_out'].any()
    check(api, lengths, rows, list(range(n)), n)                           # every object a group of one
    records = library(api, lengths, rows, list(range(n)), n)[0]
    assert records['painted_out'].tolist() == records['painted'].tolist() and not records['painted_in'].any()
    want = pr.paint(lengths, rows, GROUPS_LABEL, 3)
    assert all(rec['painted_in'] and rec['painted_out'] for rec in want[0])
    check(api, lengths, rows, GROUPS_LABEL, 3, want=want)
    check(api, lengths, rows, GROUPS_SPARSE_LABEL, 12)                     # more groups than labels used


ENDS_INPUTS = [([50, 1, 0, 9, 30, 12], [(0, 5, 0, 9, 9), (0, 5, 40, 49, 10), (0, 4, 0, 49, 30), (1, 0, 0, 0, 1), (4, 0, 29, 29, 0), (4, 1, 0, 0, 1), (4, 5, 0, 29, 29)]),
               ([0, 0, 0], []), ([5], []), ([5, 5], [(0, 0, 0, 4, 5), (1, 1, 2, 3, 0)])]      # no rows; the last: self rows only


def test_ends(api):
    """Position 0, a row that ends at len - 1, lengths 1 and 0, no rows at all, a partner that is never a query, self rows only."""
    for lengths, rows in ENDS_INPUTS:
        check(api, lengths, rows)
    records, segments, donors, run = library(api, *ENDS_INPUTS[0])
    assert records['segments'].tolist() == [3, 1, 0, 1, 2, 1] and records['top_partner'].tolist() == [4, 0, -1, -1, 5, -1]
    assert run['levels'] == 2 and library(api, *ENDS_INPUTS[3])[3] == dict(rows_kept=0, breakpoints=4, segments=2, donor_records=0, levels=0)


# ---------------------------------------------------------------- invariance
def test_order_and_threads(api, golden, tmp_path):
    rng = np.random.default_rng(28)
    g = golden
    rows = g['rows']
    first = check(api, g['lengths'], rows, g['label'], len(g['text']), want=g['grouped'])
    for _ in range(2):
        again = [rows[k] for k in rng.permutation(len(rows))]
        got = library(api, g['lengths'], again, g['label'], len(g['text']))
        assert got[0].tobytes() + got[1].tobytes() + got[2].tobytes() == first
    files = []
    for threads in (1, 16):
        paths = [tmp_path / f'{name}{threads}.tsv' for name in ('paint', 'seg', 'donors')]
        api.paint(g['out'] / 'ani.aln.tsv', g['out'] / 'ani.ids.tsv', paths[0], clusters_path=g['out'] / 'clusters.tsv', segments_path=paths[1],
                  donors_path=paths[2], num_threads=threads)
        files.append([p.read_bytes() for p in paths])
    assert files[0] == files[1]


def random_input():
    rng = np.random.default_rng(29)
    n = 200
    lengths = [int(x) for x in rng.integers(1, 3001, n)]
    rows = []
    for _ in range(20000):
        q = int(rng.integers(0, n))
        s = int(rng.integers(0, lengths[q]))
        e = min(lengths[q] - 1, s + int(rng.integers(0, 400)))
        rows.append((q, int(rng.integers(0, n)), s, e, int(rng.integers(0, e - s + 2))))
    return lengths, rows, [int(x) for x in rng.integers(0, 12, n)], 12


def test_random(api):
    """200 objects, lengths 1..3 000, 20 000 rows, labels in 12 groups."""
    check(api, *random_input())


def constructed_inputs():
    """every (lengths, rows, label, n_groups) this file builds by hand or by seed (the golden table apart), for the test that holds
    the two references to each other"""
    out = [level_edges_input()[:2] + (None, None), boundaries_input(), ties_input() + (None, None), nesting_input() + (None, None), hot_object_input(),
           random_input()]
    out += [(lengths, rows, None, None) for lengths, rows in ENDS_INPUTS]
    lengths, rows = groups_input()
    n = len(lengths)
    out += [(lengths, rows, None, None), (lengths, rows, list(range(n)), n), (lengths, rows, GROUPS_LABEL, 3), (lengths, rows, GROUPS_SPARSE_LABEL, 12)]
    return out


# ---------------------------------------------------------------- files and regions
def expected_files(g, clusters):
    import oracle_lib as orc          # (the number format of the alignment table)
    records, segments, donors, _ = g['grouped'] if clusters else g['plain']
    return (pr.summary_text(g['ids'], records, g['label'] if clusters else None, g['text'] if clusters else None),
            pr.segments_text(g['ids'], segments, orc.fmt_num), pr.donors_text(g['ids'], g['lengths'], donors))


@pytest.mark.parametrize('clusters', [False, True])
def test_file_route(api, golden, tmp_path, clusters):
    """The golden example through stages.paint and through the command module: the three files equal the restatement's bytes."""
    g = golden
    want = expected_files(g, clusters)
    aln, ids, cl = g['out'] / 'ani.aln.tsv', g['out'] / 'ani.ids.tsv', g['out'] / 'clusters.tsv'
    paths = [tmp_path / name for name in ('paint.tsv', 'segments.tsv', 'donors.tsv')]
    api.paint(aln, ids, paths[0], clusters_path=cl if clusters else None, column='cluster' if clusters else None, segments_path=paths[1], donors_path=paths[2])
    assert tuple(p.read_text() for p in paths) == want
    paths2 = [tmp_path / name for name in ('paint2.tsv', 'segments2.tsv', 'donors2.tsv')]
    r = subprocess.run([sys.executable, '-m', 'vclust_amd.paint', '-i', str(aln), '--ids', str(ids), '-o', str(paths2[0]), '--out-segments', str(paths2[1]),
                        '--out-donors', str(paths2[2])] + (['--clusters', str(cl)] if clusters else []), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert 'Running: libvclust_gpu paint' in r.stderr and 'Completed' in r.stderr and 'vg_paint_file: 12 objects, 5693 rows' in r.stderr
    assert tuple(p.read_text() for p in paths2) == want
    # without the two optional files: the summary alone
    api.paint(aln, ids, paths[0], clusters_path=cl if clusters else None)
    assert paths[0].read_text() == want[0]


def test_parse_route(api, golden, golden_dir):
    """api.paint_regions on the regions lz_align returns for the golden multi-FASTA equals paint_rows on the rows of the golden table:
    the table holds the same regions as a multiset."""
    g = golden
    gs = api.GenomeSet.load([golden_dir / 'multifasta.fna'], multisample=True)
    names = gs.names()
    assert sorted(names) == sorted(g['ids'])
    tasks = gs.align_tasks(gs.read_filter())            # no filter: every pair, as the golden table was made
    stats, regions = gs.lz_align(tasks, want_regions=True)
    assert len(tasks) == 132 and len(regions) == len(g['rows'])
    got = api.paint_regions(gs, tasks, regions)
    at = {name: i for i, name in enumerate(names)}      # the table's objects in the order of the genome set
    perm = [at[x] for x in g['ids']]
    rows = [(perm[q], perm[r], s, e, m) for q, r, s, e, m in g['rows']]
    lengths = [int(x) for x in gs.lengths()]
    want = library(api, lengths, rows)
    assert got[3] == want[3] and all(got[k].tobytes() == want[k].tobytes() for k in range(3))
    equal(got, pr.paint(lengths, rows))
