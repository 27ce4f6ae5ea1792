"""The coverage map on the MI355X (vg_cover_rows, vg_cover_file, `python -m vclust_amd.cover`) against the
sequential restatement (tests/cover_restatement.py): every field of every record, every segment and every run count is an integer and
must be equal, and the two files must equal the restatement's text byte for byte."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_stats_restatement as cs
import cover_restatement as cv

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
    ids, lengths = cv.read_ids(out / 'ani.ids.tsv')
    rows = cv.read_aln(out / 'ani.aln.tsv', ids, lengths)
    names, label, text = cs.read_clusters(out / 'clusters.tsv', ids)
    plain = cv.cover(lengths, rows)
    grouped = cv.cover(lengths, rows, label[0], len(text[0]))
    return dict(out=out, ids=ids, lengths=lengths, rows=rows, label=label[0], text=text[0], plain=plain, grouped=grouped)


def _library(api, lengths, rows, label=None, n_groups=None):
    q, r, s, e = (np.array([t[k] for t in rows], dtype=np.int64) for k in range(4))
    return api.cover_rows(lengths, q, r, s, e, label=label, n_groups=n_groups)


def _equal(got, want):
    records, segments, run = got
    w_records, w_segments, w_run = want
    assert run == w_run
    for f in cv.FIELDS:
        assert records[f].tolist() == [x[f] for x in w_records], f
    assert [tuple(t) for t in segments.tolist()] == w_segments


def _check(api, lengths, rows, label=None, n_groups=None):
    """the library's records, segments and run counts equal the restatement's; -> the library's raw bytes"""
    got = _library(api, lengths, rows, label, n_groups)
    _equal(got, cv.cover(lengths, rows, label, n_groups))
    return got[0].tobytes() + got[1].tobytes()


def pair_unions_input():
    rows = [(0, 1, 40, 59), (0, 1, 10, 19), (0, 1, 15, 30), (0, 1, 31, 35),      # overlap, then touch: 10..35
            (0, 2, 5, 90), (0, 2, 20, 30), (0, 2, 20, 30), (0, 2, 5, 5),          # nested and repeated
            (0, 3, 70, 79), (0, 3, 60, 69), (0, 3, 80, 80), (0, 3, 0, 0),         # three that touch, unsorted
            (0, 1, 40, 59), (0, 0, 0, 99)]                                        # a repeat, a self row
    return [100, 7, 7, 7], rows


def test_pair_unions(api):
    """One object, three partners: rows that overlap, nest, touch (end + 1 == next start), repeat, and come unsorted."""
    lengths, rows = pair_unions_input()
    _check(api, lengths, rows)
    got = _library(api, lengths, rows)
    # (60 is the end + 1 of partner 1 and the start of partner 3: one breakpoint, and no segment starts there)
    assert got[2] == dict(rows_kept=13, intervals=5, breakpoints=9, segments=8 + 3)
    assert got[0]['sum_in'][0] == 26 + 20 + 86 + 1 + 21


ENDS_INPUT = ([50, 1, 0, 9, 30, 12], [(0, 5, 0, 9), (0, 5, 40, 49), (0, 4, 0, 49), (1, 0, 0, 0), (4, 0, 29, 29), (4, 1, 0, 0), (4, 5, 0, 29)])
ENDS_MORE = [([0, 0, 0], []), ([5], []), ([5, 5], [(0, 0, 0, 4), (1, 1, 2, 3)])]      # no rows; the last: self rows only


def test_ends(api):
    """Position 0, a row that ends at len - 1 (a breakpoint at len), lengths 1 and 0, no rows at all, a partner that is never a query."""
    lengths, rows = ENDS_INPUT
    _check(api, lengths, rows)
    records, segments, run = _library(api, lengths, rows)
    assert [tuple(t) for t in segments.tolist() if t[0] in (1, 3, 5)] == [(1, 0, 0, 1, 0), (3, 0, 8, 0, 0), (5, 0, 11, 0, 0)]
    assert records['segments'].tolist() == [3, 1, 0, 1, 3, 1]
    for more in ENDS_MORE:
        _check(api, *more)


NET_ZERO_INPUT = ([60, 5, 5, 5], [(0, 1, 10, 29), (0, 2, 30, 49)])
NET_ZERO_LABEL = [0, 0, 1, 1]
NET_ZERO_ENDS = [([40, 5, 5], [(0, 1, 0, 19), (0, 2, 20, 39)], [0, 0, 0], 1), ([40, 5, 5], [(0, 1, 0, 19), (0, 2, 20, 39)], [0, 0, 1], 2)]


def test_net_zero_breakpoints(api):
    """Partner A ends at x and partner B starts at x + 1: one segment inside one channel, two across the channels (same total depth)."""
    lengths, rows = NET_ZERO_INPUT
    _check(api, lengths, rows)
    records, segments, run = _library(api, lengths, rows)
    assert [tuple(t) for t in segments.tolist() if t[0] == 0] == [(0, 0, 9, 0, 0), (0, 10, 49, 1, 0), (0, 50, 59, 0, 0)] and run['breakpoints'] == 3
    label = NET_ZERO_LABEL
    _check(api, lengths, rows, label, 2)
    records, segments, run = _library(api, lengths, rows, label, 2)
    assert [tuple(t) for t in segments.tolist() if t[0] == 0] == [(0, 0, 9, 0, 0), (0, 10, 29, 1, 0), (0, 30, 49, 0, 1), (0, 50, 59, 0, 0)]
    assert records['max_depth'][0] == 1
    # the same at the two ends of the object
    for case in NET_ZERO_ENDS:
        _check(api, *case)


TILE_OBJECTS = 307


def tile_edges_input():
    m = TILE_OBJECTS
    rng = np.random.default_rng(5)
    lengths = [int(x) for x in rng.integers(6, 20, m + 1)]
    rows = []
    for k in range(1, m + 1):
        partners = [p for p in rng.permutation(m + 1).tolist() if p != k][:k]
        for p in partners:
            s = int(rng.integers(0, lengths[k]))
            rows.append((k, p, s, int(rng.integers(s, lengths[k]))))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return lengths, rows, [int(x) for x in rng.integers(0, 3, m + 1)], 3


def test_tile_edges(api):
    """Object k (k = 1..m) has exactly k rows from k distinct partners, so that its first sorted row sits at offset k (k - 1) / 2 and
    the object boundary falls at every offset of a tile, in the rows, the events (two per row) and the segments.  The workgroup
    chunks: 1 024 elements (256 threads x 4) in every scan of vg_cover.hip; the rocPRIM calls (radix sorts, reduce_by_key) use the
    tuned configurations of the library, at most 1 024 x 23 = 23 552 elements per workgroup for the key-aware one (reduce_by_key).
    m = 307: 47 278 rows and 94 556 events, four times that chunk."""
    m = TILE_OBJECTS
    assert 2 * (m * (m + 1) // 2) >= 4 * 23552 and m * (m + 1) // 2 >= 4 * 1024
    _check(api, *tile_edges_input())


def hot_object_input():
    rng = np.random.default_rng(6)
    n = 2301
    lengths = [40000] + [int(x) for x in rng.integers(1, 50, n - 1)]
    rows = []
    for _ in range(5000):
        s = int(rng.integers(0, 40000))
        rows.append((0, int(rng.integers(1, 301)), s, min(39999, s + int(rng.integers(0, 400)))))
    for k in range(301, n):
        s = int(rng.integers(0, lengths[k]))
        rows.append((k, int(rng.integers(0, n)), s, int(rng.integers(s, lengths[k]))))
    return lengths, rows, [int(x) for x in rng.integers(0, 4, n)], 4


def test_hot_object(api):
    """One object with 5 000 rows from 300 partners (several workgroups of rows, events and segments in one object) beside 2 000
    objects with one row each."""
    lengths, rows, label, _ = hot_object_input()
    _check(api, lengths, rows, label, 4)
    records, segments, run = _library(api, lengths, rows, label, 4)
    assert records['segments'][0] > 4 * 1024 and records['partners_in'][0] + records['partners_out'][0] == 300


GROUPS_FULL_LABEL, GROUPS_SPARSE_LABEL = [0, 1, 0, 2, 1, 2, 1, 0, 2], [5, 1, 5, 7, 1, 7, 1, 5, 7]


def groups_full(lengths, rows):
    return rows + [(q, r, 0, lengths[q] - 1) for q in (1, 4, 6) for r in (1, 4, 6)]


def groups_input():
    rng = np.random.default_rng(7)
    n = 9
    lengths = [int(x) for x in rng.integers(20, 60, n)]
    rows = []
    for q in range(n):
        for r in range(n):
            for _ in range(2):
                s = int(rng.integers(0, lengths[q]))
                rows.append((q, r, s, int(rng.integers(s, lengths[q]))))
    return lengths, rows


def test_groups(api):
    lengths, rows = groups_input()
    n = len(lengths)
    plain = _check(api, lengths, rows)                                     # no labels
    assert plain == _check(api, lengths, rows, [0] * n, 1)
    records = _library(api, lengths, rows, list(range(n)), n)[0]           # every object its own group
    _check(api, lengths, rows, list(range(n)), n)
    assert not records['core'].any() and not records['sum_in'].any() and not records['partners_in'].any()
    # a group in which every other member covers everything: core == len
    full, label = groups_full(lengths, rows), GROUPS_FULL_LABEL
    _check(api, lengths, full, label, 3)
    records = _library(api, lengths, full, label, 3)[0]
    assert all(records['core'][q] == lengths[q] for q in (1, 4, 6))
    # more groups than labels used
    _check(api, lengths, rows, GROUPS_SPARSE_LABEL, 12)


def test_order_and_threads(api, golden, tmp_path):
    rng = np.random.default_rng(8)
    g = golden
    rows = g['rows']
    first = _check(api, g['lengths'], rows[:1500], g['label'], len(g['text']))
    for _ in range(2):
        again = [rows[k] for k in rng.permutation(1500)]
        got = _library(api, g['lengths'], again, g['label'], len(g['text']))
        assert got[0].tobytes() + got[1].tobytes() == first
    files = []
    for threads in (1, 16):
        out, seg = tmp_path / f'cover{threads}.tsv', tmp_path / f'seg{threads}.tsv'
        api.cover(g['out'] / 'ani.aln.tsv', g['out'] / 'ani.ids.tsv', out, clusters_path=g['out'] / 'clusters.tsv', segments_path=seg,
                  num_threads=threads)
        files.append((out.read_bytes(), seg.read_bytes()))
    assert files[0] == files[1]


def random_input():
    rng = np.random.default_rng(9)
    n = 200
    lengths = [int(x) for x in rng.integers(1, 3001, n)]
    rows = []
    for _ in range(20000):
        q = int(rng.integers(0, n))
        s = int(rng.integers(0, lengths[q]))
        rows.append((q, int(rng.integers(0, n)), s, min(lengths[q] - 1, s + int(rng.integers(0, 200)))))
    return lengths, rows, [int(x) for x in rng.integers(0, 12, n)], 12


def test_random(api):
    """200 objects, lengths 1..3 000, 20 000 rows, labels in 12 groups."""
    _check(api, *random_input())


def constructed_inputs():
    """every (lengths, rows, label, n_groups) this file builds by hand or by seed (the golden table apart), for the tests that hold
    the two references to each other"""
    out = [pair_unions_input() + (None, None), ENDS_INPUT + (None, None)] + [m + (None, None) for m in ENDS_MORE]
    out += [NET_ZERO_INPUT + (None, None), NET_ZERO_INPUT + (NET_ZERO_LABEL, 2)] + NET_ZERO_ENDS
    out += [tile_edges_input(), hot_object_input(), random_input()]
    lengths, rows = groups_input()
    n = len(lengths)
    out += [(lengths, rows, None, None), (lengths, rows, [0] * n, 1), (lengths, rows, list(range(n)), n),
            (lengths, groups_full(lengths, rows), GROUPS_FULL_LABEL, 3), (lengths, rows, GROUPS_SPARSE_LABEL, 12)]
    return out


def _expected_files(g, clusters):
    records, segments, _ = g['grouped'] if clusters else g['plain']
    return (cv.summary_text(g['ids'], records, g['label'] if clusters else None, g['text'] if clusters else None),
            cv.segments_text(g['ids'], segments))


@pytest.mark.parametrize('clusters', [False, True])
def test_file_route(api, golden, tmp_path, clusters):
    """The golden example through stages.cover and through the command module: both files equal the restatement's bytes."""
    g = golden
    want = _expected_files(g, clusters)
    aln, ids, cl = g['out'] / 'ani.aln.tsv', g['out'] / 'ani.ids.tsv', g['out'] / 'clusters.tsv'
    out, seg = tmp_path / 'cover.tsv', tmp_path / 'segments.tsv'
    api.cover(aln, ids, out, clusters_path=cl if clusters else None, column='cluster' if clusters else None, segments_path=seg)
    assert (out.read_text(), seg.read_text()) == want
    out2, seg2 = tmp_path / 'cover2.tsv', tmp_path / 'segments2.tsv'
    r = subprocess.run([sys.executable, '-m', 'vclust_amd.cover', '-i', str(aln), '--ids', str(ids), '-o', str(out2), '--out-segments', str(seg2)] +
                       (['--clusters', str(cl)] if clusters else []), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert 'Running: libvclust_gpu cover' in r.stderr and 'Completed' in r.stderr and 'vg_cover_file: 12 objects, 5693 rows' in r.stderr
    assert (out2.read_text(), seg2.read_text()) == want
    # without the profile: the summary alone
    api.cover(aln, ids, out, clusters_path=cl if clusters else None)
    assert out.read_text() == want[0]


def test_parse_route(api, golden, golden_dir):
    """api.cover_regions on the regions lz_align returns for the golden multi-FASTA equals cover_rows on the rows of the golden table:
    the table holds the same regions as a multiset."""
    g = golden
    gs = api.GenomeSet.load([golden_dir / 'multifasta.fna'], multisample=True)
    names = gs.names()
    assert sorted(names) == sorted(g['ids'])
    tasks = gs.align_tasks(gs.read_filter())            # no filter: every pair, as the golden table was made
    assert len(tasks) == 132
    stats, regions = gs.lz_align(tasks, want_regions=True)
    assert len(regions) == len(g['rows'])
    got = api.cover_regions(gs, tasks, regions)
    # the table's objects in the order of the genome set
    at = {name: i for i, name in enumerate(names)}
    perm = [at[x] for x in g['ids']]
    rows = [(perm[q], perm[r], s, e) for q, r, s, e in g['rows']]
    lengths = [int(x) for x in gs.lengths()]
    assert [lengths[perm[i]] for i in range(len(perm))] == g['lengths']
    want = _library(api, lengths, rows)
    assert got[2] == want[2]
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    _equal(got, cv.cover(lengths, rows))
