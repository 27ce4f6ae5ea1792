"""The coverage map on the MI355X at the sizes where the constants of vg_cover.hip switch its code paths, against the event sweep
(tests/cover_sweep.py; the mask restatement cannot hold these inputs, and tests/test_cover_sweep_cpu.py holds the sweep to it where
it can).  Everything is an integer and must be equal: every field of every record, every segment, every run count.

Carry chunks.  Each of the five scans of the stage (seg_max_op and merge_op over the kept rows in (q, r, qstart) order, depth_op
over the breakpoints, plus_op over the objects, stat_op over the segments) is three launches; the middle one, k_carry_scan, is one
workgroup that walks the tile totals 256 tiles at a time and hands a running carry from one chunk to the next.  Element index i of
a scan belongs to tile i // 1 024 and chunk i // 262 144: a second chunk, and with it the hand-over, exists only in a scan of more
than 262 144 elements.  The two inputs below have 263 200 objects, so that every scan has a second chunk of more than one tile;
every test proves that from the sweep's counts before it calls the library.
  uniform      one row per object: around element 262 144 every element of every scan carries a head (a new (q, r) run, a new
               object), so what must cross the edge is the plain sums only
  straddlers   the same background and three hot objects, placed by the prefix counts so that element 262 144 of the sorted rows,
               of the breakpoints and of the segments lies at least 1 024 elements inside one run: (a) a (q, r) run of 4 096 rows
               whose first row spans the object and whose later rows are disjoint and nested in it -- without the running maximum
               carried over, each of them would open an interval; (b) an object with 3 000 breakpoints from 1 500 nested rows of
               1 500 partners -- the edge falls near the peak of the depth, 1 500; (c) an object of 4 201 segments, whose record is
               the stat_op carried to its last segment.
Measured on one CPU core: building an input 0.3 s, the sweep 2.8 s on the uniform and 3.1 s on the straddlers input (the mask
restatement: 9.5 s for as many rows).

Key widths.  pos_bits = bit_width(max len) -- a breakpoint at len is legal --, r_bits = bit_width(n - 1), q_bits = bit_width(n),
the self key n << r_bits: lengths at powers of two with a row ending at len - 1, lengths up to 2^31 - 1, n at and above 2^16."""
import numpy as np
import pytest

import cover_restatement as cv
import cover_sweep as sw

pytestmark = pytest.mark.gpu

TILE, CHUNK = 1024, 256 * 1024
N_OBJECTS = 263200
HOT_ROWS, HOT_PARTNERS, HOT_PIECES = 4096, 1500, 2100


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


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
    want = sw.cover(lengths, rows, label, n_groups)
    _equal(_library(api, lengths, rows, label, n_groups), want)
    return want


# ---------------------------------------------------------------- carry chunks
def background_row(k, n, length):
    """the one row of background object k: to a partner a few ids away, somewhere inside the object"""
    s = (k * 7) % (length - 3)
    return (k, (k + 1 + k % 5) % n, s, min(length - 1, s + 2 + k % 9))


def chunk_input(straddlers):
    """-> (lengths, rows, label, n_groups, hot): hot = the ids of the objects (a), (b), (c), empty for the uniform input.  The
    objects are laid down in id order with the running counts of rows, breakpoints (two per row here: no two coincide inside a hot
    object, and a background object has one row) and segments; a hot object takes the place of the background object at which its
    array's count comes within half its own size of element CHUNK."""
    n = N_OBJECTS
    lengths, rows, hot = [], [], {}
    n_rows = n_breaks = n_segs = 0
    for k in range(n):
        if straddlers and 'c' not in hot and n_segs >= CHUNK - HOT_PIECES:
            # (c) HOT_PIECES disjoint rows of one partner that do not touch: 2 * HOT_PIECES + 1 segments
            hot['c'] = k
            lengths.append(4 * HOT_PIECES + 1)
            mine = [(k, (k + 1) % n, 4 * j + 1, 4 * j + 2) for j in range(HOT_PIECES)]
        elif straddlers and 'b' not in hot and n_breaks >= CHUNK - HOT_PARTNERS:
            # (b) row j of partner k + 1 + j covers j .. len - 1 - j: 2 * HOT_PARTNERS breakpoints, the depth rises to HOT_PARTNERS
            hot['b'] = k
            lengths.append(2 * HOT_PARTNERS + 40)
            mine = [(k, (k + 1 + j) % n, j, lengths[k] - 1 - j) for j in range(HOT_PARTNERS)]
        elif straddlers and 'a' not in hot and n_rows >= CHUNK - HOT_ROWS // 2:
            # (a) one run: the row that spans the object sorts first (qstart 0), the others lie inside it, apart from each other
            hot['a'] = k
            lengths.append(8 * HOT_ROWS)
            mine = [(k, (k + 3) % n, 0, lengths[k] - 1)] + [(k, (k + 3) % n, 8 * j, 8 * j + 3) for j in range(1, HOT_ROWS)]
        else:
            lengths.append(8 + (k * 11) % 33)                    # 8 .. 40
            mine = [background_row(k, n, lengths[k])]
        rows += mine
        n_rows += len(mine)
        if len(mine) == 1:
            _, _, s, e = mine[0]
            n_breaks += 2
            n_segs += (s > 0) + 1 + (e < lengths[k] - 1)
        elif k == hot.get('c'):
            n_breaks, n_segs = n_breaks + 2 * HOT_PIECES, n_segs + 2 * HOT_PIECES + 1
        elif k == hot.get('b'):
            n_breaks, n_segs = n_breaks + 2 * HOT_PARTNERS, n_segs + 2 * HOT_PARTNERS - 1
        else:
            n_breaks, n_segs = n_breaks + 2, n_segs + 1
    order = np.random.default_rng(12).permutation(len(rows)).tolist()          # (the library sorts: hand the rows over shuffled)
    return lengths, [rows[i] for i in order], [k % 3 for k in range(n)], 3, hot


@pytest.fixture(scope='module')
def uniform():
    lengths, rows, label, n_groups, _ = chunk_input(False)
    return lengths, rows, label, n_groups, sw.cover(lengths, rows, label, n_groups)


@pytest.fixture(scope='module')
def straddlers():
    lengths, rows, label, n_groups, hot = chunk_input(True)
    arrays = {}
    return lengths, rows, label, n_groups, hot, sw.cover(lengths, rows, label, n_groups, arrays=arrays), arrays


def _every_scan_has_a_second_chunk(n_objects, run):
    for count in (n_objects, run['rows_kept'], run['breakpoints'], run['segments']):
        assert count >= CHUNK + TILE


def test_carry_chunks_uniform(api, uniform):
    """All five scans enter their second chunk, with a head on every element around the edge."""
    lengths, rows, label, n_groups, want = uniform
    assert 8 <= min(lengths) and max(lengths) <= 40 and set(label) == {0, 1, 2}
    _every_scan_has_a_second_chunk(len(lengths), want[2])
    assert want[2]['intervals'] == want[2]['rows_kept'] == len(lengths) and all(rec['segments'] <= 3 for rec in want[0])
    _equal(_library(api, lengths, rows, label, n_groups), want)


def test_carry_chunks_straddlers(api, straddlers):
    """Element 262 144 of the sorted rows, of the breakpoints and of the segments lies inside a run that began at least a tile
    earlier and goes on for at least a tile: the carry that crosses the chunk edge is a running maximum without a head (a), a
    depth of hundreds (b), and the half-summed record of an object (c)."""
    lengths, rows, label, n_groups, hot, want, arrays = straddlers
    records, segments, run = want
    _every_scan_has_a_second_chunk(len(lengths), run)
    a, b, c = hot['a'], hot['b'], hot['c']
    edge = slice(CHUNK - TILE, CHUNK + TILE + 1)
    assert set(arrays['rows'][edge]) == {(a, (a + 3) % len(lengths))}                      # one (q, r) run ...
    assert records[a]['partners_in'] + records[a]['partners_out'] == 1 and records[a]['covered'] == lengths[a]
    assert records[a]['segments'] == 1                                                      # ... that is one interval
    assert {o for o, _ in arrays['breakpoints'][edge]} == {b}
    assert min(x + y for x, y in arrays['depths'][edge]) >= 2 and records[b]['max_depth'] == HOT_PARTNERS
    assert {t[0] for t in segments[edge]} == {c} and records[c]['segments'] >= 4096
    assert records[c]['covered'] == 2 * HOT_PIECES
    _equal(_library(api, lengths, rows, label, n_groups), want)


# ---------------------------------------------------------------- key widths
def power_of_two_cases(P):
    """max len exactly P with a row that ends at len - 1 (a breakpoint at P, which needs the bit P itself needs): in the middle, on
    the object of the highest id, and beside a longer object, where the longest length is not this object's"""
    return [([7, P, 12], [(1, 0, P - 5, P - 1), (1, 2, 0, P - 1), (1, 0, 3, 9), (0, 1, 0, 6), (2, 1, 11, 11)]),
            ([7, 12, P], [(2, 0, P - 5, P - 1), (2, 1, 0, P - 1), (2, 0, 3, 9), (2, 2, 0, 5), (0, 2, 6, 6), (1, 2, 0, 11)]),
            ([2 * P + 3, 9, P], [(2, 0, P - 5, P - 1), (2, 1, P - 1, P - 1), (2, 1, 0, 0), (0, 2, 2 * P + 2, 2 * P + 2), (0, 1, P - 1, P), (1, 0, 8, 8)])]


@pytest.mark.parametrize('P', [1024, 2 ** 20])
def test_longest_length_a_power_of_two(api, P):
    for lengths, rows in power_of_two_cases(P):
        want = _check(api, lengths, rows)
        last = [t for t in want[1] if t[0] == lengths.index(P)][-1]
        assert max(lengths) in (P, 2 * P + 3) and last[2] == P - 1 and last[3] >= 1        # covered up to len - 1: a breakpoint at P
        _check(api, lengths, rows, [0, 1, 0], 2)


BIG = 2 ** 31 - 1


def test_lengths_up_to_2_31(api):
    """2^31 - 1, 2^30 and 2^30 + 1 beside lengths 1 and 0: rows at position 0, at len - 1, and touching in the middle"""
    H = 2 ** 30
    lengths = [BIG, 1, 0, H, H + 1, 1, 0]
    rows = [(0, 1, 0, 0), (0, 1, BIG - 1, BIG - 1), (0, 3, H - 10, H - 1), (0, 3, H, H + 20), (0, 4, 0, BIG - 1), (0, 5, BIG - 2, BIG - 1),
            (1, 0, 0, 0), (3, 0, 0, H // 2 - 1), (3, 0, H // 2, H - 1), (3, 4, H - 1, H - 1), (3, 3, 0, H - 1),
            (4, 3, H, H), (4, 0, 0, 0), (4, 1, H - 1, H), (5, 5, 0, 0)]
    want = _check(api, lengths, rows)
    records, segments, run = want
    assert records[0]['covered'] == BIG and records[0]['sum_in'] == BIG + 1 + 1 + 31 + 2 and records[0]['max_depth'] == 3
    assert records[3]['covered'] == H and run['intervals'] == len(rows) - 2 - 2 and segments[-1] == (5, 0, 0, 0, 0)
    assert records[4]['covered'] == 3 and [t for t in segments if t[0] == 0][-1] == (0, BIG - 1, BIG - 1, 3, 0)
    _check(api, lengths, rows, [0, 0, 1, 1, 0, 2, 2], 3)
    _check(api, lengths[::-1], [(6 - q, 6 - r, s, e) for q, r, s, e in rows], [0, 0, 1, 1, 0, 2, 2], 4)


def object_count_input(n, long_object):
    """rows of the last object to the first, the last (self rows) and the one before the last, and rows that name the last"""
    lengths = [3 + k % 5 for k in range(n)]
    if long_object:
        lengths[n - 1] = BIG
    L = lengths[n - 1]
    rows = [(n - 1, 0, 0, 1), (n - 1, n - 1, 0, L - 1), (n - 1, n - 2, L - 2, L - 1), (n - 1, n - 2, 1, 1), (n - 1, 0, 2, 2), (n - 1, n - 1, 1, 1),
            (0, n - 1, 0, 2), (n - 2, n - 1, 1, lengths[n - 2] - 1), (n - 2, n - 2, 0, 0), (n - 2, 0, 0, 0), (n // 2, n - 1, 2, 2), (0, 1, 1, 1)]
    return lengths, rows


@pytest.mark.parametrize('n', [65536, 65537])
@pytest.mark.parametrize('long_object', [False, True])
def test_object_count_at_2_16(api, n, long_object):
    """n - 1 needs 16 bits at 65 536 objects and 17 at 65 537, n itself 17 at both; the self key n << r_bits must stay above every
    (q, r) key, and with a length of 2^31 - 1 present the event key is 31 bits of position under 16 or 17 bits of object"""
    lengths, rows = object_count_input(n, long_object)
    L = lengths[n - 1]
    want = _check(api, lengths, rows, [k % 2 for k in range(n)], 2)
    assert want[2]['rows_kept'] == len(rows) - 3 and want[0][n - 1]['partners_in'] + want[0][n - 1]['partners_out'] == 2
    assert want[0][n - 1]['covered'] == min(L, 5) and want[1][-1][0] == n - 1 and want[1][-1][2] == L - 1 and want[1][-1][4] >= 1
    _check(api, lengths, rows)
