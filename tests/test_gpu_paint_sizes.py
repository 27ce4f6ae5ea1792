"""The mosaic painting on the MI355X at the sizes where the constants of vg_paint.hip and vg_scan.h switch their code paths, against
the event sweep (tests/paint_sweep.py; the array restatement cannot hold these inputs, and tests/test_paint_cpu.py holds the sweep to
it where it can).  Everything is an integer and must be equal: every field of every record, every segment, every donor record, every
run count.

Carry chunks.  Each scan of the stage (the flag scan over the sorted breakpoint candidates, the segment-start scan over the
breakpoints, pstat_op over the segments, donor_op over the painted segments in (object, partner) order, top_op over the donor records)
is three launches; the middle one is one workgroup that walks the tile totals 256 tiles at a time and hands a running carry from one
chunk to the next.  Element i of a scan belongs to tile i // 1 024 and chunk i // 262 144: the hand-over exists only in a scan of more
than 262 144 elements.  The input below has 263 200 objects with a row each, so every one of the five scans has a second chunk of
more than one tile, and one hot object placed by the running count of breakpoints so that element 262 144 of the breakpoints lies
well inside a long poor row with 1 500 perfect short rows nested in it.

Key widths.  pos_bits = bit_width(max len) -- a breakpoint at len is legal --, r_bits = bit_width(n - 1) for the partner under the
object in a donor key, bit_width(n) for the object of a breakpoint key (the objects without a position sort behind the last): lengths
up to 2^31 - 1 with a row ending at len - 1, and n at and above 2^16.

Levels.  One row over 2^20 elementary segments: 21 levels, and every one of its positions must receive its priority."""
import numpy as np
import pytest

import paint_restatement as pr
import paint_sweep as sw

pytestmark = pytest.mark.gpu

TILE, CHUNK = 1024, 256 * 1024
N_OBJECTS = 263200
HOT_PIECES = 1500


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


def library(api, lengths, rows, label=None, n_groups=None):
    cols = np.array(rows, dtype=np.int64).reshape(-1, 5).T
    return api.paint_rows(lengths, *cols, label=label, n_groups=n_groups)


def equal(got, want):
    records, segments, donors, run = got
    w_records, w_segments, w_donors, w_run = want
    assert run == w_run
    for f in pr.FIELDS:
        assert records[f].tolist() == [x[f] for x in w_records], f
    assert [tuple(t) for t in segments.tolist()] == w_segments
    assert [tuple(t) for t in donors.tolist()] == w_donors


def check(api, lengths, rows, label=None, n_groups=None):
    want = sw.paint(lengths, rows, label, n_groups)
    equal(library(api, lengths, rows, label, n_groups), want)
    return want


# ---------------------------------------------------------------- carry chunks
def chunk_input():
    """-> (lengths, rows, label, n_groups, hot): the objects are laid down in id order with the running count of breakpoints; the hot
    object takes the place of the background object at which that count comes within half its own breakpoints of element CHUNK"""
    n = N_OBJECTS
    lengths, rows, hot = [], [], None
    n_breaks = 0
    for k in range(n):
        if hot is None and n_breaks >= CHUNK - HOT_PIECES:
            hot = k
            L = 4 * HOT_PIECES + 1
            lengths.append(L)
            rows.append((k, (k + 1) % n, 0, L - 1, L // 2))
            rows += [(k, (k + 2 + j % 7) % n, 4 * j + 1, 4 * j + 2, 2) for j in range(HOT_PIECES)]
            n_breaks += 2 + 2 * HOT_PIECES
            continue
        L = 8 + (k * 11) % 33                                    # 8 .. 40
        lengths.append(L)
        s = (k * 7) % (L - 3)
        e = min(L - 1, s + 2 + k % 9)
        rows.append((k, (k + 1 + k % 5) % n, s, e, (e - s + 1) - k % 3))
        n_breaks += len({0, s, e + 1, L})
    order = np.random.default_rng(32).permutation(len(rows)).tolist()          # (the library sorts: hand the rows over shuffled)
    return lengths, [rows[i] for i in order], [k % 3 for k in range(n)], 3, hot


def test_carry_chunks(api):
    lengths, rows, label, n_groups, hot = chunk_input()
    arrays = {}
    want = sw.paint(lengths, rows, label, n_groups, arrays=arrays)
    records, segments, donors, run = want
    painted_segments = sum(t[3] >= 0 for t in segments)
    for count in (2 * run['rows_kept'] + 2 * len(lengths), run['breakpoints'], run['segments'], painted_segments, run['donor_records']):
        assert count >= CHUNK + TILE                             # every scan enters its second chunk, by more than a tile
    edge = arrays['breakpoints'][CHUNK - TILE:CHUNK + TILE + 1]
    assert {o for o, _ in edge} == {hot}                         # the chunk edge of the breakpoints lies inside the hot object ...
    assert records[hot]['painted'] == lengths[hot] and records[hot]['segments'] == 2 * HOT_PIECES + 1      # ... under its long row
    assert records[hot]['switches'] == 2 * HOT_PIECES and records[hot]['donors'] == 8 and run['levels'] == (2 * HOT_PIECES + 1).bit_length()
    equal(library(api, lengths, rows, label, n_groups), want)


# ---------------------------------------------------------------- key widths
BIG = 2 ** 31 - 1


def test_lengths_up_to_2_31(api):
    """2^31 - 1, 2^30 and 2^30 + 1 beside lengths 1 and 0: rows at position 0, ending at len - 1, and touching in the middle"""
    H = 2 ** 30
    lengths = [BIG, 1, 0, H, H + 1, 1, 0]
    rows = [(0, 1, 0, 0, 1), (0, 1, BIG - 1, BIG - 1, 0), (0, 3, H - 10, H - 1, 9), (0, 3, H, H + 20, 20), (0, 4, 0, BIG - 1, BIG // 2), (0, 5, BIG - 2, BIG - 1, 2),
            (1, 0, 0, 0, 1), (3, 0, 0, H // 2 - 1, H // 2), (3, 0, H // 2, H - 1, H // 2 - 1), (3, 4, H - 1, H - 1, 1), (3, 3, 0, H - 1, H),
            (4, 3, H, H, 1), (4, 0, 0, 0, 0), (4, 1, H - 1, H, 1), (5, 5, 0, 0, 1)]
    want = check(api, lengths, rows)
    records, segments, donors, run = want
    assert records[0]['painted'] == BIG and records[0]['top_partner'] == 4 and records[0]['top_painted'] == BIG - 1 - 10 - 21 - 2
    assert [t for t in segments if t[0] == 0][-1] == (0, BIG - 2, BIG - 1, 5, BIG - 2, BIG - 1, 2) and segments[-1] == (5, 0, 0, -1, -1, -1, 0)
    assert records[3]['painted'] == H and [t[1:4] for t in segments if t[0] == 3] == [(0, H // 2 - 1, 0), (H // 2, H - 2, 0), (H - 1, H - 1, 4)]
    assert records[4]['painted'] == 3 and records[4]['segments'] == 4
    check(api, lengths, rows, [0, 0, 1, 1, 0, 2, 2], 3)
    check(api, lengths[::-1], [(6 - q, 6 - r, s, e, m) for q, r, s, e, m in rows], [0, 0, 1, 1, 0, 2, 2], 4)


def object_count_input(n, long_object):
    """rows of the last object to the first, the last (self rows) and the one before the last, and rows that name the last"""
    lengths = [3 + k % 5 for k in range(n)]
    if long_object:
        lengths[n - 1] = BIG
    L = lengths[n - 1]
    rows = [(n - 1, 0, 0, 1, 1), (n - 1, n - 1, 0, L - 1, L), (n - 1, n - 2, L - 2, L - 1, 2), (n - 1, n - 2, 1, 1, 1), (n - 1, 0, 2, 2, 0), (n - 1, n - 1, 1, 1, 1),
            (0, n - 1, 0, 2, 3), (n - 2, n - 1, 1, lengths[n - 2] - 1, 1), (n - 2, n - 2, 0, 0, 1), (n - 2, 0, 0, 0, 1), (n // 2, n - 1, 2, 2, 1), (0, 1, 1, 1, 1)]
    return lengths, rows


@pytest.mark.parametrize('n', [65536, 65537])
@pytest.mark.parametrize('long_object', [False, True])
def test_object_count_at_2_16(api, n, long_object):
    """n - 1 needs 16 bits at 65 536 objects and 17 at 65 537, n itself 17 at both: the donor key of (n - 1, n - 2) is the largest there
    is, the keys of the objects without a position -- none here -- would sit at object n, and with a length of 2^31 - 1 present a
    breakpoint key is 31 bits of position under 17 bits of object"""
    lengths, rows = object_count_input(n, long_object)
    L = lengths[n - 1]
    want = check(api, lengths, rows, [k % 2 for k in range(n)], 2)
    records, segments, donors, run = want
    assert run['rows_kept'] == len(rows) - 3 and donors[-1][:2] == (n - 1, n - 2) and donors[-2][:2] == (n - 1, 0) and records[n - 1]['donors'] == 2
    assert segments[-1][0] == n - 1 and segments[-1][2:4] == (L - 1, n - 2) and records[0]['top_partner'] == n - 1
    check(api, lengths, rows)


def test_objects_without_a_position_at_2_16(api):
    """lengths of 0 among 65 536 objects, the last among them: their candidate keys carry the object n = 2^16, one bit above n - 1"""
    n = 65536
    lengths = [(3 + k % 5) * (k % 4 != 3) for k in range(n)]
    rows = [(n - 2, n - 1, 0, lengths[n - 2] - 1, 1), (n - 4, n - 2, 1, 2, 2), (0, n - 1, 0, 0, 1)]
    want = check(api, lengths, rows)
    assert lengths[n - 1] == 0 and want[3]['breakpoints'] == 2 * (n - n // 4) + 3 and want[0][n - 1]['segments'] == 0


# ---------------------------------------------------------------- levels
def test_one_row_over_2_20_elementary_segments(api):
    """unit rows with n_match 0 on every even position of an object of 2^20 positions make each position a breakpoint; one row of
    identity 1/2 lies over all of them and must win every position: 21 levels, a single segment"""
    L = 2 ** 20
    lengths = [L, 4, 4]
    rows = [(0, 1, x, x, 0) for x in range(0, L, 2)] + [(0, 2, 0, L - 1, L // 2)]
    arrays = {}
    want = sw.paint(lengths, rows, arrays=arrays)
    assert max(arrays['spans']) == L and want[3]['levels'] == 21 and want[3]['breakpoints'] == L + 1 + 4
    assert want[1][0] == (0, 0, L - 1, 2, 0, L - 1, L // 2) and want[0][0]['segments'] == 1
    equal(library(api, lengths, rows), want)
