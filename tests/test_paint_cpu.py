"""The mosaic painting without a device: the event sweep (tests/paint_sweep.py) held equal to the sequential
restatement (tests/paint_restatement.py) on small random inputs, on every input tests/test_gpu_paint.py builds and on the golden
example; the invariants of the definition; the golden figures pinned as numbers; and the interface -- every argument error of
vg_paint_rows, vg_paint_file and `python -m vclust_amd.paint` is raised on the host, before any device use, and a valid call
without a device is VG_ENODEV."""
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import cover_restatement as cv
import oracle_lib as orc
import paint_restatement as pr
import paint_sweep as sw
import test_gpu_paint as gpu_inputs
from vclust_amd import _lib, api, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent


def small_case(rng):
    """a few objects of lengths 0..40 (0 and 1 among them) and rows drawn so that touching, nested and repeated rows, self rows, equal
    identities broken by span, by partner and by qstart, and n_match of 0 and of span all occur often"""
    n = int(rng.integers(1, 6))
    lengths = [int(rng.choice([0, 1, 2, int(rng.integers(3, 41))], p=[0.1, 0.15, 0.1, 0.65])) for _ in range(n)]
    live = [i for i in range(n) if lengths[i] > 0]
    rows = []
    for _ in range(int(rng.integers(0, 25)) if live else 0):
        how = int(rng.integers(0, 6))
        q = int(rng.choice(live))
        L = lengths[q]
        mine = [t for t in rows if t[0] == q]
        if how == 0 and mine:                            # the same row again
            rows.append(mine[int(rng.integers(0, len(mine)))])
            continue
        if how == 1 and mine:                            # same range and identity, another partner; or shifted by one: same I and span
            _, r, s, e, m = mine[int(rng.integers(0, len(mine)))]
            d = int(rng.integers(0, 2))
            if e + d < L:
                rows.append((q, int(rng.integers(0, n)) if d == 0 else r, s + d, e + d, m))
                continue
        if how == 2 and mine:                            # touches an earlier row on its right, or nests in it
            _, r, s, e, m = mine[int(rng.integers(0, len(mine)))]
            if e + 1 < L and rng.integers(0, 2):
                s2, e2 = e + 1, int(rng.integers(e + 1, L))
            else:
                s2 = int(rng.integers(s, e + 1))
                e2 = int(rng.integers(s2, e + 1))
            rows.append((q, int(rng.integers(0, n)), s2, e2, int(rng.integers(0, e2 - s2 + 2))))
            continue
        s = int(rng.integers(0, L))
        e = int(rng.integers(s, L))
        span = e - s + 1
        m = [0, span, span // 2, int(rng.integers(0, span + 1))][int(rng.integers(0, 4))]       # (span // 2 of an even span: I equal across spans)
        rows.append((q, q if how == 3 and rng.integers(0, 2) else int(rng.integers(0, n)), s, e, m))
    groups = int(rng.integers(0, 4))
    label = [int(x) for x in rng.integers(0, groups, n)] if groups else None
    return lengths, rows, label, groups or None


def tiles(lengths, segments):
    by_object = [[t for t in segments if t[0] == i] for i in range(len(lengths))]
    for i, segs in enumerate(by_object):
        assert [t[1] for t in segs] == [0][:len(segs)] + [t[2] + 1 for t in segs[:-1]]
        assert (segs[-1][2] == lengths[i] - 1) if lengths[i] else not segs
        assert all(a[3:] != b[3:] for a, b in zip(segs, segs[1:]))                      # neighbours differ: the runs are maximal
    return by_object


def invariants(lengths, rows, label, n_groups, got):
    records, segments, donors, run = got
    assert segments == sorted(segments, key=lambda t: t[:2]) and donors == sorted(donors, key=lambda t: t[:2])
    assert run['segments'] == len(segments) and run['donor_records'] == len(donors) and run['rows_kept'] == sum(t[0] != t[1] for t in rows)
    tiles(lengths, segments)
    # painted is the coverage map's `covered` on the same rows
    covered = cv.cover(lengths, [t[:4] for t in rows], label, n_groups)[0]
    assert [rec['painted'] for rec in records] == [rec['covered'] for rec in covered]
    for i, rec in enumerate(records):
        mine = [d for d in donors if d[0] == i]
        assert sum(d[2] for d in mine) == rec['painted'] == rec['painted_in'] + rec['painted_out'] and len(mine) == rec['donors']
        assert sum(d[3] for d in mine) == sum(t[0] == i and t[3] >= 0 for t in segments) and rec['switches'] <= max(0, rec['segments'] - 1)
        assert (rec['top_partner'], rec['top_painted']) == (min(mine, key=lambda d: (-d[2], d[1]))[1:3] if mine else (-1, 0))
    # every painted segment lies inside its row, and the row is one of the input's
    given = set(rows)
    assert all((o, r, s, e, m) in given and s <= a <= b <= e for o, a, b, r, s, e, m in segments if r >= 0)


def test_sweep_equals_restatement_on_small_random_inputs():
    rng = np.random.default_rng(2024)
    seen = dict(zero=0, one=0, self_rows=0, repeats=0, touching=0, nested=0, full=0, none=0, tie_span=0, tie_partner=0, tie_qstart=0)
    for _ in range(400):
        lengths, rows, label, n_groups = small_case(rng)
        want = pr.paint(lengths, rows, label, n_groups)
        assert sw.paint(lengths, rows, label, n_groups) == want
        invariants(lengths, rows, label, n_groups, want)
        # shuffling the rows changes nothing
        again = [rows[k] for k in rng.permutation(len(rows))]
        assert pr.paint(lengths, again, label, n_groups) == want and sw.paint(lengths, again, label, n_groups) == want
        seen['zero'] += 0 in lengths
        seen['one'] += 1 in lengths
        seen['self_rows'] += any(t[0] == t[1] for t in rows)
        seen['repeats'] += len(set(rows)) < len(rows)
        seen['full'] += any(t[4] == t[3] - t[2] + 1 for t in rows)
        seen['none'] += any(t[4] == 0 for t in rows)
        key = lambda t: (t[4] * 2 ** 32 // (t[3] - t[2] + 1), t[3] - t[2] + 1)
        for a in rows:
            for b in rows:
                if a[0] == b[0] and a != b and a[0] != a[1] and b[0] != b[1]:
                    seen['touching'] += a[3] + 1 == b[2]
                    seen['nested'] += a[2] < b[2] and b[3] < a[3]
                    overlap = a[2] <= b[3] and b[2] <= a[3]
                    seen['tie_span'] += overlap and key(a)[0] == key(b)[0] and key(a)[1] != key(b)[1]
                    seen['tie_partner'] += overlap and key(a) == key(b) and a[1] != b[1]
                    seen['tie_qstart'] += overlap and key(a) == key(b) and a[1] == b[1] and a[2] != b[2]
    assert all(v >= 20 for v in seen.values()), seen


DEVICE_INPUTS = gpu_inputs.constructed_inputs()


@pytest.mark.parametrize('k', range(len(DEVICE_INPUTS)))
def test_sweep_equals_restatement_on_the_device_tests_inputs(k):
    lengths, rows, label, n_groups = DEVICE_INPUTS[k]
    want = pr.paint(lengths, rows, label, n_groups)
    assert sw.paint(lengths, rows, label, n_groups) == want
    tiles(lengths, want[1])


# ---------------------------------------------------------------- the golden example
@pytest.fixture(scope='module')
def golden(golden_dir):
    out = golden_dir / 'output'
    ids, lengths = pr.read_ids(out / 'ani.ids.tsv')
    rows = pr.read_aln(out / 'ani.aln.tsv', ids, lengths)
    return ids, lengths, rows, out, pr.paint(lengths, rows)


def test_golden_example(golden):
    ids, lengths, rows, out, want = golden
    assert len(ids) == 12 and len(rows) == 5693
    assert sw.paint(lengths, rows) == want
    invariants(lengths, rows, None, None, want)
    rng = np.random.default_rng(3)
    assert pr.paint(lengths, [rows[k] for k in rng.permutation(len(rows))]) == want
    by_id = dict(zip(ids, want[0]))
    a = by_id['NC_025457.alt2']
    assert (a['segments'], a['painted'], a['donors'], ids[a['top_partner']], a['top_painted'], a['switches']) == (560, 49330, 9, 'NC_025457', 36364, 168)
    b = by_id['NC_002486']
    assert (b['segments'], b['painted'], b['donors'], ids[b['top_partner']], b['switches']) == (3, 45636, 1, 'NC_002486.alt', 0)
    c = by_id['NC_005091']
    assert (c['segments'], c['donors'], c['switches']) == (136, 2, 95)


def test_golden_segments_show_the_digits_of_their_rows(golden):
    """pident of the alignment table is 100 * nt_match / alnlen in the table's number format on every row, so a painted segment,
    printed by the same expression, shows the digits of its row"""
    ids, lengths, rows, out, want = golden
    head = open(out / 'ani.aln.tsv').readline().rstrip('\n').split('\t')
    c_match, c_len, c_pident = (head.index(x) for x in ('nt_match', 'alnlen', 'pident'))
    for ln in open(out / 'ani.aln.tsv').read().split('\n')[1:]:
        if ln:
            f = ln.split('\t')
            assert orc.fmt_num(100.0 * int(f[c_match]) / int(f[c_len])) == f[c_pident]
    text = pr.segments_text(ids, want[1], orc.fmt_num).split('\n')
    assert text[0].split('\t') == list(pr.SEGMENTS_HEADER) and len(text) == len(want[1]) + 2
    assert all(len(ln.split('\t')) == 7 for ln in text[:-1])


# ---------------------------------------------------------------- the interface, without a device
def test_symbols_and_record_types():
    lib = _lib.load()
    for name in ('vg_paint_rows', 'vg_paint_file'):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert api.PAINT_STAT_DTYPE.names == pr.FIELDS and api.PAINT_STAT_DTYPE.itemsize == 72
    assert api.PAINT_SEGMENT_DTYPE.names == pr.SEGMENT_FIELDS and api.PAINT_SEGMENT_DTYPE.itemsize == 28
    assert api.PAINT_DONOR_DTYPE.names == pr.DONOR_FIELDS and api.PAINT_DONOR_DTYPE.itemsize == 24
    assert tuple(n for n, _ in _lib.PaintRunStats._fields_) == pr.RUN_FIELDS


ROW_ERRORS = [
    # lengths, q, r, qstart, qend, n_match, keywords, code, message
    ([10, 10], [0, 2], [1, 0], [0, 0], [1, 1], [1, 1], {}, -1, 'vg_paint_rows: row 1: index 2 outside 0..1'),
    ([10, 10], [0], [7], [0], [1], [1], {}, -1, 'vg_paint_rows: row 0: index 7 outside 0..1'),
    ([10, 10], [0, 1], [1, 0], [0, -1], [1, 1], [1, 1], {}, -1, 'vg_paint_rows: row 1: qstart -1 is negative'),
    ([10, 10], [0], [1], [5], [4], [0], {}, -1, 'vg_paint_rows: row 0: qstart 5 > qend 4'),
    ([10, 4], [0, 1], [1, 0], [0, 0], [9, 4], [1, 1], {}, -1, 'vg_paint_rows: row 1: qend 4 >= len[1] = 4'),
    ([10, 0], [1], [0], [0], [0], [0], {}, -1, 'vg_paint_rows: row 0: qend 0 >= len[1] = 0'),
    ([10, 10], [0, 1], [1, 0], [0, 2], [1, 5], [2, 5], {}, -1, 'vg_paint_rows: row 1: n_match 5 > span 4'),
    ([10, 10], [0, 1], [1, 1], [0, 2], [1, 5], [-1, 9], {}, -1, 'vg_paint_rows: row 0: n_match -1 is negative'),
    ([10, -3], [], [], [], [], [], {}, -1, 'vg_paint_rows: len[1] = -3 is negative'),
    ([2 ** 31, 5], [], [], [], [], [], {}, -1, 'vg_paint_rows: len[0] = 2147483648 is 2^31 or more'),
    ([10, 10], [0], [1], [0], [1], [1], dict(label=[0, 2], n_groups=2), -1, 'vg_paint_rows: label[1] = 2 outside 0..1'),
    ([10, 10], [0], [1], [0], [1], [1], dict(label=[-1, 0], n_groups=2), -1, 'vg_paint_rows: label[0] = -1 outside 0..1'),
]


@pytest.mark.parametrize('lengths,q,r,qs,qe,nm,kw,code,message', ROW_ERRORS)
def test_paint_rows_argument_errors(lengths, q, r, qs, qe, nm, kw, code, message):
    with pytest.raises(_lib.VclustGpuError) as e:
        api.paint_rows(lengths, q, r, qs, qe, nm, **kw)
    assert e.value.code == code and message in str(e.value)
    # (the restatement refuses the same input)
    with pytest.raises(ValueError):
        pr.paint(lengths, list(zip(q, r, qs, qe, nm)), kw.get('label'), kw.get('n_groups'))


def test_paint_rows_counts_and_pointers():
    lib, C = _lib.load(), _lib.C
    out = (_lib.PaintStat * 1)()
    n_seg, n_don = C.c_int64(), C.c_int64()
    seg, don = C.POINTER(_lib.PaintSegment)(), C.POINTER(_lib.PaintDonor)()
    length = (C.c_int64 * 1)(5)
    none = (None,) * 5
    assert lib.vg_paint_rows(1 << 31, None, None, 0, *none, 0, None, None, None, None, None, None) == -6
    assert '2^31 or more objects' in lib.vg_last_error().decode()
    assert lib.vg_paint_rows(1, length, None, 0, *none, 1 << 32, out, None, None, None, None, None) == -6
    assert '2^32 or more rows' in lib.vg_last_error().decode()
    assert lib.vg_paint_rows(1, length, None, 0, *none, 0, out, None, C.byref(n_seg), None, None, None) == -1
    assert 'segments and n_segments go together' in lib.vg_last_error().decode()
    assert lib.vg_paint_rows(1, length, None, 0, *none, 0, out, C.byref(seg), None, None, None, None) == -1
    assert lib.vg_paint_rows(1, length, None, 0, *none, 0, out, None, None, C.byref(don), None, None) == -1
    assert 'donors and n_donors go together' in lib.vg_last_error().decode()
    assert lib.vg_paint_rows(1, length, None, 0, *none, 0, out, None, None, None, C.byref(n_don), None) == -1
    assert lib.vg_paint_rows(1, length, None, 0, *none, 1, out, None, None, None, None, None) == -1 and 'null argument' in lib.vg_last_error().decode()
    assert lib.vg_paint_rows(-1, None, None, 0, *none, 0, None, None, None, None, None, None) == -1 and 'negative count' in lib.vg_last_error().decode()
    # no object: nothing to compute, no device needed
    st = _lib.PaintRunStats(1, 1, 1, 1, 1)
    assert lib.vg_paint_rows(0, None, None, 0, *none, 0, None, C.byref(seg), C.byref(n_seg), C.byref(don), C.byref(n_don), C.byref(st)) == 0
    assert n_seg.value == 0 and n_don.value == 0 and _lib.as_dict(st) == dict.fromkeys(pr.RUN_FIELDS, 0)
    records, segments, donors, run = api.paint_rows([], [], [], [], [], [])
    assert len(records) == 0 and len(segments) == 0 and len(donors) == 0 and run['segments'] == 0
    assert api.paint_rows([], [], [], [], [], [], segments=False, donors=False)[1:3] == (None, None)
    with pytest.raises(ValueError):
        api.paint_rows([5, 5], [0], [1], [0], [0], [1, 1])
    with pytest.raises(ValueError):
        api.paint_rows([5, 5], [0], [1], [0], [0], [1], label=[0])
    with pytest.raises(ValueError):
        api.paint_rows([5, 5], [0], [1], [0], [0], [1], n_groups=3)


def run_module(*args):
    return subprocess.run([sys.executable, '-m', 'vclust_amd.paint', *map(str, args)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def test_valid_calls_need_a_device(golden, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    ids, lengths, rows, out, _ = golden
    with pytest.raises(_lib.VclustGpuError) as e:
        api.paint_rows([10, 10], [0], [1], [0], [9], [9])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    paths = [tmp_path / name for name in ('paint.tsv', 'seg.tsv', 'donors.tsv')]
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.paint(out / 'ani.aln.tsv', out / 'ani.ids.tsv', paths[0], clusters_path=out / 'clusters.tsv', segments_path=paths[1], donors_path=paths[2])
    assert e.value.code == -3 and not any(p.exists() for p in paths)
    r = run_module('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', paths[0])
    assert r.returncode == 1 and 'ERROR' in r.stderr and 'Running: libvclust_gpu paint' in r.stderr and 'Completed' not in r.stderr


def _table(path, head, lines):
    path.write_text('\n'.join(['\t'.join(head)] + ['\t'.join(map(str, ln)) for ln in lines]) + '\n')
    return path


IDS = [('a', 100, 1), ('b', 50, 1), ('c', 0, 1)]
ALN_HEAD = ('query', 'reference', 'pident', 'alnlen', 'qstart', 'qend', 'rstart', 'rend', 'nt_match', 'nt_mismatch')
GOOD = ('a', 'b', 90, 10, 1, 10, 1, 10, 9, 1)
FILE_ERRORS = [
    # what is broken, the file it is in, line, message
    ('aln', ALN_HEAD, [GOOD, ('a', 'x', 90, 10, 1, 10, 1, 10, 9, 1)], 3, "reference 'x' is not in the ids file"),
    ('aln', ALN_HEAD, [('y', 'b', 90, 10, 1, 10, 1, 10, 9, 1)], 2, "query 'y' is not in the ids file"),
    ('aln', ALN_HEAD[:4] + ('qbegin',) + ALN_HEAD[5:], [GOOD], 1, 'missing column qstart'),
    ('aln', ALN_HEAD[:3] + ('length',) + ALN_HEAD[4:], [GOOD], 1, 'missing column alnlen'),
    ('aln', ALN_HEAD[:8] + ('matches', 'nt_mismatch'), [GOOD], 1, 'missing column nt_match'),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, '1x', 10, 1, 10, 9, 1)], 2, "malformed qstart '1x'"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1, '', 1, 10, 9, 1)], 2, "malformed qend ''"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 'ten', 1, 10, 1, 10, 9, 1)], 2, "malformed alnlen 'ten'"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1, 10, 1, 10, '-9', 1)], 2, "malformed nt_match '-9'"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1, 10, 1, 10, 9, '')], 2, "malformed nt_mismatch ''"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 0, 10, 1, 10, 9, 1)], 2, 'qstart..qend 0..10 is not a range inside 1..100'),
    ('aln', ALN_HEAD, [('b', 'a', 90, 10, 41, 51, 1, 10, 9, 1)], 2, 'qstart..qend 41..51 is not a range inside 1..50'),
    ('aln', ALN_HEAD, [('c', 'a', 90, 10, 1, 1, 1, 10, 9, 1)], 2, 'qstart..qend 1..1 is not a range inside 1..0'),
    ('aln', ALN_HEAD, [GOOD, ('a', 'b', 90, 11, 1, 10, 1, 10, 9, 2)], 3, 'alnlen 11 is not qend - qstart + 1 = 10'),
    ('aln', ALN_HEAD[:9], [('a', 'b', 90, 10, 1, 10, 1, 10, 11)], 2, 'nt_match 11 > alnlen 10'),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1, 10, 1, 10, 9, 2)], 2, 'nt_match + nt_mismatch = 11 is not alnlen 10'),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1)], 2, 'expected 10 columns, found 5'),
    ('ids', ('id', 'length', 'no_parts'), IDS, 1, 'missing column seq_len'),
    ('ids', ('id', 'seq_len', 'no_parts'), [('a', 100, 1), ('b', '5o', 1)], 3, "malformed seq_len '5o'"),
    ('clusters', ('object', 'cluster'), [('a', 0), ('b', 0)], 3, "object 'c' of the ids file is missing"),
    ('clusters', ('object', 'cluster'), [('a', 0), ('b', 0), ('c', 'z')], 4, "malformed cluster number 'z'"),
    ('column', ('object', 'cluster', 'tani_0.9'), [('a', 0, 0), ('b', 0, 1), ('c', 1, 2)], 1, "no label column 'tani_0.8'"),
]


def _broken_files(tmp_path, what, head, lines):
    ids = _table(tmp_path / 'ids.tsv', *((head, lines) if what == 'ids' else (('id', 'seq_len', 'no_parts'), IDS)))
    aln = _table(tmp_path / 'aln.tsv', *((head, lines) if what == 'aln' else (ALN_HEAD, [GOOD])))
    clusters = _table(tmp_path / 'clusters.tsv', head, lines) if what in ('clusters', 'column') else None
    return ids, aln, clusters, ('tani_0.8' if what == 'column' else None)


@pytest.mark.parametrize('what,head,lines,line,message', FILE_ERRORS)
def test_paint_file_errors(tmp_path, what, head, lines, line, message):
    ids, aln, clusters, column = _broken_files(tmp_path, what, head, lines)
    bad = {'ids': ids, 'aln': aln}.get(what, clusters)
    paths = [tmp_path / name for name in ('out.tsv', 'seg.tsv', 'donors.tsv')]
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.paint(aln, ids, paths[0], clusters_path=clusters, column=column, segments_path=paths[1], donors_path=paths[2])
    assert e.value.code == -1 and f'{bad}:{line}: {message}' in str(e.value)
    assert not any(p.exists() for p in paths)
    # the restatement's readers refuse the same tables at the same line
    if what in ('ids', 'aln'):
        with pytest.raises(pr.TableError, match=re.escape(f'{bad}:{line}: ')):
            pr.read_aln(aln, *pr.read_ids(ids))


def test_the_coverage_map_still_reads_a_table_without_the_counts(tmp_path):
    """alnlen and nt_match are the painting's columns: vg_cover_file does not ask for them (no device: it gets as far as VG_ENODEV)"""
    ids = _table(tmp_path / 'ids.tsv', ('id', 'seq_len', 'no_parts'), IDS)
    aln = _table(tmp_path / 'aln.tsv', ('query', 'reference', 'qstart', 'qend'), [('a', 'b', 1, 10)])
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.cover(aln, ids, tmp_path / 'cover.tsv')
    assert e.value.code == -3


def test_paint_file_null_and_missing(tmp_path):
    lib = _lib.load()
    assert lib.vg_paint_file(None, b'x', None, 0, None, b'y', None, None, 0, 0) == -1 and 'null argument' in lib.vg_last_error().decode()
    assert lib.vg_paint_file(b'x', b'y', None, 0, b'cluster', b'z', None, None, 0, 0) == -1 and 'needs a clusters file' in lib.vg_last_error().decode()
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.paint(tmp_path / 'none.tsv', tmp_path / 'none.ids.tsv', tmp_path / 'out.tsv')
    assert e.value.code == -2 and 'cannot open' in str(e.value)
    with pytest.raises(ValueError):
        stages.paint('a', 'b', 'c', column='cluster')
    with pytest.raises(ValueError):
        stages.paint('a', 'b', 'c', clusters_repr=True)


def test_command_module_usage_and_library_errors(tmp_path, golden):
    ids, lengths, rows, out, _ = golden
    r = run_module('-h')
    assert r.returncode == 0 and '--out-segments' in r.stdout and '--out-donors' in r.stdout and '--clusters-repr' in r.stdout
    base = ('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv')
    for args, message in [
            (('--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv'), 'the following arguments are required: -i'),
            (('-i', out / 'ani.aln.tsv', '-o', tmp_path / 'o.tsv'), 'the following arguments are required: --ids'),
            (('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv'), 'the following arguments are required: -o'),
            (base + ('--column', 'cluster'), 'they need --clusters'),
            (base + ('--clusters-repr',), 'they need --clusters'),
            (('-i', tmp_path / 'none.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv'), 'is not a file'),
            (base + ('--clusters', tmp_path / 'none.tsv'), 'is not a file'),
            (base + ('-t', '-2'), '-t must not be negative'),
            (base + ('-v', '7'), 'invalid choice')]:
        r = run_module(*args)
        assert r.returncode == 2 and message in r.stderr, (args, r.stderr)
    # a library error: the ids file of another run
    other = _table(tmp_path / 'ids.tsv', ('id', 'seq_len', 'no_parts'), IDS)
    r = run_module('-i', out / 'ani.aln.tsv', '--ids', other, '-o', tmp_path / 'o.tsv')
    assert r.returncode == 1 and 'ERROR' in r.stderr and f"{out / 'ani.aln.tsv'}:2: query 'NC_025457.alt2' is not in the ids file" in r.stderr
    assert not (tmp_path / 'o.tsv').exists()


def test_command_module_imports_neither_numpy_nor_torch():
    code = 'import sys; import vclust_amd.paint; sys.exit(int("numpy" in sys.modules or "torch" in sys.modules))'
    assert subprocess.run([sys.executable, '-c', code], cwd=ROOT, timeout=60).returncode == 0
