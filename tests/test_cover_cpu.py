"""The coverage map without a device: the invariants of the sequential restatement (tests/cover_restatement.py)
on random inputs and on the golden example, and the interface -- every argument error of vg_cover_rows, vg_cover_file and
`python -m vclust_amd.cover` is raised on the host, before any device use, and a valid call without a device is VG_ENODEV."""
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import cluster_stats_restatement as cs
import cover_restatement as cv
from vclust_amd import _lib, api, stages

ROOT = pathlib.Path(__file__).resolve().parent.parent


def random_case(rng, n, max_len, n_rows, groups):
    lengths = [int(x) for x in rng.integers(0, max_len + 1, n)]
    rows = []
    live = [i for i in range(n) if lengths[i] > 0]
    while live and len(rows) < n_rows:
        q = int(rng.choice(live))
        r = int(rng.integers(0, n))
        s = int(rng.integers(0, lengths[q]))
        e = min(lengths[q] - 1, s + int(rng.integers(0, max(1, lengths[q] // 2))))
        rows.append((q, r, s, e))
    label = [int(x) for x in rng.integers(0, groups, n)] if groups else None
    return lengths, rows, label


CASES = [(seed, n, density, groups) for seed, (n, density, groups) in enumerate(
    [(1, 0, 0), (1, 3, 0), (2, 5, 2), (7, 2, 0), (7, 40, 3), (20, 1, 0), (20, 10, 4), (40, 3, 0), (40, 3, 40), (40, 12, 5)])]


@pytest.mark.parametrize('seed,n,density,groups', CASES)
def test_restatement_invariants(seed, n, density, groups):
    rng = np.random.default_rng(seed)
    lengths, rows, label = random_case(rng, n, 300, n * density, groups)
    records, segments, run = cv.cover(lengths, rows, label, groups or None)
    lab = label or [0] * n
    size = [lab.count(g) for g in range(max(lab) + 1)]
    assert run['segments'] == len(segments) and run['rows_kept'] == sum(q != r for q, r, _, _ in rows)
    assert segments == sorted(segments, key=lambda t: t[:2])
    by_object = [[t for t in segments if t[0] == i] for i in range(n)]
    for i, segs in enumerate(by_object):
        rec = records[i]
        # the segments partition 0..len-1, and neighbours differ
        assert [t[1] for t in segs] == [0][:len(segs)] + [t[2] + 1 for t in segs[:-1]]
        assert (segs[-1][2] == lengths[i] - 1) if lengths[i] else not segs
        assert all(a[3:] != b[3:] for a, b in zip(segs, segs[1:]))
        # the sums over the segments give every field of the record
        width = [e - s + 1 for _, s, e, _, _ in segs]
        partners = {r for q, r, _, _ in rows if q == i and r != i}
        assert rec == dict(
            len=lengths[i], partners_in=sum(lab[r] == lab[i] for r in partners), partners_out=sum(lab[r] != lab[i] for r in partners),
            covered=sum(w for w, t in zip(width, segs) if t[3] + t[4] >= 1), covered_in=sum(w for w, t in zip(width, segs) if t[3] >= 1),
            covered_out=sum(w for w, t in zip(width, segs) if t[4] >= 1),
            core=sum(w for w, t in zip(width, segs) if t[3] == size[lab[i]] - 1) if size[lab[i]] >= 2 else 0,
            sum_in=sum(w * t[3] for w, t in zip(width, segs)), sum_out=sum(w * t[4] for w, t in zip(width, segs)),
            max_depth=max((t[3] + t[4] for t in segs), default=0), segments=len(segs))
        assert rec['max_depth'] <= len(partners) and rec['core'] <= rec['covered_in'] <= rec['covered'] <= rec['len']
    if not rows:
        assert segments == [(i, 0, lengths[i] - 1, 0, 0) for i in range(n) if lengths[i]]
    # a function of the set of rows: neither their order nor repeats change anything
    shuffled = [rows[k] for k in rng.permutation(len(rows))] + [rows[k] for k in rng.integers(0, len(rows), len(rows) // 2)] if rows else []
    again = cv.cover(lengths, shuffled, label, groups or None)
    assert again[:2] == (records, segments)
    assert {k: again[2][k] for k in ('intervals', 'breakpoints', 'segments')} == {k: run[k] for k in ('intervals', 'breakpoints', 'segments')}


# ---------------------------------------------------------------- the golden example
@pytest.fixture(scope='module')
def golden(golden_dir):
    out = golden_dir / 'output'
    ids, lengths = cv.read_ids(out / 'ani.ids.tsv')
    rows = cv.read_aln(out / 'ani.aln.tsv', ids, lengths)
    return ids, lengths, rows, out


def test_golden_example_figures(golden):
    ids, lengths, rows, out = golden
    assert len(ids) == 12 and len(rows) == 5693
    records, segments, run = cv.cover(lengths, rows)
    by_id = dict(zip(ids, records))
    assert all(rec['partners_in'] == 11 and rec['partners_out'] == 0 for rec in records)
    a = by_id['NC_025457.alt2']
    assert (a['covered'], a['len'], a['max_depth']) == (49330, 64164, 7)
    b = by_id['NC_005091']
    assert b['covered'] == b['len'] and b['max_depth'] == 9
    # no two rows of a pair overlap in this table, so the depth sums are the rows' alnlen
    head = open(out / 'ani.aln.tsv').readline().rstrip('\n').split('\t')
    aln = [0] * len(ids)
    index = {x: i for i, x in enumerate(ids)}
    for ln in open(out / 'ani.aln.tsv').read().split('\n')[1:]:
        if ln:
            f = ln.split('\t')
            aln[index[f[head.index('query')]]] += int(f[head.index('alnlen')])
    assert [rec['sum_in'] + rec['sum_out'] for rec in records] == aln
    assert run['rows_kept'] == 5693 and run['intervals'] <= 5693        # (rows that touch are one interval)


def test_golden_example_with_clusters(golden):
    ids, lengths, rows, out = golden
    names, label, text = cs.read_clusters(out / 'clusters.tsv', ids)
    records, _, _ = cv.cover(lengths, rows, label[0], len(text[0]))
    size = [label[0].count(g) for g in range(len(text[0]))]
    assert 1 in size and max(size) >= 2
    for i, rec in enumerate(records):
        assert rec['core'] <= rec['covered_in'] <= rec['len']
        assert rec['partners_in'] <= size[label[0][i]] - 1 and rec['partners_in'] + rec['partners_out'] == 11
        if size[label[0][i]] == 1:
            assert rec['core'] == 0 and rec['covered_in'] == 0
    summary = cv.summary_text(ids, records, label[0], text[0]).split('\n')
    assert summary[0].split('\t') == list(cv.SUMMARY_HEADER) and len(summary) == 14
    assert all(ln.split('\t')[-1] == '-' for i, ln in enumerate(summary[1:13]) if size[label[0][i]] == 1)


# ---------------------------------------------------------------- the interface, without a device
def test_symbols_and_record_types():
    lib = _lib.load()
    for name in ('vg_cover_rows', 'vg_cover_file'):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert api.COVER_STAT_DTYPE.names == cv.FIELDS and api.COVER_STAT_DTYPE.itemsize == 88
    assert api.COVER_SEGMENT_DTYPE.names == ('object', 'start', 'end', 'depth_in', 'depth_out') and api.COVER_SEGMENT_DTYPE.itemsize == 20
    assert tuple(n for n, _ in _lib.CoverRunStats._fields_) == cv.RUN_FIELDS


ROW_ERRORS = [
    # lengths, q, r, qstart, qend, keywords, code, message
    ([10, 10], [0, 2], [1, 0], [0, 0], [1, 1], {}, -1, 'vg_cover_rows: row 1: index 2 outside 0..1'),
    ([10, 10], [0], [7], [0], [1], {}, -1, 'vg_cover_rows: row 0: index 7 outside 0..1'),
    ([10, 10], [0, 1], [1, 0], [0, -1], [1, 1], {}, -1, 'vg_cover_rows: row 1: qstart -1 is negative'),
    ([10, 10], [0], [1], [5], [4], {}, -1, 'vg_cover_rows: row 0: qstart 5 > qend 4'),
    ([10, 4], [0, 1], [1, 0], [0, 0], [9, 4], {}, -1, 'vg_cover_rows: row 1: qend 4 >= len[1] = 4'),
    ([10, 0], [1], [0], [0], [0], {}, -1, 'vg_cover_rows: row 0: qend 0 >= len[1] = 0'),
    ([10, -3], [], [], [], [], {}, -1, 'vg_cover_rows: len[1] = -3 is negative'),
    ([2 ** 31, 5], [], [], [], [], {}, -1, 'vg_cover_rows: len[0] = 2147483648 is 2^31 or more'),
    ([10, 10], [0], [1], [0], [1], dict(label=[0, 2], n_groups=2), -1, 'vg_cover_rows: label[1] = 2 outside 0..1'),
    ([10, 10], [0], [1], [0], [1], dict(label=[-1, 0], n_groups=2), -1, 'vg_cover_rows: label[0] = -1 outside 0..1'),
]


@pytest.mark.parametrize('lengths,q,r,qs,qe,kw,code,message', ROW_ERRORS)
def test_cover_rows_argument_errors(lengths, q, r, qs, qe, kw, code, message):
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cover_rows(lengths, q, r, qs, qe, **kw)
    assert e.value.code == code and message in str(e.value)


def test_cover_rows_counts_and_pointers():
    lib = _lib.load()
    out = (_lib.CoverStat * 1)()
    n_seg = _lib.C.c_int64()
    seg = _lib.C.POINTER(_lib.CoverSegment)()
    length = (_lib.C.c_int64 * 1)(5)
    assert lib.vg_cover_rows(1 << 31, None, None, 0, None, None, None, None, 0, None, None, None, None) == -6
    assert '2^31 or more objects' in lib.vg_last_error().decode()
    assert lib.vg_cover_rows(1, length, None, 0, None, None, None, None, 1 << 32, out, None, None, None) == -6
    assert '2^32 or more rows' in lib.vg_last_error().decode()
    assert lib.vg_cover_rows(1, length, None, 0, None, None, None, None, 0, out, None, _lib.C.byref(n_seg), None) == -1
    assert 'segments and n_segments go together' in lib.vg_last_error().decode()
    assert lib.vg_cover_rows(1, length, None, 0, None, None, None, None, 0, out, _lib.C.byref(seg), None, None) == -1
    # no object: nothing to compute, no device needed
    st = _lib.CoverRunStats(1, 1, 1, 1)
    assert lib.vg_cover_rows(0, None, None, 0, None, None, None, None, 0, None, _lib.C.byref(seg), _lib.C.byref(n_seg), _lib.C.byref(st)) == 0
    assert n_seg.value == 0 and _lib.as_dict(st) == dict.fromkeys(cv.RUN_FIELDS, 0)
    records, segments, run = api.cover_rows([], [], [], [], [])
    assert len(records) == 0 and len(segments) == 0 and run['segments'] == 0
    with pytest.raises(ValueError):
        api.cover_rows([5, 5], [0], [1, 0], [0], [0])
    with pytest.raises(ValueError):
        api.cover_rows([5, 5], [0], [1], [0], [0], label=[0])
    with pytest.raises(ValueError):
        api.cover_rows([5, 5], [0], [1], [0], [0], n_groups=3)


def test_valid_calls_need_a_device(golden, tmp_path):
    if api.device_count() > 0:
        pytest.skip('a HIP device is visible')
    ids, lengths, rows, out = golden
    with pytest.raises(_lib.VclustGpuError) as e:
        api.cover_rows([10, 10], [0], [1], [0], [9])
    assert e.value.code == -3 and 'no CPU fallback' in str(e.value)
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.cover(out / 'ani.aln.tsv', out / 'ani.ids.tsv', tmp_path / 'cover.tsv', clusters_path=out / 'clusters.tsv', segments_path=tmp_path / 'seg.tsv')
    assert e.value.code == -3
    assert not (tmp_path / 'cover.tsv').exists() and not (tmp_path / 'seg.tsv').exists()
    r = run_module('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'cover.tsv')
    assert r.returncode == 1 and 'ERROR' in r.stderr and 'Running: libvclust_gpu cover' in r.stderr and 'Completed' not in r.stderr


def _table(path, head, lines):
    path.write_text('\n'.join(['\t'.join(head)] + ['\t'.join(map(str, ln)) for ln in lines]) + '\n')
    return path


IDS = [('a', 100, 1), ('b', 50, 1), ('c', 0, 1)]
ALN_HEAD = ('query', 'reference', 'pident', 'alnlen', 'qstart', 'qend', 'rstart', 'rend', 'nt_match', 'nt_mismatch')
FILE_ERRORS = [
    # what is broken, the file it is in, line, message
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1, 10, 1, 10, 9, 1), ('a', 'x', 90, 10, 1, 10, 1, 10, 9, 1)], 3, "reference 'x' is not in the ids file"),
    ('aln', ALN_HEAD, [('y', 'b', 90, 10, 1, 10, 1, 10, 9, 1)], 2, "query 'y' is not in the ids file"),
    ('aln', ALN_HEAD[:4] + ('qbegin',) + ALN_HEAD[5:], [('a', 'b', 90, 10, 1, 10, 1, 10, 9, 1)], 1, 'missing column qstart'),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, '1x', 10, 1, 10, 9, 1)], 2, "malformed qstart '1x'"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1, '', 1, 10, 9, 1)], 2, "malformed qend ''"),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 0, 10, 1, 10, 9, 1)], 2, 'qstart..qend 0..10 is not a range inside 1..100'),
    ('aln', ALN_HEAD, [('b', 'a', 90, 10, 41, 51, 1, 10, 9, 1)], 2, 'qstart..qend 41..51 is not a range inside 1..50'),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 11, 10, 1, 10, 9, 1)], 2, 'qstart..qend 11..10 is not a range inside 1..100'),
    ('aln', ALN_HEAD, [('c', 'a', 90, 10, 1, 1, 1, 10, 9, 1)], 2, 'qstart..qend 1..1 is not a range inside 1..0'),
    ('aln', ALN_HEAD, [('a', 'b', 90, 10, 1)], 2, 'expected 10 columns, found 5'),
    ('ids', ('id', 'length', 'no_parts'), IDS, 1, 'missing column seq_len'),
    ('ids', ('id', 'seq_len', 'no_parts'), [('a', 100, 1), ('b', '5o', 1)], 3, "malformed seq_len '5o'"),
    ('clusters', ('object', 'cluster'), [('a', 0), ('b', 0)], 3, "object 'c' of the ids file is missing"),
    ('clusters', ('object', 'cluster'), [('a', 0), ('b', 0), ('c', 'z')], 4, "malformed cluster number 'z'"),
    ('column', ('object', 'cluster', 'tani_0.9'), [('a', 0, 0), ('b', 0, 1), ('c', 1, 2)], 1, "no label column 'tani_0.8'"),
]


def _broken_files(tmp_path, what, head, lines):
    ids = _table(tmp_path / 'ids.tsv', *((head, lines) if what == 'ids' else (('id', 'seq_len', 'no_parts'), IDS)))
    aln = _table(tmp_path / 'aln.tsv', *((head, lines) if what == 'aln' else (ALN_HEAD, [('a', 'b', 90, 10, 1, 10, 1, 10, 9, 1)])))
    clusters = _table(tmp_path / 'clusters.tsv', head, lines) if what in ('clusters', 'column') else None
    return ids, aln, clusters, ('tani_0.8' if what == 'column' else None)


@pytest.mark.parametrize('what,head,lines,line,message', FILE_ERRORS)
def test_cover_file_errors(tmp_path, what, head, lines, line, message):
    ids, aln, clusters, column = _broken_files(tmp_path, what, head, lines)
    bad = {'ids': ids, 'aln': aln}.get(what, clusters)
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.cover(aln, ids, tmp_path / 'out.tsv', clusters_path=clusters, column=column, segments_path=tmp_path / 'seg.tsv')
    assert e.value.code == -1 and f'{bad}:{line}: {message}' in str(e.value)
    assert not (tmp_path / 'out.tsv').exists() and not (tmp_path / 'seg.tsv').exists()
    # the restatement's readers refuse the same tables at the same line
    if what in ('ids', 'aln'):
        with pytest.raises(cv.TableError, match=re.escape(f'{bad}:{line}: ')):
            cv.read_aln(aln, *cv.read_ids(ids))


def test_cover_file_null_and_missing(tmp_path):
    lib = _lib.load()
    assert lib.vg_cover_file(None, b'x', None, 0, None, b'y', None, 0, 0) == -1 and 'null argument' in lib.vg_last_error().decode()
    assert lib.vg_cover_file(b'x', b'y', None, 0, b'cluster', b'z', None, 0, 0) == -1 and 'needs a clusters file' in lib.vg_last_error().decode()
    with pytest.raises(_lib.VclustGpuError) as e:
        stages.cover(tmp_path / 'none.tsv', tmp_path / 'none.ids.tsv', tmp_path / 'out.tsv')
    assert e.value.code == -2 and 'cannot open' in str(e.value)
    with pytest.raises(ValueError):
        stages.cover('a', 'b', 'c', column='cluster')
    with pytest.raises(ValueError):
        stages.cover('a', 'b', 'c', clusters_repr=True)


def run_module(*args):
    return subprocess.run([sys.executable, '-m', 'vclust_amd.cover', *map(str, args)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=120)


def test_command_module_usage_and_library_errors(tmp_path, golden):
    ids, lengths, rows, out = golden
    r = run_module('-h')
    assert r.returncode == 0 and '--out-segments' in r.stdout and '--clusters-repr' in r.stdout
    for args, message in [
            (('--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv'), 'the following arguments are required: -i'),
            (('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv', '--column', 'cluster'), 'they need --clusters'),
            (('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv', '--clusters-repr'), 'they need --clusters'),
            (('-i', tmp_path / 'none.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv'), 'is not a file'),
            (('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv', '-t', '-2'), '-t must not be negative'),
            (('-i', out / 'ani.aln.tsv', '--ids', out / 'ani.ids.tsv', '-o', tmp_path / 'o.tsv', '-v', '7'), 'invalid choice')]:
        r = run_module(*args)
        assert r.returncode == 2 and message in r.stderr, (args, r.stderr)
    # a library error: the ids file of another run
    other = _table(tmp_path / 'ids.tsv', ('id', 'seq_len', 'no_parts'), IDS)
    r = run_module('-i', out / 'ani.aln.tsv', '--ids', other, '-o', tmp_path / 'o.tsv')
    assert r.returncode == 1 and 'ERROR' in r.stderr and f"{out / 'ani.aln.tsv'}:2: query 'NC_025457.alt2' is not in the ids file" in r.stderr
    assert not (tmp_path / 'o.tsv').exists()


def test_command_module_imports_neither_numpy_nor_torch():
    code = 'import sys; import vclust_amd.cover; sys.exit(int("numpy" in sys.modules or "torch" in sys.modules))'
    assert subprocess.run([sys.executable, '-c', code], cwd=ROOT, timeout=60).returncode == 0
