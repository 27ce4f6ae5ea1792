"""Sequential restatement of the mosaic painting: the checker of vg_paint_rows, vg_paint_file and
`python -m vclust_amd.paint`.  It is the definition read aloud: per object one array that holds the best-ranked row of every
position, filled row by row, then its run-length encoding.  Its cost follows the lengths, so it is for small inputs only
(tests/paint_sweep.py is the reference whose cost follows the rows).  numpy serves as the integer arrays; every figure is an integer.

A row (q, r, qstart, qend, n_match): the positions qstart..qend (0-based, inclusive) of object q are aligned to partner r, n_match of
them matching.  Only the query side counts and a row with q == r is ignored.  A row outranks another row of its object by larger
I = n_match * 2^32 // span, then larger span, then smaller r, then smaller qstart."""
import bisect

import numpy as np

import cover_restatement as cv
from cover_restatement import TableError, read_ids  # noqa: F401

FIELDS = ('len', 'painted', 'painted_in', 'painted_out', 'donors', 'top_partner', 'top_painted', 'switches', 'segments')
SEGMENT_FIELDS = ('object', 'start', 'end', 'partner', 'row_qstart', 'row_qend', 'n_match')
DONOR_FIELDS = ('object', 'partner', 'painted', 'segments')
RUN_FIELDS = ('rows_kept', 'breakpoints', 'segments', 'donor_records', 'levels')
UNPAINTED = (-1, -1, -1, 0)                             # partner, row_qstart, row_qend, n_match of a segment nothing wins
SUMMARY_HEADER = ('id', 'len', 'group', 'painted', 'painted_in', 'painted_out', 'donors', 'top_partner', 'top_painted', 'switches', 'segments',
                  'painted_frac', 'top_frac')
SEGMENTS_HEADER = ('id', 'start', 'end', 'partner', 'pident', 'row_qstart', 'row_qend')
DONORS_HEADER = ('id', 'partner', 'painted', 'segments', 'painted_frac')


def check_input(lengths, rows, label, n_groups):
    """-> (label, n_groups) with the defaults filled in; ValueError as the library's VG_EINVAL"""
    n = len(lengths)
    if label is None:
        label, n_groups = [0] * n, 1
    elif n_groups is None:
        n_groups = max(label, default=-1) + 1
    for i, x in enumerate(lengths):
        if not 0 <= x < 2 ** 31:
            raise ValueError(f'len[{i}] = {x}')
    for i, g in enumerate(label):
        if not 0 <= g < n_groups:
            raise ValueError(f'label[{i}] = {g} outside 0..{n_groups - 1}')
    for k, (q, r, s, e, m) in enumerate(rows):
        if not (0 <= q < n and 0 <= r < n):
            raise ValueError(f'row {k}: index outside 0..{n - 1}')
        if not 0 <= s <= e < lengths[q]:
            raise ValueError(f'row {k}: {s}..{e} is not a range inside 0..{lengths[q] - 1}')
        if not 0 <= m <= e - s + 1:
            raise ValueError(f'row {k}: n_match {m} outside 0..{e - s + 1}')
    return label, n_groups


def structure_counts(lengths, kept):
    """-> (breakpoints, levels) of the kept rows: the distinct (object, position) over qstart, qend + 1, 0 and len, and
    floor(log2(the most elementary segments one row covers)) + 1"""
    breaks = [{0, L} if L else set() for L in lengths]
    for q, _, s, e, _ in kept:
        breaks[q].update((s, e + 1))
    ordered = [sorted(b) for b in breaks]
    longest = max((bisect.bisect_left(ordered[q], e + 1) - bisect.bisect_left(ordered[q], s) for q, _, s, e, _ in kept), default=0)
    return sum(len(b) for b in breaks), longest.bit_length()


def paint(lengths, rows, label=None, n_groups=None):
    """-> (records: one dict with FIELDS per object, segments: [SEGMENT_FIELDS tuples] by (object, start), donors: [DONOR_FIELDS tuples]
    by (object, partner), run_stats: dict with RUN_FIELDS)"""
    label, n_groups = check_input(lengths, rows, label, n_groups)
    n = len(lengths)
    kept = [tuple(int(x) for x in row) for row in rows if row[0] != row[1]]
    # per object and position the winning row so far: its I (-1: none yet), span, r, qstart, qend, n_match
    best = [np.full((6, L), -1, dtype=np.int64) for L in lengths]
    for q, r, s, e, m in kept:
        span = e - s + 1
        I = m * 2 ** 32 // span
        bI, bspan, br, bqs = (best[q][k, s:e + 1] for k in range(4))
        better = (I > bI) | ((I == bI) & ((span > bspan) | ((span == bspan) & ((r < br) | ((r == br) & (s < bqs))))))
        best[q][:, s:e + 1][:, better] = np.array([I, span, r, s, e, m], dtype=np.int64)[:, None]
    records, segments, donors = [], [], []
    for i in range(n):
        L = lengths[i]
        won = best[i][2:]                                # r, qstart, qend, n_match: what a segment is constant on
        first = len(segments)
        # the run-length encoding: a segment starts at 0 and wherever the position to the left has other values
        heads = ([0] + (np.flatnonzero((won[:, 1:] != won[:, :-1]).any(axis=0)) + 1).tolist()) if L else []
        for x, nxt in zip(heads, heads[1:] + [L]):
            r, s, e, m = (int(v) for v in won[:, x])
            segments.append((i, x, nxt - 1) + ((r, s, e, m) if r >= 0 else UNPAINTED))
        mine = segments[first:]
        per = {}
        for _, a, b, r, _, _, _ in mine:
            if r >= 0:
                per.setdefault(r, [0, 0])
                per[r][0] += b - a + 1
                per[r][1] += 1
        donors += [(i, r, per[r][0], per[r][1]) for r in sorted(per)]
        top = min(per, key=lambda r: (-per[r][0], r)) if per else -1
        records.append(dict(
            len=L, painted=sum(v[0] for v in per.values()),
            painted_in=sum(v[0] for r, v in per.items() if label[r] == label[i]), painted_out=sum(v[0] for r, v in per.items() if label[r] != label[i]),
            donors=len(per), top_partner=top, top_painted=per[top][0] if per else 0,
            switches=sum(a[3] >= 0 and b[3] >= 0 and a[3] != b[3] for a, b in zip(mine, mine[1:])), segments=len(mine)))
    breakpoints, levels = structure_counts(lengths, kept)
    return records, segments, donors, dict(rows_kept=len(kept), breakpoints=breakpoints, segments=len(segments), donor_records=len(donors), levels=levels)


# ---------------------------------------------------------------- files
def read_aln(path, ids, lengths):
    """-> rows (q, r, qstart, qend, n_match), 0-based inclusive, in file order; the checks of cover_restatement.read_aln, and per row
    alnlen == qend - qstart + 1 and nt_match + nt_mismatch == alnlen"""
    plain = cv.read_aln(path, ids, lengths)
    lines = cv._lines(path)
    head = lines[0].split('\t')
    for name in ('alnlen', 'nt_match'):
        if name not in head:
            raise TableError(f'{path}:1: missing column {name}')
    cols = [head.index(x) for x in ('alnlen', 'nt_match')] + ([head.index('nt_mismatch')] if 'nt_mismatch' in head else [])
    rows = []
    body = [(k, ln) for k, ln in enumerate(lines[1:], 2) if ln]
    for (k, ln), (q, r, s, e) in zip(body, plain):
        f = ln.split('\t')
        if len(f) <= max(cols):
            raise TableError(f'{path}:{k}: expected {len(head)} columns, found {len(f)}')
        for name, c in zip(('alnlen', 'nt_match', 'nt_mismatch'), cols):
            if not (f[c].isascii() and f[c].isdigit()):
                raise TableError(f"{path}:{k}: malformed {name} '{f[c]}'")
        v = [int(f[c]) for c in cols]
        if v[0] != e - s + 1:
            raise TableError(f'{path}:{k}: alnlen {v[0]} is not qend - qstart + 1 = {e - s + 1}')
        if v[1] > v[0]:
            raise TableError(f'{path}:{k}: nt_match {v[1]} > alnlen {v[0]}')
        if len(v) == 3 and v[1] + v[2] != v[0]:
            raise TableError(f'{path}:{k}: nt_match + nt_mismatch = {v[1] + v[2]} is not alnlen {v[0]}')
        rows.append((q, r, s, e, v[1]))
    return rows


def _quotient(have, a, b):
    return '%.6g' % (a / b) if have else '-'


def summary_text(ids, records, label=None, text=None):
    """The summary file.  label / text: the group of every object and the label text of every group (None: one group, printed `-`)."""
    out = ['\t'.join(SUMMARY_HEADER)]
    for i, rec in enumerate(records):
        L = rec['len']
        out.append('\t'.join([ids[i], str(L), text[label[i]] if label is not None else '-'] +
                             [str(rec[f]) for f in ('painted', 'painted_in', 'painted_out', 'donors')] +
                             [ids[rec['top_partner']] if rec['top_partner'] >= 0 else '-'] + [str(rec[f]) for f in ('top_painted', 'switches', 'segments')] +
                             [_quotient(L > 0, rec['painted'], L), _quotient(L > 0, rec['top_painted'], L)]))
    return '\n'.join(out) + '\n'


def segments_text(ids, segments, fmt_num):
    """fmt_num: the number format of the alignment table (oracle_lib.fmt_num), applied to 100 * n_match / span of the winning row"""
    out = ['\t'.join(SEGMENTS_HEADER)]
    for o, a, b, r, s, e, m in segments:
        out.append('\t'.join([ids[o], str(a + 1), str(b + 1)] + ([ids[r], fmt_num(100.0 * m / (e - s + 1)), str(s + 1), str(e + 1)] if r >= 0 else ['-'] * 4)))
    return '\n'.join(out) + '\n'


def donors_text(ids, lengths, donors):
    out = ['\t'.join(DONORS_HEADER)]
    out += [f'{ids[o]}\t{ids[r]}\t{p}\t{k}\t' + '%.6g' % (p / lengths[o]) for o, r, p, k in donors]
    return '\n'.join(out) + '\n'
