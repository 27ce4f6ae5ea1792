"""Event sweep of the coverage map: the second reference, for the inputs whose size or lengths the mask
restatement (tests/cover_restatement.py) cannot hold.  The same definition by another route: per (q, r) the rows are sorted and
merged into the disjoint intervals of C(q, r) (rows that overlap or touch are one), every interval is a +1 at its start and a -1
behind its end in the channel of its partner, and per object the events are applied in position order; a segment starts where the
pair of depths changes.  The cost follows the rows, never the lengths.  Python integers only, no numpy.
tests/test_cover_sweep_cpu.py holds it equal to the restatement; tests/test_gpu_cover_sizes.py is its only other user."""
from cover_restatement import FIELDS, RUN_FIELDS


def cover(lengths, rows, label=None, n_groups=None, arrays=None):
    """-> (records, segments, run_stats) as cover_restatement.cover returns them.  arrays: a dict that receives the three arrays
    that the stage scans beside the objects, in their order: 'rows' = the (q, r) of the kept rows by (q, r, qstart),
    'breakpoints' = the distinct (object, position), and 'depths' = the (depth_in, depth_out) behind each breakpoint."""
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
    size = [0] * n_groups
    for g in label:
        size[g] += 1
    for k, (q, r, s, e) in enumerate(rows):
        if not (0 <= q < n and 0 <= r < n):
            raise ValueError(f'row {k}: index outside 0..{n - 1}')
        if not 0 <= s <= e < lengths[q]:
            raise ValueError(f'row {k}: {s}..{e} is not a range inside 0..{lengths[q] - 1}')
    kept = sorted((int(q), int(r), int(s), int(e)) for q, r, s, e in rows if q != r)

    events = {}                 # object -> {position: [delta_in, delta_out]}
    partners = {}               # object -> [in, out]: distinct partners
    summed = {}                 # object -> [in, out]: |C(q, r)| over the partners
    intervals = 0

    def close(q, r, s, e):
        ch = 0 if label[r] == label[q] else 1
        ev = events.setdefault(q, {})
        ev.setdefault(s, [0, 0])[ch] += 1
        ev.setdefault(e + 1, [0, 0])[ch] -= 1
        summed.setdefault(q, [0, 0])[ch] += e + 1 - s

    cur = None                  # the open interval (q, r, start, end)
    for q, r, s, e in kept:
        if cur is not None and cur[0] == q and cur[1] == r:
            if s <= cur[3] + 1:                         # overlaps or touches: the same interval
                if e > cur[3]:
                    cur[3] = e
                continue
        else:
            partners.setdefault(q, [0, 0])[0 if label[r] == label[q] else 1] += 1
        if cur is not None:
            close(*cur)
        intervals += 1
        cur = [q, r, s, e]
    if cur is not None:
        close(*cur)

    records, segments, breakpoints = [], [], 0
    if arrays is not None:
        arrays['rows'] = [(q, r) for q, r, _, _ in kept]
        arrays['breakpoints'], arrays['depths'] = [], []
    for i in range(n):
        L = lengths[i]
        ev = events.get(i, {})
        breakpoints += len(ev)
        members = size[label[i]]
        first = len(segments)
        acc = [0, 0, 0, 0, 0]                           # covered, covered_in, covered_out, core, max_depth

        def emit(start, end, a, b):
            width = end - start + 1
            segments.append((i, start, end, a, b))
            acc[0] += width if a + b >= 1 else 0
            acc[1] += width if a >= 1 else 0
            acc[2] += width if b >= 1 else 0
            acc[3] += width if members >= 2 and a == members - 1 else 0
            acc[4] = max(acc[4], a + b)

        d_in = d_out = start = seg_in = seg_out = 0     # the depths behind the last event, the open segment and its depths
        for pos in sorted(ev):
            a, b = ev[pos]
            d_in, d_out = d_in + a, d_out + b
            if arrays is not None:
                arrays['breakpoints'].append((i, pos))
                arrays['depths'].append((d_in, d_out))
            if (a or b) and pos < L:                    # (a net delta of zero -- one partner ends where another starts -- changes nothing)
                if pos > 0:
                    emit(start, pos - 1, seg_in, seg_out)
                start, seg_in, seg_out = pos, d_in, d_out
        if L > 0:
            emit(start, L - 1, seg_in, seg_out)
        p, t = partners.get(i, (0, 0)), summed.get(i, (0, 0))
        records.append(dict(len=L, partners_in=p[0], partners_out=p[1], covered=acc[0], covered_in=acc[1], covered_out=acc[2],
                            core=acc[3], sum_in=t[0], sum_out=t[1], max_depth=acc[4], segments=len(segments) - first))
    run = dict(rows_kept=len(kept), intervals=intervals, breakpoints=breakpoints, segments=len(segments))
    assert tuple(run) == RUN_FIELDS and all(tuple(rec) == FIELDS for rec in records[:1])
    return records, segments, run
