"""Event sweep of the mosaic painting: the second reference, for the inputs whose size or lengths the array
restatement (tests/paint_restatement.py) cannot hold.  The same definition by another route: per object the breakpoints (every
qstart and qend + 1, 0 and len) are walked in order; a row enters a heap at its qstart, the heap's top is the best-ranked row, and a
top that has ended is thrown out when it is met (lazy deletion).  The top behind a breakpoint wins up to the next one; neighbours
with the same winner are one segment.  The cost follows the rows, never the lengths.  Python integers only, no numpy.
tests/test_paint_cpu.py holds it equal to the restatement; tests/test_gpu_paint_sizes.py is its only other user."""
import heapq

from paint_restatement import FIELDS, RUN_FIELDS, UNPAINTED, check_input


def paint(lengths, rows, label=None, n_groups=None, arrays=None):
    """-> (records, segments, donors, run_stats) as paint_restatement.paint returns them.  arrays: a dict that receives
    'breakpoints', the distinct (object, position) in order, and 'spans', per kept row the elementary segments it covers."""
    label, n_groups = check_input(lengths, rows, label, n_groups)
    n = len(lengths)
    by_object = {}
    kept = 0
    for q, r, s, e, m in rows:
        if q != r:
            kept += 1
            by_object.setdefault(int(q), []).append((int(r), int(s), int(e), int(m)))
    records, segments, donors = [], [], []
    breakpoints, longest = 0, 0
    if arrays is not None:
        arrays['breakpoints'], arrays['spans'] = [], []
    for i in range(n):
        L = lengths[i]
        mine = by_object.get(i, [])
        starts = {}
        for r, s, e, m in mine:
            span = e - s + 1
            starts.setdefault(s, []).append((-(m * 2 ** 32 // span), -span, r, s, e, m))       # the smallest tuple is the best-ranked row
        breaks = sorted({0, L} | {s for _, s, _, _ in mine} | {e + 1 for _, _, e, _ in mine}) if L else []
        breakpoints += len(breaks)
        rank = {pos: k for k, pos in enumerate(breaks)}
        for _, s, e, _ in mine:
            longest = max(longest, rank[e + 1] - rank[s])
            if arrays is not None:
                arrays['spans'].append(rank[e + 1] - rank[s])
        if arrays is not None:
            arrays['breakpoints'] += [(i, pos) for pos in breaks]
        heap = []
        first = len(segments)
        acc = dict(painted=0, painted_in=0, painted_out=0, switches=0)
        per = {}                                        # partner -> [positions, segments]

        def close(seg):
            o, a, b, r = seg[:4]
            segments.append(seg)
            if r < 0:
                return
            width = b - a + 1
            acc['painted'] += width
            acc['painted_in' if label[r] == label[i] else 'painted_out'] += width
            d = per.setdefault(r, [0, 0])
            d[0] += width
            d[1] += 1
            if len(segments) - first >= 2 and segments[-2][3] >= 0 and segments[-2][3] != r:
                acc['switches'] += 1

        cur = None                                      # the open segment: [start, winner values]
        for pos in breaks[:-1]:
            for item in starts.get(pos, ()):
                heapq.heappush(heap, item)
            while heap and heap[0][4] < pos:            # ended before pos
                heapq.heappop(heap)
            won = (heap[0][2], heap[0][3], heap[0][4], heap[0][5]) if heap else UNPAINTED
            if cur is None or cur[1] != won:
                if cur is not None:
                    close((i, cur[0], pos - 1) + cur[1])
                cur = [pos, won]
        if cur is not None:
            close((i, cur[0], L - 1) + cur[1])
        donors += [(i, r, per[r][0], per[r][1]) for r in sorted(per)]
        top = min(per, key=lambda r: (-per[r][0], r)) if per else -1
        records.append(dict(len=L, painted=acc['painted'], painted_in=acc['painted_in'], painted_out=acc['painted_out'], donors=len(per), top_partner=top,
                            top_painted=per[top][0] if per else 0, switches=acc['switches'], segments=len(segments) - first))
    run = dict(rows_kept=kept, breakpoints=breakpoints, segments=len(segments), donor_records=len(donors), levels=longest.bit_length())
    assert tuple(run) == RUN_FIELDS and all(tuple(rec) == FIELDS for rec in records[:1])
    return records, segments, donors, run
