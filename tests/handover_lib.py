"""The four-wave LZ parse (lz_parse_body<4, ...> in vclust_amd/csrc/vg_align.hip) restated from the oracle's events
-- TEST INFRASTRUCTURE ONLY (not a conftest, no fixtures: test_parse_handover_cpu.py and test_gpu_parse_handover.py import it).

  * geometry / parses: the segments of a query and the oracle's parse from every segment start (oracle_lib.LzIndex.events);
  * check_rule: what the hand-over relies on, (a) two parses that share an event with span_ok in both are the same parse
    from there on and (b) their virtual sums differ by constants from there on;
  * chain: the kernel's logs, lookups, hand-overs and final sums in plain Python, (c) its row must be the oracle's;
  * adversarial_set / arms_reached: pairs built to reach each arm of the hand-over, and the conditions ON THE ORACLE'S
    EVENTS (they hold whatever the GPU does) that say an arm is reached.
"""
import numpy as np

import lz_checks as lc
import oracle_lib as orc

WAVES = 4
SPLIT_MIN = 2048               # `lim >= S * 2048`
SEG_LOG_CAP = 250              # `constexpr int SEG_LOG_CAP = 250`
M32 = 0xffffffff
# probe widths (first probe of a wave, right after an event, after a miss): they decide only whether the one event that
# crosses the end of a wave's segment is found -- and logged -- before the wave starts looking events up
PROBE_KERNEL = (64, 32, 64)    # `int pw = 64`, PW_AFTER_EVENT, pw_miss
PROBE_NARROW = (1, 1, 1)       # never
PROBE_WIDE = (1 << 30, 1 << 30, 1 << 30)      # whenever the wave stood in front of the end
PROBES = dict(kernel=PROBE_KERNEL, narrow=PROBE_NARROW, wide=PROBE_WIDE)


def params(lz=None):
    return {**lc.DEFAULT_LZ, **(lz or {})}


def geometry(qlen, mal):
    """-> (lim, split, seg_len, [seg_start of wave w], [phase_end of wave w])"""
    lim = qlen - mal
    split = lim >= WAVES * SPLIT_MIN
    seg_len = ((-(-lim // WAVES)) + 63) & ~63 if split else max(lim, 1)
    starts = [min(w * seg_len, max(lim, 0)) for w in range(WAVES)]
    ends = [min((w + 1) * seg_len, lim) if w < WAVES - 1 else lim for w in range(WAVES)]
    return lim, split, seg_len, starts, ends


class Parse:
    """one parse of the oracle: its events as plain lists, and the row of the regions it keeps"""

    def __init__(self, ev, row):
        self.n = len(ev)
        self.i, self.pos, self.end = ev['ev_i'].tolist(), ev['ev_pos'].tolist(), ev['ev_end'].tolist()
        self.ok = [bool(x) for x in ev['span_ok'].tolist()]
        self.VM, self.VA, self.VN = ev['VM'].tolist(), ev['VA'].tolist(), ev['VN'].tolist()
        self.row = row
        self.at = {(a, b): k for k, (a, b) in enumerate(zip(self.i, self.pos))}


def parses(Q, R, lz=None):
    """[the parse a wave starts: from w * seg_len with an empty state, w = 0 the ordinary parse]"""
    lim, split, seg_len, starts, ends = geometry(len(Q), params(lz)['mal'])
    with orc.LzIndex(R, lz) as ix:
        return [Parse(*ix.events(Q, s, with_row=True)) for s in starts]


def first_common(A, B):
    """index in A and in B of the first event (i, j) both parses place with span_ok in both, or None"""
    for kb in range(B.n):
        if B.ok[kb]:
            ka = A.at.get((B.i[kb], B.pos[kb]))
            if ka is not None and A.ok[ka]:
                return ka, kb
    return None


def check_rule(F, what=''):
    """(a) and (b) on every two of the parses F; -> the number of couples that had a common event"""
    n = 0
    for x in range(len(F)):
        for y in range(x + 1, len(F)):
            A, B = F[x], F[y]
            m = first_common(A, B)
            back = first_common(B, A)
            assert (m is None) == (back is None) and (m is None or m == back[::-1]), (what, x, y, 'the first common event depends on the side', m, back)
            if m is None:
                continue
            ka, kb = m
            n += 1
            at = (what, 'waves', x, y, 'common event', (A.i[ka], A.pos[ka]))
            ta, tb = list(zip(A.i[ka:], A.pos[ka:])), list(zip(B.i[kb:], B.pos[kb:]))
            d = next((d for d, (ea, eb) in enumerate(zip(ta, tb)) if ea != eb), min(len(ta), len(tb)))
            assert ta == tb, (at, '(a) the parses differ behind it, first at', ta[d:d + 1], tb[d:d + 1], 'events left', len(ta) - d, len(tb) - d)
            for name, a, b in (('VM', A.VM, B.VM), ('VA', A.VA, B.VA), ('VN', A.VN, B.VN)):
                d = {(p - q) & M32 for p, q in zip(a[ka:], b[kb:])}
                assert len(d) == 1, (at, '(b) the difference of', name, 'moves', sorted(d)[:4])
            # the rows the two parses end with differ by the same constants
            for name, a, b, k in (('VM', A.VM, B.VM, 0), ('VA', A.VA, B.VA, 1), ('VN', A.VN, B.VN, 2)):
                assert (A.row[k] - B.row[k]) & M32 == (a[ka] - b[kb]) & M32, (at, '(b) the final sums leave the constant', name)
    return n


def phase0_count(P, seg_start, phase_end, probe):
    """how many events of a wave's parse its first phase places (`while (i < phase_end)`): an event belongs to it when
    the probe that finds it starts in front of phase_end"""
    first, after, miss = probe
    pos, width, n = seg_start, first, 0
    for k in range(P.n):
        if pos >= phase_end:
            break
        ei = P.i[k]
        s = pos if ei < pos + width else pos + width + (ei - pos - width) // miss * miss
        if s >= phase_end:
            break
        n += 1
        pos, width = P.end[k], after
    return n


def chain(qlen, F, lz=None, probe=PROBE_KERNEL, cap=SEG_LOG_CAP, reset_cursor=True, looker_ok=True, owner_ok=True):
    """The workgroup restated -> dict(row, visited = the waves the final loop goes through, sync = per wave (owner, index
    in the owner's log) or None, logged = records per wave, n0 = events of the first phase per wave).  cap and
    reset_cursor=False (the cursor keeps its place when the wave crosses into a later segment) restate lookups that MISS
    records: a missed record only delays the hand-over.  looker_ok / owner_ok = False drop one side of the span_ok
    condition: the WRONG schemes a test set must be able to tell from the right one."""
    lim, split, seg_len, starts, ends = geometry(qlen, params(lz)['mal'])
    if not split:
        return dict(row=F[0].row, visited=[0], sync=[None] * WAVES, logged=[0] * WAVES, n0=[F[0].n, 0, 0, 0], seg_len=seg_len)
    n0 = [phase0_count(F[w], starts[w], ends[w], probe) for w in range(WAVES)]
    logged = [min(n0[w], cap) for w in range(WAVES)]
    end, sync = [], []
    for w in range(WAVES):
        P = F[w]
        look_v, look_cur, s = -1, 0, None
        for k in range(n0[w], P.n):
            v = min(WAVES - 1, P.i[k] // seg_len)
            if v != look_v:
                look_v, look_cur = v, (0 if reset_cursor else look_cur)
            L = F[v]
            while look_cur < logged[v] and L.i[look_cur] < P.i[k]:
                look_cur += 1
            if ((P.ok[k] or not looker_ok) and look_cur < logged[v] and L.i[look_cur] == P.i[k] and L.pos[look_cur] == P.pos[k]
                    and (L.ok[look_cur] or not owner_ok)):
                s = (v, look_cur)
                end.append((P.VM[k], P.VA[k], P.VN[k]))
                break
        if s is None:
            end.append(P.row)
        sync.append(s)
    tm = ta = tn = bm = ba = bn = 0
    cur, visited = 0, [0]
    while True:
        tm, ta, tn = (tm + end[cur][0] - bm) & M32, (ta + end[cur][1] - ba) & M32, (tn + end[cur][2] - bn) & M32
        if sync[cur] is None:
            break
        v, k = sync[cur]
        bm, ba, bn = F[v].VM[k], F[v].VA[k], F[v].VN[k]
        cur = v
        visited.append(v)
    return dict(row=(tm, ta, tn), visited=visited, sync=sync, logged=logged, n0=n0, seg_len=seg_len)


def check_pair(Q, R, lz=None, what=''):
    """(a), (b) and (c) of one pair -> (its parses, couples of waves with a common event, the chains under every probe width)"""
    F = parses(Q, R, lz)
    row = orc.lz_pair_stat(Q, R, lz)
    assert F[0].row == row, (what, 'the events call and the ordinary parse disagree', F[0].row, row)
    n = check_rule(F, what)
    chains = {}
    for name, probe in PROBES.items():
        c = chain(len(Q), F, lz, probe)
        assert c['row'] == row, (what, '(c) the chain of hand-overs leaves the oracle row', name, c['row'], row, c['visited'], c['sync'])
        chains[name] = c
    return F, n, chains


# ---- pairs built to reach the arms
def _other(x):
    return ((x + 1) % 4).astype(np.uint8)


def mers(s, k):
    """-> (codes of the k-mers of s, which of them hold no N)"""
    n = len(s) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    c = np.zeros(n, dtype=np.int64)
    for j in range(k):
        c = c * 4 + (s[j:j + n] & 3)
    inv = np.concatenate([[0], np.cumsum(s > 3)])
    return c, (inv[k:] - inv[:-k]) == 0


class Builder:
    """A query laid base for base along the reference R (no indels): query position k lies on position rpos[k] of
    fwd | N | rc.  Every base a construction sets to a mismatch is FREE: done() re-draws free bases until no mal-mer of the
    query that holds one occurs anywhere in R or its reverse complement, and no msl-mer that holds one occurs within NEAR
    positions of its diagonal -- so that the only anchors and seeds are the ones built."""

    def __init__(self, rng, R, rpos, p):
        self.rr = canonical_rr(R)
        self.rpos = np.asarray(rpos, dtype=np.int64)
        base = self.rr[self.rpos]
        self.rng, self.base, self.q, self.p = rng, base, base.copy(), p
        self.near = p['mrd'] + p['mqd'] + p['aw'] + 16
        self.free = np.zeros(len(base), dtype=bool)
        self.blen = p['am'] + 3                                  # consecutive mismatches that stop the approximate extension
        self.isl, self.gap = p['mal'] + 5, p['mqd'] + 1          # an anchor that never spans reg; literals that drop the prediction
        assert self.blen <= p['aw'] and self.blen <= p['mqd'] and self.isl + 2 * p['ar'] < p['reg'] and p['msl'] <= 7 and 9 <= p['mal']
        c, ok = mers(self.rr, p['mal'])
        self.rr_mers = np.unique(c[ok])

    def _miss(self, at, d=1):
        self.q[at] = (self.base[at] + d) % 4
        self.free[at] = True

    def mutate(self, lo, hi, rate=0.04):
        at = lo + np.flatnonzero(self.rng.random(hi - lo) < rate)
        self.q[at] = (self.base[at] + self.rng.integers(1, 4, len(at)).astype(np.uint8)) % 4

    def breaks(self, lo, hi, step=300):
        for b in range(lo + step, hi - self.blen, step):
            self.brk(b)

    def brk(self, b):
        """mismatches over [b, b + blen): the extension stops, the prediction lives, the next match is a new event"""
        self._miss(np.arange(b, b + self.blen))

    def plain(self, lo, hi, step=300):
        self.mutate(lo, hi)
        self.breaks(lo, hi, step)

    def islands(self, lo, n):
        """n times: an island of isl matching bases, then gap bases that all mismatch on the diagonal -> the end"""
        at = lo
        for _ in range(n):
            self.exact(at, at + self.isl)
            self._miss(np.arange(at + self.isl, at + self.isl + self.gap))
            at += self.isl + self.gap
        return at

    def runs8(self, lo, hi, step=300):
        """Runs of 8 matching bases, a substitution every 9th base: seeds (>= msl) for a live prediction, no anchor (< mal)
        for a fresh parse.  Every `step` bases a break, with a whole run on either side."""
        k = (step - self.blen - 8) // 9
        at = lo
        while at + 8 < hi:
            self.exact(at, min(at + k * 9 + 8 + self.blen, hi))
            subs = at + 8 + 9 * np.arange(k)
            self._miss(subs[subs < hi], 2)
            b = at + k * 9 + 8
            self._miss(np.arange(min(b, hi), min(b + self.blen, hi)))
            at = b + self.blen

    def poly(self, lo, hi):
        self.q[lo:hi] = 0
        self.free[lo:hi] = False

    def exact(self, lo, hi):
        self.q[lo:hi] = self.base[lo:hi]
        self.free[lo:hi] = False

    def _redraw(self, windows, k):
        for a in windows.tolist():
            at = a + int(self.rng.choice(np.flatnonzero(self.free[a:a + k])))
            self.q[at] = (self.base[at] + int(self.rng.integers(1, 4))) % 4

    def done(self):
        mal, msl = self.p['mal'], self.p['msl']
        fc = np.concatenate([[0], np.cumsum(self.free)])
        free_a, free_s = (fc[mal:] - fc[:-mal]) > 0, (fc[msl:] - fc[:-msl]) > 0
        rs, rs_ok = mers(self.rr, msl)
        rs = np.where(rs_ok, rs, -1)
        for _ in range(400):
            c, ok = mers(self.q, mal)
            bad = np.flatnonzero(ok & free_a & np.isin(c, self.rr_mers))
            self._redraw(bad, mal)
            c, ok = mers(self.q, msl)
            cand = np.flatnonzero(ok & free_s)
            hit = np.zeros(len(cand), dtype=bool)
            for d in range(-self.near, self.near + 1):
                at = self.rpos[cand] + d
                inside = (at >= 0) & (at < len(rs))
                hit |= inside & (rs[np.clip(at, 0, len(rs) - 1)] == c[cand])
            self._redraw(cand[hit], msl)
            if not len(bad) and not hit.any():
                return self.q
        raise AssertionError('a chance anchor or seed could not be removed')


def _seg(qlen, p):
    return geometry(qlen, p['mal'])[2]


def adversarial_set(lz=None, with_n=False):
    """-> (seqs, cases): cases = [dict(name, q = genome of the query, r = genome of the reference)].  The constructions
    follow the parameters (break, island and gap lengths) and the segment geometry (qlen - mal)."""
    p = params(lz)
    rng = np.random.default_rng(20261021)
    mal = p['mal']
    R = lc.rand_seq(rng, 20000)
    seqs, cases = [R], []

    def add(name, q, r=0):
        seqs.append(q.astype(np.uint8))
        cases.append(dict(name=name, q=len(seqs) - 1, r=r))

    # the split threshold: lim = 8191 (one wave), 8192 (seg_len 2048), 8193 (seg_len 2112, a short last segment)
    for d in (8191, 8192, 8193):
        n = mal + d
        b = Builder(rng, R, 100 + np.arange(n), p)
        b.plain(0, n)
        add(f'threshold_{d}', b.done())
    # islands behind boundary 1: events both parses place, none with span_ok; then plain sequence
    n = mal + 16000
    s = _seg(n, p)
    b = Builder(rng, R, 200 + np.arange(n), p)
    b.plain(0, n)
    end = b.islands(s, 30)
    assert end < 2 * s - 600
    add('islands_30', b.done())
    # a short region across boundary 1: the true parse opened it reg bases in front of the boundary and keeps it, wave 1
    # meets it behind a break, too late to keep it -- the same event in both, span_ok in one
    n = mal + 8300
    s = _seg(n, p)
    b = Builder(rng, R, 250 + np.arange(n), p)
    b.plain(0, n)
    b._miss(np.arange(s - p['reg'] - b.gap, s - p['reg']))
    b.exact(s - p['reg'], s + 5)
    b.brk(s + 5)
    b.exact(s + 5 + b.blen, s + 5 + b.blen + b.isl)
    b._miss(np.arange(s + 5 + b.blen + b.isl, s + 5 + b.blen + b.isl + b.gap))
    b.exact(s + 5 + b.blen + b.isl + b.gap, s + 5 + b.blen + b.isl + b.gap + 80)
    add('short_region_over_boundary_1', b.done())
    # the other way round: the true parse follows one diagonal up to 12 bases behind boundary 1, keeps that region and opens a
    # new one on a far diagonal, which cannot reach back into the kept one; wave 1 opens the same region at the same event and
    # extends it back to the boundary (the reference repeats those 12 bases, but for two, on the far diagonal): span_ok in
    # wave 1, not in the true parse, which drops the region reg - 10 bases later
    n = mal + 8300
    s = _seg(n, p)
    d1, d2, x = 100, 3000, p['reg'] - 10
    rng2 = np.random.default_rng(20261022)          # (a stream of its own: the pairs above and below do not move)
    R2 = lc.rand_seq(rng2, d2 + n + 200)
    at = np.arange(s, s + 12)
    R2[d2 + at] = R2[d1 + at]
    R2[d2 + s + 5], R2[d2 + s + 11] = (R2[d1 + s + 5] + 1) % 4, (R2[d1 + s + 11] + 1) % 4
    at = np.arange(s + 12, s + 12 + 40)
    R2[d1 + at] = (R2[d2 + at] + 1) % 4
    seqs.append(R2)
    r2 = len(seqs) - 1
    b = Builder(rng2, R2, np.concatenate([d1 + np.arange(s + 12), d2 + np.arange(s + 12, n)]), p)
    b.plain(0, n)
    b.exact(s - 60, s + 12 + x)
    b._miss(np.arange(s + 12 + x, s + 12 + x + b.gap))            # ... and the region ends there: the true parse drops it, wave 1 keeps it
    b.exact(s + 12 + x + b.gap, s + 12 + x + b.gap + 80)
    add('region_cut_at_a_kept_one', b.done(), r2)
    # runs of 8 from in front of boundary 1 to behind boundary 2: the true parse chains seeds, wave 1 finds no anchor
    n = mal + 10000
    s = _seg(n, p)
    b = Builder(rng, R, 300 + np.arange(n), p)
    b.plain(0, n)
    b.runs8(s - 400, 2 * s + 400)
    add('runs8_over_segment_1', b.done())
    # nothing to find from in front of boundary 1 to behind boundary 2: no event of either parse in segment 1
    n = mal + 8400
    s = _seg(n, p)
    b = Builder(rng, R, 400 + np.arange(n), p)
    b.plain(0, n)
    b.poly(s - 200, 2 * s + 200)
    add('poly_over_segment_1', b.done())
    # runs of 8 to the query end: wave 0 never meets another parse
    n = mal + 9000
    b = Builder(rng, R, 500 + np.arange(n), p)
    b.exact(0, 60)
    b.runs8(60, n)
    add('runs8_to_the_end', b.done())
    # an event exactly on boundary 1 that matches 2.5 segments exactly; a match across boundary 2 alone
    n = mal + 8200
    s = _seg(n, p)
    b = Builder(rng, R, 600 + np.arange(n), p)
    b.plain(0, n)
    b.exact(s - 50, s + 5 * s // 2)
    b.brk(s - b.blen)
    b.brk(s + 5 * s // 2)
    add('exact_from_boundary_1', b.done())
    b = Builder(rng, R, 700 + np.arange(n), p)
    b.plain(0, n)
    b.exact(s + 500, 2 * s + 700)
    b.brk(s + 500 - b.blen)
    b.brk(2 * s + 700)
    add('exact_across_boundary_2', b.done())
    # strands change at boundary 1, 40 bases in front of boundary 2 and 40 bases behind boundary 3
    j1, j2, j3 = s, 2 * s - 40, 3 * s + 40
    L = len(R)
    b = Builder(rng, R, np.concatenate([800 + np.arange(j1), L + 1 + 3000 + np.arange(j2 - j1), 9000 + np.arange(j3 - j2),
                                        L + 1 + 12000 + np.arange(n - j3)]), p)
    b.mutate(0, n, 0.02)
    for lo, hi in ((0, j1), (j1, j2), (j2, j3), (j3, n)):
        b.breaks(lo + 100, hi - 100, 250)
        b.exact(max(lo, 0), lo + 60)
        b.exact(hi - 60, hi)
    add('strand_joints', b.done())
    # the log cap: 265 islands behind boundary 1 -- more events of wave 1 than its log holds -- then plain sequence
    per = p['mal'] + 5 + p['mqd'] + 1
    n = mal + 4 * (((265 * per + 900) + 63) // 64 * 64) - 100
    s = _seg(n, p)
    RB = lc.rand_seq(rng, n + 400)
    seqs.append(RB)
    rb = len(seqs) - 1
    b = Builder(rng, RB, 150 + np.arange(n), p)
    b.plain(0, n)
    end = b.islands(s, 265)
    assert end + 700 < 2 * s, (end, s)
    b.exact(end, end + 80)
    add('islands_265', b.done(), rb)
    if with_n:
        # one more genome, with N: the whole call goes to the general kernel.  An N run across boundary 2 and one inside a segment
        n = mal + 8500
        s = _seg(n, p)
        b = Builder(rng, R, 900 + np.arange(n), p)
        b.plain(0, n)
        q = b.done()
        q[2 * s - 9:2 * s + 12] = 4
        q[s + 700:s + 705] = 4
        add('n_across_boundary_2', q)
    return seqs, cases


def canonical_rr(R):
    """fwd | N | rc, N = 4"""
    f = np.where(R > 3, 4, R).astype(np.uint8)
    return np.concatenate([f, [4], np.where(f > 3, 4, 3 - f)[::-1]]).astype(np.uint8)


def exact_len(Q, RR, i, j):
    n = min(len(Q) - i, len(RR) - j)
    q = np.where(Q[i:i + n] > 3, 5, Q[i:i + n])
    d = np.flatnonzero(q != RR[j:j + n])
    return int(d[0]) if len(d) else n


ARMS = ('no split below the threshold', 'seg_len 2048 at the threshold', 'seg_len 2112 and a short last segment',
        'immediate hand-over', 'refused by span_ok', 'refused by span_ok of the owner alone', 'refused by span_ok of the looking wave alone', 'late hand-over, log not full', 'log cap', 'a wave is skipped',
        'empty log', 'no hand-over at all', 'event on a boundary', 'exact match across one boundary',
        'exact match across two boundaries', 'strands change at, before and behind a boundary')
ARM_N = 'an N run across a boundary'


def arms_reached(seqs, cases, lz=None, F_of=None):
    """{arm: [names of the pairs that meet its condition]} from the oracle's events alone.  F_of: {name: parses} already
    computed (check_pair)."""
    p = params(lz)
    out = {a: [] for a in ARMS + (ARM_N,)}
    for c in cases:
        Q, R, name = seqs[c['q']], seqs[c['r']], c['name']
        F = F_of[name] if F_of else parses(Q, R, lz)
        lim, split, s, starts, ends = geometry(len(Q), p['mal'])
        E = F[0]
        if not split:
            if lim == WAVES * SPLIT_MIN - 1:
                out['no split below the threshold'].append(name)
            continue
        if lim == 8192 and s == 2048:
            out['seg_len 2048 at the threshold'].append(name)
        if lim == 8193 and s == 2112 and 0 < lim - 3 * s < s:
            out['seg_len 2112 and a short last segment'].append(name)
        chains = [chain(len(Q), F, lz, pr) for pr in PROBES.values()]
        seg_of = lambda i: min(WAVES - 1, i // s)
        immediate = []
        for w in range(1, WAVES):
            Fw = F[w]
            m = first_common(E, Fw)
            inside = [k for k in range(E.n) if seg_of(E.i[k]) == w]
            if m and inside and m[0] == inside[0]:
                immediate.append(w)
            if m and seg_of(E.i[m[0]]) == w:
                shared_before = sum(1 for k in range(m[1]) if seg_of(Fw.i[k]) == w and (Fw.i[k], Fw.pos[k]) in E.at)
                if shared_before >= 20:
                    out['refused by span_ok'].append(name)
                if any(seg_of(Fw.i[k]) == w and not Fw.ok[k] and E.ok[E.at.get((Fw.i[k], Fw.pos[k]), 0)] and (Fw.i[k], Fw.pos[k]) in E.at
                       for k in range(m[1])):
                    out['refused by span_ok of the owner alone'].append(name)
                if any(seg_of(Fw.i[k]) == w and Fw.ok[k] and (Fw.i[k], Fw.pos[k]) in E.at and not E.ok[E.at[(Fw.i[k], Fw.pos[k])]]
                       for k in range(m[1])):
                    out['refused by span_ok of the looking wave alone'].append(name)
                if 20 <= m[1] <= 200:
                    out['late hand-over, log not full'].append(name)
                if m[1] >= 252 and sum(1 for k in range(Fw.n) if Fw.i[k] < (w + 1) * s) >= 252 and w < WAVES - 1:
                    out['log cap'].append(name)
            if not any(seg_of(i) == w for i in Fw.i):
                out['empty log'].append(name)
        if immediate == [1, 2, 3]:
            out['immediate hand-over'].append(name)
        if all(len(c_['visited']) > 1 and c_['visited'][1] >= 2 for c_ in chains):
            out['a wave is skipped'].append(name)
        if all(c_['visited'] == [0] for c_ in chains) and any(seg_of(i) == WAVES - 1 for i in E.i):
            out['no hand-over at all'].append(name)
        if any(i in (s, 2 * s, 3 * s) for i in E.i):
            out['event on a boundary'].append(name)
        RR = canonical_rr(R)
        for k in range(E.n):
            if E.end[k] - E.i[k] > s:
                xl = exact_len(Q, RR, E.i[k], E.pos[k])
                crossed = (E.i[k] + xl - 1) // s - E.i[k] // s
                if s < xl <= 2 * s and crossed == 1:
                    out['exact match across one boundary'].append(name)
                if xl > 2 * s and crossed >= 2:
                    out['exact match across two boundaries'].append(name)
        L = len(R)
        where = set()
        for k in range(1, E.n):
            if E.ok[k - 1] and E.ok[k] and (E.pos[k - 1] > L) != (E.pos[k] > L):
                for B in (s, 2 * s, 3 * s):
                    d = E.i[k] - B
                    if abs(d) <= 64:
                        where.add('at' if d == 0 else 'before' if d < 0 else 'behind')
        if where == {'at', 'before', 'behind'}:
            out['strands change at, before and behind a boundary'].append(name)
        if any(Q[B - 1] > 3 and Q[B] > 3 for B in (s, 2 * s, 3 * s)):
            out[ARM_N].append(name)
    return {a: sorted(set(v)) for a, v in out.items()}
