"""Terminal repeats of the deduplicate stage's circular mode ("Terminal repeats") as plain sequential
Python: the yardstick of vg_dedup_terminal_repeats, vg_dedup_seqs_circular_tr and vg_deduplicate_circular_tr.  Everything
not restated here is dedup_circular_restatement's and dedup_restatement's.

- tr(X, m): the largest t with m <= t <= len(X) // 2 and X[:t] == X[len(X) - t:], 0 when there is none.  Symbols compare
  literally after normalisation (upper case, no white space): N equals only N.  Borders above half the length are not looked at.
- circ(X) = X[:len(X) - tr(X, m)].
- Two records are duplicates when their circles are circular duplicates (same circle length, a rotation of the other circle or
  of its reverse complement).  The earliest record of a group is kept; strand and offset are the circular mode's over circles.
- The output FASTA is the circular mode's (kept records verbatim, repeat included); the duplicates file has the columns
  representative, duplicate, strand, offset, repeat, representative_repeat.
"""
import dedup_circular_restatement as dcr
import dedup_restatement as dr
from dedup_restatement import normalise


def tr(seq: bytes, m: int) -> int:
    """The terminal repeat of a normalised sequence for the minimum m >= 1."""
    assert m >= 1
    L = len(seq)
    for t in range(L // 2, m - 1, -1):
        if seq[:t] == seq[L - t:]:
            return t
    return 0


def circ(seq: bytes, m: int) -> bytes:
    return seq[:len(seq) - tr(seq, m)]


def group(seqs, m):
    """(representative, strand, offset, repeat) of normalised sequences: the circular group over the circles."""
    repeat = [tr(s, m) for s in seqs]
    rep, strand, offset = dcr.group([s[:len(s) - t] for s, t in zip(seqs, repeat)])
    return rep, strand, offset, repeat


def run(paths, prefixes, m):
    """-> (output FASTA bytes, duplicates file bytes, (representative, strand, offset, repeat)) of deduplicating the files
    `paths` with --circular --terminal-repeat m."""
    prefixes = [p.encode() if isinstance(p, str) else p for p in (prefixes or [b''] * len(paths))]
    recs, seqs = [], []
    for f, path in enumerate(paths):
        text = dr.read_text(path)
        for hdr, raw, at in dr.records(text):
            seqs.append(normalise(raw, dr._line_of(path, text, at)))
            recs.append((f, hdr, raw))
    rep, strand, offset, repeat = group(seqs, m)
    fasta = bytearray()
    for i, (f, hdr, raw) in enumerate(recs):
        if rep[i] != i:
            continue
        fasta += b'>' + prefixes[f] + hdr + b'\n' + raw
        if raw and not raw.endswith(b'\n'):
            fasta += b'\n'
    ident = [prefixes[f] + dr.first_token(hdr) for f, hdr, _ in recs]
    dup = bytearray(b'representative\tduplicate\tstrand\toffset\trepeat\trepresentative_repeat\n')
    for i in range(len(recs)):
        if rep[i] != i:
            dup += (ident[rep[i]] + b'\t' + ident[i] + b'\t' + (b'-' if strand[i] else b'+')
                    + b'\t%d\t%d\t%d\n' % (offset[i], repeat[i], repeat[rep[i]]))
    return bytes(fasta), bytes(dup), (rep, strand, offset, repeat)


def run_seqs(seqs, m):
    """vg_dedup_seqs_circular_tr's answer for a list of str / bytes sequences."""
    return group([normalise(s.encode() if isinstance(s, str) else bytes(s)) for s in seqs], m)
