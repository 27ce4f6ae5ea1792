"""The deduplicate stage's contained mode ("Contained mode") as plain sequential Python: the yardstick
of vg_deduplicate_contained and vg_dedup_seqs_contained.  Everything not restated here is dedup_restatement's.

- X is contained in Y when len X <= len Y and X is a contiguous substring of Y or of revcomp(Y).  Sequences are linear
  (no wrap-around) and symbols compare literally (N equals only N).  Empty records are contained in nothing; all empty
  records form one group, its earliest record kept.
- A non-empty record i is removed when some record j with len j > len i contains it, or an earlier record of the same
  length equals it or its reverse complement.
- Representative of a removed record: among the kept records that contain it, the longest; of several, the earliest.
- Strand: '+' if the record occurs in the representative, '-' if it occurs only in the representative's reverse complement.
- Offset: the smallest s with Y[s : s + len] == record, Y the representative for '+' and its reverse complement for '-'
  (bytes.find returns the smallest index).
"""
import dedup_restatement as dr
from dedup_restatement import normalise, revcomp


def contains(y: bytes, y_rc: bytes, x: bytes) -> bool:
    return len(x) <= len(y) and (x in y or x in y_rc)


def group(seqs, contained=True):
    """(representative, strand, offset) of normalised sequences."""
    n = len(seqs)
    if not contained:
        rep, strand = dr.group(seqs)
        return rep, strand, [0] * n
    rc = [revcomp(s) for s in seqs]
    removed = []
    for i, x in enumerate(seqs):
        removed.append(len(x) > 0 and any(
            (len(seqs[j]) > len(x) or (len(seqs[j]) == len(x) and j < i)) and contains(seqs[j], rc[j], x) for j in range(n) if j != i))
    empties = [i for i, x in enumerate(seqs) if len(x) == 0]
    rep, strand, offset = [], [], []
    for i, x in enumerate(seqs):
        if len(x) == 0:
            rep.append(empties[0])
            strand.append(0)
            offset.append(0)
            continue
        if not removed[i]:
            rep.append(i)
            strand.append(0)
            offset.append(0)
            continue
        holders = [j for j in range(n) if j != i and not removed[j] and contains(seqs[j], rc[j], x)]
        assert holders, 'containment is transitive: a removed record has a kept container'
        j = min(holders, key=lambda k: (-len(seqs[k]), k))
        at = seqs[j].find(x)
        rep.append(j)
        strand.append(0 if at >= 0 else 1)
        offset.append(at if at >= 0 else rc[j].find(x))
    return rep, strand, offset


def run(paths, prefixes=None, contained=True):
    """-> (output FASTA bytes, duplicates file bytes, (representative, strand, offset)) of deduplicating the files `paths`;
    contained=False gives dedup_restatement.run's bytes."""
    if not contained:
        fasta, dup, (rep, strand) = dr.run(paths, prefixes)
        return fasta, dup, (rep, strand, [0] * len(rep))
    prefixes = [p.encode() if isinstance(p, str) else p for p in (prefixes or [b''] * len(paths))]
    recs, seqs = [], []
    for f, path in enumerate(paths):
        text = dr.read_text(path)
        for hdr, raw, at in dr.records(text):
            seqs.append(normalise(raw, dr._line_of(path, text, at)))
            recs.append((f, hdr, raw))
    rep, strand, offset = group(seqs)
    fasta = bytearray()
    for i, (f, hdr, raw) in enumerate(recs):
        if rep[i] != i:
            continue
        fasta += b'>' + prefixes[f] + hdr + b'\n' + raw
        if raw and not raw.endswith(b'\n'):
            fasta += b'\n'
    ident = [prefixes[f] + dr.first_token(hdr) for f, hdr, _ in recs]
    dup = bytearray(b'representative\tduplicate\tstrand\toffset\n')
    for i in range(len(recs)):
        if rep[i] != i:
            dup += ident[rep[i]] + b'\t' + ident[i] + b'\t' + (b'-' if strand[i] else b'+') + b'\t%d\n' % offset[i]
    return bytes(fasta), bytes(dup), (rep, strand, offset)


def run_seqs(seqs, contained=True):
    """vg_dedup_seqs_contained's answer for a list of str / bytes sequences."""
    return group([normalise(s.encode() if isinstance(s, str) else bytes(s)) for s in seqs], contained)
