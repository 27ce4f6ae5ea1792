"""The deduplicate stage's circular mode ("Circular mode") as plain sequential Python: the yardstick
of vg_deduplicate_ex and vg_dedup_seqs_ex.  Everything not restated here is dedup_restatement's.

- rot(X, s)[i] = X[(i + s) mod L].  Two records of the same length L are circular duplicates when one equals rot(other, s)
  or rot(revcomp(other), s) for some s in [0, L).  All empty records form one group.
- The earliest record of a group is kept.
- Strand of a removed record: '+' if it equals some rotation of the kept record, '-' if it equals only rotations of the
  kept record's reverse complement.
- Offset: the smallest s with removed == rot(Y, s), Y the kept sequence for '+' and its reverse complement for '-'.

rot(Y, s) for s in [0, L) are exactly the length-L substrings of Y + Y that start below L, and bytes.find returns the smallest
index, so (Y + Y).find(record) is the contract's offset (a match of a length-L record in Y + Y never starts at L unless
it also starts at 0).
"""
import dedup_restatement as dr
from dedup_restatement import normalise, revcomp


def rot(seq: bytes, s: int) -> bytes:
    return seq[s:] + seq[:s]


def group(seqs, circular=True):
    """(representative, strand, offset) of normalised sequences, records visited in input order against the kept records
    of their length: forward strands of all kept records first, then their reverse complements."""
    if not circular:
        rep, strand = dr.group(seqs)
        return rep, strand, [0] * len(seqs)
    kept = {}                     # length -> indices of the kept records, in input order
    rep, strand, offset = [], [], []
    for i, s in enumerate(seqs):
        ks = kept.setdefault(len(s), [])
        found = None
        if len(s) == 0:
            if ks:
                found = (ks[0], 0, 0)
        else:
            for k in ks:
                at = (seqs[k] + seqs[k]).find(s)
                if at >= 0:
                    found = (k, 0, at)
                    break
            if found is None:
                for k in ks:
                    rc = revcomp(seqs[k])
                    at = (rc + rc).find(s)
                    if at >= 0:
                        found = (k, 1, at)
                        break
        if found is None:
            ks.append(i)
            found = (i, 0, 0)
        rep.append(found[0])
        strand.append(found[1])
        offset.append(found[2])
    return rep, strand, offset


def run(paths, prefixes=None, circular=True):
    """-> (output FASTA bytes, duplicates file bytes, (representative, strand, offset)) of deduplicating the files `paths`;
    circular=False gives dedup_restatement.run's bytes."""
    if not circular:
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


def run_seqs(seqs, circular=True):
    """vg_dedup_seqs_ex's answer for a list of str / bytes sequences."""
    return group([normalise(s.encode() if isinstance(s, str) else bytes(s)) for s in seqs], circular)
