"""The deduplicate stage's contract as plain sequential Python: the yardstick of vg_deduplicate and
vg_dedup_seqs.  Nothing here is fast; everything here is meant to be obviously the definition.

- Records: every FASTA record of every input, in command-line order and then file order (bytes before a file's first
  '>' at the start of a line belong to no record).  Header line = the record's first line without '>', sequence lines =
  everything up to the next record.
- Sequence: the sequence lines without white space (space, tab, CR, LF); the alphabet is ACGTRYSWKMBDHVN and '-',
  case-insensitive.
- Duplicates: equal sequences, or one equal to the reverse complement of the other.  The earliest record of a group is kept.
- Strand of a removed record: '+' if it equals the kept record, '-' if it equals only the kept record's reverse complement.
"""
import gzip
import pathlib
import re

ALPHABET = set(b'ACGTRYSWKMBDHVN-')
COMPLEMENT = bytes.maketrans(b'ACGTRYKMBVDHSWN-', b'TGCAYRMKVBHDSWN-')
WHITE = b' \t\r\n'
NL = b'\n'


class NotIupac(ValueError):
    pass


def revcomp(seq: bytes) -> bytes:
    """Reverse complement of an upper-case sequence (IUPAC: A-T, C-G, R-Y, K-M, B-V, D-H; S, W, N, '-' unchanged)."""
    return seq.translate(COMPLEMENT)[::-1]


def normalise(raw: bytes, where=lambda k: k) -> bytes:
    """The sequence of raw sequence lines: white space dropped, upper case; a byte outside the alphabet raises NotIupac
    with where(offset of the byte in raw) in front of the message."""
    seq = raw.translate(None, WHITE).upper()
    if not set(seq) <= ALPHABET:
        for k, ch in enumerate(raw):
            if ch not in WHITE and bytes([ch]).upper()[0] not in ALPHABET:
                raise NotIupac(f"{where(k)}: '{chr(ch)}' is not an IUPAC nucleotide code")
    return seq


def group(seqs):
    """(representative, strand) of normalised sequences: representative[i] = earliest j equal to seqs[i] or to its
    reverse complement; strand[i] = 0 if seqs[i] == seqs[rep], 1 if it equals only the reverse complement."""
    first = {}
    rep, strand = [], []
    for i, s in enumerate(seqs):
        j = first.get(s)
        if j is None:
            j = first.get(revcomp(s))
        if j is None:
            first[s] = i
            rep.append(i)
            strand.append(0)
        else:
            rep.append(j)
            strand.append(0 if seqs[j] == s else 1)
    return rep, strand


def read_text(path) -> bytes:
    data = pathlib.Path(path).read_bytes()
    return gzip.decompress(data) if data[:2] == b'\x1f\x8b' else data


def records(text: bytes):
    """[(header line, raw sequence lines, offset of the sequence lines in text)] of one file."""
    starts = [m.start() for m in re.finditer(rb'(?m)^>', text)]
    out = []
    for a, b in zip(starts, starts[1:] + [len(text)]):
        nl = text.find(b'\n', a, b)
        hdr_end, seq_at = (nl, nl + 1) if nl >= 0 else (b, b)
        out.append((text[a + 1:hdr_end], text[seq_at:b], seq_at))
    return out


def first_token(header: bytes) -> bytes:
    k = 0
    while k < len(header) and header[k] not in b' \t\r':
        k += 1
    return header[:k]


def default_prefixes(paths):
    """A bare --add-prefixes: `<file stem before the first '.'>|` per file (validate_args_deduplicate)."""
    return [pathlib.Path(p).stem.split('.')[0] + '|' for p in paths]


def _line_of(path, text, at):
    return lambda k: f'{path}:{text.count(NL, 0, at + k) + 1}'


def run(paths, prefixes=None):
    """-> (output FASTA bytes, duplicates file bytes, (representative, strand)) of deduplicating the files `paths`."""
    prefixes = [p.encode() if isinstance(p, str) else p for p in (prefixes or [b''] * len(paths))]
    recs, seqs = [], []
    for f, path in enumerate(paths):
        text = read_text(path)
        for hdr, raw, at in records(text):
            seqs.append(normalise(raw, _line_of(path, text, at)))
            recs.append((f, hdr, raw))
    rep, strand = group(seqs)
    fasta = bytearray()
    for i, (f, hdr, raw) in enumerate(recs):
        if rep[i] != i:
            continue
        fasta += b'>' + prefixes[f] + hdr + b'\n' + raw
        if raw and not raw.endswith(b'\n'):
            fasta += b'\n'
    ident = [prefixes[f] + first_token(hdr) for f, hdr, _ in recs]
    dup = bytearray(b'representative\tduplicate\tstrand\n')
    for i in range(len(recs)):
        if rep[i] != i:
            dup += ident[rep[i]] + b'\t' + ident[i] + b'\t' + (b'-' if strand[i] else b'+') + b'\n'
    return bytes(fasta), bytes(dup), (rep, strand)


def run_seqs(seqs):
    """vg_dedup_seqs' answer for a list of str / bytes sequences."""
    return group([normalise(s.encode() if isinstance(s, str) else bytes(s)) for s in seqs])
