"""The deduplicate stage on the GPU against the sequential restatement (tests/dedup_restatement.py) and the fixture's
README.txt: the CLI on the fixture (plain, gzip and BGZF inputs, gzip output), random sets through vg_dedup_seqs, forced
hash collisions, a long record, a 10^5-record file and a deduplicate -> prefilter -> align -> cluster run."""
import gzip
import pathlib
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import dedup_restatement as dr
from test_dedup_cpu import EXPECTED_DUPLICATES, EXPECTED_IDS, INPUTS

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'


def run(*args, timeout=600):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


def bgzf(data: bytes) -> bytes:
    """bgzip's format: gzip members of <= 64 KiB carrying their size in a 'BC' extra field, then the empty EOF member."""
    out = bytearray()
    for k in range(0, len(data) + 1, 60000):
        chunk = data[k:k + 60000]
        if not chunk and k:
            break
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        cdata = co.compress(chunk) + co.flush()
        out += struct.pack('<4BI2BH2BHH', 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, ord('B'), ord('C'), 2, len(cdata) + 25)
        out += cdata + struct.pack('<II', zlib.crc32(chunk), len(chunk))
    out += bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
    return bytes(out)


def expected(paths):
    fasta, dup, _ = dr.run(paths, dr.default_prefixes(paths))
    return fasta, dup


def test_cli_on_the_fixture(api, tmp_path):
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *INPUTS, '-o', out, '--add-prefixes', '-v', '1')
    assert p.returncode == 0, p.stderr
    fasta, dup = expected(INPUTS)
    assert out.read_bytes() == fasta
    assert [ln.split()[0][1:] for ln in out.read_text().splitlines() if ln.startswith('>')] == EXPECTED_IDS
    assert (tmp_path / 'nr.fna.duplicates.txt').read_text() == EXPECTED_DUPLICATES == dup.decode()
    summary = [ln for ln in p.stderr.splitlines() if 'vg_deduplicate:' in ln]
    assert len(summary) == 1 and '15 records, 7 unique, 8 removed (1 as reverse complements), 0 hash collisions' in summary[0], p.stderr


def test_gzip_output_does_not_depend_on_threads(api, tmp_path):
    fasta, dup = expected(INPUTS)
    members = []
    for t in (1, 16):
        out = tmp_path / f't{t}' / 'nr.fna'
        out.parent.mkdir()
        p = run('deduplicate', '-i', *INPUTS, '-o', out, '--add-prefixes', '--gzip-output', '--gzip-level', '5', '-t', t, '-v', '0')
        assert p.returncode == 0 and p.stderr == '', p.stderr
        gz = out.parent / 'nr.fna.gz'
        assert not out.exists() and gzip.decompress(gz.read_bytes()) == fasta
        assert (out.parent / 'nr.fna.gz.duplicates.txt').read_bytes() == dup
        members.append(gz.read_bytes())
    assert members[0] == members[1]


@pytest.mark.parametrize('kind', ['plain', 'gzip', 'bgzf'])
def test_plain_and_compressed_inputs(api, tmp_path, kind):
    paths = []
    for p in INPUTS:
        data = dr.read_text(p)
        q = tmp_path / (p.stem if kind == 'plain' else p.name)       # refseq.fna / refseq.fna.gz
        q.write_bytes({'plain': lambda d: d, 'gzip': gzip.compress, 'bgzf': bgzf}[kind](data))
        paths.append(q)
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', *paths, '-o', out, '--add-prefixes', '-v', '0')
    assert p.returncode == 0, p.stderr
    fasta, dup = expected(INPUTS)
    assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
    assert dr.run(paths, dr.default_prefixes(paths))[0] == fasta


def test_file_layout_is_copied_verbatim(api, tmp_path):
    """CR LF line ends, ragged and blank lines, lower case, no final newline, an empty record, text before the first '>'."""
    a = tmp_path / 'a.fna'
    a.write_bytes(b';comment\n>x1 first\r\nACGTN\r\nacg\r\n\r\n>x2\n>x3 rc of x1\ncgtnacgt\n>x4\nAC GT\tNA-CG\n>x5\nRYKM')
    b = tmp_path / 'b.fna.gz'
    b.write_bytes(gzip.compress(b'>y1\n\n>y2 palindrome\nACGT\n>y3\nacgt\n>y4\nKMRY\n>y5\nrykm\n'))
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', a, b, '-o', out, '--add-prefixes', 'A:', 'B:', '-v', '0')
    assert p.returncode == 0, p.stderr
    fasta, dup, _ = dr.run([a, b], ['A:', 'B:'])
    assert out.read_bytes() == fasta and (tmp_path / 'nr.fna.duplicates.txt').read_bytes() == dup
    assert b'A:x1\tA:x3\t-\n' in dup and b'A:x2\tB:y1\t+\n' in dup and b'B:y2\tB:y3\t+\n' in dup
    assert b'A:x5\tB:y4\t-\n' in dup and b'A:x5\tB:y5\t+\n' in dup and fasta.endswith(b'>A:x5\nRYKM\n>B:y2 palindrome\nACGT\n')


def check_seqs(api, seqs):
    rep, strand, st = api.deduplicate(seqs)
    erep, estrand = dr.run_seqs(seqs)
    assert rep.tolist() == erep and strand.tolist() == estrand
    assert st['records'] == len(seqs) and st['unique'] == sum(r == i for i, r in enumerate(erep))
    assert st['removed'] == len(seqs) - st['unique']
    assert st['reverse'] == sum(s for i, s in enumerate(estrand) if erep[i] != i)
    return st


SYMBOLS = np.frombuffer(b'ACGTRYSWKMBDHVN-', dtype=np.uint8)


def random_set(rng, n, lengths, iupac=False):
    seqs = []
    for _ in range(n):
        L = int(rng.choice(lengths))
        alpha = SYMBOLS if iupac else SYMBOLS[:4]
        s = alpha[rng.integers(0, len(alpha), L)].tobytes()
        r = rng.random()
        if seqs and r < 0.45:                   # a copy of an earlier one: exact, reverse complement, lower case
            src = dr.normalise(seqs[int(rng.integers(0, len(seqs)))])
            s = [src, dr.revcomp(src), src.lower(), dr.revcomp(src).lower()][int(rng.integers(0, 4))]
        elif r < 0.5:                           # a palindrome
            s = s[:L // 2] + dr.revcomp(s[:L // 2])
        seqs.append(s)
    return seqs


@pytest.mark.parametrize('seed', range(4))
def test_random_sets_equal_restatement(api, seed):
    rng = np.random.default_rng(seed)
    # every length mod 8, 0- and 1-symbol records, short and multi-chunk lengths
    lengths = list(range(0, 40)) + [63, 64, 65, 127, 128, 129, 1000, 16383, 16384, 16385, 16391, 40000]
    seqs = random_set(rng, 1500, lengths, iupac=seed % 2 == 1)
    check_seqs(api, seqs)


def test_hubs_and_iupac_heavy(api):
    rng = np.random.default_rng(11)
    base = SYMBOLS[rng.integers(0, 16, 777)].tobytes()
    hub = [base] * 500 + [dr.revcomp(base)] * 250 + [base.lower()] * 250          # 1 000 records of one group
    other = SYMBOLS[rng.integers(0, 16, 778)].tobytes()
    seqs = [other] + hub + [b'', b'', b'N', b'n', b'-', b'A', b'T', b'a'] + [other.lower(), dr.revcomp(other)] + hub[:10]
    st = check_seqs(api, seqs)
    assert st['unique'] == 6          # other, the hub, empty, N / n, '-', A / T / a


@pytest.mark.parametrize('bits', [0, 8])
def test_forced_collisions(api, bits):
    rng = np.random.default_rng(bits)
    seqs = random_set(rng, 400, [0, 1, 7, 8, 9, 31, 32, 33, 500, 16390], iupac=True)
    try:
        api.dedup_set_hash_bits(bits)
        st = check_seqs(api, seqs)
        assert st['collisions'] > 0 and st['rounds'] > 1, st
    finally:
        api.dedup_set_hash_bits(128)
    st = check_seqs(api, seqs)
    assert st['collisions'] == 0 and st['rounds'] == 1


def test_long_record_and_its_reverse_complement(api):
    rng = np.random.default_rng(3)
    s = SYMBOLS[:4][rng.integers(0, 4, 50_000_003)].tobytes()
    rc = dr.revcomp(s)
    near = s[:-1] + (b'A' if s[-1:] != b'A' else b'C')         # differs in the last symbol only
    rep, strand, st = api.deduplicate([s, near, rc, s])
    assert rep.tolist() == [0, 1, 0, 0] and strand.tolist() == [0, 0, 1, 0]
    assert st['reverse'] == 1 and st['collisions'] == 0


@pytest.mark.slow
def test_hundred_thousand_records(api, tmp_path):
    sys.path.insert(0, str(ROOT / 'tools'))
    import dedup_timing as dt
    fna = tmp_path / 'big.fna'
    exp = dt.make_redundant(fna, 100_000, 40_000)
    out = tmp_path / 'nr.fna'
    p = run('deduplicate', '-i', fna, '-o', out, '-t', '16', '-v', '1', timeout=1200)
    assert p.returncode == 0, p.stderr
    removed = exp['copies']
    assert f"100000 records, {100_000 - removed} unique, {removed} removed ({exp['reverse']} as reverse complements)" in p.stderr, p.stderr
    dup = (tmp_path / 'nr.fna.duplicates.txt').read_text().splitlines()[1:]
    assert len(dup) == removed
    rng = np.random.default_rng(0)
    for line in [dup[int(k)] for k in rng.integers(0, len(dup), 200)]:
        r, d, strand = line.split('\t')
        i, j = int(d[1:]), int(r[1:])
        assert exp['source'][i] == j
        assert strand == ('-' if exp['kind'][i] == 1 else '+')
    heads = [ln for ln in out.read_bytes().split(b'\n') if ln.startswith(b'>')]
    assert len(heads) == 100_000 - removed


def test_pipeline_from_deduplicate_to_cluster(api, tmp_path):
    nr = tmp_path / 'nr.fna'
    assert run('deduplicate', '-i', *INPUTS, '-o', nr, '--add-prefixes', '-v', '0').returncode == 0
    p = run('prefilter', '-i', nr, '-o', tmp_path / 'fltr.txt', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    p = run('align', '-i', nr, '-o', tmp_path / 'ani.tsv', '--filter', tmp_path / 'fltr.txt', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    ids = (tmp_path / 'ani.ids.tsv').read_text().splitlines()[1:]
    assert sorted(ln.split('\t')[0] for ln in ids) == sorted(EXPECTED_IDS)
    p = run('cluster', '-i', tmp_path / 'ani.tsv', '--ids', tmp_path / 'ani.ids.tsv', '-o', tmp_path / 'clusters.tsv',
            '--tani', '0.95', '-v', '0')
    assert p.returncode == 0 and p.stderr == '', p.stderr
    rows = (tmp_path / 'clusters.tsv').read_text().splitlines()
    assert rows[0] == 'object\tcluster' and sorted(r.split('\t')[0] for r in rows[1:]) == sorted(EXPECTED_IDS)
