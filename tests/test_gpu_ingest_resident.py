"""The resident loader's upload pipe with more than one stretch, at a size a test can afford.

`vclust.py prefilter` loads its genomes with the upload overlapped (vg_genomes_load_resident): the set is cut into stretches of
128 M bases, and every stretch travels as soon as its last genome is packed.  A second stretch therefore exists only in sets the
benchmark reaches.  The developer switch VG_INGEST_STRETCH_BASES makes the stretches small: 24 genomes of ~6 kb are 24 stretches at
1 024 bases and 8 stretches at 16 384 (three genomes each, the last one closed by the last genome).  Two members of one family carry
the same run of 30 N at the same offset and no other genome holds an N: one stretch uploads its mask, the others get theirs from
k_mask_of_lengths -- and if the run did not mask, the two runs would pack as equal bases and add shared k-mers.

Expected bytes: fltr.txt by the array-level route in this process -- GenomeSet.load (the host loader, then vg_genomes_to_device),
kmer_shared, write_fltr with the command's defaults --, which never touches the pipe.  A test starts one child process (the --db test two: with and without the switch)."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from vclust_amd import api, synth

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
FAMILIES, MEMBERS, N_DB = 6, 4, 16


@pytest.fixture(scope='module')
def genomes(tmp_path_factory):
    """-> (directory, expected fltr.txt bytes); s.fna = the set, db.fna / new.fna = its first 16 and last 8 genomes"""
    tmp = tmp_path_factory.mktemp('ingest_resident')
    codes, offsets, names = synth.make_families(FAMILIES, MEMBERS, length=6000)
    assert len(names) == FAMILIES * MEMBERS
    codes = codes.copy()
    for g in (2 * MEMBERS + 1, 2 * MEMBERS + 2):             # two members of family 2, the same offset
        codes[offsets[g] + 1500:offsets[g] + 1530] = 4
    assert int(np.count_nonzero(codes > 3)) == 60
    synth.write_fasta(tmp / 's.fna', codes, offsets, names)
    cut = offsets[N_DB]
    synth.write_fasta(tmp / 'db.fna', codes[:cut], offsets[:N_DB + 1], names[:N_DB])
    synth.write_fasta(tmp / 'new.fna', codes[cut:], offsets[N_DB:] - cut, names[N_DB:])
    gs = api.GenomeSet.load([str(tmp / 's.fna')], True, n_threads=4)
    gs.to_device()
    sizes, pairs = gs.kmer_shared(k=25)
    gs.write_fltr(tmp / 'expected.fltr.txt', sizes, pairs)
    del gs
    expected = (tmp / 'expected.fltr.txt').read_bytes()
    rows = expected.decode().splitlines()[1:]
    assert len(rows) == FAMILIES * MEMBERS
    for f in range(FAMILIES):                                # at least one pair inside every family: not equality of empty files
        partners = [int(c.split(':')[0]) - 1 for r in rows[f * MEMBERS:(f + 1) * MEMBERS] for c in r.rstrip(',').split(',')[1:]]
        assert any(p // MEMBERS == f for p in partners), f
    return tmp, expected


def run(args, stretch_bases):
    env = {k: v for k, v in os.environ.items() if k not in ('VG_DEV_SWITCHES', 'VG_INGEST_STRETCH_BASES')}
    if stretch_bases is not None:
        env.update(VG_DEV_SWITCHES='1', VG_INGEST_STRETCH_BASES=str(stretch_bases))
    p = subprocess.run([sys.executable, str(VCLUST), *map(str, args), '-v', '0'], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]


@pytest.mark.parametrize('stretch_bases', [1024, 16384, None])
def test_prefilter_with_small_stretches(genomes, tmp_path, stretch_bases):
    """every genome a stretch of its own; eight stretches of three genomes; one stretch (no switch): the same bytes"""
    tmp, expected = genomes
    out = tmp_path / 'fltr.txt'
    run(['prefilter', '-i', tmp / 's.fna', '-o', out], stretch_bases)
    assert out.read_bytes() == expected


def test_prefilter_db_with_small_stretches(genomes, tmp_path):
    """database + new genomes through the resident loader at 16 384 bases per stretch: the bytes of the same command without the
    switch (which the --db tests hold to the oracle)"""
    tmp, _ = genomes
    small, default = tmp_path / 'small.fltr.txt', tmp_path / 'default.fltr.txt'
    run(['prefilter', '-i', tmp / 'new.fna', '--db', tmp / 'db.fna', '-o', small], 16384)
    run(['prefilter', '-i', tmp / 'new.fna', '--db', tmp / 'db.fna', '-o', default], None)
    assert default.read_bytes().count(b':') > 0
    assert small.read_bytes() == default.read_bytes()
