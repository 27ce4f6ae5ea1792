"""`vclust.py prefilter --db` / `align --db` on a real GPU, against the reference's golden example split at run time into its first
8 records (the database) and its last 4 (the new genomes): the files must be the golden all-vs-all files restricted to the pairs that
contain a new genome."""
import collections
import pathlib
import re
import subprocess
import sys

import pytest

from test_new2all_cpu import N_DB_EXAMPLE, write_split

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
GOLD = ROOT / 'tests' / 'golden' / 'example' / 'output'


def run(*args):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('new2all_cli')
    return tmp, write_split(tmp)


def _inputs(tmp, mode):
    return (tmp / 'new.fna', tmp / 'db.fna') if mode == 'file' else (tmp / 'new', tmp / 'db')


def _plain_names(text, mode):
    """directory mode calls a genome `<2 digits>_<record name>` (test_new2all_cpu.write_split): take the numbers off"""
    return re.sub(r'(?<![\w.])\d\d_(?=NC_)', '', text) if mode == 'dir' else text


def _golden_fltr():
    rows = (GOLD / 'fltr.txt').read_text().splitlines()
    return rows[:1] + [r.split(',')[0] + ',' for r in rows[1:1 + N_DB_EXAMPLE]] + rows[1 + N_DB_EXAMPLE:]


def _golden_filter_pairs(names):
    """the pairs {name, name} of the golden filter's rows of the new genomes"""
    out = set()
    for row in _golden_fltr()[1 + N_DB_EXAMPLE:]:
        cells = row.rstrip(',').split(',')
        out |= {frozenset((cells[0], names[int(c.split(':')[0]) - 1])) for c in cells[1:]}
    return out


@pytest.mark.parametrize('mode', ['file', 'dir'])
def test_prefilter_db_writes_the_golden_rows_of_the_new_genomes(split, tmp_path, mode):
    tmp, names = split
    inp, db = _inputs(tmp, mode)
    out = tmp_path / 'fltr.txt'
    p = run('prefilter', '-i', inp, '--db', db, '-o', out)
    assert p.returncode == 0, p.stderr
    assert 'Running' in p.stderr and f'--db {db}' in p.stderr and 'Completed' in p.stderr
    want = _golden_fltr()
    assert sum(1 for r in want[1:] if not r.endswith(',') or r.count(',') > 1) == 3        # three new genomes have partners
    assert _plain_names(out.read_text(), mode) == '\n'.join(want) + '\n'


@pytest.mark.parametrize('mode', ['file', 'dir'])
def test_align_db_with_the_filter(split, tmp_path, mode):
    """ids file: all 12 genomes, byte for byte.  ani.tsv: the golden rows of the filter's pairs -- each names a new genome --, in the
    golden order.  --out-aln: the golden regions of those rows, as a multiset."""
    tmp, names = split
    inp, db = _inputs(tmp, mode)
    flt, ani, aln = tmp_path / 'fltr.txt', tmp_path / 'ani.tsv', tmp_path / 'ani.aln.tsv'
    assert run('prefilter', '-i', inp, '--db', db, '-o', flt, '-v', '0').returncode == 0
    p = run('align', '-i', inp, '--db', db, '--filter', flt, '-o', ani, '--out-aln', aln, '-v', '0')
    assert p.returncode == 0, p.stderr
    assert _plain_names((tmp_path / 'ani.ids.tsv').read_text(), mode) == (GOLD / 'ani.ids.tsv').read_text()
    pairs = _golden_filter_pairs(names)
    new = set(names[N_DB_EXAMPLE:])
    assert len(pairs) == 4 and all(pair & new for pair in pairs)
    assert any(pair <= new for pair in pairs) and any(len(pair & new) == 1 for pair in pairs)
    gold = (GOLD / 'ani.tsv').read_text().splitlines()
    want = gold[:1] + [r for r in gold[1:] if frozenset(r.split('\t')[2:4]) in pairs]
    assert len(want) == 1 + 2 * len(pairs)
    assert _plain_names(ani.read_text(), mode).splitlines() == want
    gold_aln = (GOLD / 'ani.aln.tsv').read_text().splitlines()
    want_aln = collections.Counter(r for r in gold_aln[1:] if frozenset(r.split('\t')[:2]) in pairs)
    mine = _plain_names(aln.read_text(), mode).splitlines()
    assert mine[0] == gold_aln[0] and collections.Counter(mine[1:]) == want_aln and sum(want_aln.values()) > 100


@pytest.mark.parametrize('mode', ['file', 'dir'])
def test_align_db_without_a_filter(split, tmp_path, mode):
    """every pair that contains a new genome: the rows of the all-vs-all align that name one of the four -- the run's own and the
    golden file's (which is an all-vs-all run) --, in their order."""
    tmp, names = split
    inp, db = _inputs(tmp, mode)
    ani, full = tmp_path / 'ani.tsv', tmp_path / 'full' / 'ani.tsv'
    full.parent.mkdir()
    assert run('align', '-i', inp, '--db', db, '-o', ani, '-v', '0').returncode == 0
    assert _plain_names((tmp_path / 'ani.ids.tsv').read_text(), mode) == (GOLD / 'ani.ids.tsv').read_text()
    whole = ROOT / 'tests' / 'golden' / 'example' / 'multifasta.fna'
    assert run('align', '-i', whole, '-o', full, '-v', '0').returncode == 0
    new = set(names[N_DB_EXAMPLE:])
    mine = _plain_names(ani.read_text(), mode).splitlines()
    for ref in (full.read_text().splitlines(), (GOLD / 'ani.tsv').read_text().splitlines()):
        want = ref[:1] + [r for r in ref[1:] if set(r.split('\t')[2:4]) & new]
        assert len(want) == 1 + 2 * (12 * 11 // 2 - 8 * 7 // 2)
        assert mine == want
