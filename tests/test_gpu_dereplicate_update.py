"""`dereplicate --db --prior` on the GPU against the three-command route it stands for: prefilter -i new --db db -> align -i new --db db
--filter -> cluster --prior P --algorithm cd-hit, run once per input through the command line.  clusters.tsv must be byte-equal for
every batch size, with and without -r and --prior-repr, and fewer pairs are aligned than the three-command route aligns.
Inputs: the golden example split as property P1 of DESIGN.md section 9 splits it (8 of the 12 genomes are the database, clustered by
`dereplicate`; the other 4 are new), and 8 synthetic families of 5 members of 2-4 kb (found on the CPU with oracle_lib.path_rows):
three members of six families are the database, the other 22 genomes are new.  At tani >= 0.95 that set holds a new genome whose only
passing rows go to prior members (it founds a cluster), a new genome longer than every prior representative, and new near-copies
that match no prior representative."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_update_restatement as cu
from vclust_amd import api, stages, synth

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
GOLDEN_PRIOR = (0, 1, 3, 4, 6, 8, 9, 11)          # 8 of the 12 genomes (the split of test_gpu_cluster_update.py)
FAMILIES, MEMBERS, NEW_FAMILIES, DB_MEMBERS = 8, 5, 2, 3


def run(*args):
    p = subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def _records(fasta):
    return ['>' + r for r in pathlib.Path(fasta).read_text().split('>')[1:]]


class Route:
    """One split input: db.fna, new.fna and all.fna (db, then new); the prior (`dereplicate` of db.fna, with cluster numbers and with
    representative ids); prefilter --db and align --db once; cluster --prior per option set on demand"""

    def __init__(self, records, is_db, work, tani='0.95'):
        self.work = work
        self.db, self.new, self.all = work / 'db.fna', work / 'new.fna', work / 'all.fna'
        self.db.write_text(''.join(r for r, d in zip(records, is_db) if d))
        self.new.write_text(''.join(r for r, d in zip(records, is_db) if not d))
        self.all.write_text(self.db.read_text() + self.new.read_text())
        self.n, self.n_new = len(records), len(records) - sum(is_db)
        self.prior = {False: work / 'prior.tsv', True: work / 'prior_repr.tsv'}
        run('dereplicate', '-i', self.db, '-o', self.prior[False], '--tani', tani, '-v', 0)
        run('dereplicate', '-i', self.db, '-o', self.prior[True], '--tani', tani, '-r', '-v', 0)
        self.fltr, self.ani, self.ids = work / 'fltr.txt', work / 'ani.tsv', work / 'ani.ids.tsv'
        run('prefilter', '-i', self.new, '--db', self.db, '-o', self.fltr, '-v', 0)
        run('align', '-i', self.new, '--db', self.db, '--filter', self.fltr, '-o', self.ani, '-v', 0)
        self.lines = self.ani.read_text().split('\n')[1:-1]
        self._clusters = {}

    def clusters(self, prior_repr, *flags):
        key = (prior_repr, flags)
        if key not in self._clusters:
            out = self.work / f'clusters_{len(self._clusters)}.tsv'
            run('cluster', '-i', self.ani, '--ids', self.ids, '-o', out, '--algorithm', 'cd-hit', '--prior', self.prior[prior_repr],
                *(['--prior-repr'] if prior_repr else []), *flags, '-v', 0)
            self._clusters[key] = out.read_bytes()
        return self._clusters[key]

    def update(self, out, prior_repr=False, **kw):
        """the command under test, in this process"""
        return stages.dereplicate([self.new], out, True, db_paths=[self.db], prior_path=self.prior[prior_repr], prior_repr=prior_repr, **kw)


@pytest.fixture(scope='module')
def golden(golden_dir, tmp_path_factory):
    records = _records(golden_dir / 'multifasta.fna')
    return Route(records, [i in GOLDEN_PRIOR for i in range(len(records))], tmp_path_factory.mktemp('derep_update_golden'))


@pytest.fixture(scope='module')
def families(tmp_path_factory):
    work = tmp_path_factory.mktemp('derep_update_families')
    codes, offsets, names = synth.make_families(FAMILIES, MEMBERS, length_range=(2000, 4000), seed=41, p_lo=0.001, p_hi=0.04, n_indels=1)
    synth.write_fasta(work / 'whole.fna', codes, offsets, names)
    is_db = [i // MEMBERS < FAMILIES - NEW_FAMILIES and i % MEMBERS < DB_MEMBERS for i in range(len(names))]
    return Route(_records(work / 'whole.fna'), is_db, work)


# ---------------------------------------------------------------- the golden example, through the command line
@pytest.mark.parametrize('batch', [1, 2, 3, 4096])
@pytest.mark.parametrize('prior_repr', [False, True])
@pytest.mark.parametrize('representatives', [False, True])
def test_golden_clusters_are_byte_equal_to_the_three_command_route(golden, tmp_path, representatives, prior_repr, batch):
    flags = ['--tani', '0.95'] + (['-r'] if representatives else [])
    out = tmp_path / 'clusters.tsv'
    p = run('dereplicate', '-i', golden.new, '--db', golden.db, '--prior', golden.prior[prior_repr], *(['--prior-repr'] if prior_repr else []),
            '-o', out, '--batch-genomes', batch, *flags)
    assert out.read_bytes() == golden.clusters(prior_repr, *flags), (representatives, prior_repr, batch)
    assert f'--db {golden.db} [1 database + 1 new file(s)] --prior {golden.prior[prior_repr]}' in p.stderr
    update = [line for line in p.stderr.split('\n') if line.startswith('Dereplicate update: ')]
    assert len(update) == 1 and update[0].startswith('Dereplicate update: 8 prior genomes in ') and '; 4 new genomes: ' in update[0]


# ---------------------------------------------------------------- the synthetic set
def _ranks(route):
    """-> (ids in rank order, prior_rep by rank, new ranks)"""
    ids = cr.read_ids(route.ids)
    prior = cu.read_prior(route.prior[True], ids, True)
    return ids, prior, [i for i, p in enumerate(prior) if p < 0]


def test_the_synthetic_input_holds_the_cases(families):
    """asserted on the three-command output itself: the equality tests cannot pass on a degenerate input"""
    ids, prior, news = _ranks(families)
    n = len(ids)
    assert n == FAMILIES * MEMBERS and len(news) == families.n_new == 22
    rows = cr.read_rows(families.ani, n, 'tani', 0, tani=0.95)
    label, rep, st = cu.update_graph(n, rows, prior, 'cd-hit')
    assert cr.clusters_tsv(ids, label, rep) == families.clusters(False, '--tani', '0.95')
    adj = cr.adjacency(n, cu.kept_edges(rows, prior))
    members = {i for i, p in enumerate(prior) if 0 <= p != i}
    assert members
    # a new genome with a passing row to a prior member and none to a representative before it: it founds a cluster
    beside_members = [i for i in news if any(j in members for j in adj[i]) and rep[i] == i]
    assert beside_members
    # a new genome longer than every prior representative
    assert news[0] < min(i for i, p in enumerate(prior) if p == i)
    # new near-copies that match no prior representative: one founds, the other joins it
    assert [i for i in news if rep[i] != i and prior[rep[i]] < 0] and st['joined_new'] > 0 and st['joined_prior'] > 0


@pytest.mark.parametrize('options', ['tani', 'tani -r', 'ani+qcov --prior-repr', 'tani -r --prior-repr'])
def test_families_clusters_are_byte_equal_for_every_batch_size(families, tmp_path, options):
    kw, flags = {'tani': (dict(tani=0.95), ['--tani', '0.95']),
                 'ani+qcov': (dict(metric='ani', ani=0.95, qcov=0.85), ['--metric', 'ani', '--ani', '0.95', '--qcov', '0.85'])}[options.split()[0]]
    representatives, prior_repr = '-r' in options.split(), '--prior-repr' in options.split()
    want = families.clusters(prior_repr, *flags, *(['-r'] if representatives else []))
    three_command_pairs = len(families.lines) // 2
    for batch in (1, 3, 7, families.n_new, 4096):
        out = tmp_path / f'clusters_{batch}.tsv'
        st = families.update(out, prior_repr, batch_genomes=batch, representatives=representatives, **kw)
        assert out.read_bytes() == want, (options, batch)
        assert st['joined_prior'] + st['joined_new'] + st['founded'] == families.n_new
        assert st['prior_objects'] == families.n - families.n_new and st['representatives'] == st['prior_representatives'] + st['founded']
        assert 0 < st['joined_prior_cluster'] <= st['joined_prior'] + st['joined_new']
        assert st['batches'] == -(-families.n_new // batch) and st['pairs_candidate'] == st['pairs_aligned'] + st['pairs_skipped']
        # the point of the command: the pairs (new genome, prior member) are never aligned
        assert st['pairs_aligned'] < three_command_pairs, (options, batch)


def test_a_threshold_equal_to_a_printed_value(families, tmp_path):
    """--tani set to the printed tani of a row that decides the update: the row passes (>=) exactly as in the file route"""
    header = families.ani.read_text().split('\n')[0].split('\t')
    col = header.index('tani')

    def at(t):
        return cu.run(families.ani, families.ids, families.prior[False], 'cd-hit', 'tani', tani=float(t))
    found = None
    for text in sorted({line.split('\t')[col] for line in families.lines}, key=float):
        if not 0 < float(text) < 1 or len(text) != 8:            # a value printed with six decimals
            continue
        above = f'{float(text) + 1e-6:.6f}'
        if at(text) != at(above):
            found = (text, above)
            break
    assert found, 'no row of the ani.tsv decides the update at its own value'
    text, above = found
    want = families.clusters(False, '--tani', text)
    assert want != families.clusters(False, '--tani', above)      # the row matters: one step higher, the clustering differs
    for batch in (1, 5, 4096):
        out = tmp_path / f'clusters_{batch}.tsv'
        families.update(out, batch_genomes=batch, tani=float(text))
        assert out.read_bytes() == want, (text, batch)


def test_an_empty_prior_is_the_plain_command_and_a_full_prior_comes_back(families, tmp_path):
    empty, plain, out = tmp_path / 'empty.tsv', tmp_path / 'plain.tsv', tmp_path / 'clusters.tsv'
    empty.write_text('object\tcluster\n')
    for representatives in (False, True):
        plain_st = stages.dereplicate([families.all], plain, True, batch_genomes=7, tani=0.95, representatives=representatives)
        st = stages.dereplicate([families.new], out, True, db_paths=[families.db], prior_path=empty, batch_genomes=7, tani=0.95,
                                representatives=representatives)
        assert out.read_bytes() == plain.read_bytes()
        assert {k: st[k] for k in plain_st} == plain_st and st['prior_objects'] == st['prior_representatives'] == st['joined_prior_cluster'] == 0
        # ... and the plain command's clusters as the prior of all 40: they come back, and nothing is aligned
        st = stages.dereplicate([families.new], out, True, db_paths=[families.db], prior_path=plain, prior_repr=representatives, batch_genomes=7,
                                tani=0.95, representatives=representatives)
        assert out.read_bytes() == plain.read_bytes()
        assert st['pairs_aligned'] == st['pairs_candidate'] == st['batches'] == st['founded'] == 0
        assert st['prior_objects'] == families.n and st['representatives'] == st['prior_representatives'] == plain_st['representatives']


def test_array_level_equals_the_update_of_the_three_command_rows(families):
    ids, prior, news = _ranks(families)
    n = len(ids)
    rows = cr.read_rows(families.ani, n, 'tani', 0, tani=0.95)
    q, r, w = (np.array(x) for x in zip(*rows))
    want_label, want_rep, want = api.cluster_update_graph(n, q, r, w, prior, 'cd-hit')
    gs, n_db = api.GenomeSet.load_db_new([families.db], [families.new], multisample=True)
    assert [gs.names()[i] for i in gs.align_order()] == ids
    gs.to_device()
    for batch in (1, 4, 4096):
        label, rep, st, (tasks, stats) = gs.dereplicate_set(batch_genomes=batch, tani=0.95, want_rows=True, n_db=n_db, prior_rep=prior)
        assert label.tolist() == want_label.tolist() and rep.tolist() == want_rep.tolist()
        assert st['joined_prior_cluster'] == want['joined_prior'] and st['founded'] == want['founded']
        assert st['joined_prior'] + st['joined_new'] == want['joined_prior'] + want['joined_new']
        assert len(tasks) == len(stats) == 2 * st['pairs_aligned']
        # the rows are rows of the whole task list of the combined set, in its order; none names a prior member, none two prior genomes
        order = gs.align_order()
        rank = {int(g): i for i, g in enumerate(order)}
        members = {i for i, p in enumerate(prior) if 0 <= p != i}
        pairs = np.array([(max(int(t['q']), int(t['r'])), min(int(t['q']), int(t['r'])), 0) for t in tasks[::2]], dtype=api.PAIR_DTYPE)
        assert tasks.tolist() == gs.align_tasks(pairs).tolist()
        for t in tasks:
            a, b = rank[int(t['q'])], rank[int(t['r'])]
            assert a not in members and b not in members and (prior[a] < 0 or prior[b] < 0)
        if batch == 4096:
            assert stats.tolist() == gs.lz_align(tasks).tolist()
    gs.close()


def test_every_output_of_the_command_line(families, tmp_path):
    out, table, fasta = tmp_path / 'clusters.tsv', tmp_path / 'rows.tsv', tmp_path / 'repr.fna'
    p = run('dereplicate', '-i', families.new, '--db', families.db, '--prior', families.prior[True], '--prior-repr', '-o', out, '--tani', '0.95',
            '-r', '--batch-genomes', 5, '--out-table', table, '--out-repr-fasta', fasta)
    assert out.read_bytes() == families.clusters(True, '--tani', '0.95', '-r')
    # the table: the combined set's ids, rows that the three-command table holds too, in its order
    assert (tmp_path / 'rows.ids.tsv').read_bytes() == families.ids.read_bytes()
    text = table.read_text().split('\n')
    assert text[0] == families.ani.read_text().split('\n')[0] and text[-1] == '' and len(text) > 2
    it = iter(families.lines)
    assert all(line in it for line in text[1:-1])
    # the records of the representatives, verbatim: those of --db first, each in input order
    reps = {line.split('\t')[1] for line in out.read_text().split('\n')[1:] if line}
    assert fasta.read_text() == ''.join(r for r in _records(families.all) if r[1:].split()[0] in reps)
    summary = [line for line in p.stderr.split('\n') if line.startswith('Dereplicate: ')]
    assert len(summary) == 1 and f'{len(reps)} representatives' in summary[0]
