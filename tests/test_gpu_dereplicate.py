"""`dereplicate` on the GPU against the three-step path it stands for: prefilter -> align --filter -> cluster --algorithm cd-hit,
run once per input through the command line.  clusters.tsv must be byte-equal for every batch size, the table of computed rows a
subsequence of the three-step ani.tsv, and on a redundant input fewer pairs are aligned than the three-step path aligns.
Inputs: the 12 genomes of the golden example, and 6 synthetic families of 8 members of 3 kb whose mutation rates (found on the CPU
with oracle_lib.path_rows) give, at tani >= 0.95, clusters of three and more, several clusters, and genomes that found a cluster
although they have a passing row to an earlier genome -- that genome is a member, not a representative: the case of the lemma."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
from vclust_amd import api, stages, synth

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
OPTIONS = {
    'tani': (dict(tani=0.95), ['--tani', '0.95']),
    'ani+qcov': (dict(metric='ani', ani=0.95, qcov=0.85), ['--metric', 'ani', '--ani', '0.95', '--qcov', '0.85']),
    'tani -r': (dict(tani=0.95, representatives=True), ['--tani', '0.95', '-r']),
}


def run(*args):
    p = subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


class ThreeStep:
    """prefilter and align of one input, once; cluster per option set on demand"""

    def __init__(self, fasta, work):
        self.fasta, self.work = fasta, work
        self.fltr, self.ani, self.ids = work / 'fltr.txt', work / 'ani.tsv', work / 'ani.ids.tsv'
        run('prefilter', '-i', fasta, '-o', self.fltr)
        run('align', '-i', fasta, '-o', self.ani, '--filter', self.fltr)
        self.lines = self.ani.read_text().split('\n')[1:-1]
        self.n = len(self.ids.read_text().split('\n')) - 2
        self._clusters = {}

    def clusters(self, *flags):
        if flags not in self._clusters:
            out = self.work / f'clusters_{len(self._clusters)}.tsv'
            run('cluster', '-i', self.ani, '--ids', self.ids, '-o', out, '--algorithm', 'cd-hit', *flags)
            self._clusters[flags] = out.read_bytes()
        return self._clusters[flags]


@pytest.fixture(scope='module')
def inputs(golden_dir, tmp_path_factory):
    work = tmp_path_factory.mktemp('derep')
    codes, offsets, names = synth.make_families(6, 8, length=3000, seed=41, p_lo=0.001, p_hi=0.04, n_indels=1)
    synth.write_fasta(work / 'families.fna', codes, offsets, names)
    out = {}
    for key, fasta in (('golden', golden_dir / 'multifasta.fna'), ('families', work / 'families.fna')):
        (work / key).mkdir()
        out[key] = ThreeStep(fasta, work / key)
    return out


def _batches(n):
    return (1, 3, 5, n, n + 7)


def test_the_synthetic_input_is_the_case_of_the_lemma(inputs):
    """asserted on the three-step output itself: the equality tests cannot pass on a degenerate input"""
    ts = inputs['families']
    rows = cr.read_rows(ts.ani, ts.n, 'tani', 0, tani=0.95)
    label, rep = cr.cluster_graph(ts.n, rows, 'cd-hit')
    assert cr.clusters_tsv(cr.read_ids(ts.ids), label, rep) == ts.clusters('--tani', '0.95')
    sizes = np.bincount(rep, minlength=ts.n)
    assert (sizes >= 3).sum() >= 1 and (sizes >= 1).sum() >= 2
    adj = cr.adjacency(ts.n, cr.edges(rows))
    founders_beside_members = [i for i in range(ts.n) if any(j < i for j in adj[i]) and all(rep[j] != j for j in adj[i])]
    assert founders_beside_members and all(rep[i] == i for i in founders_beside_members)


@pytest.mark.parametrize('options', list(OPTIONS))
@pytest.mark.parametrize('key', ['golden', 'families'])
def test_clusters_are_byte_equal_for_every_batch_size(inputs, tmp_path, key, options):
    ts = inputs[key]
    kw, flags = OPTIONS[options]
    want = ts.clusters(*flags)
    for batch in _batches(ts.n):
        out = tmp_path / f'clusters_{batch}.tsv'
        st = stages.dereplicate([ts.fasta], out, True, batch_genomes=batch, **kw)
        assert out.read_bytes() == want, (key, options, batch)
        assert st['joined_prior'] + st['joined_new'] + st['founded'] == ts.n
        assert st['founded'] == st['representatives'] and st['batches'] == -(-ts.n // batch)
        assert st['pairs_candidate'] == st['pairs_aligned'] + st['pairs_skipped']
        assert st['pairs_aligned'] <= len(ts.lines) // 2


def test_a_threshold_equal_to_a_printed_value(inputs, tmp_path):
    """--tani set to the printed tani of a row that decides the clustering: the row passes (>=) exactly as in the file route"""
    ts = inputs['golden']
    header = ts.ani.read_text().split('\n')[0].split('\t')
    col = header.index('tani')
    ids = cr.read_ids(ts.ids)

    def at(t):
        return cr.clusters_tsv(ids, *cr.cluster_graph(ts.n, cr.read_rows(ts.ani, ts.n, 'tani', 0, tani=float(t)), 'cd-hit'))
    found = None
    for text in sorted({line.split('\t')[col] for line in ts.lines}, key=float):
        if not 0 < float(text) < 1 or len(text) != 8:            # a value printed with six decimals
            continue
        above = f'{float(text) + 1e-6:.6f}'
        if at(text) != at(above):
            found = (text, above)
            break
    assert found, 'no row of the golden ani.tsv decides the clustering at its own value'
    text, above = found
    want = ts.clusters('--tani', text)
    assert want != ts.clusters('--tani', above)                   # the row matters: one step higher, the clustering differs
    for batch in (1, 5, ts.n):
        out = tmp_path / f'clusters_{batch}.tsv'
        run('dereplicate', '-i', ts.fasta, '-o', out, '--tani', text, '--batch-genomes', batch)
        assert out.read_bytes() == want, (text, batch)


@pytest.mark.parametrize('key', ['golden', 'families'])
def test_the_table_is_a_subsequence_of_the_three_step_table(inputs, tmp_path, key):
    ts = inputs[key]
    for batch in (3, ts.n + 7):
        table = tmp_path / f'ani_{batch}.tsv'
        st = stages.dereplicate([ts.fasta], tmp_path / 'c.tsv', True, batch_genomes=batch, tani=0.95, out_table=table)
        assert (tmp_path / f'ani_{batch}.ids.tsv').read_bytes() == ts.ids.read_bytes()
        text = table.read_text().split('\n')
        assert text[0] == ts.ani.read_text().split('\n')[0] and text[-1] == ''
        lines = text[1:-1]
        assert st['pairs_aligned'] * 2 == len(lines)
        it = iter(ts.lines)
        assert all(line in it for line in lines)                  # every line occurs, in the same relative order
        if batch >= ts.n:
            assert st['pairs_aligned'] <= len(ts.lines) // 2
        elif key == 'families':
            assert st['pairs_aligned'] < len(ts.lines) // 2 and st['pairs_skipped'] > 0


def test_command_line_with_every_output(inputs, tmp_path):
    ts = inputs['families']
    out, table, fasta = tmp_path / 'clusters.tsv', tmp_path / 'rows.tsv', tmp_path / 'repr.fna'
    p = run('dereplicate', '-i', ts.fasta, '-o', out, '--tani', '0.95', '-r', '--batch-genomes', 5, '--out-table', table, '--outfmt', 'lite',
            '--out-repr-fasta', fasta)
    assert out.read_bytes() == ts.clusters('--tani', '0.95', '-r')
    assert 'Running: libvclust_gpu dereplicate' in p.stderr and 'Completed' in p.stderr
    summary = [line for line in p.stderr.split('\n') if line.startswith('Dereplicate: ')]
    assert len(summary) == 1 and summary[0].startswith(f'Dereplicate: {ts.n} genomes, ') and 'batches' in summary[0]
    assert table.read_text().split('\n')[0] == 'qidx\tridx\ttani\tgani\tani\tqcov\trcov\tnum_alns\tlen_ratio'
    # the records of the representatives, verbatim, in input order
    reps = {line.split('\t')[1] for line in out.read_text().split('\n')[1:] if line}
    records = ['>' + r for r in ts.fasta.read_text().split('>')[1:]]
    assert fasta.read_text() == ''.join(r for r in records if r[1:].split()[0] in reps)
    assert f'{len(reps)} representatives' in summary[0]
    quiet = run('dereplicate', '-i', ts.fasta, '-o', out, '--tani', '0.95', '-v', 0)
    assert 'Dereplicate:' not in quiet.stderr


@pytest.mark.parametrize('key', ['golden', 'families'])
def test_array_level_equals_cluster_graph_on_the_three_step_rows(inputs, key):
    ts = inputs[key]
    gs = api.GenomeSet.load([ts.fasta], multisample=True)
    gs.to_device()
    sizes, pairs = gs.kmer_shared(k=25, min_shared=20)
    kept = gs.filter_pairs(sizes, pairs)
    rows = cr.read_rows(ts.ani, ts.n, 'tani', 0, tani=0.95)
    q, r, w = (np.array(x) for x in zip(*rows))
    want_label, want_rep, _ = api.cluster_graph(ts.n, q, r, w, 'cd-hit')
    for batch in (1, 4, ts.n):
        label, rep, st, (tasks, stats) = gs.dereplicate_set(batch_genomes=batch, tani=0.95, want_rows=True)
        assert label.tolist() == want_label.tolist() and rep.tolist() == want_rep.tolist()
        assert st['joined_prior'] + st['joined_new'] + st['founded'] == ts.n
        assert len(tasks) == len(stats) == 2 * st['pairs_aligned'] and st['pairs_aligned'] <= len(kept)
        # the rows are those of the whole task list
        all_tasks = gs.align_tasks(kept)
        index = {(int(t['q']), int(t['r'])): i for i, t in enumerate(all_tasks)}
        pos = [index[(int(t['q']), int(t['r']))] for t in tasks]
        assert pos == sorted(pos)
        if batch == ts.n:
            full = gs.lz_align(all_tasks)
            assert stats.tolist() == full[pos].tolist()
    gs.close()
