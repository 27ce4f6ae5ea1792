"""Markov clustering on the MI355X (vg_cluster_mcl_graph, vg_cluster_mcl, `cluster --algorithm mcl`) against the sequential restatement
(tests/mcl_restatement.py).  The definition is integer arithmetic throughout, so everything must be EQUAL: labels, representatives,
the iteration count, the convergence flag, the chaos of the last iteration and the matrix itself after 1, 2 and 3 iterations and at
the stop -- on the LDS path and, with the table shrunk to 64 slots, on the spill path; and at the default table of 4 096 slots
on graphs whose rows exceed it (mcl_cases.table_size_cases)."""
import pathlib
import subprocess
import sys

import pytest

import cluster_restatement as cr
import mcl_cases
import mcl_restatement as mr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
VCLUST = ROOT / 'vclust.py'
CASES = mcl_cases.all_cases()
DEFAULT_SLOTS, SMALL_SLOTS = 4096, 64
_TRACES, _FIGURES = {}, {}
TABLE_CASES = mcl_cases.table_size_cases()


def run(*args, timeout=300):
    return subprocess.run([sys.executable, str(VCLUST), *map(str, args)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=timeout)


@pytest.fixture(scope='module')
def out_dir(golden_dir):
    return golden_dir / 'output'


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


def _trace(name, n, rows, params):
    """the restatement's iterates of a case, computed once: (edges, start matrix, trace)"""
    if name not in _TRACES:
        e = cr.edges(rows)
        _TRACES[name] = (e, mr.start(n, e), mr.trace(n, e, **params))
    return _TRACES[name]


def _spill_rows(name, start, trace, iterations, slots):
    """rows whose candidate bound (the sum of nnz over the rows they name, at most the number of objects) exceeds the table AND whose
    distinct candidate columns fill more than 3/4 of it, over the matrices that were expanded (mcl_cases.predict, once per case
    and table)"""
    if (name, slots) not in _FIGURES:
        _FIGURES[name, slots] = mcl_cases.predict(start, trace, len(trace), slots)
    return sum(f['spilled'] for f in _FIGURES[name, slots][:iterations])


def _check(api, name, n, rows, params, slots=DEFAULT_SLOTS, limits=(1, 2, 3, None)):
    """the library against the restatement after 1, 2, 3 iterations and at the stop; -> the stats of the full run"""
    e, start, trace = _trace(name, n, rows, params)
    q, r, w = ([x[k] for x in rows] for k in range(3))
    stats = None
    for limit in limits:
        want = trace[min(limit or len(trace), len(trace)) - 1]
        kw = dict(params, max_iterations=limit) if limit else params
        label, rep, stats, (off, col, val) = api.cluster_mcl_graph(n, q, r, w, matrix=True, **kw)
        what = f'{name}, max_iterations={limit}, {slots} slots'
        assert (stats['iterations'], stats['converged'], stats['chaos']) == (want['iterations'], want['converged'], want['chaos']), what
        assert (off.tolist(), col.tolist(), val.tolist()) == mr.csr(want['matrix']), what
        want_label, want_rep = cr.labels(mr.components(n, want['matrix']))
        assert label.tolist() == want_label and rep.tolist() == want_rep, what
        assert stats['n_edges'] == len(e) and stats['nnz'] == len(col) and stats['max_row_seen'] == max(len(x) for x in want['matrix']), what
        spill = _spill_rows(name, start, trace, want['iterations'], slots)
        assert stats['spill_rows'] == spill and stats['lds_rows'] == n * want['iterations'] - spill, what
        # without the matrix outputs the call gives the same clusters
        label2, rep2, stats2 = api.cluster_mcl_graph(n, q, r, w, **kw)
        assert label2.tolist() == want_label and rep2.tolist() == want_rep and stats2 == stats, what
    return stats


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_equal_to_the_restatement(api, case):
    stats = _check(api, *case)
    assert stats['converged'] == 1 and stats['iterations'] <= 27 and stats['spill_rows'] == 0


def test_bridge_and_planted_partition(api):
    n, rows = mcl_cases.bridged_cliques()
    q, r, w = ([x[k] for x in rows] for k in range(3))
    label, rep, stats = api.cluster_mcl_graph(n, q, r, w)
    assert label.tolist() == [0] * 6 + [1] * 6 and rep.tolist() == [0] * 6 + [6] * 6
    assert api.cluster_graph(n, q, r, w, 'single')[0].tolist() == [0] * 12
    n, rows = mcl_cases.planted()
    label, rep, stats = api.cluster_mcl_graph(n, *([x[k] for x in rows] for k in range(3)))
    assert label.tolist() == [i // 8 for i in range(n)] and stats['converged'] == 1


def test_selection_goes_by_column_on_ties(api):
    for distinct in (False, True):
        n, rows = mcl_cases.hub(distinct)
        q, r, w = ([x[k] for x in rows] for k in range(3))
        label, rep, stats, (off, col, val) = api.cluster_mcl_graph(n, q, r, w, max_row=8, max_iterations=1, matrix=True)
        assert col[off[0]:off[1]].tolist() == list(range(8)) and stats['max_row_seen'] <= 8, distinct


def test_the_spill_path_gives_the_same(api):
    """the table shrunk to 64 slots: rows above that bound go through the sorted records, and nothing changes"""
    spilled = 0
    api.cluster_mcl_set_table_slots(SMALL_SLOTS)
    try:
        for case in CASES:
            spilled += _check(api, *case, slots=SMALL_SLOTS, limits=(1, 3, None))['spill_rows']
    finally:
        api.cluster_mcl_set_table_slots(0)
    assert spilled > 0
    name, n, rows, params = next(c for c in CASES if c[0] == 'widths')
    assert _check(api, name, n, rows, params, limits=(None,))['spill_rows'] == 0         # (the default is back)


@pytest.mark.parametrize('case', [c for c in TABLE_CASES if c[4] == DEFAULT_SLOTS], ids=[c[0] for c in TABLE_CASES if c[4] == DEFAULT_SLOTS])
def test_rows_above_the_real_table(api, case):
    """The default table of 4 096 slots: rows whose bound exceeds it are tried in it and kept up to 3 072 distinct columns, given to
    the spill path from 3 073; the select of the finish over thousands of candidates, in LDS and in a spill row's global segment.
    That the case does so is read off the restatement first (mcl_cases.reaches_its_path)."""
    name, n, rows, params, slots, expected = case
    e, start, trace = _trace(name, n, rows, params)
    figures = mcl_cases.reaches_its_path(case, start, trace)
    stats = _check(api, name, n, rows, params, limits=(None,))
    assert stats['spill_rows'] == sum(f['spilled'] for f in figures) and stats['iterations'] == len(figures)
    if 'widest' in expected:
        assert stats['max_row_seen'] == expected['widest']


def test_two_spill_batches(api):
    """One iteration whose spill rows need more records than are sorted at once (2^25): the batch loop takes a second trip.  The
    table is shrunk to 64 slots, or no graph of seconds would spill that much; the restatement does the same 5 x 10^7 products,
    which is what this test costs."""
    case = next(c for c in TABLE_CASES if c[4] == SMALL_SLOTS)
    name, n, rows, params, slots, expected = case
    e, start, trace = _trace(name, n, rows, params)
    figures = mcl_cases.reaches_its_path(case, start, trace)
    assert max(f['records'] for f in figures) > 1 << 25 and max(f['records'] for f in figures) < 1 << 26
    api.cluster_mcl_set_table_slots(SMALL_SLOTS)
    try:
        stats = _check(api, name, n, rows, params, slots=SMALL_SLOTS, limits=(None,))
    finally:
        api.cluster_mcl_set_table_slots(0)
    assert stats['spill_rows'] == sum(f['spilled'] for f in figures) == 2 * n and stats['converged'] == 1


def test_not_converged_is_still_a_result(api):
    n, rows = mcl_cases.path()
    stats = _check(api, 'path', n, rows, {}, limits=(1,))
    assert stats['converged'] == 0 and stats['iterations'] == 1
    assert _check(api, 'path', n, rows, {}, limits=(None,))['iterations'] == 57


def test_other_parameters(api):
    n, rows = mcl_cases.random_graph(130, 7)
    for k, params in enumerate((dict(prune=0.0, max_row=2), dict(prune=0.1, inflation=6.0), dict(chaos_eps=0.0, inflation=4.5, max_iterations=60),
                                dict(chaos_eps=0.5, inflation=2.5))):
        _check(api, f'parameters {k}', n, rows, params, limits=(1, None))


def test_cli_on_the_golden_example(api, out_dir, tmp_path):
    base = ['cluster', '-i', out_dir / 'ani.tsv', '--ids', out_dir / 'ani.ids.tsv', '--algorithm', 'mcl', '--tani', '0.7']
    for extra, representatives in (([], False), (['-r'], True)):
        out = tmp_path / f'c{int(representatives)}.tsv'
        p = run(*base, *extra, '-o', out)
        assert p.returncode == 0 and '--algorithm mcl --mcl-inflation 2' in p.stderr and 'MCL: ' in p.stderr and 'WARNING' not in p.stderr, p.stderr
        assert out.read_bytes() == mr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tani=0.7, representatives=representatives)
        assert ' 4 clusters' in p.stderr, p.stderr
    out, stats = tmp_path / 'c.tsv', tmp_path / 's.tsv'
    p = run(*base, '--mcl-inflation', '3.5', '--mcl-iterations', '1', '-o', out, '--out-stats', stats)
    assert p.returncode == 0 and p.stderr.count('Running: ') == 2 and p.stderr.count('Completed') == 2 and 'did not converge' in p.stderr, p.stderr
    assert out.read_bytes() == mr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tani=0.7, mcl_params=dict(inflation=3.5, max_iterations=1))
    blocks = {ln.split('\t')[0] for ln in stats.read_text().split('\n')[1:] if ln}
    assert blocks == {'cluster'}
    # the file call returns the stats
    got = api.cluster(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tmp_path / 'f.tsv', algorithm='mcl', tani=0.95, mcl_max_row=16)
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    want = mr.iterate(len(ids), cr.edges(cr.read_rows(out_dir / 'ani.tsv', len(ids), 'tani', tani=0.95)), max_row=16)
    assert (got['iterations'], got['converged'], got['chaos']) == (want['iterations'], want['converged'], want['chaos'])
    assert (tmp_path / 'f.tsv').read_bytes() == mr.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', tani=0.95, mcl_params=dict(max_row=16))
