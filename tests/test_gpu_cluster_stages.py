"""The launch structure of every array-level cluster call, read from the profile table (one entry per scope name, `launches` =
how often the scope was opened): one graph build per call, the rounds of each algorithm, one labelling exit, and the scopes that
never open under an algorithm.  The counts are equalities against the stats the call returns; where a count is not a function
of the stats, the constant is the one the commit before the host-side reshaping showed for that input.  Results are held to
the restatements."""
import numpy as np
import pytest

import average_restatement as ar
import cluster_restatement as cr
import cluster_stats_restatement as cs
import cluster_update_restatement as cu
import complete_restatement as cl
import linkage_restatement as lr
import mcl_restatement as mr

pytestmark = pytest.mark.gpu

BUILD = ('cluster_edges_emit', 'cluster_edges_sort', 'cluster_edges_merge', 'cluster_csr')
LEVELS = (0.95, 0.85)


@pytest.fixture(scope='module')
def api():
    from vclust_amd import api as a
    if a.device_count() < 1:
        pytest.skip('needs a HIP device')
    return a


@pytest.fixture
def slots(api):
    yield api.cluster_mcl_set_table_slots
    api.cluster_mcl_set_table_slots(0)


def profiled(api, call):
    """-> (what call() returns, {scope name: launches})"""
    api.profile_enable(True)
    api.profile_reset()
    try:
        out = call()
        scopes = {e['name']: e['launches'] for e in api.profile_get()}
    finally:
        api.profile_enable(False)
    print(scopes, next((x for x in (out if isinstance(out, tuple) else ()) if isinstance(x, dict)), ''))
    return out, scopes


def columns(rows):
    return tuple([x[k] for x in rows] for k in range(3))


def family_graph():
    """525 objects in 40 cliques of 6 to 20 (index order), every weight distinct in (0.8, 1); a weak bridge of distinct weight
    below 0.6 between neighbouring cliques at every fifth, one self row, one duplicated row and one reversed row of another weight"""
    rng = np.random.default_rng(21)
    sizes = [6 + (7 * k) % 15 for k in range(40)]
    start = np.concatenate([[0], np.cumsum(sizes)])
    pairs = [(int(a), int(b)) for k, s in enumerate(sizes) for a in range(start[k], start[k] + s) for b in range(a + 1, start[k] + s)]
    weight = 0.8 + 0.2 * (rng.permutation(len(pairs)) + 1) / (len(pairs) + 1)
    rows = [(a, b, float(x)) if (a + b) % 3 else (b, a, float(x)) for (a, b), x in zip(pairs, weight)]
    rows += [(int(start[k + 1]) - 1, int(start[k + 1]), 0.5 + 0.002 * k) for k in range(0, 39, 5)]
    rows += [(5, 5, 0.9), rows[3], (rows[4][1], rows[4][0], 0.7)]
    return int(start[-1]), [rows[int(k)] for k in rng.permutation(len(rows))]


def path_graph(n):
    return n, [(i, i + 1, 0.9) for i in range(n - 1)]


@pytest.fixture(scope='module')
def family():
    return family_graph()


def check_build(scopes, n_edges):
    """the one graph build of a call with rows, and the scopes around it"""
    assert [scopes.get(name) for name in BUILD] == [1, 1, 1, 1] and n_edges > 0


def check_only(scopes, *prefixes):
    """no scope but the build, the labels and those that start with one of the prefixes"""
    other = [name for name in scopes if name not in BUILD + ('cluster_labels',) and not name.startswith(prefixes)]
    assert not other, other


@pytest.mark.parametrize('algorithm', ['single', 'cd-hit', 'uclust', 'set-cover', 'complete'])
def test_partition_stages(api, family, algorithm):
    n, rows = family
    (label, rep, st), scopes = profiled(api, lambda: api.cluster_graph(n, *columns(rows), algorithm))
    want = cl.cluster_ids(n, rows) if algorithm == 'complete' else cr.cluster_ids(n, cr.edges(rows), algorithm)
    assert (label.tolist(), rep.tolist()) == cr.labels(want)
    check_build(scopes, st['n_edges'])
    assert scopes['cluster_labels'] == 1 and st['n_edges'] == len(cr.edges(rows))
    if algorithm == 'single':
        assert scopes['cluster_hook'] == scopes['cluster_compress'] == st['rounds'] and st['rounds'] % 4 == 0
        check_only(scopes, 'cluster_hook', 'cluster_compress')
    elif algorithm == 'complete':
        # every round but the last merges: the loop ends at the first round without a merge
        assert scopes['cluster_rank'] == 1 and scopes['cluster_complete_best'] == st['rounds'] == scopes['cluster_complete_contract'] + 1
        assert 'cluster_forest' not in scopes               # (the floor cut fetches no merge records)
        check_only(scopes, 'cluster_rank', 'cluster_complete_')
    else:
        stem = {'cd-hit': 'cluster_cdhit', 'uclust': 'cluster_uclust', 'set-cover': 'cluster_setcover'}[algorithm]
        assert scopes[stem + '_round'] == st['rounds'] >= 1
        assert scopes.get(stem + '_sweep', 0) == (st['sweep_objects'] > 0)
        check_only(scopes, stem + '_round', stem + '_sweep')


# The sweep starts when a round decides fewer than 4096 objects and fewer than 1 % of those left; a round on a path in index
# order decides a handful.  PATH = 512 is the smallest power of two at which the parent commit swept under all three algorithms
# (at 128 and 256 cd-hit and uclust swept and set-cover did not), and SWEPT its sweep_objects there: the first round decides one
# object, or three, and hands over the rest.
PATH = 512
SWEPT = {'cd-hit': 511, 'uclust': 511, 'set-cover': 509}


@pytest.mark.parametrize('algorithm', ['cd-hit', 'uclust', 'set-cover'])
def test_tail_sweep_stages(api, algorithm):
    n, rows = path_graph(PATH)
    (label, rep, st), scopes = profiled(api, lambda: api.cluster_graph(n, *columns(rows), algorithm))
    assert (label.tolist(), rep.tolist()) == cr.labels(cr.cluster_ids(n, cr.edges(rows), algorithm))
    stem = {'cd-hit': 'cluster_cdhit', 'uclust': 'cluster_uclust', 'set-cover': 'cluster_setcover'}[algorithm]
    check_build(scopes, st['n_edges'])
    assert st['sweep_objects'] > 0 and st['sweep_objects'] == SWEPT[algorithm]
    assert scopes[stem + '_round'] == st['rounds'] and scopes[stem + '_sweep'] == 1 and scopes['cluster_labels'] == 1
    check_only(scopes, stem + '_round', stem + '_sweep')


def as_rows(table):
    return [tuple(x) for x in table[['node_a', 'node_b', 'similarity', 'size', 'object_a', 'object_b']].tolist()]


@pytest.mark.parametrize('algorithm', ['single', 'complete', 'average'])
def test_table_and_cut_stages(api, family, algorithm):
    """the merge table and the cuts at two levels: each call builds the graph once and opens the scopes of its hierarchy alone"""
    n, rows = family
    table_call = {'single': api.cluster_linkage, 'complete': api.cluster_complete_linkage_graph,
                  'average': lambda *a: api.cluster_average_linkage_graph(*a, floor=0.6)}[algorithm]
    cuts_call = {'single': api.cluster_levels, 'complete': api.cluster_complete_levels_graph,
                 'average': lambda *a: api.cluster_average_levels_graph(*a, floor=0.6)}[algorithm]
    if algorithm == 'average':                              # (the restatement's merges once for the table and the cuts)
        merges = ar.merges(n, cr.edges(rows), 0.6)
        want_table, want_cuts = ar.table(n, merges), [cr.labels(ar.cut(n, merges, t)) for t in LEVELS]
    else:
        mod = lr if algorithm == 'single' else cl
        want_table, want_cuts = mod.linkage(n, rows), mod.levels(n, rows, LEVELS)
    (table, st), scopes = profiled(api, lambda: table_call(n, *columns(rows)))
    (label, rep, st2), scopes2 = profiled(api, lambda: cuts_call(n, *columns(rows), LEVELS))
    assert as_rows(table) == want_table and st == st2 and st['n_merges'] == len(want_table)
    assert [(a.tolist(), b.tolist()) for a, b in zip(label, rep)] == want_cuts
    for sc in (scopes, scopes2):
        check_build(sc, st['n_edges'])
        assert 'cluster_labels' not in sc                   # (the cuts are numbered on the host)
        if algorithm == 'single':
            assert sc['cluster_rank'] == 1 and sc['cluster_boruvka'] == st['rounds'] and sc['cluster_forest'] == 1
            check_only(sc, 'cluster_rank', 'cluster_boruvka', 'cluster_forest')
        elif algorithm == 'complete':
            assert sc['cluster_rank'] == 1 and sc['cluster_forest'] == 1
            assert sc['cluster_complete_best'] == st['rounds'] == sc['cluster_complete_contract'] + 1
            check_only(sc, 'cluster_rank', 'cluster_forest', 'cluster_complete_')
        else:
            # the floor is above 0: no zero phase, every round but the last merges; the records are sorted on the host
            assert sc['cluster_average_best'] == st['rounds'] == sc['cluster_average_contract'] + 1
            check_only(sc, 'cluster_average_')


def test_average_zero_phase_has_one_idle_round(api):
    """floor 0 and rows of weight 0: when a round finds no merge above 0 the zero phase begins with a round that contracts
    nothing, and the last round finds nothing either -- two rounds of `best` without a contraction"""
    n = 24
    rows = [(a, b, 0.9 - 0.01 * a - 0.001 * b) for k in range(0, n, 4) for a in range(k, k + 4) for b in range(a + 1, k + 4)]
    rows += [(3, 4, 0.0), (7, 8, 0.0), (11, 12, 0.0), (19, 20, 0.0)]
    (table, st), scopes = profiled(api, lambda: api.cluster_average_linkage_graph(n, *columns(rows), floor=0.0))
    assert as_rows(table) == ar.linkage(n, rows, 0.0) and st['n_merges'] == len(table) > 18
    check_build(scopes, st['n_edges'])
    assert scopes['cluster_average_best'] == st['rounds'] == scopes['cluster_average_contract'] + 2
    check_only(scopes, 'cluster_average_')


# cluster_mcl_expand_wave / _group open in an iteration that has rows of that class: a function of the input.  The counts are the
# parent commit's (wave, group) for family_graph() at the default table, where every row is a wave's in all 15 iterations, and at
# 16 slots, where the rows above the table go to the workgroup kernel as long as there are any.
EXPAND = {0: (15, 0), 16: (7, 11)}


@pytest.fixture(scope='module')
def family_trace(family):
    n, rows = family
    e = cr.edges(rows)
    return e, mr.trace(n, e)


@pytest.mark.parametrize('table_slots', [0, 16])
def test_mcl_stages(api, slots, family, family_trace, table_slots):
    n, rows = family
    e, trace = family_trace
    want = trace[-1]
    slots(table_slots)
    (label, rep, st, (off, col, val)), scopes = profiled(api, lambda: api.cluster_mcl_graph(n, *columns(rows), matrix=True))
    (label2, rep2, st2), scopes2 = profiled(api, lambda: api.cluster_mcl_graph(n, *columns(rows)))
    assert (st['iterations'], st['converged'], st['chaos']) == (want['iterations'], want['converged'], want['chaos'])
    assert (off.tolist(), col.tolist(), val.tolist()) == mr.csr(want['matrix'])
    assert (label.tolist(), rep.tolist()) == (label2.tolist(), rep2.tolist()) == cr.labels(mr.components(n, want['matrix'])) and st == st2
    assert scopes.pop('cluster_mcl_matrix') == 1 and scopes == scopes2
    check_build(scopes, st['n_edges'])
    assert scopes['cluster_mcl_start'] == scopes['cluster_mcl_last'] == scopes['cluster_labels'] == 1
    assert scopes['cluster_mcl_plan'] == st['iterations'] + 1
    assert scopes['cluster_hook'] == scopes['cluster_compress'] and scopes['cluster_hook'] % 4 == 0        # (the components of the last matrix)
    wave, group = scopes.get('cluster_mcl_expand_wave', 0), scopes.get('cluster_mcl_expand_group', 0)
    assert max(wave, group) <= st['iterations'] <= wave + group and (wave, group) == EXPAND[table_slots]
    assert st['lds_rows'] + st['spill_rows'] == n * st['iterations']
    spill = [scopes.get('cluster_mcl_spill_' + x, 0) for x in ('emit', 'sort', 'finish')]
    if table_slots:
        assert st['spill_rows'] > 0 and 1 <= spill[0] == spill[1] == spill[2] <= st['iterations']    # (one batch per iteration that spills)
    else:
        assert st['spill_rows'] == 0 and spill == [0, 0, 0]
    check_only(scopes, 'cluster_mcl_', 'cluster_hook', 'cluster_compress')


@pytest.mark.parametrize('algorithm', ['single', 'cd-hit', 'uclust'])
def test_update_stages(api, family, algorithm):
    """the last tenth of the objects new, the prior clusters those of the plain run on the rows among the others"""
    n, rows = family
    n_prior = n - n // 10
    inside = [x for x in rows if x[0] < n_prior and x[1] < n_prior]
    prior = cr.cluster_ids(n_prior, cr.edges(inside), algorithm) + [-1] * (n - n_prior)
    (label, rep, st), scopes = profiled(api, lambda: api.cluster_update_graph(n, *columns(rows), prior, algorithm))
    want_label, want_rep, want = cu.update_graph(n, rows, prior, algorithm)
    assert (label.tolist(), rep.tolist()) == (want_label, want_rep)
    assert {k: st[k] for k in want} == want and st['n_new'] == n // 10 and st['n_edges'] > 0
    check_build(scopes, st['n_edges'])
    assert scopes['cluster_update_map'] == scopes['cluster_update_seed'] == scopes['cluster_labels'] == 1
    if algorithm == 'single':
        assert scopes['cluster_hook'] == scopes['cluster_compress'] == st['rounds'] and st['rounds'] % 4 == 0
        check_only(scopes, 'cluster_update_', 'cluster_hook', 'cluster_compress')
    else:
        stem = 'cluster_uclust' if algorithm == 'uclust' else 'cluster_cdhit'
        assert scopes[stem + '_round'] == st['rounds'] and scopes.get(stem + '_sweep', 0) == (st['sweep_objects'] > 0)
        check_only(scopes, 'cluster_update_', stem + '_round', stem + '_sweep')


def test_report_stages(api, family, golden_dir, tmp_path):
    """the report of one labelling, and the file call with two label columns: the passes run per column on one graph"""
    n, rows = family
    label = np.asarray(cr.labels(cr.cluster_ids(n, cr.edges(rows), 'cd-hit'))[0], np.int32)
    k = int(label.max()) + 1
    (rec, own, oth_max, oth), scopes = profiled(api, lambda: api.cluster_stats_graph(n, *columns(rows), label, k))
    want, want_own, want_max, want_oth = cs.stats_graph(n, rows, label.tolist(), k)
    assert all(rec[f].tolist() == [x[f] for x in want] for f in cs.FIELDS)
    assert (own.tolist(), oth_max.tolist(), oth.tolist()) == (want_own, want_max, want_oth)
    check_build(scopes, len(cr.edges(rows)))
    assert scopes['cluster_stats_rows'] == scopes['cluster_stats_reduce'] == scopes['cluster_stats_nearest'] == 1
    assert set(scopes) == set(BUILD) | {'cluster_stats_rows', 'cluster_stats_reduce', 'cluster_stats_nearest'}
    out_dir = golden_dir / 'output'
    ids = cr.read_ids(out_dir / 'ani.ids.tsv')
    path = tmp_path / 'two.tsv'
    path.write_text('object\tpairs\tfives\n' + ''.join(f'{x}\t{i // 2}\t{7 + i // 5}\n' for i, x in enumerate(ids)))
    _, scopes = profiled(api, lambda: api.cluster_stats(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', path, tmp_path / 's.tsv', tani=0.7))
    assert (tmp_path / 's.tsv').read_bytes() == cs.run(out_dir / 'ani.tsv', out_dir / 'ani.ids.tsv', path, tani=0.7)
    assert [scopes.get(name) for name in BUILD] == [1, 1, 1, 1]
    assert scopes['cluster_stats_rows'] == scopes['cluster_stats_reduce'] == scopes['cluster_stats_nearest'] == 2
    assert set(scopes) == set(BUILD) | {'cluster_stats_rows', 'cluster_stats_reduce', 'cluster_stats_nearest'}


def test_no_object_opens_no_scope(api):
    calls = {'graph': lambda: api.cluster_graph(0, [], [], []), 'table': lambda: api.cluster_linkage(0, [], [], []),
             'average': lambda: api.cluster_average_linkage_graph(0, [], [], []), 'mcl': lambda: api.cluster_mcl_graph(0, [], [], []),
             'update': lambda: api.cluster_update_graph(0, [], [], [], []), 'report': lambda: api.cluster_stats_graph(0, [], [], [], [], 0)}
    for name, call in calls.items():
        assert profiled(api, call)[1] == {}, name
