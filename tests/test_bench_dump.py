"""bench.py --dump-outputs: what the last timed step returned, as float64 .npy files under a size budget (a seeded
row sample beyond it), the same files for the same arrays."""
import numpy as np

import bench


def _groups():
    rng = np.random.default_rng(7)
    u32 = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return {'genomes': {'kmer_set_sizes': rng.integers(0, 2 ** 40, 300)},
            'tasks': {'task_q': u32(20000), 'task_r': u32(20000), 'n_match': u32(20000)}}


def _read(d):
    return {p.stem: np.load(p) for p in sorted(d.glob('*.npy'))}


def test_under_budget_everything_exact(tmp_path):
    g = _groups()
    rows = bench.dump_outputs(tmp_path, g)
    got = _read(tmp_path)
    assert set(got) == {'kmer_set_sizes', 'task_q', 'task_r', 'n_match'}
    for arrs in g.values():
        for name, a in arrs.items():
            assert got[name].dtype == np.float64 and rows[name] == len(a)
            assert np.array_equal(got[name].astype(np.int64), a.astype(np.int64))


def test_over_budget_seeded_sample_of_the_same_rows(tmp_path):
    g = _groups()
    budget = 100_000
    files = []
    for run in ('a', 'b'):
        d = tmp_path / run
        bench.dump_outputs(d, g, budget=budget)
        assert sum(p.stat().st_size for p in d.glob('*.npy')) <= budget
        files.append({p.name: p.read_bytes() for p in d.glob('*.npy')})
    assert files[0] == files[1]                      # same arrays in, same files out
    got = _read(tmp_path / 'a')
    idx = got['tasks_rows'].astype(np.int64)
    assert len(idx) > 0 and np.all(np.diff(idx) > 0)
    for name in ('task_q', 'task_r', 'n_match'):
        assert np.array_equal(got[name].astype(np.int64), g['tasks'][name][idx].astype(np.int64))
    sub = got['genomes_rows'].astype(np.int64)
    assert np.array_equal(got['kmer_set_sizes'].astype(np.int64), g['genomes']['kmer_set_sizes'][sub])
    # a later dump that fits leaves no row numbers of the sampled one behind
    bench.dump_outputs(tmp_path / 'a', g)
    assert not (tmp_path / 'a' / 'tasks_rows.npy').exists() and len(_read(tmp_path / 'a')['task_q']) == 20000


def test_candidate_pairs_in_any_order_dump_the_same_files(tmp_path):
    """The single-GPU prefilter returns its pairs unordered: the same set in another order must write the same files."""
    from vclust_amd import api
    rng = np.random.default_rng(3)
    ab = np.unique(rng.integers(0, 500, (3000, 2)), axis=0)
    ab = ab[ab[:, 0] > ab[:, 1]]
    cand = np.zeros(len(ab), dtype=api.PAIR_DTYPE)
    cand['a'], cand['b'], cand['shared'] = ab[:, 0], ab[:, 1], rng.integers(20, 40000, len(ab))
    tasks = np.zeros(2 * len(ab), dtype=api.TASK_DTYPE)
    tasks['q'], tasks['r'] = ab.repeat(2, 0)[:, 0], ab.repeat(2, 0)[:, 1]
    stats = np.zeros(len(tasks), dtype=api.STAT_DTYPE)
    stats['n_match'] = rng.integers(0, 40000, len(tasks))
    sizes = rng.integers(0, 40000, 500)
    files = []
    for run, perm in (('a', rng.permutation(len(cand))), ('b', rng.permutation(len(cand)))):
        bench.dump_outputs(tmp_path / run, bench.step_outputs(sizes, cand[perm], tasks, stats))
        files.append({p.name: p.read_bytes() for p in (tmp_path / run).glob('*.npy')})
    assert files[0] == files[1]
    got = _read(tmp_path / 'a')
    key = got['pair_a'] * 1000 + got['pair_b']
    assert np.all(np.diff(key) > 0) and len(key) == len(cand)
    assert np.array_equal(got['pair_shared'].astype(np.int64), cand['shared'][np.lexsort((cand['b'], cand['a']))].astype(np.int64))
