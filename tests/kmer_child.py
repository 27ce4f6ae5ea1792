"""A child process for the prefilter tests whose run needs developer switches (read once per process) -- TEST INFRASTRUCTURE ONLY
(not a conftest, no fixtures: the test modules import it).

`run(job_dir, name, codes, offsets, calls, env)` starts `python tests/kmer_child.py job.npz out.npz`, which runs every call of
`calls` (keyword arguments of GenomeSet.kmer_shared, plus an optional 'subshards' for vg_set_subshards) on the set and hands back,
per call, the set sizes, the pairs as a dict and the launches of every profile scope.
"""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent


def pairs_dict(pairs):
    return {(int(a), int(b)): int(c) for a, b, c in zip(pairs['a'].tolist(), pairs['b'].tolist(), pairs['shared'].tolist())}


def shared_with_scopes(gs, api, lib, call):
    """One kmer_shared call -> (sizes as a list, pairs as a dict, {profile scope: launches})"""
    kw = dict(call)
    sub = int(kw.pop('subshards', 0))
    lib.vg_set_subshards(sub)
    api.profile_enable(True); api.profile_reset()
    try:
        sizes, pairs = gs.kmer_shared(**kw)
        scopes = {e['name']: int(e['launches']) for e in api.profile_get()}
    finally:
        api.profile_enable(False); lib.vg_set_subshards(0)
    return [int(x) for x in sizes], pairs_dict(pairs), scopes


def run(job_dir, name, codes, offsets, calls, env, timeout=600):
    """-> [(sizes, pairs dict, scopes)] of the calls, from a child process with the developer switches `env`"""
    job_dir = pathlib.Path(job_dir)
    fin, fout = job_dir / f'{name}.job.npz', job_dir / f'{name}.out.npz'
    np.savez(fin, codes=codes, offsets=offsets, calls=np.array(json.dumps(list(calls))))
    p = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), str(fin), str(fout)],
                       env=dict(os.environ, VG_DEV_SWITCHES='1', **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, (name, p.returncode, p.stderr[-2000:])
    d = np.load(fout)
    out = []
    for i in range(len(calls)):
        pr = d[f'pairs_{i}']
        out.append((d[f'sizes_{i}'].tolist(), {(int(a), int(b)): int(c) for a, b, c in pr.tolist()}, json.loads(str(d[f'scopes_{i}']))))
    return out


def _child_main(fin, fout):
    sys.path.insert(0, str(ROOT))
    from vclust_amd import _lib, api
    d = np.load(fin)
    calls = json.loads(str(d['calls']))
    gs = api.GenomeSet.from_codes(d['codes'], d['offsets'], ['s%d' % i for i in range(len(d['offsets']) - 1)])
    out = {}
    for i, call in enumerate(calls):
        sizes, pairs, scopes = shared_with_scopes(gs, api, _lib.load(), call)
        out[f'sizes_{i}'] = np.asarray(sizes, dtype=np.int64)
        out[f'pairs_{i}'] = np.asarray([(a, b, c) for (a, b), c in sorted(pairs.items())], dtype=np.int64).reshape(-1, 3)
        out[f'scopes_{i}'] = np.array(json.dumps(scopes))
    np.savez(fout, **out)


if __name__ == '__main__':
    _child_main(sys.argv[1], sys.argv[2])
