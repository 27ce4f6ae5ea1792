"""Timing of new genomes against a database (GenomeSet.kmer_shared_new) beside the all-vs-all pass.

  python tools/new2all_timing.py [--workload phage-100k] [--n <families>] [--fractions 0.001 0.01 0.1 0.5] [--runs 3]
                                 [--baseline-root <checkout of the parent commit, built>] [--json profiles/<file>.json]

The set is the bench's (vclust_amd.synth.make_workload); the last 0.1 %, 1 %, 10 % and 50 % of its genomes are the new ones.
Every run is a fresh process, and the processes of the three kinds alternate: baseline, unmasked, masked, baseline, ...
  baseline  the all-vs-all kmer_shared (min_shared 20), filter_pairs, align_tasks and lz_align of the whole set -- what a user pays
            today whatever the share of new genomes.  With --baseline-root the process imports vclust_amd from that tree (a checkout
            of the parent commit, built; --baseline-label names it in the output); without it, this tree's kmer_shared.
  unmasked  for each fraction: kmer_shared_new(n_db) under set_new_path(1), then filter_pairs, align_tasks, lz_align of its result.
  masked    the same under set_new_path(2): the route that indexes only what a new genome can share.
A process builds the set, makes it resident, runs every call once and discards it (allocations, code objects), then times it once
with the profile scopes on.  Reported per quantity: the range (min - max) over the runs.  Prints one JSON line per process, then the
table of DESIGN.md section 11 and the decision: the masked route is kept if at 1 % new its range lies below the unmasked route's and
that one below the baseline's; the automatic threshold is the largest measured fraction at which the masked range is still below
the unmasked one.  --json keeps everything; --design <file> replaces the table between the two `new2all_timing` marker lines."""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
K, MIN_KMERS, MIN_IDENT = 25, 20, 0.7


def timed(api, fn):
    api.profile_reset()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    return out, round(wall, 2), {e['name']: round(e['total_ms'], 3) for e in api.profile_get()}


def stage(api, gs, prefilter):
    """prefilter() -> (sizes, pairs); then the align stage of its candidates.  Everything once discarded, once timed."""
    def align(sizes, pairs):
        cand = gs.filter_pairs(sizes, pairs, k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT)
        tasks = gs.align_tasks(cand)
        return len(cand), gs.lz_align(tasks)
    align(*prefilter())
    (sizes, pairs), pre_ms, pre_scopes = timed(api, prefilter)
    (n_cand, stats), aln_ms, aln_scopes = timed(api, lambda: align(sizes, pairs))
    return dict(pairs=int(len(pairs)), candidates=int(n_cand), tasks=int(len(stats)), prefilter_ms=pre_ms, prefilter_scopes=pre_scopes,
                align_ms=aln_ms, align_scopes=aln_scopes, total_ms=round(pre_ms + aln_ms, 2))


def child(a):
    sys.path.insert(0, str(a.root))
    from vclust_amd import api, synth
    api.set_device(0)
    codes, offsets, names, desc = synth.make_workload(a.workload, a.n)
    gs = api.GenomeSet.from_codes(codes, offsets, names)
    gs.to_device()
    n = len(gs)
    api.profile_enable(True)
    out = dict(kind=a.child, workload=desc, genomes=n, library=a.label)
    if a.child == 'baseline':
        out['all_vs_all'] = stage(api, gs, lambda: gs.kmer_shared(k=K, min_shared=MIN_KMERS))
    else:
        api.set_new_path(1 if a.child == 'unmasked' else 2)
        for f in a.fractions:
            n_db = n - max(1, round(n * f))
            out[f'{f:g}'] = dict(n_db=n_db, n_new=n - n_db, **stage(api, gs, lambda: gs.kmer_shared_new(n_db, k=K, min_shared=MIN_KMERS)))
    print(json.dumps(out), flush=True)


def spread(values):
    return f'{min(values):.1f} - {max(values):.1f}'


SCOPES = ('kmer_partition', 'kmer_new_mask', 'kmer_new_sizes', 'kmer_partition2', 'bucket_sort_runs', 'spgemm_rows', 'lz_build_index')


def table(res, fractions, baseline_label):
    rows = ['| new genomes | route | pairs | prefilter call, ms | ' + ' | '.join(f'`{s}`' for s in SCOPES) + ' | align stage, ms | both, ms |',
            '|---|---|---|---|' + '---|' * len(SCOPES) + '---|---|']

    def row(label, route, runs):
        sc = lambda s: spread([r['prefilter_scopes'].get(s, r['align_scopes'].get(s, 0.0)) for r in runs])       # noqa: E731
        return (f"| {label} | {route} | {runs[0]['pairs']} | {spread([r['prefilter_ms'] for r in runs])} | " + ' | '.join(sc(s) for s in SCOPES)
                + f" | {spread([r['align_ms'] for r in runs])} | {spread([r['total_ms'] for r in runs])} |")
    rows.append(row('all', f'all-vs-all ({baseline_label})', [b['all_vs_all'] for b in res['baseline']]))
    for f in fractions:
        for kind in ('unmasked', 'masked'):
            runs = [r[f'{f:g}'] for r in res[kind]]
            rows.append(row(f"{f * 100:g} % ({runs[0]['n_new']})", kind, runs))
    return '\n'.join(rows)


def decide(res, fractions):
    """-> (keep the masked route, automatic threshold, the sentence)"""
    ms = lambda kind, f: [r[f'{f:g}']['prefilter_ms'] for r in res[kind]]       # noqa: E731
    base = [b['all_vs_all']['prefilter_ms'] for b in res['baseline']]
    below = [f for f in fractions if max(ms('masked', f)) < min(ms('unmasked', f))]
    keep = 0.01 in fractions and 0.01 in below and max(ms('unmasked', 0.01)) < min(base)
    threshold = max(below) if keep and below else 0.0
    text = (f"masked below unmasked at: {', '.join(f'{f * 100:g} %' for f in below) or 'no fraction'}; unmasked at 1 % "
            f"{'below' if 0.01 in fractions and max(ms('unmasked', 0.01)) < min(base) else 'not below'} the baseline; "
            f"the masked route is {'kept' if keep else 'dropped'}; automatic threshold {threshold:g}")
    return keep, threshold, text


MARK = '<!-- new2all_timing -->'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='phage-100k')
    ap.add_argument('--n', type=int, default=None, help='scale the workload down (families / contigs)')
    ap.add_argument('--fractions', type=float, nargs='+', default=[0.001, 0.01, 0.1, 0.5])
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--baseline-root', type=pathlib.Path, default=None)
    ap.add_argument('--baseline-label', default=None, help='what the baseline library is called in the output (default: "this tree", or the path)')
    ap.add_argument('--json', type=pathlib.Path)
    ap.add_argument('--design', type=pathlib.Path, help='a document with two marker lines; the table between them is replaced')
    ap.add_argument('--timeout', type=float, default=600, help='seconds a process may take')
    ap.add_argument('--child', choices=['baseline', 'unmasked', 'masked'])
    ap.add_argument('--root', type=pathlib.Path, default=ROOT)
    ap.add_argument('--label', default='this tree')
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    common = ['--workload', a.workload, '--fractions', *map(str, a.fractions)] + (['--n', str(a.n)] if a.n else [])
    baseline_label = a.baseline_label or (str(a.baseline_root) if a.baseline_root else 'this tree')
    res = dict(baseline=[], unmasked=[], masked=[])
    for run in range(a.runs):
        for kind, root, label in (('baseline', a.baseline_root or ROOT, baseline_label), ('unmasked', ROOT, 'this tree'), ('masked', ROOT, 'this tree')):
            p = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), '--child', kind, '--root', str(root), '--label', label, *common],
                               stdout=subprocess.PIPE, text=True, timeout=a.timeout, env={**os.environ, 'PYTHONPATH': ''})
            if p.returncode != 0:
                sys.exit(f'{kind} process of run {run} ended with status {p.returncode}; nothing further is started')
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[kind].append(json.loads(line))
    text = table(res, a.fractions, baseline_label)
    keep, threshold, decision = decide(res, a.fractions)
    print(text)
    print(decision)
    if a.json:
        a.json.write_text(json.dumps(dict(tool='tools/new2all_timing.py', k=K, min_kmers=MIN_KMERS, min_ident=MIN_IDENT, runs=a.runs,
                                          baseline=baseline_label, table=text, decision=decision, keep_masked=keep, threshold=threshold,
                                          **{'runs_' + k: v for k, v in res.items()}), indent=1) + '\n')
    if a.design:
        doc = a.design.read_text().split(MARK)
        if len(doc) != 3:
            sys.exit(f'{a.design}: expected two marker lines {MARK}')
        a.design.write_text(doc[0] + MARK + '\n' + text + '\n\n' + decision + '.\n' + MARK + doc[2])


if __name__ == '__main__':
    main()
