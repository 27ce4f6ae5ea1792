"""Share of the prefilter's row pointers that carry their only partner, counted on the CPU in numpy.

    python tools/rowptr_share.py [--families 100] [--workload phage-100k] [--k 25]

Takes the first `--families` families of the workload (a family depends on the seed and its own number only, and random 25-mers
of different families do not meet: the share of a sample of families is the set's), sorts every (canonical k-mer, genome,
position) and applies the writers' rules: an entry writes a pointer when it is neither the first of its run nor a repeat of the
entry in front of it; the pointer is an inline one when exactly one entry lies in front of it.  A throwaway reduction: nothing of
it runs in the library.
"""
import argparse
import json
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vclust_amd import synth  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--families', type=int, default=100)
    ap.add_argument('--workload', default='phage-100k')
    ap.add_argument('--k', type=int, default=25)
    args = ap.parse_args(argv)
    w = dict(synth.WORKLOADS[args.workload])
    assert w.pop('kind') == 'families'
    w['n_families'] = args.families
    codes, offsets, _ = synth.make_families(**w)
    k, n = args.k, len(codes)
    m = n - k + 1
    fwd = np.zeros(m, dtype=np.uint64); rc = np.zeros(m, dtype=np.uint64); bad = np.zeros(m, dtype=bool)
    for j in range(k):
        c = codes[j:j + m]
        bad |= c > 3
        c = (c & 3).astype(np.uint64)
        fwd = (fwd << np.uint64(2)) | c
        rc |= (np.uint64(3) - c) << np.uint64(2 * j)
    genome = (np.searchsorted(offsets, np.arange(m), side='right') - 1).astype(np.int64)
    ok = ~bad & (np.arange(m) + k <= offsets[genome + 1])              # the window stays inside its genome
    key = np.minimum(fwd, rc)[ok]; genome = genome[ok]
    del fwd, rc, bad
    order = np.lexsort((genome, key))                                   # stable: positions ascend inside (key, genome)
    key = key[order]; genome = genome[order]
    head = np.ones(len(key), dtype=bool); head[1:] = key[1:] != key[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(len(key)), 0))
    before = np.arange(len(key)) - start
    repeat = np.zeros(len(key), dtype=bool); repeat[1:] = ~head[1:] & (genome[1:] == genome[:-1])
    pointer = (before >= 1) & ~repeat
    inline = pointer & (before == 1)
    out = dict(workload=args.workload, families=args.families, genomes=len(offsets) - 1, positions=int(n), kmers=int(len(key)),
               repeats=int(repeat.sum()), pointers=int(pointer.sum()), inline_pointers=int(inline.sum()),
               pointers_per_position=round(float(pointer.sum()) / n, 4), inline_share=round(float(inline.sum()) / max(1, int(pointer.sum())), 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
