"""Sequential restatement of `dereplicate` over an abstract graph: the batch procedure of vg_dereplicate_set
in plain Python.  Objects are 0 .. n - 1 in visit order (the align stage's length order).  The graph is only reached through an
edge callback, edge(a, b) -> weight or None, and every pair the procedure asks for is recorded: the point of the procedure is
the pairs it never asks for.

Per batch of B consecutive objects, with R the representatives so far:
  1. the subset S = [R | batch];
  2. every pair (batch object, representative of an earlier batch) is asked; a batch object with an edge to one is *joined*,
     the others form U;
  3. every pair inside U is asked;
  4. the update of a prior clustering under cd-hit (cluster_update_restatement) over S, the representatives frozen, with the
     edges of 2 and 3; founders join R.
At the end, plain cd-hit (cluster_restatement) over the asked edges of all batches gives labels and representatives, and must
agree with what the batches decided."""
import cluster_restatement as cr
import cluster_update_restatement as cu


def dereplicate(n, edge, batch):
    """-> (label, representative, asked, stats): asked is the list of (a, b, kind) with a < b, kind 'rep' for a pair (earlier
    representative, batch object) and 'U' for a pair of two batch objects that joined no earlier representative."""
    if batch < 1:
        raise ValueError('batch size must be at least 1')
    reps, rep_of = [], [-1] * n
    asked, rows = [], []
    stats = dict(batches=0, joined_prior=0, joined_new=0, founded=0)
    for b0 in range(0, n, batch):
        members = reps + list(range(b0, min(n, b0 + batch)))          # subset id = position
        n_rep = len(reps)
        sub_rows = []

        def ask(i, j, kind):
            a, b = members[i], members[j]
            asked.append((a, b, kind))
            w = edge(a, b)
            if w is not None:
                sub_rows.append((j, i, w))
                rows.append((b, a, w))
            return w is not None
        joined = [False] * len(members)
        for j in range(n_rep, len(members)):
            for i in range(n_rep):
                if ask(i, j, 'rep'):
                    joined[j] = True
        free = [j for j in range(n_rep, len(members)) if not joined[j]]
        for x, j in enumerate(free):
            for i in free[:x]:
                ask(i, j, 'U')
        prior = list(range(n_rep)) + [-1] * (len(members) - n_rep)
        _, rep, st = cu.update_graph(len(members), sub_rows, prior, 'cd-hit')
        for j in range(n_rep, len(members)):
            rep_of[members[j]] = members[rep[j]]
            if rep[j] == j:
                reps.append(members[j])
        for key in ('joined_prior', 'joined_new', 'founded'):
            stats[key] += st[key]
        stats['batches'] += 1
    label, representative = cr.cluster_graph(n, rows, 'cd-hit')
    if representative != rep_of:
        raise AssertionError(f'the batches decided {rep_of}, cd-hit over the asked rows {representative}')
    stats.update(representatives=len(reps), pairs_asked=len(asked))
    return label, representative, asked, stats
