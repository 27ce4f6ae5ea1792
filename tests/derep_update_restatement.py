"""Sequential restatement of `dereplicate --db --prior` ("Update") over an abstract graph: the batch procedure
of vg_dereplicate_update_set in plain Python -- derep_restatement's procedure with a prior clustering.  Objects are 0 .. n - 1 (the
align stage's length order of the combined set); prior_rep[i] is -1 for a new object, else the representative of i's prior cluster.
The graph is only reached through the edge callback, and every pair the procedure asks for is recorded.

R starts as the prior representatives in index order; founders are appended behind them, so position in R is visit order.  The
batches run over the new objects only, in index order; a prior member is never a member of a working set.  Per batch:
  1. the working set S = [R | batch];
  2. every pair (batch object, representative in R) is asked; a batch object with an edge to one is *joined*, the others form U;
  3. every pair inside U is asked;
  4. the update of a prior clustering under cd-hit (cluster_update_restatement) over S, R frozen, with the edges of 2 and 3;
     founders join R.
At the end, the update of the full prior (cluster_update_restatement) over the asked edges of all batches gives labels and
representatives, and must agree with what the batches decided."""
import cluster_update_restatement as cu


def dereplicate_update(n, edge, batch, prior_rep):
    """-> (label, representative, asked, stats): asked is the list of (a, b, kind) with a < b, kind 'rep' for a pair (representative
    of R, batch object) and 'U' for a pair of two batch objects that joined no representative of R."""
    if batch < 1:
        raise ValueError('batch size must be at least 1')
    assert len(prior_rep) == n
    reps = [i for i in range(n) if prior_rep[i] == i]
    n_prior_reps = len(reps)
    rep_of = list(prior_rep)
    news = [i for i in range(n) if prior_rep[i] < 0]
    asked, rows = [], []
    stats = dict(batches=0, joined_prior=0, joined_new=0, founded=0, prior_objects=n - len(news), prior_representatives=n_prior_reps,
                 joined_prior_cluster=0)
    for b0 in range(0, len(news), batch):
        members = reps + news[b0:b0 + batch]                          # position in the working set
        n_rep = len(reps)
        sub_rows = []

        def ask(i, j, kind):
            a, b = members[i], members[j]
            asked.append((min(a, b), max(a, b), kind))
            w = edge(min(a, b), max(a, b))
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
            elif rep[j] < n_prior_reps:
                stats['joined_prior_cluster'] += 1
        for key in ('joined_prior', 'joined_new', 'founded'):
            stats[key] += st[key]
        stats['batches'] += 1
    label, representative, _ = cu.update_graph(n, rows, prior_rep, 'cd-hit')
    if representative != rep_of:
        raise AssertionError(f'the batches decided {rep_of}, the update over the asked rows {representative}')
    stats.update(representatives=len(reps), pairs_asked=len(asked))
    return label, representative, asked, stats
