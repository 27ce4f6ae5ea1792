// vg_derep.cpp — dereplicate: greedy incremental clustering (cd-hit) in which a genome is compared with the representatives found so
// far and with nothing else, from nothing or on top of an earlier run's clusters.  Host code only: the
// representatives R are one resident working set, and every batch of new genomes is a composition of the finer C-ABI calls --
//   derep_extend       the batch appended behind R (vg_genomes_extend, vg_subset.hip); dropped again by derep_settle
//   derep_candidates   vg_kmer_shared_new with the representatives as the database, then vg_filter_pairs
//   derep_align        vg_align_tasks + vg_lz_align of some of those pairs; the rows that pass the cluster filters as ani.tsv prints them
//   derep_decide       vg_cluster_update_graph(cd-hit) with the representatives as the prior clustering
//   derep_settle       vg_genomes_truncate back to R, then the batch's founders appended for good
// and the end is the update of the prior clustering (vg_cluster_update_graph; plain cd-hit when there is none) over the passing rows
// of all batches, which also checks the batches' decisions.
#include "vg_common.h"
#include <math.h>
#include <numeric>

namespace {
void check(int rc) { if (rc != VG_OK) throw vg_error(rc, vg_last_error()); }
struct genomes_guard { vg_genomes* g = nullptr; ~genomes_guard() { if (g) vg_genomes_free(g); } };
struct free_guard { void* p = nullptr; ~free_guard() { if (p) vg_free(p); } };

double metric_floor(const vg_cluster_params& c) { return !strcmp(c.metric, "tani") ? c.min_tani : !strcmp(c.metric, "gani") ? c.min_gani : c.min_ani; }

// every argument error, before any device use
void check_params(const char* fn, const vg_derep_params* p) {
    const std::string f(fn);
    if (p->batch_genomes < 1) throw vg_error(VG_EINVAL, f + ": batch_genomes must be at least 1, not " + std::to_string(p->batch_genomes));
    if (p->cluster.algorithm != VG_CLUSTER_CDHIT)
        throw vg_error(VG_EINVAL, f + ": the algorithm must be VG_CLUSTER_CDHIT (uclust needs the rows of joined genomes to later representatives, which are never computed)");
    if (!p->cluster.metric || (strcmp(p->cluster.metric, "tani") && strcmp(p->cluster.metric, "gani") && strcmp(p->cluster.metric, "ani")))
        throw vg_error(VG_EINVAL, f + ": metric must be tani, gani or ani");
    if (!(metric_floor(p->cluster) > 0)) throw vg_error(VG_EINVAL, f + ": the " + p->cluster.metric + " threshold must be above 0");
    if (p->k < 15 || p->k > 30) throw vg_error(VG_EINVAL, "k must be in 15..30");
    if (!(p->kmers_fraction > 0.0) || p->kmers_fraction > 1.0) throw vg_error(VG_EINVAL, "kmers_fraction must be in (0,1]");
}

// the state of the loop: objects are ranks (vg_align_order)
struct derep_state {
    const vg_genomes* g; const vg_derep_params* p;
    const std::vector<int32_t>& order;                          // rank -> input id
    const std::vector<int32_t>& prior;                          // per rank: the representative an earlier run gave it, -1 = new
    genomes_guard work;                                         // the working set: R, and behind it the batch while it is decided
    std::vector<int32_t> reps;                                  // R in visit order = position in the working set: the prior representatives
    int n_prior_reps = 0;                                       //   (ascending ranks), then the founders (ascending ranks)
    std::vector<int32_t> rep_of;                                // per rank: the representative the prior or its batch gave it
    std::vector<uint32_t> q, r; std::vector<double> w;          // the passing rows of all batches, in ranks
    struct couple { int32_t lo, hi; vg_pair_stat fwd, rev; };   // an aligned pair of ranks lo < hi: fwd = (q = hi, r = lo), rev = (q = lo, r = hi)
    std::vector<couple> couples;
    bool keep_couples = false;
    vg_derep_stats st{}; vg_derep_update_stats ust{};
};
// one batch: the working set's members as ranks (position: the first n_rep are the representatives), its kept pairs and its rows
struct derep_batch {
    std::vector<int32_t> rank; int n_rep = 0;
    vg_genomes* sub = nullptr;                                  // the working set
    free_guard kept; int64_t n_kept = 0;                        // vg_pair_count, positions, a > b, a a batch genome
    std::vector<uint32_t> q, r; std::vector<double> w;          // passing rows, positions
    std::vector<uint8_t> linked;                                // per position: has a passing row (to a representative, after step 2)
    int n() const { return (int)rank.size(); }
};

void extend_by(derep_state& S, const int32_t* ranks, size_t count) {
    std::vector<int32_t> ids(count);
    for (size_t i = 0; i < count; ++i) ids[i] = S.order[(size_t)ranks[i]];
    check(vg_genomes_extend(S.work.g, S.g, ids.data(), (int)count));
}

// R as the earlier run left it, with room for the largest batch behind it (founders beyond that make the buffers grow by half)
void derep_open(derep_state& S, const std::vector<int32_t>& news) {
    const int32_t n = S.g->n;
    for (int32_t i = 0; i < n; ++i) if (S.prior[(size_t)i] == i) S.reps.push_back(i);
    S.n_prior_reps = (int)S.reps.size();
    S.ust.prior_objects = n - (int64_t)news.size(); S.ust.prior_representatives = S.n_prior_reps;
    if (news.empty()) return;
    std::vector<int32_t> ids(S.reps.size());
    int64_t rep_bases = 0, batch_bases = 0;
    for (size_t i = 0; i < ids.size(); ++i) { ids[i] = S.order[(size_t)S.reps[i]]; rep_bases += S.g->len[(size_t)ids[i]]; }
    const size_t B = (size_t)S.p->batch_genomes;
    for (size_t b0 = 0; b0 < news.size(); b0 += B) {
        int64_t sum = 0;
        for (size_t x = b0; x < std::min(news.size(), b0 + B); ++x) sum += S.g->len[(size_t)S.order[(size_t)news[x]]];
        batch_bases = std::max(batch_bases, sum);
    }
    check(vg_genomes_subset(S.g, ids.data(), (int)ids.size(), &S.work.g));
    check(vg_genomes_reserve(S.work.g, rep_bases + batch_bases, (int64_t)ids.size() + (int64_t)std::min(news.size(), B)));
}

void derep_extend(derep_state& S, derep_batch& B, const int32_t* ranks, size_t count) {
    B.rank = S.reps; B.n_rep = (int)S.reps.size();
    B.rank.insert(B.rank.end(), ranks, ranks + count);
    extend_by(S, ranks, count);
    B.sub = S.work.g;
    B.linked.assign((size_t)B.n(), 0);
}

void derep_candidates(derep_state& S, derep_batch& B) {
    if (B.n() < 2) return;
    const vg_derep_params* p = S.p;
    std::vector<int64_t> sizes((size_t)B.n());
    free_guard pairs; int64_t np = 0;
    check(vg_kmer_shared_new(B.sub, B.n_rep, p->k, p->kmers_fraction, (uint32_t)std::max(1, p->min_kmers), sizes.data(), (vg_pair_count**)&pairs.p, &np));
    check(vg_filter_pairs(p->k, p->min_kmers, p->min_ident, sizes.data(), B.n(), (const vg_pair_count*)pairs.p, np, (vg_pair_count**)&B.kept.p, &B.n_kept));
    S.st.pairs_candidate += B.n_kept;
}

// align the kept pairs that `take` selects; their passing rows go to the batch (positions) and to the state (ranks)
template <class Take> void derep_align(derep_state& S, derep_batch& B, Take take) {
    const vg_pair_count* kept = (const vg_pair_count*)B.kept.p;
    std::vector<vg_pair_count> sel;
    for (int64_t i = 0; i < B.n_kept; ++i) if (take(kept[i])) sel.push_back(kept[i]);
    if (sel.empty()) return;
    free_guard tasks; int64_t nt = 0;
    check(vg_align_tasks(B.sub, sel.data(), (int64_t)sel.size(), (vg_task**)&tasks.p, &nt));
    const vg_task* tk = (const vg_task*)tasks.p;
    std::vector<vg_pair_stat> stats((size_t)nt);
    check(vg_lz_align(B.sub, tk, nt, &S.p->lz, stats.data(), nullptr, nullptr));
    S.st.pairs_aligned += nt / 2;
    const vg_genomes* sub = B.sub;
    // the printed numbers of every row (formatter + from_chars: the cost of the stage's host side) on a few threads, then the rows in order
    std::vector<uint8_t> pass((size_t)nt); std::vector<double> weight((size_t)nt);
    vg_parallel_chunks(nt, std::max(1, std::min(vg_host_threads(), 16)), [&](int64_t lo, int64_t hi, int) {
        for (int64_t t = lo; t < hi; ++t) {
            const int64_t lq = sub->len[tk[t].q], lr = sub->len[tk[t].r];
            vg_ani_row raw, printed;
            vg_ani_row_values(lq, lr, stats[(size_t)t], stats[(size_t)(t ^ 1)], raw);
            vg_ani_row_printed(lq, lr, raw, printed);
            pass[(size_t)t] = vg_cluster_row_passes(&S.p->cluster, printed, &weight[(size_t)t]);
        }
    });
    for (int64_t t = 0; t < nt; ++t) {
        if (!pass[(size_t)t]) continue;
        B.q.push_back(tk[t].q); B.r.push_back(tk[t].r); B.w.push_back(weight[(size_t)t]);
        B.linked[tk[t].q] = B.linked[tk[t].r] = 1;
        S.q.push_back((uint32_t)B.rank[tk[t].q]); S.r.push_back((uint32_t)B.rank[tk[t].r]); S.w.push_back(weight[(size_t)t]);
    }
    if (S.keep_couples)
        for (int64_t t = 0; t < nt; t += 2) {
            // A prior representative may be shorter than a batch genome, so a position says nothing about the order of a couple: the
            // ranks do.  Task t is (q, r) and task t + 1 its reverse, whichever of the two the working set's own order put first.
            const int32_t a = B.rank[tk[t].q], b = B.rank[tk[t].r];
            if (a > b) S.couples.push_back({ b, a, stats[(size_t)t], stats[(size_t)t + 1] });
            else S.couples.push_back({ a, b, stats[(size_t)t + 1], stats[(size_t)t] });
        }
}

// -> the batch's founders, as ranks
std::vector<int32_t> derep_decide(derep_state& S, derep_batch& B) {
    std::vector<int32_t> prior((size_t)B.n(), -1), label((size_t)B.n()), rep((size_t)B.n()), founders;
    for (int i = 0; i < B.n_rep; ++i) prior[(size_t)i] = i;
    vg_cluster_update_stats us{};
    check(vg_cluster_update_graph(B.n(), B.q.data(), B.r.data(), B.w.data(), (int64_t)B.q.size(), VG_CLUSTER_CDHIT, prior.data(), label.data(), rep.data(), &us));
    for (int i = B.n_rep; i < B.n(); ++i) {
        S.rep_of[(size_t)B.rank[(size_t)i]] = B.rank[(size_t)rep[(size_t)i]];
        if (rep[(size_t)i] == i) founders.push_back(B.rank[(size_t)i]);
        else if (rep[(size_t)i] < S.n_prior_reps) S.ust.joined_prior_cluster++;
    }
    S.st.joined_prior += us.joined_prior; S.st.joined_new += us.joined_new; S.st.founded += us.founded;
    S.st.batches++;
    return founders;
}

// the working set back to R, and R grown by the founders: behind the last one, so position stays visit order
void derep_settle(derep_state& S, const derep_batch& B, const std::vector<int32_t>& founders) {
    check(vg_genomes_truncate(S.work.g, B.n_rep));
    extend_by(S, founders.data(), founders.size());
    S.reps.insert(S.reps.end(), founders.begin(), founders.end());
}

// the aligned couples as vg_write_ani wants them: input-order ids, couples ascending in (lo, hi) of the ranks (with a prior, the order
// they were aligned in is not that order: a later batch may hold a rank below an earlier founder's)
void derep_table(derep_state& S, vg_task** tasks, vg_pair_stat** rows, int64_t* n_tasks) {
    std::sort(S.couples.begin(), S.couples.end(), [](const derep_state::couple& x, const derep_state::couple& y) { return x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi; });
    const size_t nc = S.couples.size();
    vg_task* t = (vg_task*)malloc(sizeof(vg_task) * std::max<size_t>(1, 2 * nc));
    vg_pair_stat* s = (vg_pair_stat*)malloc(sizeof(vg_pair_stat) * std::max<size_t>(1, 2 * nc));
    if (!t || !s) { free(t); free(s); throw vg_error(VG_ENOMEM, "out of host memory"); }
    for (size_t c = 0; c < nc; ++c) {
        const uint32_t hi = (uint32_t)S.order[(size_t)S.couples[c].hi], lo = (uint32_t)S.order[(size_t)S.couples[c].lo];
        t[2 * c] = { hi, lo }; t[2 * c + 1] = { lo, hi };
        s[2 * c] = S.couples[c].fwd; s[2 * c + 1] = S.couples[c].rev;
    }
    *tasks = t; *rows = s; *n_tasks = (int64_t)(2 * nc);
}

// prior: per rank, -1 everywhere for the plain command
void dereplicate_set(const char* fn, vg_genomes* g, const vg_derep_params* p, const std::vector<int32_t>& prior, int32_t* label, int32_t* representative,
                     vg_task** tasks, vg_pair_stat** rows, int64_t* n_tasks, vg_derep_stats* st, vg_derep_update_stats* ust) {
    vg_require_device();
    check(vg_genomes_to_device(g));
    vg_length_order(g);
    const int32_t n = g->n;
    derep_state S{ g, p, g->len_order, prior };
    S.rep_of = prior;
    S.keep_couples = tasks != nullptr;
    std::vector<int32_t> news;                                  // the new objects in index order: their visit order
    for (int32_t i = 0; i < n; ++i) if (prior[(size_t)i] < 0) news.push_back(i);
    derep_open(S, news);
    for (size_t b0 = 0; b0 < news.size(); b0 += (size_t)p->batch_genomes) {
        derep_batch B;
        derep_extend(S, B, news.data() + b0, std::min(news.size() - b0, (size_t)p->batch_genomes));
        derep_candidates(S, B);
        // a batch genome against the representatives so far; then the genomes that joined none, among themselves
        derep_align(S, B, [&](const vg_pair_count& c) { return (int)c.b < B.n_rep; });
        const std::vector<uint8_t> joined = B.linked;
        derep_align(S, B, [&](const vg_pair_count& c) { return (int)c.b >= B.n_rep && !joined[c.a] && !joined[c.b]; });
        derep_settle(S, B, derep_decide(S, B));
    }
    S.st.pairs_skipped = S.st.pairs_candidate - S.st.pairs_aligned;
    S.st.representatives = (int64_t)S.reps.size();
    // the file's numbering, and the check of every batch decision: the update of the prior over the rows of all batches (no prior: plain cd-hit)
    check(vg_cluster_update_graph(n, S.q.data(), S.r.data(), S.w.data(), (int64_t)S.q.size(), VG_CLUSTER_CDHIT, prior.data(), label, representative, nullptr));
    for (int32_t i = 0; i < n; ++i)
        if (representative[i] != S.rep_of[(size_t)i])
            throw vg_error(VG_EHIP, std::string(fn) + ": internal error: object " + std::to_string(i) + " (" + g->names[(size_t)g->len_order[(size_t)i]] + ") has the representative " +
                           std::to_string(S.rep_of[(size_t)i]) + " by its batch and " + std::to_string(representative[i]) + " by cd-hit over all rows");
    if (tasks) derep_table(S, tasks, rows, n_tasks);
    if (st) *st = S.st;
    if (ust) *ust = S.ust;
}

void check_set_call(const char* fn, const vg_genomes* g, const vg_derep_params* p, const int32_t* label, const int32_t* representative, vg_task** tasks,
                    vg_pair_stat** stats_rows, int64_t* n_tasks) {
    const std::string f(fn);
    if (!g || !p || (g->n && (!label || !representative))) throw vg_error(VG_EINVAL, f + ": null argument");
    if ((tasks || stats_rows || n_tasks) && !(tasks && stats_rows && n_tasks)) throw vg_error(VG_EINVAL, f + ": tasks, stats_rows and n_tasks go together");
    check_params(fn, p);
    if (tasks) { *tasks = nullptr; *stats_rows = nullptr; *n_tasks = 0; }
}

// The file-level command, with and without a database: FASTA in, clusters.tsv out.  db_paths = nullptr is the plain command.
void dereplicate_files(const char* fn, const char* const* db_paths, int n_db_paths, const char* const* fasta_paths, int n_paths, const char* prior_path,
                       bool prior_is_repr, const char* out_path, const vg_derep_file_params* p, vg_derep_update_stats* ust_out) {
    const std::string f(fn);
    const bool update = db_paths != nullptr;
    check_params(fn, &p->derep);
    if (p->out_table_path && (!p->out_columns || p->n_out_columns <= 0)) throw vg_error(VG_EINVAL, f + ": the table needs its columns");
    if (p->out_repr_fasta_path && !(n_paths == 1 && p->is_multifasta && (!update || n_db_paths == 1)))
        throw vg_error(VG_EINVAL, f + (update ? ": the representatives' FASTA is written for one multi-FASTA file on each side only" : ": the representatives' FASTA is written for one multi-FASTA input only"));
    if (p->stats) *p->stats = vg_derep_stats{};
    if (ust_out) *ust_out = vg_derep_update_stats{};
    vg_require_device();
    genomes_guard gg;
    int n_db = 0;
    if (!update) check(vg_genomes_load_resident(fasta_paths, n_paths, p->is_multifasta, p->num_threads, &gg.g));
    else check(vg_genomes_load_db_new_resident(db_paths, n_db_paths, fasta_paths, n_paths, p->is_multifasta, p->num_threads, &gg.g, &n_db));
    const vg_genomes* g = gg.g;
    const int64_t n = g->n;
    vg_length_order(g);
    std::vector<std::string> ids((size_t)n);
    for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = g->names[(size_t)g->len_order[(size_t)i]];
    // the prior clusters by name, as `cluster --prior` reads them against the ids file of the combined set
    std::vector<int32_t> prior((size_t)n, -1);
    if (update) vg_cluster_read_prior(prior_path, ids, prior_is_repr, prior);
    std::vector<int32_t> label((size_t)std::max<int64_t>(n, 1)), rep(label.size());
    free_guard tasks, rows; int64_t nt = 0;
    vg_derep_stats st{}; vg_derep_update_stats ust{};
    const bool table = p->out_table_path != nullptr;
    if (!update)
        check(vg_dereplicate_set(gg.g, &p->derep, label.data(), rep.data(), table ? (vg_task**)&tasks.p : nullptr, table ? (vg_pair_stat**)&rows.p : nullptr,
                                 table ? &nt : nullptr, &st));
    else
        check(vg_dereplicate_update_set(gg.g, n_db, &p->derep, prior.data(), label.data(), rep.data(), table ? (vg_task**)&tasks.p : nullptr,
                                        table ? (vg_pair_stat**)&rows.p : nullptr, table ? &nt : nullptr, &st, &ust));
    vg_cluster_write(out_path, ids, label.data(), rep.data(), p->representatives != 0);
    if (table) {
        vg_align_params ap{};
        ap.lz = p->derep.lz; ap.out_columns = p->out_columns; ap.n_out_columns = p->n_out_columns; ap.num_threads = p->num_threads;
        check(vg_write_ani(g, (const vg_task*)tasks.p, (const vg_pair_stat*)rows.p, nt, nullptr, 0, p->out_table_path, &ap));
    }
    if (p->out_repr_fasta_path) {
        // multi-FASTA: genome i is record i of the files read one behind the other (the database's first); the representatives in input order
        std::vector<const char*> files;
        if (update) files.push_back(db_paths[0]);
        files.push_back(fasta_paths[0]);
        vg_fasta_text text;
        vg_fasta_read(files.data(), (int)files.size(), std::max(1, p->num_threads), text);
        if ((int64_t)text.recs.size() != n) throw vg_error(VG_EIO, std::string(fasta_paths[0]) + ": the file changed while it was processed");
        std::vector<int64_t> which;
        for (int64_t i = 0; i < n; ++i) if (rep[(size_t)i] == i) which.push_back(g->len_order[(size_t)i]);
        std::sort(which.begin(), which.end());
        vg_fasta_write_records(p->out_repr_fasta_path, text, which);
    }
    if (p->verbosity >= 1) {
        fprintf(stderr, "Dereplicate: %lld genomes, %lld representatives, %lld batches, %lld pairs aligned (%lld candidates skipped)\n", (long long)n,
                (long long)st.representatives, (long long)st.batches, (long long)st.pairs_aligned, (long long)st.pairs_skipped);
        if (update)
            fprintf(stderr, "Dereplicate update: %lld prior genomes in %lld clusters kept; %lld new genomes: %lld joined a prior cluster, %lld another new genome, %lld founded a cluster\n",
                    (long long)ust.prior_objects, (long long)ust.prior_representatives, (long long)(n - ust.prior_objects), (long long)ust.joined_prior_cluster,
                    (long long)(st.joined_prior + st.joined_new - ust.joined_prior_cluster), (long long)st.founded);
    }
    if (p->stats) *p->stats = st;
    if (ust_out) *ust_out = ust;
}
}  // namespace

extern "C" int vg_dereplicate_set(vg_genomes* g, const vg_derep_params* p, int32_t* label, int32_t* representative, vg_task** tasks,
                                  vg_pair_stat** stats_rows, int64_t* n_tasks, vg_derep_stats* st) {
    VG_API_BEGIN
    check_set_call("vg_dereplicate_set", g, p, label, representative, tasks, stats_rows, n_tasks);
    if (st) *st = vg_derep_stats{};
    dereplicate_set("vg_dereplicate_set", g, p, std::vector<int32_t>((size_t)g->n, -1), label, representative, tasks, stats_rows, n_tasks, st, nullptr);
    VG_API_END
}

extern "C" int vg_dereplicate_update_set(vg_genomes* g, int n_db, const vg_derep_params* p, const int32_t* prior_rep, int32_t* label, int32_t* representative,
                                         vg_task** tasks, vg_pair_stat** stats_rows, int64_t* n_tasks, vg_derep_stats* st, vg_derep_update_stats* ust) {
    VG_API_BEGIN
    const char* fn = "vg_dereplicate_update_set";
    check_set_call(fn, g, p, label, representative, tasks, stats_rows, n_tasks);
    if (g->n && !prior_rep) throw vg_error(VG_EINVAL, "vg_dereplicate_update_set: null argument");
    if (n_db < 0 || n_db > g->n) throw vg_error(VG_EINVAL, "vg_dereplicate_update_set: n_db = " + std::to_string(n_db) + " is outside 0.." + std::to_string(g->n) + " (the genomes of the set)");
    const std::vector<int32_t> prior(prior_rep, prior_rep + g->n);
    for (int32_t i = 0; i < g->n; ++i) {
        const int32_t r = prior[(size_t)i];
        if (r < -1 || r >= g->n)
            throw vg_error(VG_EINVAL, "vg_dereplicate_update_set: prior_rep[" + std::to_string(i) + "] = " + std::to_string(r) + " outside -1.." + std::to_string(g->n - 1));
        if (r >= 0 && prior[(size_t)r] != r)
            throw vg_error(VG_EINVAL, "vg_dereplicate_update_set: prior_rep[" + std::to_string(i) + "] = " + std::to_string(r) + " is not its own representative");
    }
    if (st) *st = vg_derep_stats{};
    if (ust) *ust = vg_derep_update_stats{};
    dereplicate_set(fn, g, p, prior, label, representative, tasks, stats_rows, n_tasks, st, ust);
    VG_API_END
}

extern "C" int vg_dereplicate(const char* const* fasta_paths, int n_paths, const char* out_path, const vg_derep_file_params* p) {
    VG_API_BEGIN
    if (!fasta_paths || n_paths <= 0 || !out_path || !p) throw vg_error(VG_EINVAL, "vg_dereplicate: null argument");
    dereplicate_files("vg_dereplicate", nullptr, 0, fasta_paths, n_paths, nullptr, false, out_path, p, nullptr);
    VG_API_END
}

extern "C" int vg_dereplicate_update(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, const char* prior_path, int prior_is_repr,
                                     const char* out_path, const vg_derep_file_params* p, vg_derep_update_stats* ust) {
    VG_API_BEGIN
    if (!db_paths || n_db <= 0 || !new_paths || n_new <= 0 || !prior_path || !out_path || !p) throw vg_error(VG_EINVAL, "vg_dereplicate_update: null argument");
    dereplicate_files("vg_dereplicate_update", db_paths, n_db, new_paths, n_new, prior_path, prior_is_repr != 0, out_path, p, ust);
    VG_API_END
}
