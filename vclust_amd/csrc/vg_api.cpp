// vg_api.cpp — the whole-stage entry points, files in and files out.  The three the reference's front-end needs:
//   vg_prefilter  replaces kmer-db build + all2all + distance (vclust.py:1433-1471); vg_prefilter_new: new genomes against a database
//   vg_align      replaces lz-ani all2all                    (vclust.py:1497-1521); vg_align_new: likewise
//   vg_cluster    replaces clusty for single / cd-hit / uclust / set-cover (vclust.py:1539-1557), and the floor cut of complete and
//                 average linkage
// and four more on the parse of vg_cluster (cluster_stage):
//   vg_cluster_mcl          Markov clustering (vg_cluster_mcl_graph)
//   vg_cluster_update       a prior clusters.tsv read back, then its clusters extended by the new objects (vg_cluster_update_graph)
//   vg_cluster_linkage      the single-, complete- or average-linkage merge table and its cuts at several levels
//   vg_cluster_stats_file   a clusters.tsv read back, then the per-cluster report of every label column
// and one on the alignment table of vg_align:
//   vg_cover_file           the coverage map of every genome (vg_cover_rows)
//   vg_paint_file           the closest partner of every genome at every position (vg_paint_rows)
// All are compositions of the finer C-ABI calls (ingest -> HBM -> integer kernels -> writers).
#include "vg_common.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <thread>
#include <vector>

namespace {
// vg_set_process_ends_after_call(1) (vclust.py, for its one-shot `prefilter` / `align` processes): the process ends right
// after the call, so the genome set -- 1.5 GB of host arrays to unmap, 1.4 GB of device blocks to hand back -- is left to
// the exit instead of being released first (0.1 s that the caller would wait for).  A setter, not an environment variable:
// an embedding process that merely inherits an environment keeps the library's normal ownership.
static bool g_leak_at_exit = false;
static bool leak_at_exit() { return g_leak_at_exit; }
struct genomes_guard { vg_genomes* g = nullptr; ~genomes_guard() { if (g && !leak_at_exit()) vg_genomes_free(g); } };
struct free_guard { void* p = nullptr; ~free_guard() { if (p) vg_free(p); } };
void check(int rc) { if (rc != VG_OK) throw vg_error(rc, vg_last_error()); }
// parked clean-up (vg_defer) is released when the stage's kernels are in flight, and in any case when the call ends
struct defer_scope { defer_scope() { vg_defer_mode(true); } ~defer_scope() { vg_defer_mode(false); vg_deferred_start(); } };
// The HIP context (120-170 ms on a cold process) is created on a helper thread while the FASTA is parsed; the
// caller joins before its first device call.  Failures are left to that call, which reports them.
// It also pays the other one-time costs of the first device operations there: the runtime's fill kernel (the first
// hipMemsetAsync of a process loads it: 50-90 ms were seen in front of the first kernel of vg_kmer_shared) and the code
// object of the stage's own kernels.
enum warm_stage { WARM_PREFILTER, WARM_ALIGN, WARM_CLUSTER };
struct device_warmup {
    std::thread th;
    explicit device_warmup(warm_stage stage) {
        try {
            th = std::thread([stage] {
                try {
                    vg_require_device(); hipStream_t s = vg_stream(); (void)hipFree(nullptr);
                    void* p = vg_dev_alloc(4096);
                    (void)hipMemsetAsync(p, 0, 4096, s);
                    if (stage == WARM_ALIGN) vg_warm_align(s);
                    else if (stage == WARM_PREFILTER) { vg_warm_prefilter(s); (void)vg_side_stream(); }     // (a second queue costs 8-20 ms to create)
                    (void)hipStreamSynchronize(s);
                    vg_dev_free(p);
                    vg_host_mark("device warm");
                } catch (...) {}
            });
        } catch (...) {}
    }
    void join() { if (th.joinable()) th.join(); }
    ~device_warmup() { join(); }
};
}
namespace {
// vg_release_device_memory on a helper thread for the lifetime of the object (joined at its end, also when the writer throws)
struct background_release {
    std::thread th;
    // (best effort: the thread selects the library's device first -- a fresh thread starts on device 0 --, and nothing it
    // throws may leave it: a failure only means the blocks stay cached until the next release)
    static void release() noexcept { try { vg_require_device(); vg_release_device_memory(); } catch (...) { (void)hipGetLastError(); } }
    background_release() { try { th = std::thread([] { release(); }); } catch (...) { release(); } }
    ~background_release() { if (th.joinable()) th.join(); }
};
}
extern "C" void vg_set_process_ends_after_call(int on) { g_leak_at_exit = on != 0; }

// The genome set of a whole-stage call: one path list (vg_prefilter, vg_align), or the database's list in front of it (the _new
// entries).  load() returns the resident set and n_db, the number of database genomes: -1 without a database.
struct stage_input {
    const char* const* paths; int n_paths; const char* const* db_paths; int n_db_paths;
    bool ok() const { return paths && n_paths > 0 && (!db_paths ? n_db_paths == 0 : n_db_paths > 0); }
    int load(int multisample, int n_threads, vg_genomes** g) const {
        int n_db = -1;
        if (!db_paths) check(vg_genomes_load_resident(paths, n_paths, multisample, n_threads, g));
        else check(vg_genomes_load_db_new_resident(db_paths, n_db_paths, paths, n_paths, multisample, n_threads, g, &n_db));
        return n_db;
    }
};

static void prefilter_stage(const char* fn, const stage_input& in, const char* out_path, const vg_prefilter_params* p) {
    if (!in.ok() || !out_path || !p) throw vg_error(VG_EINVAL, std::string(fn) + ": null argument");
    if (p->k < 15 || p->k > 30) throw vg_error(VG_EINVAL, "k must be in 15..30");
    if (!(p->kmers_fraction > 0.0) || p->kmers_fraction > 1.0) throw vg_error(VG_EINVAL, "kmers_fraction must be in (0,1]");
    vg_host_mark((std::string(fn) + ": enter").c_str());
    vg_one_shot_scope one_shot;
    defer_scope parked;
    device_warmup warm(WARM_PREFILTER);
    genomes_guard gg;
    const int n_db = in.load(p->is_multifasta, p->num_threads, &gg.g);
    warm.join();
    vg_require_device();
    std::vector<int64_t> sizes((size_t)std::max(1, vg_genomes_count(gg.g)));
    free_guard pairs; int64_t np = 0;
    // on a single device the --min-kmers cut can be applied on the GPU already
    uint32_t min_emit = (uint32_t)std::max(1, p->min_kmers);
    if (n_db < 0) check(vg_kmer_shared(gg.g, p->k, p->kmers_fraction, 0, 1, min_emit, sizes.data(), (vg_pair_count**)&pairs.p, &np));
    else check(vg_kmer_shared_new(gg.g, n_db, p->k, p->kmers_fraction, min_emit, sizes.data(), (vg_pair_count**)&pairs.p, &np));
    // a one-shot process: the tens of GB of workspace go back to the driver NOW, so that the scrub of that memory
    // runs beside the writer and the start of the next process (`vclust.py align`) instead of in front of its
    // first allocation
    // (handing ~10 GB back is tens of milliseconds inside the driver: on a helper thread, beside the writer, which is host work only)
    {
        background_release rel;
        check(vg_write_fltr(gg.g, p->k, p->kmers_fraction, p->min_kmers, p->min_ident, p->max_seqs,
                            sizes.data(), (const vg_pair_count*)pairs.p, np, out_path));
    }
    vg_host_mark("fltr.txt written");
}
extern "C" int vg_prefilter(const char* const* fasta_paths, int n_paths, const char* out_path,
                            const vg_prefilter_params* p) {
    VG_API_BEGIN
    prefilter_stage("vg_prefilter", { fasta_paths, n_paths, nullptr, 0 }, out_path, p);
    VG_API_END
}
extern "C" int vg_prefilter_new(const char* const* db_paths, int n_db_paths, const char* const* new_paths, int n_new_paths,
                                const char* out_path, const vg_prefilter_params* p) {
    VG_API_BEGIN
    if (!db_paths) throw vg_error(VG_EINVAL, "vg_prefilter_new: null argument");
    prefilter_stage("vg_prefilter_new", { new_paths, n_new_paths, db_paths, n_db_paths }, out_path, p);
    VG_API_END
}

static void align_stage(const char* fn, const stage_input& in, const char* out_path, const vg_align_params* p) {
    if (!in.ok() || !out_path || !p) throw vg_error(VG_EINVAL, std::string(fn) + ": null argument");
    vg_host_mark((std::string(fn) + ": enter").c_str());
    vg_one_shot_scope one_shot;
    defer_scope parked;
    device_warmup warm(WARM_ALIGN);
    genomes_guard gg;
    const int n_db = in.load(p->is_multifasta, p->num_threads, &gg.g);
    warm.join();
    vg_require_device();
    free_guard pairs, tasks, regions; int64_t np = 0, nt = 0, nr = 0;
    if (n_db > 0 && !p->filter_path) {
        // no filter: every pair that contains a new genome (a filter written by vg_prefilter_new holds no other pair already)
        const int64_t n = vg_genomes_count(gg.g);
        np = n * (n - 1) / 2 - (int64_t)n_db * (n_db - 1) / 2;
        vg_pair_count* v = (vg_pair_count*)malloc(sizeof(vg_pair_count) * (size_t)std::max<int64_t>(1, np));
        if (!v) throw vg_error(VG_ENOMEM, "out of host memory");
        pairs.p = v;
        for (uint32_t a = (uint32_t)n_db; a < (uint32_t)n; ++a) for (uint32_t b = 0; b < a; ++b) *v++ = { a, b, 0 };
    } else
    check(vg_read_filter(gg.g, p->filter_path, p->filter_threshold, (vg_pair_count**)&pairs.p, &np));
    vg_host_mark("filter read");
    check(vg_lz_prepare(gg.g, (const vg_pair_count*)pairs.p, np, &p->lz));          // (the first index batch is built beside the task list)
    check(vg_align_tasks(gg.g, (const vg_pair_count*)pairs.p, np, (vg_task**)&tasks.p, &nt));
    std::vector<vg_pair_stat> stats((size_t)std::max<int64_t>(1, nt));
    const bool want_aln = p->out_aln_path != nullptr;
    check(vg_lz_align(gg.g, (const vg_task*)tasks.p, nt, &p->lz, stats.data(), want_aln ? (vg_region**)&regions.p : nullptr, &nr));
    {
        background_release rel;
        check(vg_write_ani(gg.g, (const vg_task*)tasks.p, stats.data(), nt, (const vg_region*)regions.p, nr, out_path, p));
    }
    vg_host_mark("ani.tsv written");
}
extern "C" int vg_align(const char* const* fasta_paths, int n_paths, const char* out_path, const vg_align_params* p) {
    VG_API_BEGIN
    align_stage("vg_align", { fasta_paths, n_paths, nullptr, 0 }, out_path, p);
    VG_API_END
}
extern "C" int vg_align_new(const char* const* db_paths, int n_db_paths, const char* const* new_paths, int n_new_paths,
                            const char* out_path, const vg_align_params* p) {
    VG_API_BEGIN
    if (!db_paths) throw vg_error(VG_EINVAL, "vg_align_new: null argument");
    align_stage("vg_align_new", { new_paths, n_new_paths, db_paths, n_db_paths }, out_path, p);
    VG_API_END
}

// the minimum of the metric that is the edge weight: the floor of the average-linkage hierarchy and the lowest level of any
static double metric_floor(const vg_cluster_params* p) {
    return !strcmp(p->metric, "tani") ? p->min_tani : !strcmp(p->metric, "gani") ? p->min_gani : p->min_ani;
}

// The skeleton of the file-level cluster entries, each of which checks its own null arguments and its algorithm first (`fn` names
// the entry in the error texts): the metric, the levels if any (none may lie below the metric's minimum), both files parsed beside
// the creation of the HIP context, then the entry's parts --
//   compute(in)    its further input (the prior clustering, the clusters file) and the array-level call, marked `computed`
//   write(in)      the output files
//   summary(in)    the line on stderr at verbosity 2
struct cluster_input {
    std::vector<std::string> ids; std::vector<uint32_t> q, r; std::vector<double> w;
    int64_t n() const { return (int64_t)ids.size(); }
    int64_t n_rows() const { return (int64_t)q.size(); }
};
template <class Compute, class Write, class Summary>
static void cluster_stage(const std::string& fn, const char* ani_path, const char* ids_path, const vg_cluster_params* p, const double* levels,
                          int n_levels, const char* computed, Compute compute, Write write, Summary summary) {
    if (strcmp(p->metric, "tani") && strcmp(p->metric, "gani") && strcmp(p->metric, "ani"))
        throw vg_error(VG_EINVAL, fn + ": metric must be tani, gani or ani, not " + p->metric);
    for (int l = 0; l < n_levels; ++l)
        if (!(levels[l] >= metric_floor(p)))          // (also a NaN)
            throw vg_error(VG_EINVAL, fn + ": level " + std::to_string(levels[l]) + " is below the " + p->metric + " minimum (rows below it are not edges)");
    vg_host_mark((fn + ": enter").c_str());
    cluster_input in;
    {
        device_warmup warm(WARM_CLUSTER);     // (the HIP context is created beside the parse)
        vg_cluster_read_ids(ids_path, in.ids);
        if (in.n() >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, std::string(ids_path) + ": 2^31 or more objects");
        vg_cluster_read_rows(ani_path, in.n(), p, in.q, in.r, in.w);
        vg_host_mark("ani.tsv parsed");
    }
    compute(in);
    vg_host_mark(computed);
    write(in);
    if (p->verbosity >= 2) summary(in);
}
// ... of the three entries that write one partition: compute(in, label, rep) fills what vg_cluster_write puts out
template <class Compute, class Summary>
static void partition_stage(const char* fn, const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p,
                            Compute compute, Summary summary) {
    std::vector<int32_t> label, rep;
    cluster_stage(fn, ani_path, ids_path, p, nullptr, 0, "clusters computed", [&](const cluster_input& in) {
        label.resize((size_t)std::max<int64_t>(in.n(), 1)); rep.resize(label.size());
        compute(in, label.data(), rep.data());
    }, [&](const cluster_input& in) { vg_cluster_write(out_path, in.ids, label.data(), rep.data(), p->representatives != 0); }, summary);
}

extern "C" int vg_cluster(const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p) {
    VG_API_BEGIN
    if (!ani_path || !ids_path || !out_path || !p || !p->metric) throw vg_error(VG_EINVAL, "vg_cluster: null argument");
    if (p->algorithm < VG_CLUSTER_SINGLE || p->algorithm > VG_CLUSTER_AVERAGE) throw vg_error(VG_EINVAL, "vg_cluster: unknown algorithm");
    vg_cluster_stats st{};
    partition_stage("vg_cluster", ani_path, ids_path, out_path, p, [&](const cluster_input& in, int32_t* label, int32_t* rep) {
        if (p->algorithm == VG_CLUSTER_AVERAGE) {               // the average-linkage hierarchy down to the metric's minimum, every merge joined
            vg_forest f;
            vg_cluster_forest("vg_cluster", in.n(), in.q.data(), in.r.data(), in.w.data(), in.n_rows(), f, VG_CLUSTER_AVERAGE, metric_floor(p));
            vg_forest_cut(in.n(), f, -HUGE_VAL, label, rep);
            st.rounds = f.stats.rounds; st.n_edges = f.stats.n_edges;
        } else
            check(vg_cluster_graph(in.n(), in.q.data(), in.r.data(), in.w.data(), in.n_rows(), p->algorithm, label, rep, &st));
    }, [&](const cluster_input& in) {
        fprintf(stderr, "vg_cluster: %lld objects, %lld rows passed, %lld edges, %lld rounds, %lld objects by the tail sweep\n",
                (long long)in.n(), (long long)in.n_rows(), (long long)st.n_edges, (long long)st.rounds, (long long)st.sweep_objects);
    });
    VG_API_END
}

extern "C" int vg_cluster_mcl(const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p,
                              const vg_mcl_params* params, vg_mcl_stats* stats) {
    VG_API_BEGIN
    if (!ani_path || !ids_path || !out_path || !p || !p->metric || !params) throw vg_error(VG_EINVAL, "vg_cluster_mcl: null argument");
    if (p->algorithm != VG_CLUSTER_MCL) throw vg_error(VG_EINVAL, "vg_cluster_mcl: the algorithm must be VG_CLUSTER_MCL");
    if (stats) *stats = vg_mcl_stats{};
    vg_mcl_stats st{};
    partition_stage("vg_cluster_mcl", ani_path, ids_path, out_path, p, [&](const cluster_input& in, int32_t* label, int32_t* rep) {
        check(vg_cluster_mcl_graph(in.n(), in.q.data(), in.r.data(), in.w.data(), in.n_rows(), params, label, rep, nullptr, nullptr, nullptr, &st));
    }, [&](const cluster_input& in) {
        fprintf(stderr, "vg_cluster_mcl: %lld objects, %lld rows passed, %lld edges, %lld iterations (%s), %lld entries, %lld LDS + %lld spill rows\n",
                (long long)in.n(), (long long)in.n_rows(), (long long)st.n_edges, (long long)st.iterations, st.converged ? "converged" : "not converged",
                (long long)st.nnz, (long long)st.lds_rows, (long long)st.spill_rows);
    });
    if (stats) *stats = st;
    VG_API_END
}

extern "C" int vg_cluster_update(const char* ani_path, const char* ids_path, const char* prior_path, int prior_is_repr,
                                 const char* out_path, const vg_cluster_params* p, vg_cluster_update_stats* stats) {
    VG_API_BEGIN
    if (!ani_path || !ids_path || !prior_path || !out_path || !p || !p->metric) throw vg_error(VG_EINVAL, "vg_cluster_update: null argument");
    if (p->algorithm != VG_CLUSTER_SINGLE && p->algorithm != VG_CLUSTER_CDHIT && p->algorithm != VG_CLUSTER_UCLUST)
        throw vg_error(VG_EINVAL, "vg_cluster_update: the update of a prior clustering is single, cd-hit or uclust");
    if (stats) *stats = vg_cluster_update_stats{};
    std::vector<int32_t> prior;
    vg_cluster_update_stats st{};
    partition_stage("vg_cluster_update", ani_path, ids_path, out_path, p, [&](const cluster_input& in, int32_t* label, int32_t* rep) {
        vg_cluster_read_prior(prior_path, in.ids, prior_is_repr != 0, prior);
        vg_host_mark("prior clusters parsed");
        check(vg_cluster_update_graph(in.n(), in.q.data(), in.r.data(), in.w.data(), in.n_rows(), p->algorithm, prior.data(), label, rep, &st));
    }, [&](const cluster_input& in) {
        fprintf(stderr, "vg_cluster_update: %lld prior + %lld new objects, %lld rows passed, %lld kept edges, %lld rounds, %lld objects by the tail sweep\n",
                (long long)st.n_prior, (long long)st.n_new, (long long)in.n_rows(), (long long)st.n_edges, (long long)st.rounds, (long long)st.sweep_objects);
    });
    if (stats) *stats = st;
    VG_API_END
}

extern "C" int vg_cluster_stats_file(const char* ani_path, const char* ids_path, const char* clusters_path, int clusters_is_repr,
                                     const vg_cluster_params* p, const char* out_path) {
    VG_API_BEGIN
    if (!ani_path || !ids_path || !clusters_path || !out_path || !p || !p->metric) throw vg_error(VG_EINVAL, "vg_cluster_stats_file: null argument");
    vg_label_columns cols;
    std::vector<std::vector<vg_cluster_stat>> stats;
    cluster_stage("vg_cluster_stats_file", ani_path, ids_path, p, nullptr, 0, "cluster report computed", [&](const cluster_input& in) {
        vg_cluster_read_columns(clusters_path, in.ids, clusters_is_repr != 0, cols);
        vg_host_mark("clusters.tsv parsed");
        const size_t nc = cols.names.size();
        stats.resize(nc);
        std::vector<const int32_t*> label(nc); std::vector<int64_t> n_clusters(nc); std::vector<vg_cluster_stat*> out(nc);
        for (size_t c = 0; c < nc; ++c) {
            stats[c].resize(cols.text[c].size());
            label[c] = cols.label[c].data(); n_clusters[c] = (int64_t)cols.text[c].size(); out[c] = stats[c].data();
        }
        vg_cluster_stats_run("vg_cluster_stats_file", in.n(), in.q.data(), in.r.data(), in.w.data(), in.n_rows(), (int)nc, label.data(),
                             n_clusters.data(), out.data(), nullptr, nullptr, nullptr);
    }, [&](const cluster_input& in) { vg_cluster_stats_write(out_path, p->metric, in.ids, cols, stats); },
    [&](const cluster_input& in) {
        fprintf(stderr, "vg_cluster_stats_file: %lld objects, %lld rows passed, %d label column(s)\n", (long long)in.n(), (long long)in.n_rows(), (int)cols.names.size());
    });
    VG_API_END
}

// The coverage map of an alignment table: both files and, if given, the clusters file parsed beside the
// creation of the HIP context, one array-level call, two writers.
extern "C" int vg_cover_file(const char* aln_path, const char* ids_path, const char* clusters_path, int clusters_is_repr, const char* column,
                             const char* out_path, const char* segments_path, int num_threads, int verbosity) {
    VG_API_BEGIN
    if (!aln_path || !ids_path || !out_path) throw vg_error(VG_EINVAL, "vg_cover_file: null argument");
    if (column && !clusters_path) throw vg_error(VG_EINVAL, "vg_cover_file: a label column needs a clusters file");
    vg_host_mark("vg_cover_file: enter");
    const int n_threads = num_threads > 0 ? num_threads : vg_host_threads();
    std::vector<std::string> ids; std::vector<int64_t> len;
    std::vector<uint32_t> q, r; std::vector<int32_t> qs, qe;
    vg_label_columns cols; size_t c = 0;
    {
        device_warmup warm(WARM_CLUSTER);
        vg_cluster_read_ids(ids_path, ids, &len);
        if ((int64_t)ids.size() >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, std::string(ids_path) + ": 2^31 or more objects");
        vg_cover_read_rows(aln_path, ids, len, n_threads, q, r, qs, qe);
        vg_host_mark("alignment table parsed");
        if (clusters_path) {
            vg_cluster_read_columns(clusters_path, ids, clusters_is_repr != 0, cols);
            if (column) {
                c = (size_t)(std::find(cols.names.begin(), cols.names.end(), std::string(column)) - cols.names.begin());
                if (c == cols.names.size()) throw vg_error(VG_EINVAL, std::string(clusters_path) + ":1: no label column '" + column + "'");
            }
            vg_host_mark("clusters.tsv parsed");
        }
    }
    const int64_t n = (int64_t)ids.size();
    const int32_t* group = clusters_path ? cols.label[c].data() : nullptr;
    std::vector<int64_t> group_size(clusters_path ? cols.text[c].size() : 1, clusters_path ? 0 : n);
    if (group) for (int64_t i = 0; i < n; ++i) ++group_size[(size_t)group[i]];
    std::vector<vg_cover_stat> stats((size_t)std::max<int64_t>(n, 1));
    free_guard seg; int64_t n_seg = 0;
    vg_cover_run_stats st{};
    check(vg_cover_rows(n, len.data(), group, (int64_t)group_size.size(), q.data(), r.data(), qs.data(), qe.data(), (int64_t)q.size(), stats.data(),
                        segments_path ? (vg_cover_segment**)&seg.p : nullptr, segments_path ? &n_seg : nullptr, &st));
    vg_host_mark("coverage computed");
    vg_cover_write(out_path, ids, group, clusters_path ? &cols.text[c] : nullptr, group_size, stats.data(), n_threads);
    if (segments_path) vg_cover_write_segments(segments_path, ids, (const vg_cover_segment*)seg.p, n_seg, n_threads);
    if (verbosity >= 1)
        fprintf(stderr, "vg_cover_file: %lld objects, %lld rows (%lld kept), %lld intervals, %lld breakpoints, %lld segments\n", (long long)n,
                (long long)q.size(), (long long)st.rows_kept, (long long)st.intervals, (long long)st.breakpoints, (long long)st.segments);
    VG_API_END
}

// The painting of an alignment table: read as vg_cover_file reads, one array-level call, three writers.
extern "C" int vg_paint_file(const char* aln_path, const char* ids_path, const char* clusters_path, int clusters_is_repr, const char* column,
                             const char* out_path, const char* segments_path, const char* donors_path, int num_threads, int verbosity) {
    VG_API_BEGIN
    if (!aln_path || !ids_path || !out_path) throw vg_error(VG_EINVAL, "vg_paint_file: null argument");
    if (column && !clusters_path) throw vg_error(VG_EINVAL, "vg_paint_file: a label column needs a clusters file");
    vg_host_mark("vg_paint_file: enter");
    const int n_threads = num_threads > 0 ? num_threads : vg_host_threads();
    std::vector<std::string> ids; std::vector<int64_t> len;
    std::vector<uint32_t> q, r; std::vector<int32_t> qs, qe, nm;
    vg_label_columns cols; size_t c = 0;
    {
        device_warmup warm(WARM_CLUSTER);
        vg_cluster_read_ids(ids_path, ids, &len);
        if ((int64_t)ids.size() >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, std::string(ids_path) + ": 2^31 or more objects");
        vg_cover_read_rows(aln_path, ids, len, n_threads, q, r, qs, qe, &nm);
        vg_host_mark("alignment table parsed");
        if (clusters_path) {
            vg_cluster_read_columns(clusters_path, ids, clusters_is_repr != 0, cols);
            if (column) {
                c = (size_t)(std::find(cols.names.begin(), cols.names.end(), std::string(column)) - cols.names.begin());
                if (c == cols.names.size()) throw vg_error(VG_EINVAL, std::string(clusters_path) + ":1: no label column '" + column + "'");
            }
            vg_host_mark("clusters.tsv parsed");
        }
    }
    const int64_t n = (int64_t)ids.size();
    const int32_t* group = clusters_path ? cols.label[c].data() : nullptr;
    std::vector<vg_paint_stat> stats((size_t)std::max<int64_t>(n, 1));
    free_guard seg, donor; int64_t n_seg = 0, n_donor = 0;
    vg_paint_run_stats st{};
    check(vg_paint_rows(n, len.data(), group, clusters_path ? (int64_t)cols.text[c].size() : 1, q.data(), r.data(), qs.data(), qe.data(), nm.data(),
                        (int64_t)q.size(), stats.data(), segments_path ? (vg_paint_segment**)&seg.p : nullptr, segments_path ? &n_seg : nullptr,
                        donors_path ? (vg_paint_donor**)&donor.p : nullptr, donors_path ? &n_donor : nullptr, &st));
    vg_host_mark("painting computed");
    vg_paint_write(out_path, ids, group, clusters_path ? &cols.text[c] : nullptr, stats.data(), n_threads);
    if (segments_path) vg_paint_write_segments(segments_path, ids, (const vg_paint_segment*)seg.p, n_seg, n_threads);
    if (donors_path) vg_paint_write_donors(donors_path, ids, len, (const vg_paint_donor*)donor.p, n_donor, n_threads);
    if (verbosity >= 1)
        fprintf(stderr, "vg_paint_file: %lld objects, %lld rows (%lld kept), %lld breakpoints, %lld levels, %lld segments, %lld donor records\n", (long long)n,
                (long long)q.size(), (long long)st.rows_kept, (long long)st.breakpoints, (long long)st.levels, (long long)st.segments, (long long)st.donor_records);
    VG_API_END
}

extern "C" int vg_cluster_linkage(const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p,
                                  const char* linkage_path, const double* levels, int n_levels) {
    VG_API_BEGIN
    if (!ani_path || !ids_path || !out_path || !p || !p->metric || n_levels < 0 || (n_levels && !levels))
        throw vg_error(VG_EINVAL, "vg_cluster_linkage: null argument");
    if (p->algorithm != VG_CLUSTER_SINGLE && p->algorithm != VG_CLUSTER_COMPLETE && p->algorithm != VG_CLUSTER_AVERAGE)
        throw vg_error(VG_EINVAL, "vg_cluster_linkage: the merge table is single, complete or average linkage (algorithm must be one of the three)");
    vg_forest f;
    cluster_stage("vg_cluster_linkage", ani_path, ids_path, p, levels, n_levels, "forest computed", [&](const cluster_input& in) {
        vg_cluster_forest("vg_cluster_linkage", in.n(), in.q.data(), in.r.data(), in.w.data(), in.n_rows(), f, p->algorithm, metric_floor(p));
    }, [&](const cluster_input& in) {
        // column 0: every merge (the cut at the floor, i.e. the algorithm on the passing rows); then one cut per level
        const int64_t n = in.n();
        const size_t cols = (size_t)n_levels + 1, stride = (size_t)std::max<int64_t>(n, 1);
        std::vector<int32_t> label(cols * stride), rep(cols * stride);
        std::vector<std::string> names = { "cluster" };
        std::vector<const int32_t*> lab_col, rep_col;
        for (size_t c = 0; c < cols; ++c) {
            vg_forest_cut(n, f, c ? levels[c - 1] : -HUGE_VAL, label.data() + c * stride, rep.data() + c * stride);
            lab_col.push_back(label.data() + c * stride); rep_col.push_back(rep.data() + c * stride);
            if (c) { char buf[64]; snprintf(buf, sizeof buf, "%g", levels[c - 1]); names.push_back(std::string(p->metric) + "_" + buf); }
        }
        if (linkage_path) {
            const size_t nf = std::max<size_t>(f.a.size(), 1);
            std::vector<int64_t> node_a(nf), node_b(nf), size(nf);
            vg_forest_table(n, f, node_a.data(), node_b.data(), size.data());
            vg_linkage_write(linkage_path, f, node_a.data(), node_b.data(), size.data());
        }
        vg_cluster_write_columns(out_path, in.ids, names, lab_col, rep_col, p->representatives != 0);
    }, [&](const cluster_input& in) {
        fprintf(stderr, "vg_cluster_linkage: %lld objects, %lld rows passed, %lld edges, %lld rounds, %lld merges, %d levels\n",
                (long long)in.n(), (long long)in.n_rows(), (long long)f.stats.n_edges, (long long)f.stats.rounds, (long long)f.stats.n_merges, n_levels);
    });
    VG_API_END
}
