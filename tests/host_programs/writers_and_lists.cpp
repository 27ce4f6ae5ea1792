// writers_and_lists — the threaded writers and list builders of the library's host side on generated arrays:
//   vg_write_fltr, vg_write_ani (all columns, with the alignment table), vg_filter_pairs below and above its 2^17-pair threaded
//   path, vg_align_tasks below and above its 2^21-pair parallel path, vg_align_pairs_share above 2^17 pairs.
//
//   writers_and_lists [threads ...]        (default: 1 3 16)
//
// The host thread count is read once per process, so every count runs in a forked child that sets VG_HOST_THREADS before its
// first call and leaves its files and arrays in a directory of its own; the parent compares them byte for byte across the
// counts and prints length and digest of each (the same in every build).  Exit status 0 only if every property held.
#include "host_programs.h"
#include "vg_common.h"
#include <sys/wait.h>

namespace {
using hp::fail;
const char* const OUTPUTS[] = { "fltr.txt", "fltr_max5.txt", "fltr_big.txt", "ani.tsv", "ani.ids.tsv", "ani.aln.tsv", "ani_filtered.tsv", "ani_filtered.ids.tsv",
                                "filter_small.bin", "filter_big.bin", "tasks_small.bin", "tasks_big.bin", "share_small.bin", "share_big.bin" };

void must(int status, const char* what) { if (status != VG_OK) { printf("FAILED %s: status %d %s\n", what, status, vg_last_error()); fflush(stdout); _exit(1); } }
void dump(const std::string& dir, const char* name, const void* p, size_t bytes) { hp::write_file(dir + "/" + name, std::string((const char*)p, bytes)); }

// 400 genomes of uneven length; partners skewed towards the low ids (a few genomes meet almost everyone)
std::vector<vg_pair_count> make_pairs(hp::rng64& r, int n, size_t count, const std::vector<int64_t>& sizes) {
    std::vector<vg_pair_count> v;
    while (v.size() < count) {
        const uint32_t a = 1 + (uint32_t)r.below((uint64_t)n - 1);
        const double u = (double)r.below(1u << 20) / (double)(1u << 20);
        const uint32_t b = (uint32_t)((double)a * u * u * u);
        const int64_t mn = std::min(sizes[a], sizes[b]);
        v.push_back({ a, b, (uint32_t)r.below((uint64_t)mn + 1) });
    }
    return v;
}

void child(int threads, const std::string& dir) {
    setenv("VG_HOST_THREADS", std::to_string(threads).c_str(), 1);
    hp::rng64 r{ 99 };
    const int n = 400;
    std::vector<uint8_t> codes; std::vector<int64_t> off{ 0 }; std::vector<std::string> names; std::vector<const char*> nm;
    for (int i = 0; i < n; ++i) { const size_t len = 20 + (size_t)r.below(i % 7 == 0 ? 30 : 3000); for (size_t k = 0; k < len; ++k) codes.push_back((uint8_t)r.below(5)); off.push_back((int64_t)codes.size()); names.push_back("gen" + std::to_string(1000 + i)); }
    for (const std::string& s : names) nm.push_back(s.c_str());
    vg_genomes* g = nullptr;
    must(vg_genomes_from_codes(codes.data(), off.data(), n, nm.data(), &g), "vg_genomes_from_codes");
    std::vector<int64_t> sizes; for (int i = 0; i < n; ++i) sizes.push_back(100 + (int64_t)r.below(5000));
    const std::vector<vg_pair_count> small = make_pairs(r, n, 3000, sizes), mid = make_pairs(r, n, 20000, sizes), big = make_pairs(r, n, 150000, sizes),
                                     huge = make_pairs(r, n, (1u << 21) + 4321, sizes);

    // fltr.txt
    must(vg_write_fltr(g, 25, 1.0, 20, 0.7, 0, sizes.data(), small.data(), (int64_t)small.size(), (dir + "/fltr.txt").c_str()), "vg_write_fltr");
    must(vg_write_fltr(g, 25, 0.2, 20, 0.7, 5, sizes.data(), small.data(), (int64_t)small.size(), (dir + "/fltr_max5.txt").c_str()), "vg_write_fltr, max_seqs");
    must(vg_write_fltr(g, 21, 1.0, 5, 0.5, 0, sizes.data(), big.data(), (int64_t)big.size(), (dir + "/fltr_big.txt").c_str()), "vg_write_fltr, 150 000 pairs");
    // the kept pairs, below and above the threaded path
    for (const auto& c : { std::make_pair(&small, "filter_small.bin"), std::make_pair(&big, "filter_big.bin") }) {
        vg_pair_count* kept = nullptr; int64_t nk = 0;
        must(vg_filter_pairs(25, 20, 0.7, sizes.data(), n, c.first->data(), (int64_t)c.first->size(), &kept, &nk), "vg_filter_pairs");
        // (a restatement of the rule, pair by pair)
        int64_t at = 0;
        for (const vg_pair_count& p : *c.first) {
            const bool keep = (int64_t)p.shared >= 20 && vg_ani_shorter(p.shared, sizes[p.a], sizes[p.b], 25) >= 0.7;
            if (keep && (at >= nk || kept[at].a != p.a || kept[at].b != p.b || kept[at].shared != p.shared)) { fail(std::string(c.second) + ": not the pairs of the rule, in order"); break; }
            at += keep;
        }
        if (at != nk) fail(std::string(c.second) + ": another number of kept pairs");
        dump(dir, c.second, kept, sizeof(vg_pair_count) * (size_t)nk);
        vg_free(kept);
    }
    // task lists, below and above the parallel path
    vg_task* mid_tasks = nullptr; int64_t n_mid_tasks = 0;
    for (const auto& c : { std::make_pair(&mid, "tasks_small.bin"), std::make_pair(&huge, "tasks_big.bin") }) {
        vg_task* tasks = nullptr; int64_t nt = 0;
        must(vg_align_tasks(g, c.first->data(), (int64_t)c.first->size(), &tasks, &nt), "vg_align_tasks");
        if (nt != 2 * (int64_t)c.first->size()) fail(std::string(c.second) + ": not two tasks per pair");
        for (int64_t t = 0; t + 1 < nt; t += 2) if (tasks[t].q != tasks[t + 1].r || tasks[t].r != tasks[t + 1].q) { fail(std::string(c.second) + ": a couple is not (q, r), (r, q)"); break; }
        dump(dir, c.second, tasks, sizeof(vg_task) * (size_t)nt);
        if (c.first == &mid) { mid_tasks = tasks; n_mid_tasks = nt; } else vg_free(tasks);
    }
    // a rank's share of the tasks
    for (const auto& c : { std::make_pair(&small, "share_small.bin"), std::make_pair(&big, "share_big.bin") }) {
        std::string all; int64_t total = 0;
        for (int rank = 0; rank < 4; ++rank) {
            vg_task* tasks = nullptr; int64_t nt = 0;
            must(vg_align_pairs_share(g, c.first->data(), (int64_t)c.first->size(), 4, rank, &tasks, &nt), "vg_align_pairs_share");
            all.append((const char*)tasks, sizeof(vg_task) * (size_t)nt); all += "|"; total += nt;
            vg_free(tasks);
        }
        if (total != 2 * (int64_t)c.first->size()) fail(std::string(c.second) + ": the ranks' shares do not add up to two tasks per pair");
        dump(dir, c.second, all.data(), all.size());
    }
    // ani.tsv with every column, its ids file and the alignment table: 40 000 rows are three pieces of the writer
    {
        std::vector<vg_pair_stat> stats((size_t)n_mid_tasks);
        std::vector<int64_t> len((size_t)n); vg_genomes_lengths(g, len.data());
        for (int64_t t = 0; t < n_mid_tasks; ++t) {
            const int64_t lq = len[mid_tasks[t].q];
            const uint32_t aln = (uint32_t)r.below((uint64_t)lq + 1);
            stats[(size_t)t] = { (uint32_t)r.below((uint64_t)aln + 1), aln, (uint32_t)r.below(9) };
        }
        std::vector<vg_region> regions;
        for (int k = 0; k < 5000; ++k) {
            vg_region x; memset(&x, 0, sizeof x);
            x.task = (uint32_t)r.below((uint64_t)n_mid_tasks + 3);
            const int64_t lq = len[mid_tasks[x.task < n_mid_tasks ? x.task : 0].q], lr = len[mid_tasks[x.task < n_mid_tasks ? x.task : 0].r];
            x.qstart = (int)r.below((uint64_t)lq); x.qend = x.qstart + (int)r.below((uint64_t)(lq - x.qstart));
            x.rstart = (int)r.below((uint64_t)(2 * lr + 1)); x.rend = x.rstart + (x.qend - x.qstart);
            x.n_match = (int)r.below((uint64_t)(x.qend - x.qstart + 2));
            regions.push_back(x);
        }
        static const char* const columns[] = { "qidx", "ridx", "query", "reference", "tani", "gani", "ani", "qcov", "rcov", "num_alns", "len_ratio", "qlen", "rlen", "nt_match", "nt_mismatch" };
        vg_align_params p; memset(&p, 0, sizeof p);
        p.out_columns = columns; p.n_out_columns = 15; p.num_threads = threads;
        const std::string aln = dir + "/ani.aln.tsv"; p.out_aln_path = aln.c_str();
        must(vg_write_ani(g, mid_tasks, stats.data(), n_mid_tasks, regions.data(), (int64_t)regions.size(), (dir + "/ani.tsv").c_str(), &p), "vg_write_ani");
        p.out_aln_path = nullptr; p.out_ani = 0.5; p.out_qcov = 0.3; p.n_out_columns = 11;
        must(vg_write_ani(g, mid_tasks, stats.data(), n_mid_tasks, nullptr, 0, (dir + "/ani_filtered.tsv").c_str(), &p), "vg_write_ani, filtered");
        p.n_out_columns = 15; static const char* const unknown[] = { "qidx", "no_such_column" }; p.out_columns = unknown; p.n_out_columns = 2;
        if (vg_write_ani(g, mid_tasks, stats.data(), n_mid_tasks, nullptr, 0, (dir + "/never.tsv").c_str(), &p) != VG_EINVAL || !*vg_last_error()) fail("vg_write_ani: an unknown column was taken");
        if (vg_write_ani(g, mid_tasks, stats.data(), n_mid_tasks - 1, nullptr, 0, (dir + "/never.tsv").c_str(), &p) != VG_EINVAL) fail("vg_write_ani: an odd task count was taken");
    }
    // a pair outside the set is an error of every list builder, on the threaded path too
    {
        std::vector<vg_pair_count> bad = big; bad[bad.size() - 7].a = (uint32_t)n;
        vg_pair_count* kept = nullptr; int64_t nk = 0; vg_task* tasks = nullptr; int64_t nt = 0;
        if (vg_filter_pairs(25, 20, 0.7, sizes.data(), n, bad.data(), (int64_t)bad.size(), &kept, &nk) != VG_EINVAL) fail("vg_filter_pairs: a pair outside the set was taken");
        if (vg_align_tasks(g, bad.data(), (int64_t)bad.size(), &tasks, &nt) != VG_EINVAL) fail("vg_align_tasks: a pair outside the set was taken");
        if (vg_align_pairs_share(g, bad.data(), (int64_t)bad.size(), 4, 1, &tasks, &nt) != VG_EINVAL) fail("vg_align_pairs_share: a pair outside the set was taken");
    }
    vg_free(mid_tasks);
    delete g;
}
}  // namespace

int main(int argc, char** argv) {
    std::vector<int> threads;
    for (int i = 1; i < argc; ++i) threads.push_back(atoi(argv[i]));
    if (threads.empty()) threads = { 1, 3, 16 };
    hp::scratch_dir top;            // (its destructor removes the files and directories named here, whatever became of the children)
    std::vector<std::string> dirs;
    for (const int t : threads) {
        const std::string sub = "t" + std::to_string(t);
        for (const char* name : OUTPUTS) top.file(sub + "/" + name);
        top.file(sub + "/never.tsv");
        dirs.push_back(top.dir(sub));
        fflush(stdout);
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); return 2; }
        if (pid == 0) { child(t, dirs.back()); fflush(stdout); _exit(hp::failures() ? 1 : 0); }
        int st = 0;
        if (waitpid(pid, &st, 0) != pid || !WIFEXITED(st) || WEXITSTATUS(st) != 0) fail("the run with " + std::to_string(t) + " threads did not end well");
    }
    for (const char* name : OUTPUTS) {
        std::string first;
        for (size_t k = 0; k < dirs.size(); ++k) {
            std::string bytes;
            if (!hp::read_file(dirs[k] + "/" + name, bytes)) { fail(std::string(name) + ": missing at " + std::to_string(threads[k]) + " threads"); continue; }
            if (k == 0) { first = bytes; printf("%-22s %9zu bytes  %016llx\n", name, bytes.size(), (unsigned long long)hp::fnv(bytes.data(), bytes.size())); }
            else if (bytes != first) fail(std::string(name) + ": other bytes at " + std::to_string(threads[k]) + " threads than at " + std::to_string(threads[0]));
        }
    }
    return hp::finish();
}
