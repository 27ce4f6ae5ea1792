// vg_io.cpp — host side of the two stages: everything that turns the GPU's integers into the
// reference's files.  Floating point appears only here (ani-shorter uses log; ANI ratios are
// fp64 quotients of integers), so file identity with the CPU oracle reduces to integer identity.
//   fltr.txt            layout of example/output/fltr.txt        
//   ani.tsv, ids.tsv    layout of example/output/ani{,.ids}.tsv  
//   ani.aln.tsv         layout of example/output/ani.aln.tsv     
//   cluster stage       ids file + ani.tsv rows in, clusters.tsv out
#include "vg_common.h"
#include <climits>
#include <cmath>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <mutex>
#include <numeric>
#include <charconv>
#include <string_view>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

// ---------------------------------------------------------------- numbers
double vg_ani_shorter(int64_t shared, int64_t na, int64_t nb, int k) {
    int64_t mn = std::min(na, nb);
    if (mn <= 0 || shared <= 0) return 0.0;
    double j = (double)shared / (double)mn;
    return 1.0 + log(2.0 * j / (1.0 + j)) / (double)k;
}

// LZ-ANI prints a double with the shortest "%.{1..6}g" that reproduces it exactly, else with six
// significant digits in fixed notation (zeros kept), exact decimal ties rounded away from zero.
static int fmt_num_exact(double x, char* buf) {
    for (int prec = 1; prec <= 6; ++prec) {
        char t[64];
        snprintf(t, sizeof t, "%.*g", prec, x);
        if (strtod(t, nullptr) == x) { strcpy(buf, t); return (int)strlen(buf); }
    }
    bool neg = x < 0; double ax = neg ? -x : x;
    char full[400];
    snprintf(full, sizeof full, "%.150f", ax);                 // exact binary expansion
    std::string digits; int int_len = 0; bool seen_dot = false;
    for (char* c = full; *c; ++c) { if (*c == '.') { seen_dot = true; continue; } digits.push_back(*c); if (!seen_dot) ++int_len; }
    size_t first = 0; while (first < digits.size() && digits[first] == '0') ++first;
    size_t keep = std::min(digits.size(), first + 6);
    bool up = keep < digits.size() && digits[keep] >= '5';
    digits.resize(keep);
    if (up) {
        int j = (int)keep - 1;
        while (j >= 0 && digits[j] == '9') { digits[j] = '0'; --j; }
        if (j >= 0) digits[j]++; else { digits.insert(digits.begin(), '1'); ++int_len; }
    }
    std::string out = neg ? "-" : "";
    if ((int)digits.size() <= int_len) { out += digits; out.append(int_len - digits.size(), '0'); }
    else { out += digits.substr(0, int_len); out.push_back('.'); out += digits.substr(int_len); }
    strcpy(buf, out.c_str());
    return (int)out.size();
}

// Fast path for the overwhelmingly common case (a generic quotient that has no <= 6-digit decimal
// representation and is not near a rounding tie): six significant digits by one multiplication.
// Anything within 1e-6 of a short decimal or of a tie goes through the exact routine above.
int vg_fmt_num(double x, char* buf) {
    static const double P10[] = { 1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18 };
    if (!(x > 1e-12 && x < 1e6)) return fmt_num_exact(x, buf);
    int e = 0;                                                  // x in [10^e, 10^(e+1))
    if (x >= 1.0) { while (e < 6 && x >= P10[e + 1]) ++e; }
    else { e = -1; while (e > -13 && x < 1.0 / P10[-e]) --e; }
    const int k = 5 - e;                                        // y = x * 10^k in [1e5, 1e6)
    const double y = (k >= 0) ? x * P10[k] : x / P10[-k];
    const double fl = floor(y); const double fr = y - fl;
    if (!(y >= 1e5 && y < 999999.0)) return fmt_num_exact(x, buf);
    if (fr < 1e-6 || fr > 1.0 - 1e-6 || (fr > 0.5 - 1e-6 && fr < 0.5 + 1e-6)) return fmt_num_exact(x, buf);
    long d = (long)fl + (fr > 0.5 ? 1 : 0);                     // 6 significant digits
    char dig[8]; for (int i = 5; i >= 0; --i) { dig[i] = (char)('0' + d % 10); d /= 10; }
    int o = 0;
    if (e >= 0) {                                               // e+1 integer digits (e <= 5)
        for (int i = 0; i <= e; ++i) buf[o++] = dig[i];
        if (e < 5) { buf[o++] = '.'; for (int i = e + 1; i < 6; ++i) buf[o++] = dig[i]; }
    } else {
        buf[o++] = '0'; buf[o++] = '.';
        for (int i = 0; i < -e - 1; ++i) buf[o++] = '0';
        for (int i = 0; i < 6; ++i) buf[o++] = dig[i];
    }
    buf[o] = 0;
    return o;
}

int vg_fmt_len_ratio(int64_t a, int64_t b, char* buf) {
    if (a == b) { strcpy(buf, "1"); return 1; }
    return snprintf(buf, 32, "%.4f", (double)std::min(a, b) / (double)std::max(a, b));
}

// ---------------------------------------------------------------- files: the three shared pieces
void vg_write_file(const char* path, const std::vector<std::string_view>& parts) {
    struct closer { void operator()(FILE* f) const { fclose(f); } };
    std::unique_ptr<FILE, closer> f(fopen(path, "w"));
    if (!f) throw vg_error(VG_EIO, std::string("cannot write ") + path);
    bool ok = true;
    for (const std::string_view& p : parts) ok = ok && (p.empty() || fwrite(p.data(), 1, p.size(), f.get()) == p.size());
    ok = fclose(f.release()) == 0 && ok;
    if (!ok) throw vg_error(VG_EIO, std::string("write error on ") + path);
}

namespace {
// head, then the rows [0, n) formatted in pieces of `piece` rows by n_threads threads (fn(lo, hi, out) appends the rows
// lo .. hi - 1 to out) and written in order: the pieces are cut by row number alone, so the bytes do not depend on n_threads
template <class F> void write_rows(const char* path, const std::string& head, int64_t n, int64_t piece, int n_threads, F fn) {
    std::vector<std::string> text((size_t)((n + piece - 1) / piece));
    vg_parallel_for((int64_t)text.size(), n_threads, [&](int64_t c) { fn(c * piece, std::min(n, (c + 1) * piece), text[(size_t)c]); });
    std::vector<std::string_view> parts{ head };
    parts.insert(parts.end(), text.begin(), text.end());
    vg_write_file(path, parts);
}

// a whole text file, read-only: a regular non-empty file is mapped, anything else (a pipe, a file without a size) is read into
// memory; an empty file has n == 0.  `what` goes into the one error, "cannot open <what><path>"
struct text_file {
    const char* p = nullptr; size_t n = 0;
    explicit text_file(const char* path, const char* what = "") {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) throw vg_error(VG_EIO, std::string("cannot open ") + what + path);
        struct closer { int fd; ~closer() { close(fd); } } cl{ fd };
        struct stat sb;
        if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
            m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) { n = (size_t)sb.st_size; (void)madvise(m, n, MADV_WILLNEED); p = (const char*)m; return; }
        }
        char buf[1 << 16];
        for (ssize_t r; (r = read(fd, buf, sizeof buf)) > 0;) own.append(buf, (size_t)r);
        p = own.data(); n = own.size();
    }
    ~text_file() { if (m != MAP_FAILED) munmap(m, n); }
    text_file(const text_file&) = delete; text_file& operator=(const text_file&) = delete;
    const char* end() const { return p + n; }
    const char* line_end(const char* a) const { const char* e = (const char*)memchr(a, '\n', (size_t)(end() - a)); return e ? e : end(); }
    int64_t line_of(const char* at) const {          // 1-based line number of a position (errors only)
        int64_t l = 1;
        for (const char* x = p; (x = (const char*)memchr(x, '\n', (size_t)(at - x))) != nullptr; ++x) ++l;
        return l;
    }
private:
    void* m = MAP_FAILED; std::string own;
};
// fn(line number from 1, the line without its '\n' and without a '\r' in front of that) for every line; nothing is skipped
template <class F> void for_each_line(const text_file& f, F fn) {
    int64_t line = 0;
    for (const char* a = f.p; a < f.end();) {
        const char* e = f.line_end(a);
        fn(++line, std::string_view(a, (size_t)((e > a && e[-1] == '\r' ? e - 1 : e) - a)));
        a = e + 1;
    }
}
void split_fields(std::string_view text, char sep, std::vector<std::string_view>& fields) {
    fields.clear();
    for (size_t a = 0;;) {
        const size_t t = text.find(sep, a);
        fields.push_back(text.substr(a, t == std::string_view::npos ? t : t - a));
        if (t == std::string_view::npos) break;
        a = t + 1;
    }
}
// an array the C ABI hands to its caller (vg_free): never of size 0
template <class T> std::unique_ptr<T, decltype(&free)> host_array(size_t n) {
    std::unique_ptr<T, decltype(&free)> o((T*)malloc(sizeof(T) * std::max<size_t>(1, n)), &free);
    if (!o) throw vg_error(VG_ENOMEM, "out of host memory");
    return o;
}
}  // namespace

// ---------------------------------------------------------------- fltr.txt
extern "C" int vg_filter_pairs(int k, int min_kmers, double min_ident, const int64_t* set_sizes, int64_t n_genomes,
                               const vg_pair_count* pairs, int64_t n_pairs, vg_pair_count** out, int64_t* n_out) {
    VG_API_BEGIN
    if (!set_sizes || (!pairs && n_pairs) || !out || !n_out) throw vg_error(VG_EINVAL, "vg_filter_pairs: null argument");
    // ani >= min_ident  <=>  j = shared / min(|A|, |B|) >= J*, J* = E / (2 - E), E = exp((min_ident - 1) k): one
    // division per pair instead of a logarithm.  A pair within 1e-9 (relative) of the threshold is decided by the
    // formula itself, so the kept set is exactly the formula's.
    vg_host_mark("filter_pairs: enter");
    const double E = std::exp((min_ident - 1.0) * (double)k);
    const double Jstar = E < 2.0 ? E / (2.0 - E) : INFINITY;
    auto kept_pairs = host_array<vg_pair_count>((size_t)n_pairs);
    vg_pair_count* const o = kept_pairs.get();
    int64_t total = 0;
    auto keeps = [&](const vg_pair_count& p) {
        if ((int64_t)p.a >= n_genomes || (int64_t)p.b >= n_genomes) throw vg_error(VG_EINVAL, "pair id out of range");
        if ((int64_t)p.shared < min_kmers) return false;
        const int64_t mn = std::min(set_sizes[p.a], set_sizes[p.b]);
        if (mn <= 0 || p.shared == 0) return 0.0 >= min_ident;
        const double j = (double)p.shared / (double)mn;
        if (std::isfinite(Jstar) && std::fabs(j - Jstar) > 1e-9 * Jstar) return j > Jstar;
        return vg_ani_shorter(p.shared, set_sizes[p.a], set_sizes[p.b], k) >= min_ident;
    };
    // (10^5 .. 10^6 pairs -- every rank of a sharded call does this between the stages --: chunks over a few threads, kept pairs counted, then written in order)
    const int T = n_pairs >= (1 << 17) ? std::max(1, std::min(vg_host_threads(), 8)) : 1;
    if (T == 1) { for (int64_t i = 0; i < n_pairs; ++i) if (keeps(pairs[i])) o[total++] = pairs[i]; }
    else {
        std::vector<int64_t> kept((size_t)T + 1, 0);
        std::vector<uint8_t> flag((size_t)n_pairs);
        vg_parallel_chunks(n_pairs, T, [&](int64_t a, int64_t b, int t) { int64_t c = 0; for (int64_t i = a; i < b; ++i) { flag[(size_t)i] = keeps(pairs[i]); c += flag[(size_t)i]; } kept[(size_t)t + 1] = c; });
        for (int t = 0; t < T; ++t) kept[(size_t)t + 1] += kept[(size_t)t];
        vg_parallel_chunks(n_pairs, T, [&](int64_t a, int64_t b, int t) { int64_t at = kept[(size_t)t]; for (int64_t i = a; i < b; ++i) if (flag[(size_t)i]) o[at++] = pairs[i]; });
        total = kept[(size_t)T];
    }
    vg_host_mark("filter_pairs: done");
    *out = kept_pairs.release(); *n_out = total;
    VG_API_END
}

extern "C" int vg_write_fltr(const vg_genomes* g, int k, double fraction, int min_kmers, double min_ident,
                             int max_seqs, const int64_t* set_sizes, const vg_pair_count* pairs,
                             int64_t n_pairs, const char* out_path) {
    VG_API_BEGIN
    if (!g || !set_sizes || (!pairs && n_pairs) || !out_path) throw vg_error(VG_EINVAL, "vg_write_fltr: null argument");
    // rows by a counting sort on the row genome (the pairs arrive in no order), then every row sorted by column
    const size_t ng = (size_t)std::max(g->n, 0);
    std::vector<size_t> first(ng + 2, 0);
    for (int64_t i = 0; i < n_pairs; ++i) { const uint32_t a = std::max(pairs[i].a, pairs[i].b); if (a < ng) first[a + 1]++; }
    for (size_t a = 0; a < ng; ++a) first[a + 1] += first[a];
    struct cell { uint32_t b, shared; };
    std::vector<cell> cells(first[ng]);
    {
        std::vector<size_t> cur(first.begin(), first.begin() + (std::ptrdiff_t)ng);
        for (int64_t i = 0; i < n_pairs; ++i) {
            const uint32_t a = std::max(pairs[i].a, pairs[i].b), bb = std::min(pairs[i].a, pairs[i].b);
            if (a < ng) cells[cur[a]++] = { bb, pairs[i].shared };
        }
    }
    char buf[64];
    std::string head(buf, (size_t)snprintf(buf, sizeof buf, "kmer-length: %d fraction: %g ,", k, fraction));
    for (int i = 0; i < g->n; ++i) { head += g->names[i]; head += ','; }
    head += '\n';
    write_rows(out_path, head, (int64_t)ng, 512, std::max(1, std::min(vg_host_threads(), 16)), [&](int64_t lo, int64_t hi, std::string& o) {
        struct ent { uint32_t col; double ani; };
        std::vector<ent> row; char buf[64];
        for (int64_t a = lo; a < hi; ++a) {
            o += g->names[(size_t)a]; o += ',';
            cell* c0 = cells.data() + first[(size_t)a]; cell* c1 = cells.data() + first[(size_t)a + 1];
            std::sort(c0, c1, [](const cell& x, const cell& y) { return x.b < y.b; });
            row.clear();
            for (cell* c = c0; c < c1;) {
                uint64_t sh = 0; const uint32_t bcol = c->b;
                for (; c < c1 && c->b == bcol; ++c) sh += c->shared;           // per-shard partial counts add up
                if ((int64_t)sh < min_kmers || bcol >= (uint32_t)g->n || bcol == (uint32_t)a) continue;
                const double ani = vg_ani_shorter((int64_t)sh, set_sizes[a], set_sizes[bcol], k);
                if (ani >= min_ident) row.push_back({ bcol, ani });
            }
            if (max_seqs > 0 && (int)row.size() > max_seqs) {
                std::sort(row.begin(), row.end(), [](const ent& x, const ent& y) { return x.ani != y.ani ? x.ani > y.ani : x.col < y.col; });
                row.resize((size_t)max_seqs);
                std::sort(row.begin(), row.end(), [](const ent& x, const ent& y) { return x.col < y.col; });
            }
            for (auto& e : row) { const int n = snprintf(buf, sizeof buf, "%u:%.6f,", e.col + 1, e.ani); o.append(buf, (size_t)n); }
            o += '\n';
        }
    });
    VG_API_END
}

// ---------------------------------------------------------------- align: order, filter, tasks
void vg_length_order(const vg_genomes* g) {
    if ((int)g->len_order.size() == g->n && (int)g->len_rank.size() == g->n) return;
    std::vector<int32_t> order((size_t)g->n), rank((size_t)g->n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return g->len[x] > g->len[y]; });
    for (int i = 0; i < g->n; ++i) rank[(size_t)order[(size_t)i]] = i;
    g->len_order.swap(order); g->len_rank.swap(rank);
}

extern "C" int vg_align_order(const vg_genomes* g, int32_t* order) {
    VG_API_BEGIN
    if (!g || !order) throw vg_error(VG_EINVAL, "vg_align_order: null argument");
    vg_length_order(g);
    if (g->n) memcpy(order, g->len_order.data(), sizeof(int32_t) * (size_t)g->n);
    VG_API_END
}

// the filter file, in stages: header columns, one cell, a byte range of whole rows, the order of the couples
namespace {
// names -> genome ids.  A filter written from the same FASTA lists the genomes in the set's own order: a name is first compared
// with the name the order predicts (one string compare); the hash map over all names is only built when a name turns up
// somewhere else.
struct name_lookup {
    const vg_genomes* g;
    std::unordered_map<std::string_view, uint32_t> by_name; std::once_flag by_name_once;
    bool is(int64_t id, std::string_view name) const { return id >= 0 && id < (int64_t)g->n && g->names[(size_t)id] == name; }
    int64_t operator()(std::string_view name, int64_t guess) {
        if (is(guess, name)) return guess;
        std::call_once(by_name_once, [&] { by_name.reserve((size_t)g->n * 2); for (int i = 0; i < g->n; ++i) by_name.emplace(g->names[i], (uint32_t)i); });
        auto it = by_name.find(name);
        return it == by_name.end() ? -1 : (int64_t)it->second;
    }
};
// header: the genome id of every column (-1: a name the set does not have)
std::vector<int64_t> filter_columns(std::string_view header, name_lookup& lookup) {
    std::vector<std::string_view> fields;
    split_fields(header, ',', fields);
    std::vector<int64_t> col_id;
    for (size_t c = 1; c + 1 < fields.size(); ++c) col_id.push_back(lookup(fields[c], (int64_t)c - 1));     // (behind the last ',': nothing)
    return col_id;
}
// one cell "column:value" -> the 0-based column (anything but digits: what atol makes of it) and the value
bool filter_cell(const char* q, const char* fe, long& ci, double& val) {
    const char* colon = (const char*)memchr(q, ':', (size_t)(fe - q));
    if (!colon) return false;
    ci = 0;
    const char* d = q; bool ok = d < colon;
    // (a column number too long for a long saturates, as atol's does: such a column does not exist)
    for (; d < colon; ++d) { if (*d < '0' || *d > '9') { ok = false; break; } ci = ci > (LONG_MAX - 9) / 10 ? LONG_MAX : ci * 10 + (*d - '0'); }
    if (!ok) ci = atol(std::string(q, colon).c_str());
    if (ci > LONG_MIN) ci -= 1;
    // value: digits '.' digits with <= 15 digits is exact as mantissa / 10^k; anything else goes to strtod
    static const double p10[16] = { 1, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15 };
    uint64_t m = 0; int nd = 0, frac = -1; bool plain = colon + 1 < fe;
    for (const char* x = colon + 1; x < fe && plain; ++x) {
        if (*x >= '0' && *x <= '9') { m = m * 10 + (uint64_t)(*x - '0'); ++nd; if (frac >= 0) ++frac; }
        else if (*x == '.' && frac < 0) frac = 0; else plain = false;
    }
    val = plain && nd <= 15 ? (double)m / p10[frac < 0 ? 0 : frac] : atof(std::string(colon + 1, fe).c_str());
    return true;
}
// the rows of the byte range [lo, hi) of the body, cut to whole lines (a line belongs to the range its first byte is in),
// parsed in place (no per-field strings)
void filter_rows(const text_file& f, const char* body, size_t lo, size_t hi, const std::vector<int64_t>& col_id, name_lookup& lookup,
                 double thr, std::vector<vg_pair_count>& out) {
    const vg_genomes* g = lookup.g;
    auto behind = [&](const char* nl) { return nl < f.end() ? nl + 1 : nl; };               // (the start of the line behind a line end)
    auto line_start = [&](size_t at) { return at == 0 ? body : behind(f.line_end(body + at - 1)); };
    const char* a = line_start(lo); const char* const stop = body + hi < f.end() ? line_start(hi) : f.end();
    // the row in front of this one, + 1.  The first row of a range has no row in front of it: the first range starts at
    // genome 0, the others look around the genome their byte offset suggests (rows of similar length: a few thousand name
    // compares at most) before the hash map over all names is built for them
    int64_t guess = lo == 0 ? 0 : -1;
    bool first_row = lo > 0;
    while (a < stop) {
        const char* nl = f.line_end(a);
        const char* q = a; const char* const e = nl > a && nl[-1] == '\r' ? nl - 1 : nl;
        a = behind(nl);
        const char* c = (const char*)memchr(q, ',', (size_t)(e - q)); if (!c) continue;
        const std::string_view name(q, (size_t)(c - q));
        if (first_row) {
            first_row = false;
            const int64_t est = (int64_t)((double)g->n * (double)(a - body) / (double)std::max<size_t>(1, (size_t)(f.end() - body)));
            for (int64_t d = 0; d <= 4096 && guess < 0; ++d)
                for (int64_t cand : { est + d, est - d }) if (lookup.is(cand, name)) { guess = cand; break; }
        }
        const int64_t row = lookup(name, guess);
        if (row >= 0) guess = row + 1;
        for (q = c + 1; q < e;) {
            const char* n2 = (const char*)memchr(q, ',', (size_t)(e - q)); const char* fe = n2 ? n2 : e;
            long ci; double val;
            if (filter_cell(q, fe, ci, val) && row >= 0 && ci >= 0 && ci < (long)col_id.size() && col_id[(size_t)ci] >= 0 && col_id[(size_t)ci] != row && val >= thr) {
                const uint32_t x = (uint32_t)row, y = (uint32_t)col_id[(size_t)ci];
                out.push_back({ std::max(x, y), std::min(x, y), 0 });
            }
            if (!n2) break;
            q = n2 + 1;
        }
    }
}
// ascending (a, b), every couple once: long lists by two stable counting passes over the genome ids (b, then a), short ones
// by a comparison sort
void order_couples(std::vector<vg_pair_count>& v, int n) {
    if ((int64_t)v.size() > 4 * (int64_t)n) {
        std::vector<vg_pair_count> tmp(v.size()); std::vector<int64_t> at((size_t)n + 1);
        for (int pass = 0; pass < 2; ++pass) {
            std::fill(at.begin(), at.end(), 0);
            for (const auto& e : v) at[(size_t)(pass ? e.a : e.b) + 1]++;
            for (int i = 0; i < n; ++i) at[(size_t)i + 1] += at[(size_t)i];
            for (const auto& e : v) tmp[(size_t)at[(size_t)(pass ? e.a : e.b)]++] = e;
            v.swap(tmp);
        }
    } else
        std::sort(v.begin(), v.end(), [](const vg_pair_count& x, const vg_pair_count& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    v.erase(std::unique(v.begin(), v.end(), [](const vg_pair_count& x, const vg_pair_count& y) { return x.a == y.a && x.b == y.b; }), v.end());
}
}  // namespace

extern "C" int vg_read_filter(const vg_genomes* g, const char* path, double thr, vg_pair_count** pairs, int64_t* n_pairs) {
    VG_API_BEGIN
    if (!g || !pairs || !n_pairs) throw vg_error(VG_EINVAL, "vg_read_filter: null argument");
    std::vector<vg_pair_count> v;
    if (!path) {
        for (uint32_t a = 1; a < (uint32_t)g->n; ++a) for (uint32_t b = 0; b < a; ++b) v.push_back({ a, b, 0 });
    } else {
        const text_file f(path, "filter ");
        name_lookup lookup{ g };
        const char* hdr_end = f.line_end(f.p);
        const std::vector<int64_t> col_id = filter_columns(std::string_view(f.p, (size_t)((hdr_end > f.p && hdr_end[-1] == '\r' ? hdr_end - 1 : hdr_end) - f.p)), lookup);
        // rows: parsed by several threads, each a range of whole lines
        const char* body = hdr_end < f.end() ? hdr_end + 1 : hdr_end;
        const int n_thr = std::max(1, std::min(vg_host_threads(), 16));
        std::vector<std::vector<vg_pair_count>> part((size_t)n_thr);
        vg_parallel_chunks((int64_t)(f.end() - body), n_thr, [&](int64_t lo, int64_t hi, int t) { filter_rows(f, body, (size_t)lo, (size_t)hi, col_id, lookup, thr, part[(size_t)t]); });
        for (auto& pv : part) v.insert(v.end(), pv.begin(), pv.end());
        order_couples(v, g->n);
    }
    auto o = host_array<vg_pair_count>(v.size());
    if (!v.empty()) memcpy(o.get(), v.data(), sizeof(vg_pair_count) * v.size());
    *pairs = o.release(); *n_pairs = (int64_t)v.size();
    VG_API_END
}

extern "C" int vg_align_tasks(const vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs,
                              vg_task** tasks, int64_t* n_tasks) {
    return vg_align_tasks_perm(g, pairs, n_pairs, tasks, n_tasks, nullptr);
}
// the same, also telling which pair every canonical couple came from (perm[c] = index into `pairs` of the couple whose
// rows are tasks 2c and 2c + 1): the sharded align stage places gathered rows through it
int vg_align_tasks_perm(const vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs,
                        vg_task** tasks, int64_t* n_tasks, uint32_t* perm) {
    VG_API_BEGIN
    if (!g || (!pairs && n_pairs) || !tasks || !n_tasks) throw vg_error(VG_EINVAL, "vg_align_tasks: null argument");
    if (perm && n_pairs >= (1LL << 32)) throw vg_error(VG_EOVERFLOW, "more than 2^32 pairs");
    vg_host_mark("align_tasks: enter");
    vg_length_order(g);
    vg_host_mark("align_tasks: length order");
    const std::vector<int32_t>& order = g->len_order; const std::vector<int32_t>& rank = g->len_rank;
    // couples sorted by (lo, hi) of the length ranks; couple i of the sorted list becomes the task rows 2i and 2i + 1
    struct rp { int32_t lo, hi; uint32_t idx; };
    auto couple = [&](int64_t i) {
        if (pairs[i].a >= (uint32_t)g->n || pairs[i].b >= (uint32_t)g->n) throw vg_error(VG_EINVAL, "pair id out of range");
        const int32_t x = rank[pairs[i].a], y = rank[pairs[i].b];
        return rp{ std::min(x, y), std::max(x, y), (uint32_t)i };
    };
    auto o = host_array<vg_task>(2 * (size_t)n_pairs);
    vg_task* const row = o.get();
    auto emit = [&](int64_t i, const rp& c) {
        row[2 * i] = { (uint32_t)order[(size_t)c.hi], (uint32_t)order[(size_t)c.lo] };        // row (q = b, r = a)
        row[2 * i + 1] = { (uint32_t)order[(size_t)c.lo], (uint32_t)order[(size_t)c.hi] };    // row (q = a, r = b)
        if (perm) perm[i] = c.idx;
    };
    if (n_pairs >= (1 << 21) && vg_host_threads() > 1) {
        // millions of couples (contigs-1M: 3.5 M, 75 ms on one thread): range partition on lo over the threads (counts,
        // offsets, scatter), every range sorted on its own, the task couples written in parallel
        const int T = std::max(2, std::min(vg_host_threads(), 16));
        const int64_t ng = std::max<int64_t>(1, g->n);
        std::vector<rp, no_init_alloc<rp>> v, tmp; v.resize((size_t)n_pairs); tmp.resize((size_t)n_pairs);      // (84 MB at 3.5 M couples: not cleared by one thread first)
        std::vector<std::vector<int64_t>> cnt((size_t)T, std::vector<int64_t>((size_t)T + 1, 0));
        auto bucket_of = [&](int32_t lo) { return (int)((int64_t)lo * T / ng); };
        vg_parallel_chunks(n_pairs, T, [&](int64_t a, int64_t b, int t) {
            for (int64_t i = a; i < b; ++i) { v[(size_t)i] = couple(i); cnt[(size_t)t][(size_t)bucket_of(v[(size_t)i].lo)]++; }
        });
        std::vector<int64_t> b_first((size_t)T + 1, 0);
        { int64_t run = 0; for (int bk = 0; bk < T; ++bk) { b_first[(size_t)bk] = run; for (int t = 0; t < T; ++t) { const int64_t c = cnt[(size_t)t][(size_t)bk]; cnt[(size_t)t][(size_t)bk] = run; run += c; } } b_first[(size_t)T] = run; }
        vg_parallel_chunks(n_pairs, T, [&](int64_t a, int64_t b, int t) {
            for (int64_t i = a; i < b; ++i) tmp[(size_t)cnt[(size_t)t][(size_t)bucket_of(v[(size_t)i].lo)]++] = v[(size_t)i];
        });
        vg_parallel_for(T, T, [&](int64_t bk) {
            std::sort(tmp.begin() + b_first[(size_t)bk], tmp.begin() + b_first[(size_t)bk + 1], [](const rp& x, const rp& y) { return x.lo != y.lo ? x.lo < y.lo : (x.hi != y.hi ? x.hi < y.hi : x.idx < y.idx); });
            for (int64_t i = b_first[(size_t)bk]; i < b_first[(size_t)bk + 1]; ++i) emit(i, tmp[(size_t)i]);
        });
    } else {
        // two stable counting passes, on hi and then on lo (LSD order).  One thread: 10^5..10^6 couples are a few
        // milliseconds of cache-resident work, less than starting helpers costs.
        std::vector<rp> v((size_t)n_pairs), tmp((size_t)n_pairs);
        std::vector<int64_t> at_lo((size_t)g->n + 1, 0), at_hi((size_t)g->n + 1, 0);
        for (int64_t i = 0; i < n_pairs; ++i) { v[(size_t)i] = couple(i); at_lo[(size_t)v[(size_t)i].lo + 1]++; at_hi[(size_t)v[(size_t)i].hi + 1]++; }
        for (int key = 0; key < g->n; ++key) { at_lo[(size_t)key + 1] += at_lo[(size_t)key]; at_hi[(size_t)key + 1] += at_hi[(size_t)key]; }
        for (int64_t i = 0; i < n_pairs; ++i) tmp[(size_t)at_hi[(size_t)v[(size_t)i].hi]++] = v[(size_t)i];
        for (int64_t i = 0; i < n_pairs; ++i) v[(size_t)at_lo[(size_t)tmp[(size_t)i].lo]++] = tmp[(size_t)i];
        for (int64_t i = 0; i < n_pairs; ++i) emit(i, v[(size_t)i]);
    }
    vg_host_mark("align_tasks: done");
    *tasks = o.release(); *n_tasks = 2 * n_pairs;
    VG_API_END
}

// ---------------------------------------------------------------- ani.tsv / ids.tsv / aln.tsv
void vg_ani_row_values(int64_t lq, int64_t lr, const vg_pair_stat& x, const vg_pair_stat& rev, vg_ani_row& row) {
    row.ani = x.aln_len ? (double)x.n_match / (double)x.aln_len : 0.0;
    row.gani = lq ? (double)x.n_match / (double)lq : 0.0;
    row.qcov = lq ? (double)x.aln_len / (double)lq : 0.0;
    row.rcov = lr ? (double)rev.aln_len / (double)lr : 0.0;
    row.tani = (lq + lr) ? (double)((uint64_t)x.n_match + rev.n_match) / (double)(lq + lr) : 0.0;
    row.len_ratio = lq == lr ? 1.0 : (double)std::min(lq, lr) / (double)std::max(lq, lr);
    row.num_alns = x.n_regions;
}
void vg_ani_row_printed(int64_t lq, int64_t lr, const vg_ani_row& row, vg_ani_row& printed) {
    char buf[64];
    auto reread = [&](int n) {
        double v = 0;
        const auto r = std::from_chars(buf, buf + n, v);
        if (r.ec != std::errc() || r.ptr != buf + n) throw vg_error(VG_EHIP, std::string("a printed number does not read back: ") + buf);
        return v;
    };
    printed.tani = reread(vg_fmt_num(row.tani, buf)); printed.gani = reread(vg_fmt_num(row.gani, buf));
    printed.ani = reread(vg_fmt_num(row.ani, buf)); printed.qcov = reread(vg_fmt_num(row.qcov, buf));
    printed.rcov = reread(vg_fmt_num(row.rcov, buf));
    printed.len_ratio = reread(vg_fmt_len_ratio(lq, lr, buf));
    printed.num_alns = row.num_alns;
}
bool vg_cluster_row_passes(const vg_cluster_params* p, const vg_ani_row& v, double* w) {
    *w = !strcmp(p->metric, "tani") ? v.tani : !strcmp(p->metric, "gani") ? v.gani : v.ani;
    const std::pair<double, double> filters[] = { { v.tani, p->min_tani }, { v.gani, p->min_gani }, { v.ani, p->min_ani },
                                                  { v.qcov, p->min_qcov }, { v.rcov, p->min_rcov }, { v.len_ratio, p->min_len_ratio } };
    for (auto& fl : filters) if (fl.second > 0 && !(fl.first >= fl.second)) return false;
    return !(p->max_num_alns > 0) || (double)v.num_alns <= (double)p->max_num_alns;
}
void vg_fasta_write_records(const char* path, const vg_fasta_text& text, const std::vector<int64_t>& which) {
    std::vector<std::string_view> parts;
    for (const int64_t i : which) {
        const vg_fasta_rec& r = text.recs[(size_t)i];
        parts.emplace_back(r.hdr - 1, (size_t)(r.end - (r.hdr - 1)));       // from the '>' to the start of the next record
        if (r.end[-1] != '\n') parts.emplace_back("\n");                      // (the last record of a file without a final line end)
    }
    vg_write_file(path, parts);
}

// the deduplicate stage's output FASTA: the kept records (rep[i] == i) in input order, assembled in memory by all threads, then
// written plain or as gzip members of GZ_BLOCK uncompressed bytes each (compressed in parallel: the bytes do not depend on the thread count)
constexpr size_t GZ_BLOCK = 4u << 20;
void vg_fasta_write_kept(const char* path, const vg_fasta_text& in, const std::vector<std::string>& prefix, const int32_t* rep, int level, int T) {
    const int64_t n = (int64_t)in.recs.size();
    std::vector<int64_t> kept;
    for (int64_t i = 0; i < n; ++i) if (rep[i] == (int32_t)i) kept.push_back(i);
    auto size_of = [&](const vg_fasta_rec& r) {
        const int64_t sl = r.end - r.seq;
        return (int64_t)(1 + prefix[(size_t)r.file].size() + (r.hdr_end - r.hdr) + 1 + sl + (sl > 0 && r.end[-1] != '\n'));
    };
    std::vector<int64_t> at(kept.size() + 1, 0);
    for (size_t k = 0; k < kept.size(); ++k) at[k + 1] = at[k] + size_of(in.recs[(size_t)kept[k]]);
    std::vector<char, no_init_alloc<char>> buf((size_t)at.back());
    vg_parallel_for((int64_t)kept.size(), T, [&](int64_t k) {
        const vg_fasta_rec& r = in.recs[(size_t)kept[(size_t)k]];
        char* o = buf.data() + at[(size_t)k];
        const std::string& pf = prefix[(size_t)r.file];
        *o++ = '>'; memcpy(o, pf.data(), pf.size()); o += pf.size();
        memcpy(o, r.hdr, (size_t)(r.hdr_end - r.hdr)); o += r.hdr_end - r.hdr; *o++ = '\n';
        memcpy(o, r.seq, (size_t)(r.end - r.seq)); o += r.end - r.seq;
        if (r.end > r.seq && r.end[-1] != '\n') *o++ = '\n';
    });
    if (level <= 0) { vg_write_file(path, { { buf.data(), buf.size() } }); return; }
    const int64_t nb = std::max<int64_t>(1, ((int64_t)buf.size() + (int64_t)GZ_BLOCK - 1) / (int64_t)GZ_BLOCK);
    std::vector<std::vector<unsigned char>> member((size_t)nb);
    vg_parallel_for(nb, T, [&](int64_t b) {
        const size_t lo = (size_t)b * GZ_BLOCK, len = std::min(GZ_BLOCK, buf.size() - std::min(buf.size(), lo));
        z_stream zs; memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw vg_error(VG_ENOMEM, "deflateInit2 failed");
        std::vector<unsigned char>& out = member[(size_t)b];
        out.resize(deflateBound(&zs, (uLong)len) + 32);
        zs.next_in = (Bytef*)(buf.data() + lo); zs.avail_in = (uInt)len;
        zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
        const int rc = deflate(&zs, Z_FINISH);
        out.resize(out.size() - zs.avail_out);
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) throw vg_error(VG_EIO, "gzip compression failed");
    });
    std::vector<std::string_view> parts;
    for (auto& m : member) parts.emplace_back((const char*)m.data(), m.size());
    vg_write_file(path, parts);
}

extern "C" int vg_write_ani(const vg_genomes* g, const vg_task* tasks, const vg_pair_stat* stats, int64_t n_tasks,
                            const vg_region* regions, int64_t n_regions, const char* out_path, const vg_align_params* p) {
    VG_API_BEGIN
    if (!g || (!tasks && n_tasks) || (!stats && n_tasks) || !out_path || !p) throw vg_error(VG_EINVAL, "vg_write_ani: null argument");
    // the arguments first: an error leaves no file behind
    if (n_tasks & 1) throw vg_error(VG_EINVAL, "vg_write_ani: tasks must come in (q,r),(r,q) couples");
    enum column { QIDX, RIDX, QUERY, REFERENCE, TANI, GANI, ANI, QCOV, RCOV, NUM_ALNS, LEN_RATIO, QLEN, RLEN, NT_MATCH, NT_MISMATCH };
    constexpr int N_COLUMNS = NT_MISMATCH + 1;
    static const char* const known[N_COLUMNS] = { "qidx", "ridx", "query", "reference", "tani", "gani", "ani", "qcov", "rcov", "num_alns",
                                                  "len_ratio", "qlen", "rlen", "nt_match", "nt_mismatch" };
    std::vector<column> columns;
    std::string head;
    for (int c = 0; c < p->n_out_columns; ++c) {
        const char* const* kn = std::find_if(known, known + N_COLUMNS, [&](const char* x) { return !strcmp(x, p->out_columns[c]); });
        if (kn == known + N_COLUMNS) throw vg_error(VG_EINVAL, std::string("unknown output column ") + p->out_columns[c]);
        columns.push_back((column)(kn - known));
        if (c) head += '\t';
        head += *kn;
    }
    head += '\n';
    for (int64_t t = 0; t < n_tasks; ++t)
        if (tasks[t ^ 1].q != tasks[t].r || tasks[t ^ 1].r != tasks[t].q) throw vg_error(VG_EINVAL, "vg_write_ani: task couple mismatch");
    vg_length_order(g);
    const std::vector<int32_t>& order = g->len_order; const std::vector<int32_t>& rank = g->len_rank;
    {
        std::string ids(out_path);
        if (ids.size() > 4 && ids.compare(ids.size() - 4, 4, ".tsv") == 0) ids.resize(ids.size() - 4);
        ids += ".ids.tsv";
        std::string o = "id\tseq_len\tno_parts\n";
        for (int32_t i : order) { o += g->names[(size_t)i]; o += '\t'; o += std::to_string(g->len[(size_t)i]); o += '\t'; o += std::to_string(g->n_parts[(size_t)i]); o += '\n'; }
        vg_write_file(ids.c_str(), { o });
    }
    const int nthreads = std::max(1, std::min(p->num_threads > 0 ? p->num_threads : 8, 64));
    const int64_t chunk = 1 << 14;
    write_rows(out_path, head, n_tasks, chunk, nthreads, [&](int64_t lo, int64_t hi, std::string& o) {
        o.reserve((size_t)chunk * 96);
        char buf[64];
        for (int64_t t = lo; t < hi; ++t) {
            const vg_task& tk = tasks[t]; const vg_pair_stat& x = stats[t]; const vg_pair_stat& rev = stats[t ^ 1];
            int64_t lq = g->len[tk.q], lr = g->len[tk.r];
            vg_ani_row row; vg_ani_row_values(lq, lr, x, rev, row);
            const double ani = row.ani, gani = row.gani, qcov = row.qcov, rcov = row.rcov, tani = row.tani;
            if (p->out_tani > 0 && tani < p->out_tani) continue;
            if (p->out_gani > 0 && gani < p->out_gani) continue;
            if (p->out_ani > 0 && ani < p->out_ani) continue;
            if (p->out_qcov > 0 && qcov < p->out_qcov) continue;
            if (p->out_rcov > 0 && rcov < p->out_rcov) continue;
            auto num = [&](double v) { o.append(buf, (size_t)vg_fmt_num(v, buf)); };
            for (size_t c = 0; c < columns.size(); ++c) {
                if (c) o.push_back('\t');
                switch (columns[c]) {
                case QIDX: o += std::to_string(rank[tk.q]); break;
                case RIDX: o += std::to_string(rank[tk.r]); break;
                case QUERY: o += g->names[tk.q]; break;
                case REFERENCE: o += g->names[tk.r]; break;
                case TANI: num(tani); break;
                case GANI: num(gani); break;
                case ANI: num(ani); break;
                case QCOV: num(qcov); break;
                case RCOV: num(rcov); break;
                case NUM_ALNS: o += std::to_string(x.n_regions); break;
                case LEN_RATIO: o.append(buf, (size_t)vg_fmt_len_ratio(lq, lr, buf)); break;
                case QLEN: o += std::to_string(lq); break;
                case RLEN: o += std::to_string(lr); break;
                case NT_MATCH: o += std::to_string(x.n_match); break;
                case NT_MISMATCH: o += std::to_string(x.aln_len - x.n_match); break;
                }
            }
            o.push_back('\n');
        }
    });

    if (p->out_aln_path && regions) {
        std::vector<vg_region> v(regions, regions + n_regions);
        std::sort(v.begin(), v.end(), [](const vg_region& x, const vg_region& y) {
            if (x.task != y.task) return x.task < y.task;
            int lx = x.qend - x.qstart, ly = y.qend - y.qstart;
            if (lx != ly) return lx > ly;
            return x.qstart < y.qstart;
        });
        std::string o = "query\treference\tpident\talnlen\tqstart\tqend\trstart\trend\tnt_match\tnt_mismatch\n";
        for (auto& r : v) {
            if ((int64_t)r.task >= n_tasks) continue;
            const vg_task& tk = tasks[r.task];
            int64_t L = g->len[tk.r];
            // fwd | N | rc space -> 1-based forward; the strand of a region is that of its rstart (rend is a
            // virtual end and may lie past the end of the strand)
            const bool rev = r.rstart > L;
            auto fwd1 = [&](int64_t rr) { return rev ? L - (rr - (L + 1)) : rr + 1; };
            int alnlen = r.qend - r.qstart + 1; char buf[64], row[160];
            vg_fmt_num(100.0 * r.n_match / alnlen, buf);
            o += g->names[tk.q]; o += '\t'; o += g->names[tk.r];
            o.append(row, (size_t)snprintf(row, sizeof row, "\t%s\t%d\t%d\t%d\t%lld\t%lld\t%d\t%d\n", buf, alnlen,
                                           r.qstart + 1, r.qend + 1, (long long)fwd1(r.rstart), (long long)fwd1(r.rend), r.n_match, alnlen - r.n_match));
        }
        vg_write_file(p->out_aln_path, { o });
    }
    VG_API_END
}

// ---------------------------------------------------------------- cluster stage: ids file, ani.tsv rows, clusters.tsv
namespace {
[[noreturn]] void row_error(const char* path, int64_t line, const std::string& what) {
    throw vg_error(VG_EINVAL, std::string(path) + ":" + std::to_string(line) + ": " + what);
}
bool parse_double(const char* a, const char* b, double& v) {
    auto r = std::from_chars(a, b, v);
    return r.ec == std::errc() && r.ptr == b && a != b;
}
}  // namespace

void vg_cluster_read_ids(const char* path, std::vector<std::string>& ids, std::vector<int64_t>* seq_len) {
    const text_file f(path);
    ids.clear();
    if (seq_len) seq_len->clear();
    std::vector<std::string_view> fields;
    size_t len_col = 0;
    for_each_line(f, [&](int64_t line, std::string_view text) {
        if (line > 1 && !text.empty()) ids.emplace_back(text.substr(0, text.find('\t')));       // (line 1: the header)
        if (!seq_len || (line > 1 && text.empty())) return;
        split_fields(text, '\t', fields);
        if (line == 1) {
            len_col = (size_t)(std::find(fields.begin(), fields.end(), std::string_view("seq_len")) - fields.begin());
            if (len_col == fields.size()) row_error(path, 1, "missing column seq_len");
            return;
        }
        if (fields.size() <= len_col) row_error(path, line, "expected at least " + std::to_string(len_col + 1) + " columns, found " + std::to_string(fields.size()));
        const std::string_view v = fields[len_col];
        uint64_t x = 0;
        const auto rr = std::from_chars(v.data(), v.data() + v.size(), x);
        if (rr.ec != std::errc() || rr.ptr != v.data() + v.size() || x >= (1ull << 31)) row_error(path, line, "malformed seq_len '" + std::string(v) + "'");
        seq_len->push_back((int64_t)x);
    });
    if (seq_len && !f.n) row_error(path, 1, "empty file (no header)");
}

void vg_cluster_read_rows(const char* path, int64_t n_objects, const vg_cluster_params* p,
                          std::vector<uint32_t>& q, std::vector<uint32_t>& r, std::vector<double>& w) {
    const text_file f(path);
    if (!f.n) row_error(path, 1, "empty file (no header)");
    const char* end = f.end();
    const char* hdr_end = f.line_end(f.p);
    std::vector<std::string_view> fields;
    split_fields(std::string_view(f.p, (size_t)(hdr_end - f.p)), '\t', fields);
    const std::vector<std::string> names(fields.begin(), fields.end());
    auto col_of = [&](const char* name) {
        for (size_t c = 0; c < names.size(); ++c) if (names[c] == name) return (int)c;
        row_error(path, 1, std::string("missing column ") + name);
    };
    // columns: 0 qidx, 1 ridx, 2 the metric, then the active minimums and num_alns
    std::vector<int> cols = { col_of("qidx"), col_of("ridx"), col_of(p->metric) };
    std::vector<double> mins;
    const std::pair<const char*, double> filters[] = { { "tani", p->min_tani }, { "gani", p->min_gani }, { "ani", p->min_ani },
                                                       { "qcov", p->min_qcov }, { "rcov", p->min_rcov }, { "len_ratio", p->min_len_ratio } };
    for (auto& fl : filters) if (fl.second > 0) { cols.push_back(col_of(fl.first)); mins.push_back(fl.second); }
    const int na_slot = p->max_num_alns > 0 ? (int)cols.size() : -1;
    if (na_slot >= 0) cols.push_back(col_of("num_alns"));
    const int max_col = *std::max_element(cols.begin(), cols.end());

    // the body cut into chunks at line starts, one per thread; each chunk keeps its passing rows and its first error
    const char* body = hdr_end < end ? hdr_end + 1 : end;
    const int nthr = (int)std::max<int64_t>(1, std::min<int64_t>(p->num_threads > 0 ? p->num_threads : vg_host_threads(),
                                                                 (int64_t)((end - body) >> 20) + 1));
    std::vector<const char*> cut((size_t)nthr + 1, end);
    cut[0] = body;
    for (int t = 1; t < nthr; ++t) {
        const char* x = body + (end - body) * t / nthr;
        x = std::max(x, cut[(size_t)t - 1]);
        cut[(size_t)t] = x < end ? std::min(end, f.line_end(x) + 1) : end;
    }
    struct part { std::vector<uint32_t> q, r; std::vector<double> w; const char* err_at = nullptr; std::string err; };
    std::vector<part> parts((size_t)nthr);
    vg_parallel_for(nthr, nthr, [&](int64_t t) {
        part& pt = parts[(size_t)t];
        std::vector<const char*> fb((size_t)max_col + 1), fe((size_t)max_col + 1);
        std::vector<double> v(cols.size());
        for (const char* a = cut[(size_t)t]; a < cut[(size_t)t + 1];) {
            const char* e = f.line_end(a);
            if (e == a) { a = e + 1; continue; }                // (blank line)
            int nf = 0;
            for (const char* x = a; nf <= max_col;) {
                const char* tb = (const char*)memchr(x, '\t', (size_t)(e - x));
                fb[(size_t)nf] = x; fe[(size_t)nf] = tb ? tb : e; ++nf;
                if (!tb) break;
                x = tb + 1;
            }
            if (nf <= max_col) { pt.err_at = a; pt.err = "expected " + std::to_string(names.size()) + " columns, found " + std::to_string(nf); return; }
            uint64_t idx[2];
            for (int k = 0; k < 2; ++k) {
                const char* x = fb[(size_t)cols[(size_t)k]]; const char* y = fe[(size_t)cols[(size_t)k]];
                auto rr = std::from_chars(x, y, idx[k]);
                if (rr.ec != std::errc() || rr.ptr != y || x == y) { pt.err_at = a; pt.err = "malformed " + names[(size_t)cols[(size_t)k]] + " '" + std::string(x, y) + "'"; return; }
                if (idx[k] >= (uint64_t)n_objects) {
                    pt.err_at = a; pt.err = names[(size_t)cols[(size_t)k]] + " " + std::to_string(idx[k]) + " outside the ids file (" + std::to_string(n_objects) + " objects)"; return;
                }
            }
            for (size_t k = 2; k < cols.size(); ++k) {
                const char* x = fb[(size_t)cols[k]]; const char* y = fe[(size_t)cols[k]];
                if (!parse_double(x, y, v[k])) { pt.err_at = a; pt.err = "malformed " + names[(size_t)cols[k]] + " '" + std::string(x, y) + "'"; return; }
            }
            bool pass = idx[0] != idx[1];
            for (size_t k = 0; k < mins.size() && pass; ++k) pass = v[3 + k] >= mins[k];
            if (pass && na_slot >= 0) pass = v[(size_t)na_slot] <= (double)p->max_num_alns;
            if (pass) { pt.q.push_back((uint32_t)idx[0]); pt.r.push_back((uint32_t)idx[1]); pt.w.push_back(v[2]); }
            a = e + 1;
        }
    });
    size_t total = 0;
    for (auto& pt : parts) {
        if (pt.err_at) row_error(path, f.line_of(pt.err_at), pt.err);
        total += pt.q.size();
    }
    q.clear(); r.clear(); w.clear();
    q.reserve(total); r.reserve(total); w.reserve(total);
    for (auto& pt : parts) {
        q.insert(q.end(), pt.q.begin(), pt.q.end()); r.insert(r.end(), pt.r.begin(), pt.r.end()); w.insert(w.end(), pt.w.begin(), pt.w.end());
    }
}

namespace {
// an "object, then label column(s)" file against the ids: line 1 is the header, every other line that is not empty names an
// object of the ids file once and carries one value per label column.  The views point into the file.
struct label_file {
    std::unordered_map<std::string_view, int32_t> index;       // id -> object
    std::vector<std::string_view> names;                        // the header behind "object"
    std::vector<int32_t> listed;                                // the objects in the order of their lines
    std::vector<int64_t> line_of;                               // per object: its line (0: it has none)
    std::vector<std::string_view> value;                        // value[i * n_cols + c]
    size_t n_cols = 0;
    int64_t n_lines = 0;
};
// prior: the header is exactly object<TAB>cluster (and the texts of the two "malformed" errors are those of the prior file)
void read_label_file(const text_file& f, const char* path, const std::vector<std::string>& ids, bool prior, label_file& lf) {
    if (!f.n) row_error(path, 1, "empty file (no header)");
    lf.index.reserve(ids.size() * 2);
    for (size_t i = 0; i < ids.size(); ++i) lf.index.emplace(ids[i], (int32_t)i);
    lf.line_of.assign(ids.size(), 0);
    std::vector<std::string_view> fields;
    for_each_line(f, [&](int64_t line, std::string_view text) {
        lf.n_lines = line;
        if (line > 1 && text.empty()) return;
        split_fields(text, '\t', fields);
        bool ok = line == 1 ? fields.size() >= 2 && fields[0] == "object" : fields.size() == lf.n_cols + 1;
        for (const std::string_view& x : fields) ok = ok && !x.empty();
        if (line == 1) {
            if (prior ? text != "object\tcluster" : !ok)
                row_error(path, 1, prior ? "malformed header (expected object<TAB>cluster)" : "malformed header (expected object<TAB>cluster, then further label columns)");
            lf.names.assign(fields.begin() + 1, fields.end());
            lf.n_cols = lf.names.size();
            lf.value.assign(ids.size() * lf.n_cols, std::string_view());
            return;
        }
        if (!ok) row_error(path, line, prior ? "malformed line (expected <object><TAB><cluster>)" : "malformed line (expected " + std::to_string(lf.n_cols + 1) + " fields)");
        const auto it = lf.index.find(fields[0]);
        if (it == lf.index.end()) row_error(path, line, "object '" + std::string(fields[0]) + "' is not in the ids file");
        const size_t i = (size_t)it->second;
        if (lf.line_of[i]) row_error(path, line, "object '" + std::string(fields[0]) + "' is listed twice");
        lf.line_of[i] = line;
        lf.listed.push_back(it->second);
        std::copy(fields.begin() + 1, fields.end(), lf.value.begin() + (std::ptrdiff_t)(i * lf.n_cols));
    });
}
// a cluster number up to `max`; the whole value must be one
uint64_t cluster_number(const char* path, int64_t line, std::string_view v, uint64_t max) {
    uint64_t number = 0;
    const auto rr = std::from_chars(v.data(), v.data() + v.size(), number);
    if (rr.ec != std::errc() || rr.ptr != v.data() + v.size() || number > max) row_error(path, line, "malformed cluster number '" + std::string(v) + "'");
    return number;
}
}  // namespace

void vg_cluster_read_prior(const char* path, const std::vector<std::string>& ids, bool is_repr, std::vector<int32_t>& prior_rep) {
    const text_file f(path);
    label_file lf;
    read_label_file(f, path, ids, true, lf);
    prior_rep.assign(ids.size(), -1);
    if (is_repr) {
        // the value names an object of this file; then: that object names itself
        for (const int32_t obj : lf.listed) {
            const auto it = lf.index.find(lf.value[(size_t)obj]);
            if (it == lf.index.end() || !lf.line_of[(size_t)it->second])
                row_error(path, lf.line_of[(size_t)obj], "representative '" + std::string(lf.value[(size_t)obj]) + "' is not an object of this file");
            prior_rep[(size_t)obj] = it->second;
        }
        for (const int32_t obj : lf.listed)
            if (prior_rep[(size_t)prior_rep[(size_t)obj]] != prior_rep[(size_t)obj])
                row_error(path, lf.line_of[(size_t)obj], "representative '" + std::string(lf.value[(size_t)obj]) + "' is not its own representative");
        return;
    }
    // cluster numbers (any 64-bit one): the representative is the earliest member in the ids file
    std::unordered_map<uint64_t, int32_t> first;
    std::vector<uint64_t> number(ids.size());
    for (const int32_t obj : lf.listed) {
        number[(size_t)obj] = cluster_number(path, lf.line_of[(size_t)obj], lf.value[(size_t)obj], UINT64_MAX);
        const auto ins = first.emplace(number[(size_t)obj], obj);
        if (!ins.second && obj < ins.first->second) ins.first->second = obj;
    }
    for (const int32_t obj : lf.listed) prior_rep[(size_t)obj] = first[number[(size_t)obj]];
}

void vg_cluster_read_columns(const char* path, const std::vector<std::string>& ids, bool is_repr, vg_label_columns& out) {
    const text_file f(path);
    label_file lf;
    read_label_file(f, path, ids, false, lf);
    const size_t n_cols = lf.n_cols;
    const std::vector<std::string_view>& value = lf.value;
    out.names.assign(lf.names.begin(), lf.names.end());
    if (!is_repr)
        for (const int32_t obj : lf.listed)
            for (size_t c = 0; c < n_cols; ++c) cluster_number(path, lf.line_of[(size_t)obj], value[(size_t)obj * n_cols + c], (1ull << 31) - 1);
    for (size_t i = 0; i < ids.size(); ++i)
        if (!lf.line_of[i]) row_error(path, lf.n_lines, "object '" + ids[i] + "' of the ids file is missing");
    // representative ids: the value names an object, and that object names itself in the same column
    if (is_repr)
        for (size_t i = 0; i < ids.size(); ++i)
            for (size_t c = 0; c < n_cols; ++c) {
                const std::string_view v = value[i * n_cols + c];
                const auto it = lf.index.find(v);
                if (it == lf.index.end()) row_error(path, lf.line_of[i], "representative '" + std::string(v) + "' is not in the ids file");
                if (value[(size_t)it->second * n_cols + c] != v)
                    row_error(path, lf.line_of[i], "representative '" + std::string(v) + "' is not a member of its cluster");
            }
    // the clusters of a column, numbered by their earliest member
    out.label.assign(n_cols, std::vector<int32_t>(ids.size()));
    out.text.assign(n_cols, {});
    for (size_t c = 0; c < n_cols; ++c) {
        std::unordered_map<std::string_view, int32_t> by_text; std::unordered_map<uint64_t, int32_t> by_number;
        for (size_t i = 0; i < ids.size(); ++i) {
            const std::string_view v = value[i * n_cols + c];
            const int32_t next = (int32_t)out.text[c].size();
            int32_t k;
            if (is_repr) k = by_text.emplace(v, next).first->second;
            else { uint64_t number = 0; std::from_chars(v.data(), v.data() + v.size(), number); k = by_number.emplace(number, next).first->second; }
            if (k == next) out.text[c].emplace_back(v);
            out.label[c][i] = k;
        }
    }
}

void vg_cluster_stats_write(const char* path, const char* metric, const std::vector<std::string>& ids, const vg_label_columns& cols,
                            const std::vector<std::vector<vg_cluster_stat>>& stats) {
    const std::string m(metric);
    std::string o = "column\tcluster\tsize\trepresentative\tpairs\tlinked\tmin_" + m + "\tmean_linked\tmean_all\texternal\tnearest\tnearest_" + m +
                    "\tnearest_mean\tmisfits\n";
    char buf[64];
    auto num = [&](uint64_t v) { o.push_back('\t'); o += std::to_string(v); };
    // the double nearest S / (P * 2^32), by the exact division of the average-linkage table; no denominator (or no value): `-`
    auto quotient = [&](bool have, uint64_t S, uint64_t P) {
        o.push_back('\t');
        if (!have || P == 0) { o.push_back('-'); return; }
        snprintf(buf, sizeof buf, "%.6g", vg_cluster_average_similarity(S, P));
        o += buf;
    };
    for (size_t c = 0; c < cols.names.size(); ++c)
        for (size_t k = 0; k < stats[c].size(); ++k) {
            const vg_cluster_stat& s = stats[c][k];
            if (s.size == 0) continue;
            const bool near = s.nearest >= 0;
            o += cols.names[c]; o.push_back('\t'); o += cols.text[c][k];
            num((uint64_t)s.size); o.push_back('\t'); o += ids[(size_t)s.rep];
            num(s.pairs); num(s.linked);
            quotient(s.linked != 0, s.min, 1); quotient(true, s.sum, s.linked); quotient(true, s.sum, s.pairs);
            num(s.external);
            o.push_back('\t'); o += near ? cols.text[c][(size_t)s.nearest] : std::string("-");
            quotient(near, s.nearest_max, 1);
            quotient(near, s.nearest_sum, near ? (uint64_t)s.size * (uint64_t)stats[c][(size_t)s.nearest].size : 0);
            num((uint64_t)s.misfits);
            o.push_back('\n');
        }
    vg_write_file(path, { o });
}

void vg_cluster_write(const char* path, const std::vector<std::string>& ids, const int32_t* label, const int32_t* rep, bool representatives) {
    std::string o = "object\tcluster\n";
    o.reserve(ids.size() * 24 + 16);
    for (size_t i = 0; i < ids.size(); ++i) {
        o += ids[i]; o.push_back('\t');
        if (representatives) o += ids[(size_t)rep[i]]; else o += std::to_string(label[i]);
        o.push_back('\n');
    }
    vg_write_file(path, { o });
}

void vg_cluster_write_columns(const char* path, const std::vector<std::string>& ids, const std::vector<std::string>& names,
                              const std::vector<const int32_t*>& label, const std::vector<const int32_t*>& rep, bool representatives) {
    std::string o = "object";
    for (const std::string& nm : names) { o.push_back('\t'); o += nm; }
    o.push_back('\n');
    o.reserve(ids.size() * 24 * (names.size() + 1) + 64);
    for (size_t i = 0; i < ids.size(); ++i) {
        o += ids[i];
        for (size_t c = 0; c < names.size(); ++c) {
            o.push_back('\t');
            if (representatives) o += ids[(size_t)rep[c][i]]; else o += std::to_string(label[c][i]);
        }
        o.push_back('\n');
    }
    vg_write_file(path, { o });
}

void vg_linkage_write(const char* path, const vg_forest& f, const int64_t* node_a, const int64_t* node_b, const int64_t* size) {
    std::string o = "node_a\tnode_b\tsimilarity\tsize\tobject_a\tobject_b\n";
    o.reserve(f.a.size() * 48 + 64);
    char buf[160];
    for (size_t k = 0; k < f.a.size(); ++k) {
        snprintf(buf, sizeof buf, "%lld\t%lld\t%.6g\t%lld\t%d\t%d\n", (long long)node_a[k], (long long)node_b[k], f.w[k], (long long)size[k],
                 (int)f.a[k], (int)f.b[k]);
        o += buf;
    }
    vg_write_file(path, { o });
}

// ---------------------------------------------------------------- coverage stage: the alignment table, the two output files
void vg_cover_read_rows(const char* path, const std::vector<std::string>& ids, const std::vector<int64_t>& len, int n_threads,
                        std::vector<uint32_t>& q, std::vector<uint32_t>& r, std::vector<int32_t>& qs, std::vector<int32_t>& qe, std::vector<int32_t>* nm) {
    const text_file f(path);
    if (!f.n) row_error(path, 1, "empty file (no header)");
    const char* end = f.end();
    const char* hdr_end = f.line_end(f.p);
    std::vector<std::string_view> names;
    split_fields(std::string_view(f.p, (size_t)((hdr_end > f.p && hdr_end[-1] == '\r' ? hdr_end - 1 : hdr_end) - f.p)), '\t', names);
    // columns: 0 query, 1 reference, 2 qstart, 3 qend
    const char* const wanted[4] = { "query", "reference", "qstart", "qend" };
    size_t col[4];
    for (int k = 0; k < 4; ++k) {
        col[k] = (size_t)(std::find(names.begin(), names.end(), std::string_view(wanted[k])) - names.begin());
        if (col[k] == names.size()) row_error(path, 1, std::string("missing column ") + wanted[k]);
    }
    size_t max_col = *std::max_element(col, col + 4);
    // with nm also: 0 alnlen, 1 nt_match, and 2 nt_mismatch if the table has it
    const char* const counted[3] = { "alnlen", "nt_match", "nt_mismatch" };
    size_t ccol[3] = { 0, 0, 0 };
    int n_counted = 0;
    if (nm) {
        for (int k = 0; k < 3; ++k) {
            ccol[k] = (size_t)(std::find(names.begin(), names.end(), std::string_view(counted[k])) - names.begin());
            if (ccol[k] == names.size()) { if (k < 2) row_error(path, 1, std::string("missing column ") + counted[k]); break; }
            max_col = std::max(max_col, ccol[k]);
            n_counted = k + 1;
        }
    }
    std::unordered_map<std::string_view, uint32_t> index;
    index.reserve(ids.size() * 2);
    for (size_t i = 0; i < ids.size(); ++i) index.emplace(ids[i], (uint32_t)i);

    // the body cut into chunks at line starts, one per thread; each chunk keeps its rows and its first error
    const char* body = hdr_end < end ? hdr_end + 1 : end;
    const int nthr = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads > 0 ? n_threads : vg_host_threads(), (int64_t)((end - body) >> 20) + 1));
    std::vector<const char*> cut((size_t)nthr + 1, end);
    cut[0] = body;
    for (int t = 1; t < nthr; ++t) {
        const char* x = std::max(body + (end - body) * t / nthr, cut[(size_t)t - 1]);
        cut[(size_t)t] = x < end ? std::min(end, f.line_end(x) + 1) : end;
    }
    struct part { std::vector<uint32_t> q, r; std::vector<int32_t> qs, qe, nm; const char* err_at = nullptr; std::string err; };
    std::vector<part> parts((size_t)nthr);
    vg_parallel_for(nthr, nthr, [&](int64_t t) {
        part& pt = parts[(size_t)t];
        std::vector<std::string_view> fields;
        for (const char* a = cut[(size_t)t]; a < cut[(size_t)t + 1];) {
            const char* e = f.line_end(a);
            const std::string_view text(a, (size_t)((e > a && e[-1] == '\r' ? e - 1 : e) - a));
            if (text.empty()) { a = e + 1; continue; }          // (blank line)
            split_fields(text, '\t', fields);
            if (fields.size() <= max_col) { pt.err_at = a; pt.err = "expected " + std::to_string(names.size()) + " columns, found " + std::to_string(fields.size()); return; }
            uint32_t obj[2];
            for (int k = 0; k < 2; ++k) {
                const auto it = index.find(fields[col[k]]);
                if (it == index.end()) { pt.err_at = a; pt.err = std::string(wanted[k]) + " '" + std::string(fields[col[k]]) + "' is not in the ids file"; return; }
                obj[k] = it->second;
            }
            uint64_t pos[2];
            for (int k = 0; k < 2; ++k) {
                const std::string_view v = fields[col[2 + k]];
                const auto rr = std::from_chars(v.data(), v.data() + v.size(), pos[k]);
                if (rr.ec != std::errc() || rr.ptr != v.data() + v.size()) { pt.err_at = a; pt.err = std::string("malformed ") + wanted[2 + k] + " '" + std::string(v) + "'"; return; }
            }
            if (pos[0] < 1 || pos[0] > pos[1] || pos[1] > (uint64_t)len[obj[0]]) {
                pt.err_at = a;
                pt.err = "qstart..qend " + std::to_string(pos[0]) + ".." + std::to_string(pos[1]) + " is not a range inside 1.." + std::to_string(len[obj[0]]);
                return;
            }
            if (nm) {
                uint64_t cnt[3] = { 0, 0, 0 };
                for (int k = 0; k < n_counted; ++k) {
                    const std::string_view v = fields[ccol[k]];
                    const auto rr = std::from_chars(v.data(), v.data() + v.size(), cnt[k]);
                    if (rr.ec != std::errc() || rr.ptr != v.data() + v.size()) { pt.err_at = a; pt.err = std::string("malformed ") + counted[k] + " '" + std::string(v) + "'"; return; }
                }
                const uint64_t span = pos[1] - pos[0] + 1;
                if (cnt[0] != span) { pt.err_at = a; pt.err = "alnlen " + std::to_string(cnt[0]) + " is not qend - qstart + 1 = " + std::to_string(span); return; }
                if (cnt[1] > cnt[0]) { pt.err_at = a; pt.err = "nt_match " + std::to_string(cnt[1]) + " > alnlen " + std::to_string(cnt[0]); return; }
                if (n_counted == 3 && cnt[1] + cnt[2] != cnt[0]) {
                    pt.err_at = a;
                    pt.err = "nt_match + nt_mismatch = " + std::to_string(cnt[1] + cnt[2]) + " is not alnlen " + std::to_string(cnt[0]);
                    return;
                }
                pt.nm.push_back((int32_t)cnt[1]);
            }
            pt.q.push_back(obj[0]); pt.r.push_back(obj[1]); pt.qs.push_back((int32_t)(pos[0] - 1)); pt.qe.push_back((int32_t)(pos[1] - 1));
            a = e + 1;
        }
    });
    for (auto& pt : parts) if (pt.err_at) row_error(path, f.line_of(pt.err_at), pt.err);
    q.clear(); r.clear(); qs.clear(); qe.clear();
    for (auto& pt : parts) {
        q.insert(q.end(), pt.q.begin(), pt.q.end()); r.insert(r.end(), pt.r.begin(), pt.r.end());
        qs.insert(qs.end(), pt.qs.begin(), pt.qs.end()); qe.insert(qe.end(), pt.qe.begin(), pt.qe.end());
    }
    if (nm) {
        nm->clear();
        for (auto& pt : parts) nm->insert(nm->end(), pt.nm.begin(), pt.nm.end());
    }
}

void vg_cover_write(const char* path, const std::vector<std::string>& ids, const int32_t* group, const std::vector<std::string>* group_text,
                    const std::vector<int64_t>& group_size, const vg_cover_stat* stats, int n_threads) {
    const std::string head = "id\tlen\tgroup\tgroup_size\tpartners_in\tpartners_out\tcovered\tcovered_in\tcovered_out\tcore\tmax_depth\tmean_depth\tcovered_frac\tcore_frac\n";
    write_rows(path, head, (int64_t)ids.size(), 1 << 14, n_threads, [&](int64_t lo, int64_t hi, std::string& o) {
        char buf[64];
        auto num = [&](int64_t v) { o.push_back('\t'); o += std::to_string(v); };
        auto quotient = [&](bool have, int64_t a, int64_t b) {
            o.push_back('\t');
            if (!have) { o.push_back('-'); return; }
            snprintf(buf, sizeof buf, "%.6g", (double)a / (double)b);
            o += buf;
        };
        for (int64_t i = lo; i < hi; ++i) {
            const vg_cover_stat& s = stats[i];
            const int64_t members = group_size[(size_t)(group ? group[i] : 0)];
            o += ids[(size_t)i];
            num(s.len);
            o.push_back('\t'); o += group_text ? (*group_text)[(size_t)group[i]] : std::string("-");
            num(members); num(s.partners_in); num(s.partners_out); num(s.covered); num(s.covered_in); num(s.covered_out); num(s.core); num(s.max_depth);
            quotient(s.len > 0, s.sum_in + s.sum_out, s.len); quotient(s.len > 0, s.covered, s.len); quotient(s.len > 0 && members >= 2, s.core, s.len);
            o.push_back('\n');
        }
    });
}

void vg_cover_write_segments(const char* path, const std::vector<std::string>& ids, const vg_cover_segment* seg, int64_t n_segments, int n_threads) {
    write_rows(path, "id\tstart\tend\tdepth_in\tdepth_out\n", n_segments, 1 << 16, n_threads, [&](int64_t lo, int64_t hi, std::string& o) {
        char buf[64];
        for (int64_t k = lo; k < hi; ++k) {
            o += ids[(size_t)seg[k].object];
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%d\t%d\n", (long long)seg[k].start + 1, (long long)seg[k].end + 1, (int)seg[k].depth_in, (int)seg[k].depth_out);
            o += buf;
        }
    });
}

// ---------------------------------------------------------------- painting stage: the three output files
void vg_paint_write(const char* path, const std::vector<std::string>& ids, const int32_t* group, const std::vector<std::string>* group_text,
                    const vg_paint_stat* stats, int n_threads) {
    const std::string head = "id\tlen\tgroup\tpainted\tpainted_in\tpainted_out\tdonors\ttop_partner\ttop_painted\tswitches\tsegments\tpainted_frac\ttop_frac\n";
    write_rows(path, head, (int64_t)ids.size(), 1 << 14, n_threads, [&](int64_t lo, int64_t hi, std::string& o) {
        char buf[64];
        auto num = [&](int64_t v) { o.push_back('\t'); o += std::to_string(v); };
        auto quotient = [&](bool have, int64_t a, int64_t b) {
            o.push_back('\t');
            if (!have) { o.push_back('-'); return; }
            snprintf(buf, sizeof buf, "%.6g", (double)a / (double)b);
            o += buf;
        };
        for (int64_t i = lo; i < hi; ++i) {
            const vg_paint_stat& s = stats[i];
            o += ids[(size_t)i];
            num(s.len);
            o.push_back('\t'); o += group_text ? (*group_text)[(size_t)group[i]] : std::string("-");
            num(s.painted); num(s.painted_in); num(s.painted_out); num(s.donors);
            o.push_back('\t'); o += s.top_partner >= 0 ? ids[(size_t)s.top_partner] : std::string("-");
            num(s.top_painted); num(s.switches); num(s.segments);
            quotient(s.len > 0, s.painted, s.len); quotient(s.len > 0, s.top_painted, s.len);
            o.push_back('\n');
        }
    });
}

void vg_paint_write_segments(const char* path, const std::vector<std::string>& ids, const vg_paint_segment* seg, int64_t n_segments, int n_threads) {
    write_rows(path, "id\tstart\tend\tpartner\tpident\trow_qstart\trow_qend\n", n_segments, 1 << 16, n_threads, [&](int64_t lo, int64_t hi, std::string& o) {
        char buf[96], pident[64];
        for (int64_t k = lo; k < hi; ++k) {
            const vg_paint_segment& g = seg[k];
            o += ids[(size_t)g.object];
            o.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%lld\t%lld\t", (long long)g.start + 1, (long long)g.end + 1));
            if (g.partner < 0) { o += "-\t-\t-\t-\n"; continue; }
            vg_fmt_num(100.0 * g.n_match / (g.row_qend - g.row_qstart + 1), pident);       // (the expression of the alignment table's pident)
            o += ids[(size_t)g.partner];
            o.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%s\t%lld\t%lld\n", pident, (long long)g.row_qstart + 1, (long long)g.row_qend + 1));
        }
    });
}

void vg_paint_write_donors(const char* path, const std::vector<std::string>& ids, const std::vector<int64_t>& len, const vg_paint_donor* donor, int64_t n_donors,
                           int n_threads) {
    write_rows(path, "id\tpartner\tpainted\tsegments\tpainted_frac\n", n_donors, 1 << 16, n_threads, [&](int64_t lo, int64_t hi, std::string& o) {
        char buf[96];
        for (int64_t k = lo; k < hi; ++k) {
            const vg_paint_donor& d = donor[k];
            o += ids[(size_t)d.object]; o.push_back('\t'); o += ids[(size_t)d.partner];
            o.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%lld\t%lld\t%.6g\n", (long long)d.painted, (long long)d.segments,
                                           (double)d.painted / (double)len[(size_t)d.object]));
        }
    });
}
