// text_readers — every text reader of the library that finishes before a device is needed, on well-formed and damaged files:
//   filter   vg_read_filter                                   (fltr.txt)
//   ids      vg_cluster_read_ids                              (ani.ids.tsv)
//   prior    vg_cluster_read_prior   -> read_label_file       (clusters.tsv)
//   columns  vg_cluster_read_columns -> read_label_file       (clusters.tsv)
//   rows     vg_cluster_read_rows                             (ani.tsv, up to the point where the stage has its rows)
//
//   text_readers <tests/golden/example>
//
// Every case prints "reader file case: status count digest message".  Properties: the call returns; an error has a message; on
// the well-formed files the values are the ones the CPU tests pin.  The lines are the same in every build.  Files padded or cut
// to exactly 4 096 and 8 192 bytes without a final newline are mapped with no zero byte behind them: a reader that looks one
// byte too far faults.  Exit status 0 only if every property held.
#include "host_programs.h"
#include "vg_common.h"
#include <functional>

namespace {
using hp::fail;
hp::scratch_dir* g_dir;
std::string g_case_file;

struct outcome { int status = 0; std::string message; size_t count = 0; uint64_t digest = 0; };
template <class F> outcome guarded(F body) {       // the internal readers report by exception, as the C ABI's wrapper sees them
    outcome o;
    try { body(o); }
    catch (const vg_error& e) { o.status = e.code; o.message = e.what(); }
    catch (const std::exception& e) { o.status = VG_EINVAL; o.message = e.what(); }
    return o;
}

std::vector<std::string> g_names, g_ids;
vg_genomes* g_set;

outcome read_filter(const std::string& path, double thr, std::vector<vg_pair_count>* keep = nullptr) {
    outcome o; vg_pair_count* pairs = nullptr; int64_t n = 0;
    o.status = vg_read_filter(g_set, path.c_str(), thr, &pairs, &n);
    if (o.status != VG_OK) { o.message = vg_last_error(); return o; }
    o.count = (size_t)n; o.digest = hp::fnv(pairs, sizeof(vg_pair_count) * (size_t)n);
    if (keep) keep->assign(pairs, pairs + n);
    vg_free(pairs);
    return o;
}
outcome read_ids(const std::string& path, std::vector<std::string>* keep = nullptr) {
    return guarded([&](outcome& o) {
        std::vector<std::string> ids; vg_cluster_read_ids(path.c_str(), ids);
        o.count = ids.size(); for (const std::string& s : ids) o.digest = hp::fnv(s.data(), s.size() + 1, o.digest ? o.digest : 1);
        if (keep) *keep = ids;
    });
}
outcome read_prior(const std::string& path, bool is_repr, std::vector<int32_t>* keep = nullptr) {
    return guarded([&](outcome& o) {
        std::vector<int32_t> rep; vg_cluster_read_prior(path.c_str(), g_ids, is_repr, rep);
        o.count = rep.size(); o.digest = hp::fnv(rep.data(), rep.size() * sizeof(int32_t));
        if (keep) *keep = rep;
    });
}
outcome read_columns(const std::string& path, bool is_repr, vg_label_columns* keep = nullptr) {
    return guarded([&](outcome& o) {
        vg_label_columns c; vg_cluster_read_columns(path.c_str(), g_ids, is_repr, c);
        o.count = c.names.size();
        for (size_t k = 0; k < c.names.size(); ++k) { o.digest = hp::fnv(c.names[k].data(), c.names[k].size(), o.digest ? o.digest : 1); o.digest = hp::fnv(c.label[k].data(), c.label[k].size() * sizeof(int32_t), o.digest); }
        if (keep) *keep = c;
    });
}
struct rows { std::vector<uint32_t> q, r; std::vector<double> w; };
outcome read_rows(const std::string& path, const vg_cluster_params& p, rows* keep = nullptr) {
    return guarded([&](outcome& o) {
        rows x; vg_cluster_read_rows(path.c_str(), (int64_t)g_ids.size(), &p, x.q, x.r, x.w);
        o.count = x.q.size();
        o.digest = hp::fnv(x.q.data(), x.q.size() * 4); o.digest = hp::fnv(x.r.data(), x.r.size() * 4, o.digest); o.digest = hp::fnv(x.w.data(), x.w.size() * 8, o.digest);
        if (keep) *keep = x;
    });
}

void report(const char* reader, const std::string& file, const std::string& what, const outcome& o) {
    std::string msg = o.message;
    for (size_t at; (at = msg.find(g_dir->path)) != std::string::npos;) msg.replace(at, g_dir->path.size(), "<dir>");
    printf("%-8s %-16s %-28s status %2d count %4zu digest %016llx %s\n", reader, file.c_str(), what.c_str(), o.status, o.count, (unsigned long long)o.digest, msg.c_str());
    if (o.status != VG_OK && o.message.empty()) fail(std::string(reader) + " " + file + " " + what + ": an error without a message");
    if (o.status > 0 || o.status < VG_EOVERFLOW) fail(std::string(reader) + " " + file + " " + what + ": an unknown status");
}

// ---- damage
std::vector<std::string> lines_of(const std::string& text) {       // with their line ends
    std::vector<std::string> l;
    for (size_t a = 0; a < text.size();) { const size_t e = text.find('\n', a); l.push_back(text.substr(a, e == std::string::npos ? e : e - a + 1)); if (e == std::string::npos) break; a = e + 1; }
    return l;
}
std::string join(const std::vector<std::string>& l) { std::string t; for (const std::string& s : l) t += s; return t; }
// line `row` with field `field` (separated by sep; a cell "col:value" of the filter is one field) replaced; field == -1: a field
// removed at the end, field == -2: one appended
std::string with_field(const std::string& text, size_t row, char sep, int field, const std::string& value) {
    std::vector<std::string> l = lines_of(text);
    if (row >= l.size()) return text;
    std::string body = l[row], eol;
    while (!body.empty() && (body.back() == '\n' || body.back() == '\r')) { eol.insert(eol.begin(), body.back()); body.pop_back(); }
    const bool closed = !body.empty() && body.back() == sep;            // (filter rows end with the separator)
    if (closed) body.pop_back();
    std::vector<std::string> f;
    for (size_t a = 0;;) { const size_t t = body.find(sep, a); f.push_back(body.substr(a, t == std::string::npos ? t : t - a)); if (t == std::string::npos) break; a = t + 1; }
    if (field == -1) { if (f.size() > 1) f.pop_back(); } else if (field == -2) f.push_back(value); else if ((size_t)field < f.size()) f[(size_t)field] = value;
    body.clear();
    for (size_t i = 0; i < f.size(); ++i) { if (i) body.push_back(sep); body += f[i]; }
    if (closed) body.push_back(sep);
    l[row] = body + eol;
    return join(l);
}
// exactly `size` bytes, no line end at the end: body lines repeated (or the text cut)
std::string sized(const std::string& text, size_t size) {
    std::string t = text;
    const std::vector<std::string> l = lines_of(text);
    if (!t.empty() && t.back() != '\n') t.push_back('\n');
    for (size_t k = 1; t.size() < size && l.size() > 1; k = k % (l.size() - 1) + 1) { t += l[k]; if (t.back() != '\n') t.push_back('\n'); }
    t.resize(size, 'x');
    if (t.back() == '\n' || t.back() == '\r') t.back() = '7';
    return t;
}

struct reader { const char* name; std::function<outcome(const std::string&)> call; };
// one file through its readers: as it is, and damaged.  sep / row / number fields: where the damage goes
void run_file(const std::string& tag, const std::string& text, const std::vector<reader>& readers, char sep, const std::vector<int>& number_fields,
              const std::function<std::string(const std::string&)>& as_number_field = nullptr) {
    auto each = [&](const std::string& what, const std::string& bytes) {
        hp::write_file(g_case_file, bytes);
        for (const reader& rd : readers) report(rd.name, tag, what, rd.call(g_case_file));
    };
    each("as it is", text);
    if (text.size() < 4096) for (size_t n = 0; n < text.size(); ++n) each("cut at " + std::to_string(n), text.substr(0, n));
    { std::string t = text; while (!t.empty() && (t.back() == '\n' || t.back() == '\r')) t.pop_back(); each("no final newline", t); }
    each("only a newline", "\n");
    each("empty", "");
    each("a lone CR", "\r");
    each("a CR behind the text", text + "\r");
    each("a field of 5000", with_field(text, 1, sep, 0, std::string(5000, 'x')));
    each("a last field of 5000", with_field(text, 1, sep, -2, std::string(5000, 'y')));
    for (const int f : number_fields)
        for (const char* v : { "-", "1e999", "nan", "0x10", "1234567890123456789012345678901234567890", "-99999999999999999999999999", "" }) {
            const std::string value = as_number_field ? as_number_field(v) : std::string(v);
            for (const size_t row : { (size_t)1, (size_t)3 }) each("row " + std::to_string(row) + " field " + std::to_string(f) + " = '" + value + "'", with_field(text, row, sep, f, value));
        }
    each("a field too few", with_field(text, 2, sep, -1, ""));
    each("a field too many", with_field(text, 2, sep, -2, "1"));
    each("header a field too few", with_field(text, 0, sep, -1, ""));
    for (const size_t size : { (size_t)4096, (size_t)8192 }) {
        each("exactly " + std::to_string(size), sized(text, size));
        each("exactly " + std::to_string(size) + " in one line", sized(lines_of(text)[0].substr(0, lines_of(text)[0].find_last_not_of("\r\n") + 1), size));
    }
}

template <class T> std::string list(const std::vector<T>& v) { std::string s; for (const T& x : v) s += std::to_string(x) + " "; return s; }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: text_readers <golden example directory>\n"); return 2; }
    const std::string golden = std::string(argv[1]) + "/output/";
    hp::scratch_dir dir; g_dir = &dir; g_case_file = dir.file("case.txt");
    std::string fltr, ids_text, clusters, ani;
    if (!hp::read_file(golden + "fltr.txt", fltr) || !hp::read_file(golden + "ani.ids.tsv", ids_text) || !hp::read_file(golden + "clusters.tsv", clusters) ||
        !hp::read_file(golden + "ani.tsv", ani)) { fprintf(stderr, "cannot read the golden files under %s\n", golden.c_str()); return 2; }

    // the genome set of the filter: the names of the golden header, four bases each
    {
        const std::string head = lines_of(fltr)[0];
        for (size_t a = head.find(',') + 1;;) { const size_t t = head.find(',', a); if (t == std::string::npos) break; g_names.push_back(head.substr(a, t - a)); a = t + 1; }
        std::vector<uint8_t> codes(4 * g_names.size(), 1); std::vector<int64_t> off; std::vector<const char*> nm;
        for (size_t i = 0; i <= g_names.size(); ++i) off.push_back((int64_t)(4 * i));
        for (const std::string& s : g_names) nm.push_back(s.c_str());
        if (vg_genomes_from_codes(codes.data(), off.data(), (int)g_names.size(), nm.data(), &g_set) != VG_OK) { fprintf(stderr, "vg_genomes_from_codes: %s\n", vg_last_error()); return 2; }
    }

    // ---- well-formed files: the values the CPU tests pin
    {
        hp::write_file(g_case_file, fltr);
        std::vector<vg_pair_count> p;
        if (read_filter(g_case_file, 0.0, &p).count != 13 || read_filter(g_case_file, 0.99).count != 8) fail("golden fltr.txt: not 13 couples at 0 and 8 at 0.99");
        for (size_t i = 0; i < p.size(); ++i) if (!(p[i].a > p[i].b) || (i && !(p[i - 1].a < p[i].a || (p[i - 1].a == p[i].a && p[i - 1].b < p[i].b)))) fail("golden fltr.txt: couples not ascending with a > b");
        const std::vector<std::string>& nm = g_names;
        const std::vector<std::string> corpus = { "kmer-length: 25 fraction: 1," + [&] { std::string s; for (const std::string& x : nm) s += x + ","; return s; }(), "", nm[1] + ",1:0.5,",
                                                  nm[2] + ",1:1e-1,2:0.12345678901234567,", nm[3] + ",x:0.9,99:0.9,4:0.9,3:.5,", "not_in_the_set,1:0.9," };
        for (const char* form : { "lf", "crlf", "no final newline" }) {
            const std::string eol = !strcmp(form, "crlf") ? "\r\n" : "\n";
            std::string text; for (size_t i = 0; i < corpus.size(); ++i) { text += corpus[i]; if (i + 1 < corpus.size() || strcmp(form, "no final newline")) text += eol; }
            hp::write_file(g_case_file, text);
            std::vector<vg_pair_count> c; read_filter(g_case_file, 0.1, &c);
            std::string got; for (const vg_pair_count& x : c) got += "(" + std::to_string(x.a) + "," + std::to_string(x.b) + ")";
            if (got != "(1,0)(2,0)(2,1)(3,2)") fail(std::string("filter corpus, ") + form + ": " + got);
            run_file(std::string("corpus-") + (form[0] == 'n' ? "nofinal" : form), text, { { "filter", [](const std::string& f) { return read_filter(f, 0.1); } } }, ',', { 1, 2 },
                     [](const std::string& v) { return v + ":0.9"; });
            run_file(std::string("corpus-") + (form[0] == 'n' ? "nofinal" : form) + "-v", text, { { "filter", [](const std::string& f) { return read_filter(f, 0.1); } } }, ',', { 1 },
                     [](const std::string& v) { return "1:" + v; });
        }
    }
    {
        hp::write_file(g_case_file, ids_text);
        if (read_ids(g_case_file, &g_ids).count != 12) fail("golden ani.ids.tsv: not 12 ids");
        const std::vector<std::string> l = lines_of(ids_text);
        for (size_t i = 0; i < g_ids.size() && i + 1 < l.size(); ++i) if (l[i + 1].compare(0, g_ids[i].size() + 1, g_ids[i] + "\t")) fail("golden ani.ids.tsv: id " + std::to_string(i));
    }
    vg_cluster_params cp; memset(&cp, 0, sizeof cp); cp.metric = "tani"; cp.num_threads = 3;
    vg_cluster_params cf = cp; cf.metric = "ani"; cf.min_ani = 0.7; cf.min_qcov = 0.5; cf.max_num_alns = 40;
    {
        // clusters.tsv: a restatement (the representative of a cluster number is its earliest object in the ids file; clusters numbered by earliest member)
        std::vector<int64_t> number(g_ids.size(), -1);
        const std::vector<std::string> l = lines_of(clusters);
        for (size_t k = 1; k < l.size(); ++k) { const size_t t = l[k].find('\t'); for (size_t i = 0; i < g_ids.size(); ++i) if (g_ids[i] == l[k].substr(0, t)) number[i] = atol(l[k].c_str() + t + 1); }
        std::vector<int32_t> want_rep(g_ids.size()), want_label(g_ids.size()); int32_t next = 0;
        for (size_t i = 0; i < g_ids.size(); ++i) { size_t e = 0; while (number[e] != number[i]) ++e; want_rep[i] = (int32_t)e; want_label[i] = e == i ? next++ : want_label[e]; }
        hp::write_file(g_case_file, clusters);
        std::vector<int32_t> rep; vg_label_columns cols;
        if (read_prior(g_case_file, false, &rep).status != VG_OK || rep != want_rep) fail("golden clusters.tsv as a prior: " + list(rep));
        if (read_columns(g_case_file, false, &cols).status != VG_OK || cols.names != std::vector<std::string>{ "cluster" } || cols.label[0] != want_label) fail("golden clusters.tsv as label columns");
        // ani.tsv: 132 rows of 12 objects, every one kept without filters
        hp::write_file(g_case_file, ani);
        rows x;
        if (read_rows(g_case_file, cp, &x).count != 132 || x.q[0] != 1 || x.r[0] != 0 || x.w[0] != 0.0137651 || x.q[131] == x.r[131]) fail("golden ani.tsv: not its 132 rows");
        const std::vector<std::string> al = lines_of(ani); size_t want = 0;
        for (size_t k = 1; k < al.size(); ++k) { std::vector<std::string> f; for (size_t a = 0;;) { const size_t t = al[k].find('\t', a); f.push_back(al[k].substr(a, t - a)); if (t == std::string::npos) break; a = t + 1; }
                                                 want += atof(f[6].c_str()) >= 0.7 && atof(f[7].c_str()) >= 0.5 && atof(f[9].c_str()) <= 40; }
        if (read_rows(g_case_file, cf).count != want) fail("golden ani.tsv: the filtered rows are not the restatement's " + std::to_string(want));
    }

    // ---- every file, as it is and damaged
    run_file("fltr.txt", fltr, { { "filter", [](const std::string& f) { return read_filter(f, 0.5); } } }, ',', { 1 }, [](const std::string& v) { return v + ":0.99"; });
    run_file("fltr.txt-v", fltr, { { "filter", [](const std::string& f) { return read_filter(f, 0.5); } } }, ',', { 1 }, [](const std::string& v) { return "1:" + v; });
    run_file("ani.ids.tsv", ids_text, { { "ids", [](const std::string& f) { return read_ids(f); } } }, '\t', { 1 });
    run_file("clusters.tsv", clusters, { { "prior", [](const std::string& f) { return read_prior(f, false); } }, { "prior-r", [](const std::string& f) { return read_prior(f, true); } },
                                         { "columns", [](const std::string& f) { return read_columns(f, false); } }, { "columns-r", [](const std::string& f) { return read_columns(f, true); } } }, '\t', { 1 });
    run_file("ani.tsv", ani, { { "rows", [&](const std::string& f) { return read_rows(f, cp); } }, { "rows-f", [&](const std::string& f) { return read_rows(f, cf); } } }, '\t', { 0, 1, 4, 7, 9 });
    {   // a body above 1 MiB: the rows are parsed as several ranges
        std::string big = ani; const std::vector<std::string> l = lines_of(ani);
        while (big.size() < (3u << 20)) for (size_t k = 1; k < l.size(); ++k) big += l[k];
        hp::write_file(g_case_file, big); report("rows", "ani.tsv x many", "as it is", read_rows(g_case_file, cp));
        hp::write_file(g_case_file, with_field(big, 20000, '\t', 4, "nan")); report("rows", "ani.tsv x many", "row 20000 field 4 = 'nan'", read_rows(g_case_file, cp));
        hp::write_file(g_case_file, sized(big, 512 * 4096)); report("rows", "ani.tsv x many", "exactly 2 MiB", read_rows(g_case_file, cp));
    }
    delete g_set;
    return hp::finish();
}
