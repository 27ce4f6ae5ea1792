// fasta_ingest — the FASTA readers of the library on plain, gzip and BGZF files, well-formed and damaged:
//   vg_genomes_load (host part: no upload)      names, lengths and vg_genomes_codes against a restatement of the format
//   ... in directory mode, vg_genomes_load_db_new   one genome per file (records joined by N), database + new genomes and its refusals
//   vg_fasta_read / vg_fasta_write_records     the records of the deduplicate stage, read and written back byte for byte
//   vg_fasta_write_kept                         the deduplicate stage's output, plain and as gzip members at levels 1, 5 and 9
//
//   fasta_ingest <tests/golden/example> [threads ...]        (default: 1 3 16)
//
// Every container of a text (plain, gzip through the own decoder, several members, BGZF) must give what the plain text gives; a
// damaged container gives an error or -- where the damage leaves a valid file -- the whole set, never a short one.  One line
// per case, the same in every build and for every thread count.  Exit status 0 only if every property held.
#include "host_programs.h"
#include "vg_common.h"
#include <zlib.h>

namespace {
using hp::fail;
hp::scratch_dir* g_dir;
int g_file_no = 0;
std::string fresh(const std::string& bytes, const char* suffix) {          // (a file of its own per case: a mapping of an earlier one may still exist)
    const std::string p = g_dir->file("f" + std::to_string(g_file_no++) + suffix);
    hp::write_file(p, bytes);
    return p;
}

const char MESSY[] = ">g1 first genome\tdescription\r\nACGTacgtNNnnRYKM\r\n\r\nacgtACGT\r\n"
                     ">g2\nAC\nGT\n\n>empty_record\n>g4|pipes and spaces  \nTTTTGGGGCCCCAAAA-*.\nacgu";

// ---- the format, restated: a record starts with '>' at the start of a line; its name is the header up to the first blank, tab or
// CR; its bases are the bytes of its other lines that are no white space, A C G T in either case, anything else N (4)
struct record { std::string name, verbatim; std::vector<uint8_t> codes; };
std::vector<record> restate(const std::string& t) {
    std::vector<record> out;
    size_t at = 0;
    while (at < t.size() && !(t[at] == '>' && (at == 0 || t[at - 1] == '\n'))) ++at;
    while (at < t.size()) {
        size_t end = at + 1;
        while (end < t.size() && !(t[end] == '>' && t[end - 1] == '\n')) ++end;
        record r; r.verbatim = t.substr(at, end - at);
        size_t nl = t.find('\n', at); if (nl == std::string::npos || nl > end) nl = end;
        size_t q = at + 1; while (q < nl && t[q] != ' ' && t[q] != '\t' && t[q] != '\r') ++q;
        r.name = t.substr(at + 1, q - at - 1);
        for (size_t i = nl; i < end; ++i) {
            const char c = t[i];
            if (c == '\n' || c == '\r' || c == ' ' || c == '\t') continue;
            r.codes.push_back(c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 4);
        }
        out.push_back(r);
        at = end;
    }
    return out;
}

// ---- containers
std::string gz(const std::string& text, int level, int window = 15 + 16) {
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, window, 8, Z_DEFAULT_STRATEGY) != Z_OK) exit(2);
    std::string out(deflateBound(&zs, (uLong)text.size()) + 64, '\0');
    zs.next_in = (Bytef*)text.data(); zs.avail_in = (uInt)text.size(); zs.next_out = (Bytef*)&out[0]; zs.avail_out = (uInt)out.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) exit(2);
    out.resize(out.size() - zs.avail_out); deflateEnd(&zs);
    return out;
}
void le(std::string& o, uint32_t v, int bytes) { for (int i = 0; i < bytes; ++i) o.push_back((char)(v >> (8 * i))); }
// bgzip's container: gzip members of at most `block` bytes of text with their size in a 'BC' extra field, then the empty member
std::string bgzf(const std::string& text, size_t block, std::vector<size_t>* starts = nullptr) {
    std::string out;
    for (size_t o = 0;; o += block) {
        const std::string chunk = o < text.size() ? text.substr(o, block) : std::string();
        const std::string cdata = gz(chunk, 6, -15);
        if (starts) starts->push_back(out.size());
        out += std::string("\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", 16);
        le(out, (uint32_t)(12 + 6 + cdata.size() + 8 - 1), 2);
        out += cdata;
        le(out, (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)chunk.data(), (uInt)chunk.size()), 4); le(out, (uint32_t)chunk.size(), 4);
        if (o >= text.size()) break;
    }
    return out;
}

// ---- the calls
struct loaded { int status = 0; std::string message; std::vector<record> recs; std::vector<int> n_parts; int n_db = -1; };
// vg_genomes_load of `paths`, or (db not empty) vg_genomes_load_db_new of the database files `db` and the new files `paths`
loaded load_set(const std::vector<std::string>& db, const std::vector<std::string>& paths, int multisample, int threads) {
    loaded l; vg_genomes* g = nullptr; std::vector<const char*> d, p;
    for (const std::string& s : db) d.push_back(s.c_str());
    for (const std::string& s : paths) p.push_back(s.c_str());
    l.status = db.empty() ? vg_genomes_load(p.data(), (int)p.size(), multisample, threads, &g)
                          : vg_genomes_load_db_new(d.data(), (int)d.size(), p.data(), (int)p.size(), multisample, threads, &g, &l.n_db);
    if (l.status != VG_OK) { l.message = vg_last_error(); return l; }
    std::vector<int64_t> len((size_t)vg_genomes_count(g));
    if (!len.empty()) vg_genomes_lengths(g, len.data());
    for (int i = 0; i < vg_genomes_count(g); ++i) {
        record r; r.name = vg_genomes_name(g, i); r.codes.resize((size_t)len[(size_t)i] + 1, 0xee);     // one byte more: nothing is written behind the length
        if (vg_genomes_codes(g, i, r.codes.data()) != VG_OK || r.codes.back() != 0xee) l.message = "vg_genomes_codes failed";
        r.codes.pop_back();
        l.recs.push_back(r); l.n_parts.push_back(g->n_parts[(size_t)i]);
    }
    delete g;
    return l;
}
loaded load(const std::string& path, int threads) { return load_set({}, { path }, 1, threads); }
bool same(const std::vector<record>& a, const std::vector<record>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].name != b[i].name || a[i].codes != b[i].codes) return false;
    return true;
}
std::string digest(const std::vector<record>& r) {
    uint64_t h = 1; size_t bases = 0;
    for (const record& x : r) { h = hp::fnv(x.name.data(), x.name.size() + 1, h); h = hp::fnv(x.codes.data(), x.codes.size(), h); bases += x.codes.size(); }
    char b[96]; snprintf(b, sizeof b, "%zu genomes %zu bases %016llx", r.size(), bases, (unsigned long long)h);
    return b;
}
std::string scrub(std::string msg) { for (size_t at; (at = msg.find(g_dir->path)) != std::string::npos;) msg.replace(at, g_dir->path.size(), "<dir>"); size_t f = msg.find("<dir>/f"); if (f != std::string::npos) { size_t e = f + 7; while (e < msg.size() && isdigit((unsigned char)msg[e])) ++e; msg.replace(f + 7, e - f - 7, "N"); } return msg; }

std::vector<int> g_threads;
std::vector<std::string> g_lines;              // the lines of the first thread count: the others must print the same
size_t g_line_at = 0; bool g_first = true;
void line(const std::string& s) {
    if (g_first) { g_lines.push_back(s); printf("%s\n", s.c_str()); }
    else if (g_line_at >= g_lines.size() || g_lines[g_line_at++] != s) fail("another result at another thread count: " + s);
}

// the deduplicate stage's writer on the records just read: every third record dropped, a prefix in front of the headers; plain and
// gzip at levels 1, 5 and 9 must hold the expected records byte for byte (the gzip files through zlib).  The line carries the digest
// of the FILE, so the bytes are the same at every thread count.
void write_kept(const std::string& tag, const vg_fasta_text& ft, const std::vector<record>& want, int threads) {
    std::vector<int32_t> rep(want.size());
    const std::vector<std::string> prefix = { "pfx|" };
    std::string expect;
    for (size_t i = 0; i < want.size(); ++i) {
        rep[i] = i % 3 == 2 ? (int32_t)i - 1 : (int32_t)i;
        if (rep[i] != (int32_t)i) continue;
        const std::string& v = want[i].verbatim; const size_t nl = v.find('\n');
        expect += ">" + prefix[0] + v.substr(1, nl == std::string::npos ? nl : nl - 1) + "\n";
        if (nl != std::string::npos && nl + 1 < v.size()) { expect += v.substr(nl + 1); if (expect.back() != '\n') expect += '\n'; }
    }
    for (const int level : { 0, 1, 5, 9 }) {
        if (level > 1 && expect.size() > (2u << 20)) continue;      // (the large text is there for the second gzip member, which no level changes)
        const std::string out = g_dir->file("kept" + std::to_string(g_file_no++) + (level ? ".fna.gz" : ".fna"));
        std::string bytes, text;
        try { vg_fasta_write_kept(out.c_str(), ft, prefix, rep.data(), level, threads); }
        catch (const std::exception& e) { fail("vg_fasta_write_kept " + tag + " level " + std::to_string(level) + ": " + e.what()); continue; }
        hp::read_file(out, bytes);
        if (level == 0) text = bytes;
        else if (!hp::zlib_gunzip((const unsigned char*)bytes.data(), bytes.size(), text) && !(bytes.empty() && expect.empty())) fail("vg_fasta_write_kept " + tag + " level " + std::to_string(level) + ": zlib does not read the file");
        if (text != expect) fail("vg_fasta_write_kept " + tag + " level " + std::to_string(level) + ": not the kept records byte for byte");
        char b[160]; snprintf(b, sizeof b, "kept  %s level %d: %zu bytes %016llx, %zu bytes of text", tag.c_str(), level, bytes.size(), (unsigned long long)hp::fnv(bytes.data(), bytes.size()), text.size());
        line(b);
    }
}

// a well-formed text in every container
void well_formed(const std::string& tag, const std::string& text, int threads) {
    const std::vector<record> want = restate(text);
    struct form { const char* name; std::string bytes; const char* suffix; };
    std::vector<form> forms = { { "plain", text, ".fna" } };
    if (!text.empty() && text.size() <= (2u << 20)) {      // (the 7 MB text is there for the writer: plain only)
        forms.push_back({ "gzip-1", gz(text, 1), ".fna.gz" }); forms.push_back({ "gzip-9", gz(text, 9), ".fna.gz" }); forms.push_back({ "stored", gz(text, 0), ".fna.gz" });
        forms.push_back({ "members", gz(text.substr(0, text.size() / 2), 6) + gz("", 6) + gz(text.substr(text.size() / 2), 3), ".fna.gz" });
        forms.push_back({ "bgzf", bgzf(text, 65280), ".fna.gz" }); forms.push_back({ "bgzf-small", bgzf(text, 997), ".fna.gz" });
    }
    for (const form& f : forms) {
        if (!strcmp(f.name, "bgzf-small") && text.size() > 300000) continue;
        const std::string path = fresh(f.bytes, f.suffix);
        const loaded l = load(path, threads);
        line("load  " + tag + " " + f.name + ": status " + std::to_string(l.status) + " " + (l.status ? scrub(l.message) : digest(l.recs)));
        if (l.status != VG_OK || !l.message.empty() || !same(l.recs, want)) fail("load " + tag + " " + f.name + ": not the genomes of the text" + (l.message.empty() ? "" : " (" + l.message + ")"));
        // the records of the deduplicate stage, and written back
        vg_fasta_text ft; const char* paths[1] = { path.c_str() };
        try {
            vg_fasta_read(paths, 1, threads, ft);
            bool ok = ft.recs.size() == want.size(); std::vector<int64_t> all, odd;
            for (size_t i = 0; ok && i < want.size(); ++i) {
                const vg_fasta_rec& r = ft.recs[i];
                ok = std::string(r.hdr - 1, r.end) == want[i].verbatim && r.hdr_end >= r.hdr && r.hdr_end <= r.seq && r.seq <= r.end && r.file == 0;
                all.push_back((int64_t)i); if (i & 1) odd.push_back((int64_t)i);
            }
            if (!ok) fail("vg_fasta_read " + tag + " " + f.name + ": not the records of the text");
            for (const std::vector<int64_t>* which : { &all, &odd }) {
                const std::string out = g_dir->file("out" + std::to_string(g_file_no++) + ".fna");
                vg_fasta_write_records(out.c_str(), ft, *which);
                std::string got, expect;
                hp::read_file(out, got);
                for (const int64_t i : *which) { expect += want[(size_t)i].verbatim; if (expect.back() != '\n') expect += '\n'; }
                if (got != expect) fail("vg_fasta_write_records " + tag + " " + f.name + ": the records do not come back byte for byte");
            }
            line("read  " + tag + " " + f.name + ": " + std::to_string(ft.recs.size()) + " records");
            if (ok && (!strcmp(f.name, "plain") || !strcmp(f.name, "bgzf"))) write_kept(tag + " " + f.name, ft, want, threads);
        } catch (const std::exception& e) { fail("vg_fasta_read " + tag + " " + f.name + ": " + e.what()); }
    }
}
// a damaged container of a text: an error, or the whole set
void damaged(const std::string& tag, const std::string& bytes, const std::string& text, int threads, bool must_fail) {
    const std::vector<record> want = restate(text);
    const std::string path = fresh(bytes, ".fna.gz");
    const loaded l = load(path, threads);
    line("load  " + tag + ": status " + std::to_string(l.status) + " " + (l.status ? scrub(l.message) : digest(l.recs)));
    if (l.status == VG_OK && (!same(l.recs, want) || must_fail)) fail("load " + tag + ": a damaged file was taken" + (must_fail ? "" : " as a short or altered set"));
    if (l.status != VG_OK && l.message.empty()) fail("load " + tag + ": an error without a message");
    vg_fasta_text ft; const char* paths[1] = { path.c_str() };
    try {
        vg_fasta_read(paths, 1, threads, ft);
        bool ok = ft.recs.size() == want.size() && !must_fail;
        for (size_t i = 0; ok && i < want.size(); ++i) ok = std::string(ft.recs[i].hdr - 1, ft.recs[i].end) == want[i].verbatim;
        if (!ok) fail("vg_fasta_read " + tag + ": a damaged file was taken");
        line("read  " + tag + ": " + std::to_string(ft.recs.size()) + " records");
    } catch (const vg_error& e) { line("read  " + tag + ": status " + std::to_string(e.code) + " " + scrub(e.what())); if (!*e.what()) fail("vg_fasta_read " + tag + ": an error without a message"); }
}

// ---- the loader's other two modes
// directory mode: a file is one genome, its records joined by one N (code 4) each and named by the file; a file without a record is none
void file_genome(const std::string& path, const std::string& text, std::vector<record>& out) {
    const std::vector<record> parts = restate(text);
    if (parts.empty()) return;
    record r; r.name = path.substr(path.find_last_of('/') + 1);
    for (size_t k = 0; k < parts.size(); ++k) { if (k) r.codes.push_back(4); r.codes.insert(r.codes.end(), parts[k].codes.begin(), parts[k].codes.end()); }
    out.push_back(r);
}
void report(const std::string& tag, const loaded& l) {
    std::string s = "load  " + tag + ": status " + std::to_string(l.status) + " " + (l.status ? scrub(l.message) : digest(l.recs));
    if (l.status == VG_OK) { s += ", parts"; for (const int n : l.n_parts) s += " " + std::to_string(n); if (l.n_db >= 0) s += ", n_db " + std::to_string(l.n_db); }
    line(s);
}
void refused(const std::string& tag, const loaded& l, int status, const std::string& message) {
    report(tag, l);
    if (l.status != status || scrub(l.message) != message) fail("load " + tag + ": expected status " + std::to_string(status) + " " + message);
}
void loader_modes(int threads) {
    const std::string one = ">solo one record\nACGTNACGTTGCA\nGGA\n", three = ">p1 x\nACGT\n>p2\nGG\nCC\n>p3\nTTNA\n", two = ">t1\nACGTACGTAC\n>t2\nGGGGCCCCNN\nTT\n";
    const std::string none = "no record in this file\nACGT\n", crlf = ">c x\r\nACGT\r\nNNAC\r\n>d\r\nTT\r\n";
    {   // directory mode over five files
        const std::vector<std::string> paths = { fresh(one, ".fna"), fresh(three, ".fna"), fresh(gz(two, 6), ".fna.gz"), fresh(none, ".fna"), fresh(crlf, ".fna") };
        const std::string* texts[] = { &one, &three, &two, &none, &crlf };
        std::vector<record> want;
        for (size_t i = 0; i < paths.size(); ++i) file_genome(paths[i], *texts[i], want);
        const loaded l = load_set({}, paths, 0, threads);
        report("directory, five files", l);
        if (l.status != VG_OK || !l.message.empty() || !same(l.recs, want) || l.n_parts != std::vector<int>({ 1, 3, 2, 2 })) { fail("load directory: not one genome per file with a record, named by the file, in path order"); return; }
        const std::vector<uint8_t>& c = l.recs[1].codes;      // p1 (4 bases) N p2 (4) N p3 (4)
        if (c.size() != 4 + 4 + 4 + 2 || c[4] != 4 || c[9] != 4) fail("load directory: the three records are not joined by one N each");
    }
    const std::string db = ">d1 the database\nACGTACGT\n>d2\nGGNCC\n", fresh_ones = ">n1\nTTTT\nAC\n>n2 x\r\nACGU\r\n";
    {   // database + new, multi-FASTA: the genomes of the two files behind one another
        const loaded l = load_set({ fresh(db, ".fna") }, { fresh(fresh_ones, ".fna") }, 1, threads), whole = load(fresh(db + fresh_ones, ".fna"), threads);
        report("db + new, multi-FASTA", l);
        if (l.status != VG_OK || whole.status != VG_OK || !same(l.recs, whole.recs) || !same(l.recs, restate(db + fresh_ones)) || l.n_db != 2) fail("load db + new, multi-FASTA: not vg_genomes_load of the concatenation with 2 database genomes");
    }
    {   // database + new, directory mode
        const std::vector<std::string> d = { fresh(one, ".fna"), fresh(three, ".fna") }, n = { fresh(gz(two, 6), ".fna.gz") };
        std::vector<record> want;
        file_genome(d[0], one, want); file_genome(d[1], three, want); file_genome(n[0], two, want);
        const loaded l = load_set(d, n, 0, threads);
        report("db + new, directory", l);
        if (l.status != VG_OK || !same(l.recs, want) || l.n_db != 2 || l.n_parts != std::vector<int>({ 1, 3, 2 })) fail("load db + new, directory: not the three files' genomes with 2 database genomes");
    }
    refused("db + new, a name on both sides", load_set({ fresh(db, ".fna") }, { fresh(">n1\nTT\n>d2 again\nCC\n", ".fna") }, 1, threads), VG_EINVAL,
            "vg_genomes_load_db_new: the name d2 occurs in the database and in the new genomes");
    refused("db + new, one genome in all", load_set({ fresh(">d1\nACGT\n", ".fna") }, { fresh(none, ".fna") }, 1, threads), VG_EINVAL,
            "vg_genomes_load_db_new: the database and the new genomes together are 1 genome(s); pairs need at least 2");
    refused("db + new, two database files in multi-FASTA mode", load_set({ fresh(db, ".fna"), fresh(one, ".fna") }, { fresh(fresh_ones, ".fna") }, 1, threads), VG_EINVAL,
            "vg_genomes_load_db_new: multi-FASTA mode takes one database file and one file of new genomes");
    refused("db + new, a missing new file", load_set({ fresh(db, ".fna") }, { g_dir->path + "/missing.fna" }, 1, threads), VG_EIO, "cannot open <dir>/missing.fna");
}

std::string sized(const std::string& unit, size_t size, char last) {
    std::string t; while (t.size() < size) t += unit;
    t.resize(size); t.back() = last;
    return t;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: fasta_ingest <golden example directory> [threads ...]\n"); return 2; }
    for (int i = 2; i < argc; ++i) g_threads.push_back(atoi(argv[i]));
    if (g_threads.empty()) g_threads = { 1, 3, 16 };
    hp::scratch_dir dir; g_dir = &dir;
    vg_defer_mode(true);              // (the loader hands its mappings to a helper thread to unmap; here they are simply kept)
    std::string golden;
    if (!hp::read_file(std::string(argv[1]) + "/multifasta.fna", golden)) { fprintf(stderr, "cannot read %s/multifasta.fna\n", argv[1]); return 2; }
    std::string golden_gz; hp::read_file(std::string(argv[1]) + "/multifasta.fna.gz", golden_gz);
    const std::string messy(MESSY, sizeof MESSY - 1);
    for (const int threads : g_threads) {
        g_file_no = 0; g_line_at = 0;
        well_formed("messy", messy, threads);
        well_formed("golden", golden, threads);
        { std::string many; for (int k = 0; k < 12; ++k) many += golden; well_formed("golden-x12", many, threads); }      // 7 MB, 4.7 MB of them kept: two gzip members of the writer
        well_formed("empty", "", threads);
        well_formed("header-only", ">only a header", threads);
        well_formed("header-and-newline", ">only a header\n", threads);
        well_formed("gt-last", ">a\nACGT\n>", threads);
        well_formed("ends-in-sequence", ">a\nACGT\nACG", threads);
        well_formed("crlf", ">a x\r\nACGT\r\nNNAC\r\n>b\r\nTT\r\n", threads);
        well_formed("empty-between", ">a\nACGT\n>none\n>b\nGGCC\n", threads);
        well_formed("text-in-front", "stray\n>a\nAC>GT\n", threads);
        for (const size_t size : { (size_t)4096, (size_t)8192 }) {
            const std::string s = std::to_string(size);
            well_formed("page-" + s + "-in-sequence", sized(">r\nACGTNacgt\nTTGACA\n", size, 'G'), threads);
            well_formed("page-" + s + "-gt-last", sized(">r\nACGTNacgt\nTTGACA\n", size - 1, '\n') + ">", threads);
            well_formed("page-" + s + "-in-header", sized("ACGT\n", size - 7, '\n') + ">header", threads);
            well_formed("page-" + s + "-one-line", ">" + std::string(size - 1, 'A'), threads);
        }
        {   // the golden set, damaged
            const std::string one = gz(golden, 6);
            std::string bad = one; bad[bad.size() / 3] ^= 0x10; damaged("golden gzip, a flipped bit", bad, golden, threads, true);
            damaged("golden gzip, cut", one.substr(0, one.size() - 100), golden, threads, true);
            bad = one; bad[bad.size() - 1] ^= 0x40; damaged("golden gzip, ISIZE of 1 GiB more", bad, golden, threads, true);
            bad = one; bad[bad.size() - 8] ^= 1; damaged("golden gzip, wrong CRC", bad, golden, threads, true);
            std::vector<size_t> starts; const std::string blocks = bgzf(golden, 65280, &starts);
            bad = blocks; bad[(starts[1] + starts[2]) / 2] ^= 0x04; damaged("golden bgzf, a damaged block", bad, golden, threads, true);
            bad = blocks; bad[starts[1] + 16] = (char)(bad[starts[1] + 16] + 1); damaged("golden bgzf, BC size one more", bad, golden, threads, false);
            bad = blocks; bad[starts[1] + 16] = (char)(bad[starts[1] + 16] - 1); damaged("golden bgzf, BC size one less", bad, golden, threads, false);
            bad = blocks; bad[starts[2] - 1] ^= 0x01; damaged("golden bgzf, ISIZE of a block", bad, golden, threads, true);
            damaged("golden bgzf, cut inside a block", blocks.substr(0, starts[2] + 40), golden, threads, true);
            damaged("golden bgzf, cut to exactly 8192", blocks.substr(0, 8192), golden, threads, true);
            if (!golden_gz.empty()) { const std::string p = fresh(golden_gz, ".fna.gz"); if (!same(load(p, threads).recs, restate(golden))) fail("the golden multifasta.fna.gz does not give the genomes of multifasta.fna"); }
        }
        loader_modes(threads);
        g_first = false;
    }
    return hp::finish();
}
