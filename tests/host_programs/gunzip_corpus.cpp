// gunzip_corpus — vg_fast_gunzip (vg_inflate.cpp) against zlib on valid and damaged gzip streams.
//
//   gunzip_corpus [random-sample count, default 200]     the corpus; prints one line per stream and the fall-back classes
//   gunzip_corpus --big                                  one text above 32 MiB (more than one 16 MiB CRC piece) at 3 and 16 threads
//
// Property of every call: it returns false, or it returns exactly the text zlib gives for the same bytes.  Every input lives in
// a heap block of exactly its size, so a read behind it is seen by the address sanitizer.  Built without a sanitizer
// (VG_HP_PLAIN) the program first limits its own address space to 1 GiB: deflate expands at most 1032:1, every input here is
// at most 512 KiB, so nothing the decoder does for them may need more -- whatever the trailer claims.
// Exit status 0 only if every property held.
#include "host_programs.h"
#include <zlib.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/resource.h>
#include <sys/wait.h>
#include <time.h>
#include <algorithm>

bool vg_fast_gunzip(const unsigned char* in, size_t n, int n_threads, char** out_p, size_t* out_n);      // vg_inflate.cpp

// Every realloc of the program goes through here (the recipe links it with --wrap=realloc): the decoder's output buffer is the one
// caller, and the largest request of a call is what the memory bound is checked against.
static size_t g_largest_request = 0;
extern "C" void* __real_realloc(void* p, size_t n);
extern "C" void* __wrap_realloc(void* p, size_t n) { if (n > g_largest_request) g_largest_request = n; return __real_realloc(p, n); }

namespace {
using hp::rng64; using hp::fail;

// ---- texts
const char* const KINDS[4] = { "acgt", "fasta", "runs", "bytes" };
std::string make_text(int kind, size_t len, rng64& r) {
    std::string t; t.reserve(len + 128);
    if (kind == 0) { while (t.size() < len) t.push_back("ACGT"[r.below(4)]); }
    else if (kind == 1) {
        for (int rec = 0; t.size() < len; ++rec) {
            t += ">rec" + std::to_string(rec) + " sample text\n";
            const size_t n = r.below(4000), w = 40 + r.below(40); const bool crlf = r.below(4) == 0, lower = r.below(3) == 0;
            for (size_t i = 0; i < n; ++i) {
                const uint64_t x = r.below(200);
                t.push_back(x == 0 ? 'N' : x == 1 ? 'n' : (lower ? "acgt" : "ACGT")[x & 3]);
                if ((i + 1) % w == 0 || i + 1 == n) { if (crlf) t.push_back('\r'); t.push_back('\n'); }
            }
        }
    } else if (kind == 2) { while (t.size() < len) t.append((size_t)(1 + r.below(5000)), (char)r.below(256)); }
    else { while (t.size() < len) t.push_back((char)r.below(256)); }
    t.resize(len);
    return t;
}

// ---- streams
std::string gz_member(const std::string& text, int level, int strategy, bool named) {
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, 15 + 16, 8, strategy) != Z_OK) { fprintf(stderr, "deflateInit2 failed\n"); exit(2); }
    gz_header h; memset(&h, 0, sizeof h);
    if (named) { h.name = (Bytef*)"genomes.fna"; h.comment = (Bytef*)"a comment"; h.time = 12345; h.os = 3; deflateSetHeader(&zs, &h); }
    std::string out(deflateBound(&zs, (uLong)text.size()) + 64, '\0');
    zs.next_in = (Bytef*)text.data(); zs.avail_in = (uInt)text.size();
    zs.next_out = (Bytef*)&out[0]; zs.avail_out = (uInt)out.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { fprintf(stderr, "deflate failed\n"); exit(2); }
    out.resize(out.size() - zs.avail_out);
    deflateEnd(&zs);
    return out;
}
// one call on a heap block of exactly n bytes; true = the property held
// TOO_MUCH: the call asked for more memory than n bytes of deflate can need.  The text is at most 1032 n bytes; the output buffer
// grows when the text plus a chunk (64 KiB, a stored block, or the reservation, itself at most 1032 n) does not fit, to that plus
// 1 MiB or to one and a half times its size, whichever is more: never above 1.5 (1032 n + 2 MiB).
enum verdict { REJECTED, ACCEPTED, WRONG, TOO_MUCH };
verdict run_one(const unsigned char* bytes, size_t n, int n_threads, std::string* text_out = nullptr) {
    unsigned char* block = (unsigned char*)malloc(n ? n : 1);
    if (!block) { fprintf(stderr, "out of memory\n"); exit(2); }
    if (n) memcpy(block, bytes, n);
    char* o = nullptr; size_t on = 0;
    g_largest_request = 0;
    const bool took = vg_fast_gunzip(block, n, n_threads, &o, &on);
    const bool too_much = g_largest_request > (1032 * n + (2u << 20)) / 2 * 3;
    verdict v = REJECTED;
    if (took) {
        std::string ref;
        v = hp::zlib_gunzip(block, n, ref) && ref.size() == on && (on == 0 || !memcmp(ref.data(), o, on)) ? ACCEPTED : WRONG;
        if (text_out) text_out->assign(o, on);
        free(o);
    }
    free(block);
    return too_much ? TOO_MUCH : v;
}

struct stream { std::string name; std::string bytes; std::string text; size_t trailer; bool must_accept; };

// a worker's findings go into the text it hands back: the parent prints them in stream order
void note(std::string& log, const std::string& line) { log += line; log += '\n'; }
void failed(std::string& log, const std::string& what) { note(log, "FAILED " + what); ++hp::failures(); }

// every damaged variant of one valid stream; reports how many of them the decoder accepted (each with zlib's text)
void damage(const stream& s, int n_random, rng64& r, std::string& log) {
    const size_t m = s.bytes.size();
    std::vector<unsigned char> v(s.bytes.begin(), s.bytes.end());
    long n_var = 0, n_acc = 0;
    auto check = [&](size_t n, const char* what, size_t where) {
        ++n_var;
        const verdict d = run_one(v.data(), n, 2);
        if (d == ACCEPTED) ++n_acc;
        if (d == WRONG) failed(log, s.name + ": " + what + " at " + std::to_string(where) + ": accepted with a text that is not zlib's");
        if (d == TOO_MUCH) failed(log, s.name + ": " + what + " at " + std::to_string(where) + ": more memory asked for than the input can need");
    };
    auto flip = [&](size_t bit) { v[bit >> 3] ^= (unsigned char)(1u << (bit & 7)); check(m, "bit flip", bit); v[bit >> 3] ^= (unsigned char)(1u << (bit & 7)); };
    const size_t head = m < 64 ? m : 64, tail = m - head < 16 ? head : m - 16;
    for (size_t bit = 0; bit < head * 8; ++bit) flip(bit);
    for (size_t bit = tail * 8; bit < m * 8; ++bit) flip(bit);
    if (tail > head) for (int k = 0; k < n_random; ++k) flip(head * 8 + r.below((tail - head) * 8));
    if (m < 2048) for (size_t n = 0; n < m; ++n) check(n, "cut", n);
    else for (int k = 0; k < n_random; ++k) { const size_t n = r.below(m); check(n, "cut", n); }
    // the last member's trailer: CRC-32, then ISIZE
    uint32_t isz; memcpy(&isz, &v[s.trailer + 4], 4);
    for (const uint32_t x : { 0u, 0xffffffffu, isz + 1, isz - 1 }) {
        if (x == isz) continue;
        memcpy(&v[s.trailer + 4], &x, 4); check(m, "ISIZE", x); memcpy(&v[s.trailer + 4], &isz, 4);
    }
    v[s.trailer] ^= 1; check(m, "CRC", s.trailer); v[s.trailer] ^= 1;
    char line[160];
    snprintf(line, sizeof line, "stream %-28s bytes %7zu  variants %5ld  accepted %3ld", s.name.c_str(), m, n_var, n_acc);
    note(log, line);
}
// one valid stream and its variants
void one_stream(const stream& s, size_t index, int n_random, std::string& log) {
    if (s.bytes.size() > (512u << 10)) { failed(log, s.name + ": the stream is above 512 KiB, the memory bound does not cover it"); return; }
    std::string got;
    const verdict d = run_one((const unsigned char*)s.bytes.data(), s.bytes.size(), 2, &got);
    if (d == WRONG || (d == ACCEPTED && got != s.text)) failed(log, s.name + ": the valid stream gives another text");
    if (d == TOO_MUCH) failed(log, s.name + ": the valid stream asks for more memory than the input can need");
    if (d == REJECTED) {
        std::string ref;
        if (!hp::zlib_gunzip((const unsigned char*)s.bytes.data(), s.bytes.size(), ref) || ref != s.text) failed(log, s.name + ": zlib does not give the text back");
        if (s.must_accept) failed(log, s.name + ": a valid stream of a class the fast path must take was declined");
        else note(log, "fell back: " + s.name);
    }
    rng64 r{ 1000 + index };
    damage(s, n_random, r, log);
}

// Named cases: the smallest inputs that showed a fault of the decoder, kept in the corpus.
//   cut-costs-no-more: a stream cut in the middle of a block was decoded on, zeros for bits, until a whole output chunk
//     (1 MiB and more) was full: 40 times the work of the valid stream for 5 000 bases.  CPU time of 300 cut streams against 300
//     valid ones (the margin is a factor of four and 10 ms; the fault was a factor of forty).
//   isize-4gib: a trailer that claims 0xffffffff bytes made the decoder reserve 4 GiB before it had verified anything.  The valid
//     stream with that trailer is declined, and the largest request of the call stays within what its bytes can need (every call of
//     the corpus is held to the same bound, see TOO_MUCH).
void named_cases(const std::vector<stream>& streams, std::string& log) {
    const stream* s = nullptr;
    for (const stream& x : streams) if (x.name == "level6 acgt-5000") s = &x;
    if (!s) { failed(log, "named cases: no stream level6 acgt-5000"); return; }
    const int rounds = 300;
    auto seconds = [&](size_t n, bool want) {
        struct timespec t0, t1; clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &t0);
        for (int k = 0; k < rounds; ++k) {
            char* o = nullptr; size_t on = 0;
            const bool took = vg_fast_gunzip((const unsigned char*)s->bytes.data(), n, 1, &o, &on);
            if (took) free(o);
            if (took != want) failed(log, "named cases: cut-costs-no-more: another verdict");
        }
        clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &t1);
        return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    };
    const double whole = seconds(s->bytes.size(), true), cut = seconds(s->bytes.size() / 2, false);
    fprintf(stderr, "cut-costs-no-more: %d valid streams %.4f s, %d cut streams %.4f s\n", rounds, whole, rounds, cut);
    if (cut > 4 * whole + 0.01) failed(log, "named cases: cut-costs-no-more: a cut stream costs more than four valid ones");
    std::string claims = s->bytes; memset(&claims[claims.size() - 4], 0xff, 4);
    const verdict d = run_one((const unsigned char*)claims.data(), claims.size(), 1);
    if (d != REJECTED) failed(log, d == TOO_MUCH ? "named cases: isize-4gib: memory reserved from the unverified trailer" : "named cases: isize-4gib: accepted");
    note(log, "named cases: cut-costs-no-more, isize-4gib");
}

void corpus(int n_random) {
    rng64 r{ 20240611 };
    static const size_t LENGTHS[] = { 0, 1, 7, 300, 5000, 70000, 300000 };
    std::vector<stream> streams;
    for (const size_t len : LENGTHS)
        for (int kind = 0; kind < (len ? 4 : 1); ++kind) {
            const std::string text = make_text(kind, len, r);
            const std::string tag = std::string(len ? KINDS[kind] : "empty") + "-" + std::to_string(len);
            auto add = [&](const std::string& cls, const std::string& bytes, size_t pad, bool must) {
                streams.push_back({ cls + " " + tag, bytes, text, bytes.size() - pad - 8, must });
            };
            for (int level = 0; level <= 9; ++level)
                add("level" + std::to_string(level), gz_member(text, level, Z_DEFAULT_STRATEGY, false), 0, level == 0 || level == 1 || level == 6 || level == 9);
            add("fixed", gz_member(text, 6, Z_FIXED, false), 0, true);
            add("huffman", gz_member(text, 6, Z_HUFFMAN_ONLY, false), 0, false);
            add("rle", gz_member(text, 6, Z_RLE, false), 0, false);
            const size_t c1 = len / 3, c2 = len - len / 4;
            add("two-members", gz_member(text.substr(0, c1), 6, Z_DEFAULT_STRATEGY, false) + gz_member(text.substr(c1), 2, Z_DEFAULT_STRATEGY, false), 0, true);
            add("three-members", gz_member(text.substr(0, c1), 9, Z_DEFAULT_STRATEGY, false) + gz_member(text.substr(c1, c2 - c1), 0, Z_DEFAULT_STRATEGY, false) +
                                 gz_member(text.substr(c2), 4, Z_FIXED, false), 0, true);
            add("empty-middle", gz_member(text.substr(0, c1), 6, Z_DEFAULT_STRATEGY, false) + gz_member("", 6, Z_DEFAULT_STRATEGY, false) +
                                gz_member(text.substr(c1), 2, Z_DEFAULT_STRATEGY, false), 0, true);
            add("named", gz_member(text, 6, Z_DEFAULT_STRATEGY, true), 0, true);
            add("zero-padded", gz_member(text, 6, Z_DEFAULT_STRATEGY, false) + std::string(37, '\0'), 37, false);
        }
    // The streams are dealt out to worker processes (one call at a time in each, so the address-space limit holds per call);
    // every worker leaves one file of "<stream index>\t<line>" and the parent prints the lines in stream order.
    const int workers = (int)std::max<long>(1, std::min<long>(8, sysconf(_SC_NPROCESSORS_ONLN)));
    hp::scratch_dir dir;
    std::vector<std::string> files; std::vector<pid_t> pids;
    for (int w = 0; w < workers; ++w) files.push_back(dir.file("worker" + std::to_string(w)));
    fflush(stdout);
    for (int w = 0; w < workers; ++w) {
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); exit(2); }
        if (pid == 0) {
            prctl(PR_SET_PDEATHSIG, SIGKILL);          // (a parent that is ended at a time limit takes its workers with it)
            std::string all;
            for (size_t i = (size_t)w; i < streams.size(); i += (size_t)workers) {
                std::string log;
                one_stream(streams[i], i, n_random, log);
                for (size_t a = 0; a < log.size();) { const size_t e = log.find('\n', a); all += std::to_string(i) + "\t" + log.substr(a, e - a + 1); a = e + 1; }
            }
            hp::write_file(files[(size_t)w], all);
            _exit(hp::failures() ? 1 : 0);
        }
        pids.push_back(pid);
    }
    for (const pid_t pid : pids) {
        int st = 0;
        if (waitpid(pid, &st, 0) != pid || !WIFEXITED(st) || WEXITSTATUS(st) > 1) fail("a worker process did not finish (killed, or out of memory under the limit)");
        else if (WEXITSTATUS(st) == 1) ++hp::failures();
    }
    std::vector<std::string> lines(streams.size());
    for (const std::string& f : files) {
        std::string text;
        if (!hp::read_file(f, text)) continue;
        for (size_t a = 0; a < text.size();) { const size_t e = text.find('\n', a), tab = text.find('\t', a); lines[(size_t)atol(text.c_str() + a)] += text.substr(tab + 1, e - tab); a = e + 1; }
    }
    std::string rest, fell; size_t n_fell = 0;
    for (const std::string& l : lines)
        for (size_t a = 0; a < l.size();) {
            const size_t e = l.find('\n', a); const std::string one = l.substr(a, e - a + 1); a = e + 1;
            if (one.compare(0, 10, "fell back:") == 0) { fell += one; ++n_fell; } else rest += one;
        }
    std::string log;
    named_cases(streams, log);
    printf("%s%s%sfell back: %zu valid streams\n", rest.c_str(), log.c_str(), fell.c_str(), n_fell);
}

// the CRC-32 pieces on worker threads: a text above 32 MiB has three 16 MiB pieces
void big() {
    rng64 r{ 7 };
    std::string text; text.reserve(40u << 20);
    const std::string unit = make_text(1, 1u << 20, r);
    while (text.size() < (40u << 20) + 12345) { text += unit; text += make_text(0, 1000, r); }
    const std::string one = gz_member(text, 1, Z_DEFAULT_STRATEGY, false);
    const std::string two = gz_member(text.substr(0, 36u << 20), 1, Z_DEFAULT_STRATEGY, false) + gz_member(text.substr(36u << 20), 6, Z_DEFAULT_STRATEGY, false);
    for (const std::string* s : { &one, &two })
        for (const int threads : { 1, 3, 16 }) {
            std::string got;
            const verdict d = run_one((const unsigned char*)s->data(), s->size(), threads, &got);
            if (d != ACCEPTED || got != text) fail("big text, " + std::to_string(threads) + " threads: not the text");
            printf("big %s members, %2d threads: %s, %zu bytes\n", s == &one ? "one" : "two", threads, d == ACCEPTED ? "accepted" : "not accepted", got.size());
        }
    std::string bad = one; bad[bad.size() - 8] ^= 1;                // the CRC of the last piece decides
    if (run_one((const unsigned char*)bad.data(), bad.size(), 16) != REJECTED) fail("big text with a wrong CRC was not declined");
}
}  // namespace

int main(int argc, char** argv) {
    const bool is_big = argc > 1 && !strcmp(argv[1], "--big");
#ifdef VG_HP_PLAIN
    if (!is_big) {
        struct rlimit lim = { (rlim_t)1 << 30, (rlim_t)1 << 30 };
        if (setrlimit(RLIMIT_AS, &lim) != 0) { perror("setrlimit"); return 2; }
        fprintf(stderr, "address space limited to 1 GiB\n");
    }
#endif
    if (is_big) big(); else corpus(argc > 1 ? atoi(argv[1]) : 200);
    return hp::finish();
}
