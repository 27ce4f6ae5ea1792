// vg_genomes.cpp — FASTA / FASTA.gz ingest, 2-bit packing, HBM residency.
// Input conventions follow the reference front-end (vclust.py:687-702, 962-963, 1159-1160):
// a single (multi-)FASTA file = one genome per record, a directory = one genome per file.
#include "vg_common.h"
#include <sys/mman.h>
#include <zlib.h>
#include <string.h>
#include <stdlib.h>
#include <thread>
#include <atomic>
#include <algorithm>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <unordered_set>

static inline uint8_t code_of(unsigned char ch) {
    switch (ch) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

void vg_genomes_append(vg_genomes* g, const std::string& name, const uint8_t* codes, int64_t len, int n_parts) {
    const int64_t off = vg_layout_append(g, len), padded = g->base_off.back() - off;
    g->packed.resize((off + padded) / 16, 0u);
    g->nmask.resize((off + padded) / 32, 0u);
    uint32_t* pk = g->packed.data() + off / 16;
    uint32_t* mk = g->nmask.data() + off / 32;
    bool any_n = false;
    for (int64_t i = 0; i < len; ++i) {
        uint8_t c = codes[i];
        if (c > 3) { mk[i >> 5] |= 1u << (i & 31); any_n = true; }
        else pk[i >> 4] |= (uint32_t)c << (2 * (i & 15));
    }
    for (int64_t i = len; i < padded; ++i) mk[i >> 5] |= 1u << (i & 31);
    g->names.push_back(name);
    g->len.push_back(len);
    g->n_parts.push_back(n_parts);
    g->has_n.push_back(any_n ? 1 : 0);
    g->n++;
}

int vg_choose_align_shift(int64_t total_len, int64_t n) {
    int64_t mean = n > 0 ? total_len / n : 0;
    int sh = 6;
    while (sh < 12 && (1LL << (sh + 1)) <= mean / 16) ++sh;
    return sh;
}

void vg_genomes_finish(vg_genomes* g) {
    if (g->base_off.empty()) g->base_off.push_back(0);
    // slack so that kernels may read a few words past the last genome
    g->packed.resize(g->padded_total() / 16 + 16, 0u);
    g->nmask.resize(g->padded_total() / 32 + 16, 0xffffffffu);
    vg_layout_close(g);
}

bool vg_fast_gunzip(const unsigned char* in, size_t n, int n_threads, char** out_p, size_t* out_n);      // vg_inflate.cpp

namespace {
// ---- whole-file buffers ---------------------------------------------------------------------
struct filebuf {            // plain files are mapped (no copy), gzip files are inflated into `own`
    std::vector<char> own; char* own_raw = nullptr; const char* ptr = nullptr; size_t len = 0; void* map = nullptr; size_t map_len = 0;
    std::mutex hole_mu; std::vector<std::pair<size_t, size_t>> holes;      // page ranges of the mapping already given back
    filebuf() {}
    filebuf(const filebuf&) = delete; filebuf& operator=(const filebuf&) = delete;
    // Unmapping 4 GB of FASTA in one call holds the address-space lock for 55-80 ms: wherever that call was put -- a
    // helper thread right after the ingest, or parked until the kernels run -- allocations, mappings and page faults of
    // the main thread queued up behind it (120 ms in front of the first small hipMalloc of vg_kmer_shared, 50 ms inside
    // the filter reader, 80 ms inside the bucket pipeline).  So the text is given back WHILE it is packed: the thread
    // that completes a stretch of genomes unmaps the whole pages of that stretch (drop; ~130 MB, 1-2 ms, beside 63
    // threads that do not fault), and what is left at the end (page edges, files of a directory) goes in slices.
    void drop(const char* lo, const char* hi) {
        if (!map || hi <= lo) return;
        const size_t pg = 4096;
        size_t a = ((size_t)(lo - (const char*)map) + pg - 1) / pg * pg, b = (size_t)(hi - (const char*)map) / pg * pg;
        if (b > map_len) b = map_len / pg * pg;
        if (b <= a) return;
        { std::lock_guard<std::mutex> lk(hole_mu); holes.emplace_back(a, b); }
        munmap((char*)map + a, b - a);
    }
    ~filebuf() {
        free(own_raw);
        if (!map) return;
        std::sort(holes.begin(), holes.end());
        const size_t slice = 32u << 20;
        auto give = [&](size_t a, size_t b) { for (size_t off = a; off < b; off += slice) munmap((char*)map + off, std::min(slice, b - off)); };
        size_t at = 0;
        for (auto& h : holes) { if (h.first > at) give(at, h.first); at = std::max(at, h.second); }
        if (map_len > at) give(at, map_len);
    }
    const char* data() const { return ptr; }
    size_t size() const { return len; }
};

// BGZF (bgzip, htslib): a series of gzip members of <= 64 KiB each, every member carrying its own compressed size in
// a 'BC' extra subfield -- the members can be found without inflating anything, so they are inflated in parallel.
// Returns false (nothing touched) when the file is not BGZF from its first to its last byte.
struct bgzf_block { size_t cdata, clen, out_off; uint32_t isize, crc; };
bool bgzf_blocks(const unsigned char* p, size_t n, std::vector<bgzf_block>& blocks, size_t* total) {
    size_t at = 0, out = 0;
    while (at < n) {
        if (n - at < 28 || p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || !(p[at + 3] & 4)) return false;
        const size_t xlen = (size_t)p[at + 10] | ((size_t)p[at + 11] << 8);
        if (at + 12 + xlen > n) return false;
        size_t bsize = 0;
        for (size_t x = at + 12; x + 4 <= at + 12 + xlen;) {
            const size_t slen = (size_t)p[x + 2] | ((size_t)p[x + 3] << 8);
            if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= at + 12 + xlen) bsize = ((size_t)p[x + 4] | ((size_t)p[x + 5] << 8)) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || at + bsize > n || (p[at + 3] & ~4)) return false;     // (no name / comment / hcrc fields in BGZF)
        const unsigned char* tail = p + at + bsize - 8;
        bgzf_block b; b.cdata = at + 12 + xlen; b.clen = bsize - 12 - xlen - 8; b.out_off = out;
        b.crc = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
        b.isize = (uint32_t)tail[4] | ((uint32_t)tail[5] << 8) | ((uint32_t)tail[6] << 16) | ((uint32_t)tail[7] << 24);
        if (b.isize > 65536u) return false;
        out += b.isize; at += bsize;
        blocks.push_back(b);
    }
    *total = out;
    return !blocks.empty();
}

// an open file mapped whole and read-only (no mapping: empty or not mappable), given back on the way out unless handed over
struct mapped_file {
    long long size; void* p = MAP_FAILED;
    explicit mapped_file(FILE* f) { fseek(f, 0, SEEK_END); size = ftell(f); if (size > 0) p = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fileno(f), 0); }
    mapped_file(const mapped_file&) = delete; mapped_file& operator=(const mapped_file&) = delete;
    ~mapped_file() { if (p != MAP_FAILED) munmap(p, (size_t)size); }
    explicit operator bool() const { return p != MAP_FAILED; }
    void advise(int advice) const { (void)madvise(p, (size_t)size, advice); }
    void hand_over(filebuf& fb) { fb.map = p; fb.map_len = (size_t)size; fb.ptr = (const char*)p; fb.len = (size_t)size; p = MAP_FAILED; }
};

bool slurp_bgzf(const std::string& path, FILE* f, filebuf& fb, int n_threads) {
    const mapped_file m(f);
    if (m.size < 28 || !m) return false;
    const unsigned char* p = (const unsigned char*)m.p;
    std::vector<bgzf_block> blocks; size_t total = 0;
    if (!bgzf_blocks(p, (size_t)m.size, blocks, &total)) return false;
    vg_host_mark("ingest: bgzf members found");
    m.advise(MADV_WILLNEED);
    // (not a std::vector: its resize would clear 800 MB on one thread before the workers overwrite them)
    fb.own_raw = (char*)malloc(std::max<size_t>(total, 1));
    if (!fb.own_raw) throw vg_error(VG_ENOMEM, "out of host memory");
    char* const text = fb.own_raw;
    std::atomic<bool> bad(false);
    // runs of 64 blocks (<= 4 MiB of text) per work item
    const int64_t n_items = ((int64_t)blocks.size() + 63) / 64;
    vg_parallel_for(n_items, n_threads, [&](int64_t it) {
        z_stream zs; memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) { bad = true; return; }
        for (size_t b = (size_t)it * 64; b < std::min(blocks.size(), (size_t)(it + 1) * 64) && !bad.load(std::memory_order_relaxed); ++b) {
            const bgzf_block& k = blocks[b];
            // (zlib: for 64 KiB members the own decoder's table builds and scratch copy cost more than its loop saves --
            // 3.3 s against 2.4 s for 814 MB on one thread)
            if (b != (size_t)it * 64 && inflateReset(&zs) != Z_OK) { bad = true; break; }
            zs.next_in = (Bytef*)(p + k.cdata); zs.avail_in = (uInt)k.clen;
            zs.next_out = (Bytef*)text + k.out_off; zs.avail_out = k.isize;
            const int rc = inflate(&zs, Z_FINISH);
            if (rc != Z_STREAM_END || zs.avail_out != 0 || zs.avail_in != 0 ||
                (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)text + k.out_off, k.isize) != k.crc) { bad = true; break; }
        }
        inflateEnd(&zs);
    });
    vg_host_mark("ingest: bgzf inflated");
    if (bad.load()) throw vg_error(VG_EIO, "read error in " + path + " (corrupt BGZF block)");
    fb.ptr = text; fb.len = total;
    return true;
}

void slurp(const std::string& path, filebuf& fb, int n_threads) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw vg_error(VG_EIO, "cannot open " + path);
    unsigned char magic[2] = { 0, 0 };
    size_t got = fread(magic, 1, 2, f);
    const bool gz = got == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
    if (!gz) {
        mapped_file m(f);
        if (m) { m.advise(MADV_WILLNEED); m.hand_over(fb); fclose(f); return; }
        fseek(f, 0, SEEK_SET);                           // not mappable (pipe, special file): read it
        fb.own.resize((size_t)std::max<long long>(m.size, 0));
        size_t off = 0;
        while (off < fb.own.size()) { size_t r = fread(fb.own.data() + off, 1, fb.own.size() - off, f); if (!r) break; off += r; }
        fclose(f);
        if (off != fb.own.size()) throw vg_error(VG_EIO, "read error in " + path);
        fb.ptr = fb.own.data(); fb.len = fb.own.size();
        return;
    }
    // bgzip output inflates block-parallel; any other gzip stream (one member, or members of unknown size) serially:
    // first by the library's own decoder (vg_inflate.cpp: ~1.3x zlib's inflate per thread, CRC-32 on worker threads,
    // every member verified), and by zlib if that one declines the file (VG_GZ=zlib: always zlib)
    bool done = false;
    try { done = slurp_bgzf(path, f, fb, n_threads); } catch (...) { fclose(f); throw; }
    static const bool zlib_only = [] { const char* e = vg_dev_getenv("VG_GZ"); return e && !strcmp(e, "zlib"); }();
    if (!done && !zlib_only) {
        const mapped_file m(f);
        if (m) {
            m.advise(MADV_SEQUENTIAL);
            char* o = nullptr; size_t on = 0;
            if (vg_fast_gunzip((const unsigned char*)m.p, (size_t)m.size, n_threads, &o, &on)) { fb.own_raw = o; fb.ptr = o; fb.len = on; done = true; vg_host_mark("ingest: gzip inflated by the own decoder"); }
        }
    }
    fclose(f);
    if (done) return;
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) throw vg_error(VG_EIO, "cannot open " + path);
    gzbuffer(g, 1 << 20);
    size_t off = 0; fb.own.resize(1 << 22);
    for (;;) {
        if (fb.own.size() - off < (1 << 20)) fb.own.resize(fb.own.size() * 2);
        int n = gzread(g, fb.own.data() + off, (unsigned)std::min<size_t>(fb.own.size() - off, 1u << 30));
        if (n < 0) { gzclose(g); throw vg_error(VG_EIO, "read error in " + path); }
        if (n == 0) break;
        off += (size_t)n;
    }
    int zerr = 0; (void)gzerror(g, &zerr);
    gzclose(g);
    if (zerr != Z_OK && zerr != Z_STREAM_END) throw vg_error(VG_EIO, "read error in " + path);
    fb.own.resize(off);
    fb.ptr = fb.own.data(); fb.len = off;
}

// every file whole in memory (gz inflated), files in parallel.  The first failure ends the reading and comes out as VG_EIO
// with that file's message, whatever its own code was (an allocation that failed in the BGZF path included).
void read_files(const char* const* paths, int n_paths, int T, std::vector<filebuf>& bufs) {
    bufs = std::vector<filebuf>((size_t)std::max(n_paths, 0));
    std::string first_err; std::atomic<bool> failed(false);
    vg_parallel_for(n_paths, T, [&](int64_t i) {
        if (failed.load()) return;
        try { slurp(paths[i], bufs[(size_t)i], std::max(1, T / (int)std::min<int64_t>(n_paths, T))); }
        catch (const std::exception& e) { if (!failed.exchange(true)) first_err = e.what(); }
    });
    if (failed.load()) throw vg_error(VG_EIO, first_err);
}

// one FASTA record inside a buffer: [hdr, hdr_end) header line without '>', [seq, end) sequence lines
struct record { const char* hdr; const char* hdr_end; const char* seq; const char* end; int64_t len; };

struct code_lut { uint8_t t[256]; code_lut() { for (int i = 0; i < 256; ++i) t[i] = code_of((unsigned char)i); } };
const code_lut LUT;
inline bool is_ws(char ch) { return ch == '\n' || ch == '\r' || ch == ' ' || ch == '\t'; }

void find_records(const filebuf& fb, std::vector<record>& out, int n_threads) {
    const char* p = fb.data(); const char* e = p + fb.size();
    // record starts: '>' at the beginning of a line, found chunk-parallel with memchr
    const int T = std::max(1, n_threads);
    std::vector<std::vector<const char*>> starts(T);
    vg_parallel_for(T, T, [&](int64_t t) {
        const char* lo = p + fb.size() * t / T; const char* hi = p + fb.size() * (t + 1) / T;
        // piece by piece: the pages of a piece are mapped in one call (instead of one minor fault per 64 KB) and scanned
        // while they are hot.  Small pieces on purpose: a populate call holds the address-space lock shared, and the
        // HIP context that is being created on the warm-up thread needs it exclusively for every mapping it makes --
        // with one call per 64 MB stretch the context took 350 ms instead of 150.
        const size_t piece = 2u << 20;
        for (const char* c0 = lo; c0 < hi; c0 += piece) {
            const char* c1 = std::min(hi, c0 + piece);
#ifdef MADV_POPULATE_READ
            if (fb.map) {
                const uintptr_t a = (uintptr_t)c0 & ~(uintptr_t)4095, b = ((uintptr_t)c1 + 4095) & ~(uintptr_t)4095;
                (void)madvise((void*)a, (size_t)(b - a), MADV_POPULATE_READ);
            }
#endif
            for (const char* q = c0; q < c1;) {
                const char* g = (const char*)memchr(q, '>', (size_t)(c1 - q));
                if (!g) break;
                if (g == p || g[-1] == '\n') starts[t].push_back(g);
                q = g + 1;
            }
        }
    });
    std::vector<const char*> all;
    for (auto& v : starts) all.insert(all.end(), v.begin(), v.end());
    out.resize(all.size());
    // (the header line of every record is touched here: 10^5 cache misses when done by one thread)
    vg_parallel_for(((int64_t)all.size() + 1023) / 1024, T, [&](int64_t c) {
        for (size_t i = (size_t)c * 1024; i < std::min(all.size(), (size_t)(c + 1) * 1024); ++i) {
            record& r = out[i];
            r.hdr = all[i] + 1;
            const char* rec_end = i + 1 < all.size() ? all[i + 1] : e;
            const char* nl = (const char*)memchr(r.hdr, '\n', (size_t)(rec_end - r.hdr));
            r.hdr_end = nl ? nl : rec_end; r.seq = nl ? nl + 1 : rec_end; r.end = rec_end; r.len = 0;
        }
    });
}

// pack the bases of one record into the set's arrays starting at padded base position `at` (2-bit codes + N mask);
// returns true if an N was seen.  Callers own disjoint word ranges and the arrays are zero.  Line by line (memchr
// for the line end), sixteen symbols per trip: sixteen table look-ups OR-ed into one 32-bit group, no per-symbol
// branch, appended to the output through a 64-bit shift register (the output need not be word aligned).  A group
// with anything unusual in it (N, white space inside a line) goes symbol by symbol.
struct pack_lut { uint8_t t[256]; pack_lut() { for (int i = 0; i < 256; ++i) { const char ch = (char)i; t[i] = is_ws(ch) ? 5 : code_of((unsigned char)i); } } };
const pack_lut PLUT;
bool pack_record(const record& r, vg_genomes* g, int64_t at, int64_t* n_symbols) {
    uint32_t* pk = g->packed.data(); uint32_t* mk = g->nmask.data();
    bool any_n = false; int64_t i = at;                       // i = position of the next symbol
    uint64_t acc = 0; int nb = 2 * (int)(at & 15);            // pending output bits of word (i - pending symbols) >> 4
    int64_t wo = at >> 4;                                     // word the low bits of acc belong to
    auto flush = [&]() { while (nb >= 32) { pk[wo++] |= (uint32_t)acc; acc >>= 32; nb -= 32; } };
    const char* q = r.seq; const char* const end = r.end;
    while (q < end) {
        const char* nl = (const char*)memchr(q, '\n', (size_t)(end - q));
        const char* const le = nl ? nl : end;
        while (q < le) {
            const int m = (int)std::min<int64_t>(16, le - q);
            uint32_t w = 0, bad = 0;
            for (int j = 0; j < m; ++j) { const uint32_t c = PLUT.t[(unsigned char)q[j]]; w |= (c & 3u) << (2 * j); bad |= c; }
            if (bad < 4) { acc |= (uint64_t)w << nb; nb += 2 * m; i += m; q += m; flush(); continue; }
            for (int j = 0; j < m; ++j) {
                const uint32_t c = PLUT.t[(unsigned char)q[j]];
                if (c == 5) continue;
                if (c == 4) { mk[i >> 5] |= 1u << (i & 31); any_n = true; } else acc |= (uint64_t)c << nb;
                nb += 2; ++i; flush();
            }
            q += m;
        }
        q = nl ? nl + 1 : end;
    }
    if (nb > 0) pk[wo] |= (uint32_t)acc;
    *n_symbols = i - at;
    return any_n;
}

std::string first_token(const char* b, const char* e) {
    const char* q = b; while (q < e && *q != ' ' && *q != '\t' && *q != '\r') ++q;
    return std::string(b, q);
}
}  // namespace

// The N mask of a genome without N is its padding and nothing else: it is written on the device from the genome's
// length instead of travelling (a third of the upload of a set).  One thread per mask word; words of genomes that do
// hold an N are left alone (they are uploaded).
__global__ void __launch_bounds__(256)
k_mask_of_lengths(uint32_t* __restrict__ nmask, int64_t n_words, const uint32_t* __restrict__ blk2g, int align_shift,
                  const int64_t* __restrict__ base_off, const int64_t* __restrict__ len, const uint8_t* __restrict__ has_n) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p0 = w * 32;
        const uint32_t gi = blk2g[p0 >> align_shift];
        if (has_n[gi]) continue;
        const int64_t end = base_off[gi] + len[gi];              // first padding position of the genome
        nmask[w] = end >= p0 + 32 ? 0u : end <= p0 ? 0xffffffffu : (0xffffffffu << (uint32_t)(end - p0));
    }
}

// the small arrays of a set on the device (stream s): offsets, lengths, N flags, block -> genome
static void upload_tables(vg_genomes* g, hipStream_t s) {
    g->d_base_off.alloc(g->base_off.size()); g->d_base_off.upload(g->base_off.data(), g->base_off.size(), s);
    g->d_len.alloc(std::max<size_t>(1, g->len.size())); if (g->n) g->d_len.upload(g->len.data(), g->len.size(), s);
    g->d_has_n.alloc(std::max<size_t>(1, g->has_n.size())); if (g->n) g->d_has_n.upload(g->has_n.data(), g->has_n.size(), s);
    g->d_blk2g.alloc(g->blk2g.size()); g->d_blk2g.upload(g->blk2g.data(), g->blk2g.size(), s);
}

namespace {      // ---- the loader: stages over one state (Ingest)
// n_db_paths >= 0 (vg_genomes_load_db_new): the first n_db_paths files are the database, the others the new genomes; multisample
// then means one genome per record of BOTH files.  resident: the set comes back on the library's device (upload_pipe).
struct load_request { const char* const* paths; int n_paths; int multisample; int n_threads; bool resident; int n_db_paths; };
// The text and its records.  They go to a helper thread at the end: unmapping 4 GB of FASTA costs ~80 ms the caller need not wait for.
struct ingest_input { std::vector<filebuf> bufs; std::vector<std::vector<record>> recs; };
struct deferred_delete { void operator()(ingest_input* p) const { try { vg_defer([p] { delete p; }); } catch (...) { delete p; } } };
struct gdesc { int file; size_t r0, r1; int64_t len; };      // a genome: records [r0, r1) of a file, its length (an upper bound until packed)
struct ingest {
    const load_request& rq; const int T; const bool multi;
    std::unique_ptr<ingest_input, deferred_delete> in{ new ingest_input() };
    std::vector<gdesc> gd; int64_t total = 0;
    std::unique_ptr<vg_genomes> g{ new vg_genomes() };
    explicit ingest(const load_request& r) : rq(r), T(std::max(1, r.n_threads)), multi(r.multisample && (r.n_db_paths >= 0 || r.n_paths == 1)) {}
};

// records -> genomes and their lengths
void plan_genomes(ingest& s) {
    std::vector<std::vector<record>>& recs = s.in->recs = std::vector<std::vector<record>>((size_t)s.rq.n_paths);
    for (int i = 0; i < s.rq.n_paths; ++i) {
        find_records(s.in->bufs[(size_t)i], recs[(size_t)i], s.multi ? s.T : 1);
        if (s.multi) for (size_t r = 0; r < recs[(size_t)i].size(); ++r) s.gd.push_back({ i, r, r + 1, 0 });
        else if (!recs[(size_t)i].empty()) s.gd.push_back({ i, 0, recs[(size_t)i].size(), 0 });
    }
    // No counting pass over the text: the layout is made from an UPPER BOUND of every genome's length -- the bytes of its
    // sequence lines, line ends included (1/60 more than the truth for 60-column FASTA) --, the true length is what the
    // packer has written when it reaches the end of the record, and the difference is padding (masked like the padding
    // that aligns the next genome anyway).  One pass over 4 GB of text less per process.
    for (auto& d : s.gd) {
        for (size_t r = d.r0; r < d.r1; ++r) d.len += (int64_t)(recs[(size_t)d.file][r].end - recs[(size_t)d.file][r].seq);
        d.len += (int64_t)(d.r1 - d.r0) - 1;                 // records of one genome are joined by one N
        s.total += d.len;
    }
}

// the layout rule over the upper bounds, and the names.  A database/new load is checked here, before anything is packed or any
// device is asked for: *n_db_genomes receives the database's genome count, a name on both sides is VG_EINVAL
void lay_out(ingest& s, int* n_db_genomes) {
    vg_genomes* g = s.g.get();
    g->align_shift = vg_choose_align_shift(s.total, (int64_t)s.gd.size()); g->base_off.push_back(0);
    for (auto& d : s.gd) {
        vg_layout_append(g, d.len);
        g->len.push_back(0); g->n_parts.push_back((int32_t)(d.r1 - d.r0)); g->has_n.push_back(0);      // (the length: set by the packer)
        const record& r0 = s.in->recs[(size_t)d.file][d.r0];
        if (s.multi) g->names.push_back(first_token(r0.hdr, r0.hdr_end));
        else { std::string pth = s.rq.paths[d.file]; size_t sl = pth.find_last_of('/'); g->names.push_back(sl == std::string::npos ? pth : pth.substr(sl + 1)); }
        g->n++;
    }
    if (s.rq.n_db_paths < 0) return;
    int n_db = 0; while (n_db < g->n && s.gd[(size_t)n_db].file < s.rq.n_db_paths) ++n_db;
    std::unordered_set<std::string> db_names(g->names.begin(), g->names.begin() + n_db);
    for (int i = n_db; i < g->n; ++i)
        if (db_names.count(g->names[(size_t)i]))
            throw vg_error(VG_EINVAL, "vg_genomes_load_db_new: the name " + g->names[(size_t)i] + " occurs in the database and in the new genomes");
    *n_db_genomes = n_db;
    if (g->n < 2) throw vg_error(VG_EINVAL, "vg_genomes_load_db_new: the database and the new genomes together are " + std::to_string(g->n) + " genome(s); pairs need at least 2");
}

// first touch in parallel: the arrays are written by the packing threads right after
void clear_arrays(ingest& s) {
    vg_genomes* g = s.g.get();
    g->packed.reserve((size_t)(g->padded_total() / 16) + 16); g->nmask.reserve((size_t)(g->padded_total() / 32) + 16);   // + the slack vg_genomes_finish adds
    g->packed.resize((size_t)(g->padded_total() / 16)); g->nmask.resize((size_t)(g->padded_total() / 32));
    const int64_t chunk = 1 << 20, np = ((int64_t)g->packed.size() + chunk - 1) / chunk, nm = ((int64_t)g->nmask.size() + chunk - 1) / chunk;
    vg_parallel_for(np + nm, s.T, [&](int64_t c) {
        std::vector<uint32_t, no_init_alloc<uint32_t>>& v = c < np ? g->packed : g->nmask;
        const int64_t lo = (c < np ? c : c - np) * chunk, hi = std::min<int64_t>(lo + chunk, (int64_t)v.size());
#ifdef MADV_POPULATE_WRITE
        {   // fresh anonymous memory: populate the chunk's whole pages in one call (they come zeroed) instead of faulting page by page
            const uintptr_t a = ((uintptr_t)(v.data() + lo) + 4095) & ~(uintptr_t)4095, b = (uintptr_t)(v.data() + hi) & ~(uintptr_t)4095;
            if (b > a) (void)madvise((void*)a, (size_t)(b - a), MADV_POPULATE_WRITE);
        }
#endif
        memset(v.data() + lo, 0, (size_t)(hi - lo) * sizeof(uint32_t));
    });
}

// Stretches of genomes, the unit of the overlapped upload: the first genome of every stretch, then the genome count.  A stretch is
// closed by the genome that fills it, and never starts behind the last genome.
int64_t stretch_bases() {      // 128 M bases (= 32 MB packed + 16 MB mask); developer switch VG_INGEST_STRETCH_BASES, at least 64
    static const int64_t bases = [] { const char* e = vg_dev_getenv("VG_INGEST_STRETCH_BASES"); const long long v = e ? atoll(e) : 0; return v >= 64 ? (int64_t)v : (int64_t)(128LL << 20); }();
    return bases;
}
std::vector<int64_t> cut_stretches(const std::vector<int64_t>& base_off, int64_t want) {
    const int64_t n_g = (int64_t)base_off.size() - 1;
    std::vector<int64_t> first{ 0 };
    for (int64_t gi = 0; gi + 1 < n_g; ++gi) if (base_off[(size_t)gi + 1] - base_off[(size_t)first.back()] >= want) first.push_back(gi + 1);
    first.push_back(n_g); return first;
}
// The upload pipe: the packed arrays travel to the HBM of the library's device WHILE the genomes are packed.  A helper thread with a
// stream of its own uploads every stretch of genomes as soon as its last genome is done.  The pipe owns that thread and everything
// it shares with the packing threads, which only push; the thread reads the set's host arrays and layout and writes d_packed / d_nmask.
class upload_pipe {
    struct item { int64_t stretch; bool with_mask; };
    std::thread th; std::mutex mu; std::condition_variable cv; std::vector<item> queue; bool closed = false; std::string err;
    void run(vg_genomes* g, const std::vector<int64_t>& first) {
        try {
            vg_require_device();
            hipStream_t st; VG_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            for (;;) {
                item it;
                { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !queue.empty() || closed; }); if (queue.empty()) break; it = queue.back(); queue.pop_back(); }      // (the newest first)
                const int64_t b0 = g->base_off[(size_t)first[(size_t)it.stretch]], b1 = g->base_off[(size_t)first[(size_t)it.stretch + 1]];      // multiples of 64 bases
                VG_HIP(hipMemcpyAsync(g->d_packed.p + b0 / 16, g->packed.data() + b0 / 16, (size_t)(b1 - b0) / 16 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                if (it.with_mask) VG_HIP(hipMemcpyAsync(g->d_nmask.p + b0 / 32, g->nmask.data() + b0 / 32, (size_t)(b1 - b0) / 32 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                VG_HIP(hipStreamSynchronize(st));
            }
            (void)hipStreamDestroy(st);
        } catch (const std::exception& e) { std::lock_guard<std::mutex> lk(mu); err = e.what(); }
    }
    void shut() { if (!th.joinable()) return; { std::lock_guard<std::mutex> lk(mu); closed = true; } cv.notify_all(); th.join(); }
public:
    // the device arrays of g (with the slack vg_genomes_finish adds) and the thread; `stretches` (cut_stretches) outlives the pipe
    void open(vg_genomes* g, const std::vector<int64_t>& stretches) {
        vg_require_device();
        g->d_packed.alloc((size_t)(g->padded_total() / 16) + 16); g->d_nmask.alloc((size_t)(g->padded_total() / 32) + 16);
        th = std::thread([this, g, &stretches] { run(g, stretches); });
    }
    // a stretch whose genomes are all packed; with_mask: one of them holds an N, so its mask travels too
    void push(int64_t stretch, bool with_mask) { { std::lock_guard<std::mutex> lk(mu); queue.push_back({ stretch, with_mask }); } cv.notify_one(); }
    // every pushed stretch is on the device (the thread's stream has been drained), or the thread's error is thrown
    void close() { shut(); if (!err.empty()) throw vg_error(VG_EHIP, "upload of the genome arrays failed: " + err); }
    ~upload_pipe() { shut(); }
};

// parallel packing straight into the 2-bit arrays; the thread that completes a stretch hands it to the pipe (if any) and drops its text
void pack_genomes(ingest& s, const std::vector<int64_t>& st_first, upload_pipe* pipe) {
    vg_genomes* g = s.g.get(); const std::vector<gdesc>& gd = s.gd; std::vector<filebuf>& bufs = s.in->bufs; const std::vector<std::vector<record>>& recs = s.in->recs;
    // per stretch: the genomes still to pack, and whether one of them holds an N (its mask travels)
    struct stretch_state { std::atomic<int64_t> left; std::atomic<int> has_n; };
    const int64_t n_st = (int64_t)st_first.size() - 1;
    std::unique_ptr<stretch_state[]> st(new stretch_state[(size_t)n_st]);
    for (int64_t c = 0; c < n_st; ++c) { st[(size_t)c].left.store(st_first[(size_t)c + 1] - st_first[(size_t)c]); st[(size_t)c].has_n.store(0); }
    vg_parallel_for((int64_t)gd.size(), s.T, [&](int64_t gi) {
        const gdesc& d = gd[(size_t)gi];
        int64_t at = g->base_off[(size_t)gi]; bool any_n = false;
        for (size_t r = d.r0; r < d.r1; ++r) {
            if (r > d.r0) { g->nmask[(size_t)(at >> 5)] |= 1u << (at & 31); ++at; any_n = true; }   // joining N
            int64_t n_sym = 0;
            any_n |= pack_record(recs[(size_t)d.file][r], g, at, &n_sym);
            at += n_sym;
        }
        g->len[(size_t)gi] = at - g->base_off[(size_t)gi];
        {   // padding up to the next genome: single bits up to a word boundary, then whole words
            int64_t i = at; const int64_t e = g->base_off[(size_t)gi + 1];
            for (; i < e && (i & 31); ++i) g->nmask[(size_t)(i >> 5)] |= 1u << (i & 31);
            for (; i + 32 <= e; i += 32) g->nmask[(size_t)(i >> 5)] = 0xffffffffu;
            for (; i < e; ++i) g->nmask[(size_t)(i >> 5)] |= 1u << (i & 31);
        }
        g->has_n[(size_t)gi] = any_n ? 1 : 0;
        const int64_t c = std::upper_bound(st_first.begin(), st_first.end(), gi) - st_first.begin() - 1;      // the genome's stretch
        if (any_n) st[(size_t)c].has_n.store(1);
        if (st[(size_t)c].left.fetch_sub(1) != 1) return;
        // the last genome of its stretch: the stretch can travel, and nobody reads its text again
        if (pipe) pipe->push(c, st[(size_t)c].has_n.load() != 0);
        if (s.multi) {
            const gdesc& d0 = gd[(size_t)st_first[(size_t)c]]; const gdesc& d1 = gd[(size_t)st_first[(size_t)c + 1] - 1];
            if (d0.file == d1.file) bufs[(size_t)d0.file].drop(recs[(size_t)d0.file][d0.r0].hdr - 1, recs[(size_t)d1.file][d1.r1 - 1].end);
        }
    });
}

// what the pipe did not carry: the slack words behind the last genome, the small arrays, the masks of the genomes without N
void finish_resident(vg_genomes* g) {
    int dev = 0; VG_HIP(hipGetDevice(&dev)); hipStream_t s = vg_stream();
    const size_t pk_tail = (size_t)(g->padded_total() / 16), mk_tail = (size_t)(g->padded_total() / 32);
    VG_HIP(hipMemcpyAsync(g->d_packed.p + pk_tail, g->packed.data() + pk_tail, (g->packed.size() - pk_tail) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    VG_HIP(hipMemcpyAsync(g->d_nmask.p + mk_tail, g->nmask.data() + mk_tail, (g->nmask.size() - mk_tail) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    upload_tables(g, s);
    // the masks that did not travel (the pipe's stream has been drained: its copies are in place)
    hipLaunchKernelGGL(k_mask_of_lengths, dim3(4096), dim3(256), 0, s, g->d_nmask.p, (int64_t)mk_tail, (const uint32_t*)g->d_blk2g.p, g->align_shift,
                       (const int64_t*)g->d_base_off.p, (const int64_t*)g->d_len.p, (const uint8_t*)g->d_has_n.p);
    VG_HIP(hipStreamSynchronize(s));
    g->device = dev;
}

void load_genomes(const load_request& rq, vg_genomes** out, int* n_db_genomes = nullptr) {
    if (!rq.paths || rq.n_paths <= 0 || !out) throw vg_error(VG_EINVAL, "vg_genomes_load: bad arguments");
    ingest s(rq);
    vg_host_mark("ingest: enter");
    read_files(rq.paths, rq.n_paths, s.T, s.in->bufs);
    vg_host_mark("ingest: files mapped");
    plan_genomes(s);
    vg_host_mark("ingest: records found");
    lay_out(s, n_db_genomes);
    vg_host_mark("ingest: layout");
    clear_arrays(s);
    vg_host_mark("ingest: arrays cleared");
    const std::vector<int64_t> stretches = cut_stretches(s.g->base_off, stretch_bases());
    const bool resident = rq.resident && s.g->n > 0;
    upload_pipe pipe;                                       // (behind s: the thread is joined before the set and the text can go)
    if (resident) pipe.open(s.g.get(), stretches);
    pack_genomes(s, stretches, resident ? &pipe : nullptr);
    vg_genomes_finish(s.g.get());
    vg_host_mark("ingest: packed");
    if (resident) { pipe.close(); finish_resident(s.g.get()); vg_host_mark("ingest: resident"); }
    *out = s.g.release();
}

// database files then new files as one path list for the loader; multi-FASTA mode wants exactly one file on each side
void load_db_new(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, int multisample, int n_threads, bool resident,
                 vg_genomes** out, int* n_db_genomes) {
    if (!db_paths || !new_paths || n_db <= 0 || n_new <= 0 || !out || !n_db_genomes) throw vg_error(VG_EINVAL, "vg_genomes_load_db_new: bad arguments");
    if (multisample && (n_db != 1 || n_new != 1)) throw vg_error(VG_EINVAL, "vg_genomes_load_db_new: multi-FASTA mode takes one database file and one file of new genomes");
    std::vector<const char*> all(db_paths, db_paths + n_db); all.insert(all.end(), new_paths, new_paths + n_new);
    load_genomes({ all.data(), (int)all.size(), multisample, n_threads, resident, n_db }, out, n_db_genomes);
}
}  // namespace

// the four entries: host set or resident set (internal, vg_api.cpp: the upload overlapped), one list of files or database + new
extern "C" int vg_genomes_load(const char* const* paths, int n_paths, int multisample, int n_threads, vg_genomes** out) {
    VG_API_BEGIN load_genomes({ paths, n_paths, multisample, n_threads, false, -1 }, out); VG_API_END
}
int vg_genomes_load_resident(const char* const* paths, int n_paths, int multisample, int n_threads, vg_genomes** out) {
    VG_API_BEGIN load_genomes({ paths, n_paths, multisample, n_threads, true, -1 }, out); VG_API_END
}
extern "C" int vg_genomes_load_db_new(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, int multisample,
                                      int n_threads, vg_genomes** out, int* n_db_genomes) {
    VG_API_BEGIN load_db_new(db_paths, n_db, new_paths, n_new, multisample, n_threads, false, out, n_db_genomes); VG_API_END
}
int vg_genomes_load_db_new_resident(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, int multisample,
                                    int n_threads, vg_genomes** out, int* n_db_genomes) {
    VG_API_BEGIN load_db_new(db_paths, n_db, new_paths, n_new, multisample, n_threads, true, out, n_db_genomes); VG_API_END
}

extern "C" int vg_genomes_from_codes(const uint8_t* codes, const int64_t* offsets, int n_genomes,
                                     const char* const* names, vg_genomes** out) {
    VG_API_BEGIN
    if (!codes || !offsets || n_genomes < 0 || !out) throw vg_error(VG_EINVAL, "vg_genomes_from_codes: bad arguments");
    vg_genomes* g = new vg_genomes();
    g->align_shift = vg_choose_align_shift(n_genomes > 0 ? offsets[n_genomes] - offsets[0] : 0, n_genomes);
    for (int i = 0; i < n_genomes; ++i) {
        std::string nm = names && names[i] ? names[i] : ("g" + std::to_string(i));
        vg_genomes_append(g, nm, codes + offsets[i], offsets[i + 1] - offsets[i], 1);
    }
    vg_genomes_finish(g);
    *out = g;
    VG_API_END
}

extern "C" void vg_genomes_free(vg_genomes* g) { if (g) vg_lz_drop_prepared(g); delete g; }
extern "C" int vg_genomes_count(const vg_genomes* g) { return g ? g->n : 0; }
extern "C" int64_t vg_genomes_total_len(const vg_genomes* g) {
    int64_t t = 0; if (g) for (auto l : g->len) t += l; return t;
}
extern "C" int vg_genomes_lengths(const vg_genomes* g, int64_t* out) {
    if (!g || !out) return VG_EINVAL;
    for (int i = 0; i < g->n; ++i) out[i] = g->len[i];
    return VG_OK;
}
extern "C" const char* vg_genomes_name(const vg_genomes* g, int idx) {
    if (!g || idx < 0 || idx >= g->n) return "";
    return g->names[idx].c_str();
}

extern "C" int vg_genomes_codes(const vg_genomes* g, int idx, uint8_t* out) {
    if (!g || !out || idx < 0 || idx >= g->n) return VG_EINVAL;
    VG_API_BEGIN
    const int64_t p0 = g->base_off[(size_t)idx], len = g->len[(size_t)idx];
    // a subset gathered on the device has no host copy: the words of this genome are downloaded (genomes start at multiples of 64 bases)
    std::vector<uint32_t> pk, mk;
    if (g->device_only && len > 0) {
        vg_require_device();
        pk.resize((size_t)((len + 15) / 16)); mk.resize((size_t)((len + 31) / 32));
        VG_HIP(hipMemcpy(pk.data(), g->d_packed.p + p0 / 16, pk.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        VG_HIP(hipMemcpy(mk.data(), g->d_nmask.p + p0 / 32, mk.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    const uint32_t* packed = g->device_only ? pk.data() : g->packed.data();
    const uint32_t* nmask = g->device_only ? mk.data() : g->nmask.data();
    for (int64_t j = 0; j < len; ++j) {
        const int64_t p = g->device_only ? j : p0 + j;
        const bool n = (nmask[(size_t)(p >> 5)] >> (p & 31)) & 1u;
        out[j] = n ? 4 : (uint8_t)((packed[(size_t)(p >> 4)] >> (2 * (p & 15))) & 3u);
    }
    VG_API_END
}

extern "C" int vg_genomes_to_device(vg_genomes* g) {
    VG_API_BEGIN
    if (!g) throw vg_error(VG_EINVAL, "null genome set");
    vg_require_device();
    int dev = 0; VG_HIP(hipGetDevice(&dev));
    if (g->device == dev) return VG_OK;
    if (g->device_only) throw vg_error(VG_EINVAL, "a subset lives on the device it was gathered on (device " + std::to_string(g->device) + "): it has no host copy to upload to another");
    if (g->device >= 0) {
        // resident on another device: the allocator knows every block's device and returns these to THAT device's
        // driver instead of caching them here (vg_dev_free)
        g->d_packed.release(); g->d_planes.release(); g->d_nmask.release(); g->d_base_off.release(); g->d_len.release(); g->d_has_n.release(); g->d_blk2g.release();
        g->device = -1;
    }
    hipStream_t s = vg_stream();
    g->d_packed.alloc(g->packed.size()); g->d_packed.upload(g->packed.data(), g->packed.size(), s);
    g->d_nmask.alloc(g->nmask.size());   g->d_nmask.upload(g->nmask.data(), g->nmask.size(), s);
    upload_tables(g, s);
    VG_HIP(hipStreamSynchronize(s));
    g->device = dev;
    vg_host_mark("genomes uploaded");
    VG_API_END
}

// the deduplicate stage's input (vg_dedup.hip): every file whole in memory, every record in file order
void vg_fasta_read(const char* const* paths, int n_paths, int n_threads, vg_fasta_text& out) {
    const int T = std::max(1, n_threads);
    auto bufs = std::make_shared<std::vector<filebuf>>();
    out.bufs = bufs; read_files(paths, n_paths, T, *bufs);
    out.file_data.clear(); out.file_len.clear(); out.recs.clear();
    std::vector<record> rv;
    for (int i = 0; i < n_paths; ++i) {
        const filebuf& fb = (*bufs)[(size_t)i];
        out.file_data.push_back(fb.data()); out.file_len.push_back(fb.size());
        rv.clear();
        find_records(fb, rv, T);
        for (const record& r : rv) out.recs.push_back({ r.hdr, r.hdr_end, r.seq, r.end, i });
    }
}
