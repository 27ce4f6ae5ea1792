// vg_dedup.hip — the deduplicate stage on the GPU (in place of mfasta-tool, cmd_mfasta_deduplicate, vclust.py:810-866).
// DESIGN.md section 10 states the contract and the design.
//   pack      host threads, one record at a time: every symbol -> 4 bits, its set of bases (A=1 C=2 G=4 T=8, '-'=0), eight
//             per uint32 word, records starting on 4-word boundaries; the alphabet is checked in the same pass; stretches of
//             records travel to the HBM while later ones are packed
//   hash      one wave per (record, chunk of HASH_CHUNK words): 16-byte loads, a 128-bit sum of mixed (word index, word) terms
//             of the forward strand and of the reverse complement (complement = bit reversal of a nibble, so
//             v_bfrev_b32 of an 8-symbol word is its reverse complement; v_alignbit_b32 re-frames the words when the length
//             is not a multiple of 8); the sums are added with 64-bit atomics, so the result does not depend on the order
//   sort      key (length, min(fw, rc)): LSD radix passes (rocPRIM) over the two hash halves and the length; the
//             orientation bit says which strand gave the minimum
//   verify    rounds over the unresolved records in key order: the earliest record of every run of equal keys is the
//             candidate head, every other member is compared in full with it (one wave per (member, chunk)) in the
//             orientation the two bits imply; members that differ (hash collisions) stay for the next round
//   labels    representative (int32) and strand (int8) per record, the only arrays that come back
// Circular mode (vg_dedup_options.circular): duplicates up to rotation and strand.
//   chash     one wave per (record, chunk): every cyclic window of 16 symbols is one 64-bit value, its reverse complement the
//             bit reversal of it; mixed terms of min(window, reverse complement) are summed, so the 128-bit sum depends
//             neither on where the circle was opened nor on the strand
//   ccand     per (member, chunk): the positions of the head's strands whose window equals the member's first window are
//             the candidate offsets (code = strand, offset) of the candidate list below
//   cverify   the list's compare with the functor rotation_words: the member against the head rotated by the candidate
//             (v_alignbit_b32 re-frames by offset mod 8, the word index wraps); the smallest equal (strand, offset) is the answer
// Terminal repeats (vg_deduplicate_circular_tr): an exact repeat of the record's first t >= m symbols at its end is taken off
// before the circular mode runs.
//   tcand     one wave per (record, chunk): the starts u in the record's second half whose min(16, m) symbols equal the
//             record's first ones are the candidates (code = u) of the candidate list below
//   compare   the list's compare with the functor repeat_words: the prefix against the symbols from u (v_alignbit_b32
//             re-frames by u mod 8); the smallest equal u is the largest repeat
//   trim      the effective length L - t per record; the symbols behind it become zero in the device copy of the words
// The candidate list, one engine for both: an owner (a member's sort position; a record) has candidates (owner, code).
//   collect   the mode's candidate kernel hands out slots through put_candidates: a wave's ballot, one atomic on the list's
//             total and one on the owner's counter; what lies past the list's end is counted and not written, and the host
//             then grows the list to the count and runs the pass again
//   order     two radix sorts: by code, then (stable) by owner; a scan of the counters gives every owner's segment
//   verify    batches of 1, 2, 4, ... candidates per owner still without a result, in increasing code: k_batch counts the
//             tasks, k_compare<functor> runs one wave per (owner, candidate, chunk) -- a mismatch sets the candidate's flag,
//             a set flag ends its other chunks early -- and k_pick takes the atomicMin of the codes without a flag
// Contained mode (vg_deduplicate_contained): a record that is a substring of a longer record, or of its reverse complement,
// is removed as well.
//   windows   one thread per symbol position of a pass: the 16 symbols from it as one 64-bit key, the first symbol in the
//             top bits (the bit reversal of the packed window, so a symbol's code is its complement's: still one code per symbol)
//   sort      rocPRIM radix sort of (key, position)
//   lookup    per (record, strand): the anchor (the first min(anchor, L) symbols of X or of revcomp(X)) is a key range of
//             the sorted windows, found by two binary searches; the hits are cut into slices, and a hit in a longer record
//             that leaves room for the whole record (or at 0 in an earlier record of the same length) is a candidate
//   verify    one wave per (candidate, chunk): X, or revcomp(X) made by v_bfrev_b32, against the container re-framed by
//             v_alignbit_b32; a mismatch sets the candidate's flag (32-bit atomic) and ends its other chunks early
//   pick      64-bit atomicMax per record of (container's rank by length and index, strand, offset) over the equal candidates
// The host side of a call, in call order: the entry point's own checks, check_seq_arrays and pack_seqs (array-level calls) or the
// reader and pack_and_upload (files); run_mode, the one dispatch: contained_device, or repeats_device (with a minimum repeat) and
// then dedup_device on the circles' lengths, then the counts.  dedup_device: record_table (first word, symbols, first task per
// record), hash and keys by mode, sort_by_key, then the loop over the unresolved records -- the mode's round (plain_round or
// circular_round: run_heads, the compare, the labels), the number of members that differ, the compaction -- and the download.
// What both modes' rounds use is round_bufs; plain_state and circular_state are allocated by their mode alone.
// contained_device: plan_contained (positions, key bits, length order, positions per pass: before anything is allocated), then a
// contained_run: index_pass per pass, verify_slice per 2^20 hits, and contained_labels decodes the keys on the host.  A count
// kernel, its exclusive scan and the read-back of the total are scan_total wherever they occur.
#include "vg_common.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <sys/stat.h>

namespace {
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int64_t HASH_CHUNK = 2048;        // words (16 Ki symbols) per hash task: 8 trips of 64 lanes x 16 bytes
constexpr int64_t VERIFY_CHUNK = 2048;      // words per verification task
constexpr int64_t STRETCH_WORDS = 8 << 20;  // 32 MiB of packed symbols: the unit of the overlapped upload

std::atomic<int> g_hash_bits(128);
std::atomic<int> g_anchor_symbols(16);      // contained mode: symbols of an anchor (test knob)
std::atomic<int64_t> g_index_positions(0);  // contained mode: container positions indexed per pass, 0 = from the free HBM (test knob)
constexpr int64_t CAND_SLICE = 1 << 20;     // contained mode: anchor hits per candidate launch (the candidate queue's size)
constexpr int64_t INDEX_BYTES = 48;         // contained mode: HBM per indexed position (key, value, the sort's second pair and scratch)
constexpr int64_t MAX_PASS_POSITIONS = 1LL << 30;

// ---------------------------------------------------------------- host: packing
// byte -> 4-bit set of bases; 0x10 = white space (skipped), 0x20 = not in the alphabet
struct nib_lut {
    uint8_t t[256];
    nib_lut() {
        for (int i = 0; i < 256; ++i) t[i] = 0x20;
        t[(int)' '] = t[(int)'\t'] = t[(int)'\r'] = t[(int)'\n'] = 0x10;
        const char* sym = "-ACMGRSVTWYHKDBN";          // index = the set of bases (A=1, C=2, G=4, T=8)
        for (int v = 0; v < 16; ++v) { t[(unsigned char)sym[v]] = (uint8_t)v; t[(unsigned char)(sym[v] | 0x20)] = (uint8_t)v; }
    }
};
const nib_lut NLUT;

// The symbols of [q, end) into out[0 ..], eight per word, the first in the low bits; the words up to out_end are written
// (the last symbol word with zero nibbles behind the sequence, then zero words).  Eight bytes per trip while they are all
// symbols; line ends and anything unusual go byte by byte.  Returns the first byte outside the alphabet, or nullptr.
const char* pack_nibbles(const char* q, const char* end, uint32_t* out, uint32_t* out_end, int64_t* n_sym) {
    uint64_t acc = 0; int nb = 0; int64_t n = 0; uint32_t* o = out;
    while (q < end) {
        if (end - q >= 8) {
            uint32_t w = 0, f = 0;
            for (int j = 0; j < 8; ++j) { const uint32_t c = NLUT.t[(unsigned char)q[j]]; w |= (c & 15u) << (4 * j); f |= c; }
            if (f < 16) { acc |= (uint64_t)w << nb; *o++ = (uint32_t)acc; acc >>= 32; n += 8; q += 8; continue; }
        }
        const uint32_t c = NLUT.t[(unsigned char)*q];
        if (c & 0x20) { *n_sym = n; return q; }
        ++q;
        if (c & 0x10) continue;
        acc |= (uint64_t)c << nb; nb += 4; ++n;
        if (nb == 32) { *o++ = (uint32_t)acc; acc = 0; nb = 0; }
    }
    if (nb > 0) *o++ = (uint32_t)acc;
    while (o < out_end) *o++ = 0;
    *n_sym = n;
    return nullptr;
}

// the packed records, host and device
struct packed_set {
    int64_t n = 0;
    std::vector<int64_t> woff, len;                               // word offset (a multiple of 4) and symbols per record
    std::vector<uint32_t, no_init_alloc<uint32_t>> words;
    dbuf<uint32_t> d_words;
    int64_t bad_rec = -1; const char* bad_at = nullptr;          // the earliest record holding a byte outside the alphabet
};

// Packs seq[i] = [first, second) for every record.  The device copy is made while the packing goes on; when there is no
// device, or the upload fails, the packing still ends (a byte outside the alphabet is the error the caller reports first)
// and the device error is thrown after it.
void pack_and_upload(const std::vector<std::pair<const char*, const char*>>& seq, int n_threads, packed_set& ps) {
    const int64_t n = (int64_t)seq.size();
    ps.n = n;
    ps.woff.assign((size_t)n + 1, 0); ps.len.assign((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {           // an upper bound of the symbols: the bytes of the sequence lines
        const int64_t ub = (int64_t)(seq[(size_t)i].second - seq[(size_t)i].first);
        ps.woff[(size_t)i + 1] = ps.woff[(size_t)i] + ((ub + 31) >> 5 << 2);
    }
    const int64_t total = ps.woff[(size_t)n];
    ps.words.resize((size_t)total + 4);
    ps.words[(size_t)total] = ps.words[(size_t)total + 1] = ps.words[(size_t)total + 2] = ps.words[(size_t)total + 3] = 0;
    // stretches of records: the unit of the upload
    std::vector<int64_t> st_first{ 0 };
    for (int64_t i = 0; i < n; ++i)
        if (ps.woff[(size_t)i + 1] - ps.woff[(size_t)st_first.back()] >= STRETCH_WORDS && i + 1 < n) st_first.push_back(i + 1);
    st_first.push_back(n);
    const int64_t n_st = (int64_t)st_first.size() - 1;
    std::vector<int32_t> st_of((size_t)n);
    for (int64_t c = 0; c < n_st; ++c) for (int64_t i = st_first[(size_t)c]; i < st_first[(size_t)c + 1]; ++i) st_of[(size_t)i] = (int32_t)c;
    std::unique_ptr<std::atomic<int64_t>[]> st_left(new std::atomic<int64_t>[(size_t)std::max<int64_t>(n_st, 1)]);
    for (int64_t c = 0; c < n_st; ++c) st_left[(size_t)c].store(st_first[(size_t)c + 1] - st_first[(size_t)c]);

    std::mutex mu; std::condition_variable cv; std::vector<int64_t> queue; bool done = false;
    int dev_code = VG_OK; std::string dev_err;
    std::thread uploader([&]() {
        hipStream_t st = nullptr;
        try {
            vg_require_device();
            ps.d_words.alloc((size_t)total + 4);
            VG_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        } catch (const vg_error& e) { std::lock_guard<std::mutex> lk(mu); dev_code = e.code; dev_err = e.what(); }
        catch (const std::exception& e) { std::lock_guard<std::mutex> lk(mu); dev_code = VG_EHIP; dev_err = e.what(); }
        for (;;) {
            int64_t c;
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !queue.empty() || done; }); if (queue.empty()) break; c = queue.back(); queue.pop_back(); }
            if (dev_code != VG_OK) continue;          // (no device: the packing goes on, the error is reported after it)
            const int64_t w0 = ps.woff[(size_t)st_first[(size_t)c]], w1 = ps.woff[(size_t)st_first[(size_t)c + 1]];
            const hipError_t e = hipMemcpyAsync(ps.d_words.p + w0, ps.words.data() + w0, (size_t)(w1 - w0) * 4, hipMemcpyHostToDevice, st);
            const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
            if (e2 != hipSuccess) { std::lock_guard<std::mutex> lk(mu); dev_code = VG_EHIP; dev_err = std::string("upload of the packed records: ") + hipGetErrorString(e2); }
        }
        if (st) (void)hipStreamDestroy(st);
    });
    struct join_guard { std::thread& t; std::mutex& m; std::condition_variable& cv; bool& done;
                        ~join_guard() { { std::lock_guard<std::mutex> lk(m); done = true; } cv.notify_all(); if (t.joinable()) t.join(); } } jg{ uploader, mu, cv, done };
    std::vector<const char*> bad((size_t)n, nullptr);
    vg_parallel_for(n, n_threads, [&](int64_t i) {
        int64_t ns = 0;
        uint32_t* o = ps.words.data() + ps.woff[(size_t)i];
        bad[(size_t)i] = pack_nibbles(seq[(size_t)i].first, seq[(size_t)i].second, o, ps.words.data() + ps.woff[(size_t)i + 1], &ns);
        ps.len[(size_t)i] = ns;
        if (st_left[(size_t)st_of[(size_t)i]].fetch_sub(1) == 1) {
            { std::lock_guard<std::mutex> lk(mu); queue.push_back(st_of[(size_t)i]); }
            cv.notify_one();
        }
    });
    { std::lock_guard<std::mutex> lk(mu); done = true; }
    cv.notify_all(); uploader.join();
    vg_host_mark("dedup: packed");
    for (int64_t i = 0; i < n; ++i) if (bad[(size_t)i]) { ps.bad_rec = i; ps.bad_at = bad[(size_t)i]; break; }
    if (ps.bad_rec >= 0) return;
    if (dev_code != VG_OK) throw vg_error(dev_code, dev_err);
    if (n) {    // (the zero words behind the last record)
        hipStream_t s = vg_stream();
        VG_HIP(hipMemcpyAsync(ps.d_words.p + total, ps.words.data() + total, 16, hipMemcpyHostToDevice, s));
    }
}

std::string quote_byte(char ch) {
    char b[8];
    if ((unsigned char)ch >= 0x20 && (unsigned char)ch < 0x7f) snprintf(b, sizeof b, "%c", ch);
    else snprintf(b, sizeof b, "\\x%02x", (unsigned char)ch);
    return b;
}

// ---------------------------------------------------------------- device: hash
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}
// the term of symbol word x at word index w of a strand: two 64-bit sums
__device__ __forceinline__ void term(uint64_t w, uint32_t x, uint64_t& lo, uint64_t& hi) {
    const uint64_t a = fmix64(((w + 1) * 0x9e3779b97f4a7c15ull) ^ (uint64_t)x);
    lo += a;
    hi += (a ^ (a >> 29)) * 0xbf58476d1ce4e5b9ull;
}
// reverse-complement word of the 8 forward symbols starting at symbol 8k + r (hi = word k + 1, lo = word k)
__device__ __forceinline__ uint32_t rc_word(uint32_t hi, uint32_t lo, int r) {
    return __builtin_bitreverse32(__builtin_amdgcn_alignbit(hi, lo, (uint32_t)(4 * r)));
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    return v;
}
// the last i in [0, n) with beg[i] <= t (beg ascending, beg[0] = 0)
__device__ __forceinline__ int64_t owner_of(const int64_t* beg, int64_t n, int64_t t) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (beg[mid] <= t) lo = mid; else hi = mid; }
    return lo;
}

// Record i, L symbols, nw = ceil(L / 8) words, q = L / 8, r = L % 8.  Reverse-complement word w holds the complements of
// forward symbols L-1-8w down to L-8-8w, i.e. the forward window starting at 8k + r with k = q - 1 - w (k = -1 for the
// last one when r > 0: its missing symbols are zero, the complement of '-' padding, as in the forward strand's last word).
// A lane loads forward words j .. j+3 (16 bytes; records start on 4-word boundaries) and word j + 4 when it needs it.
__global__ void __launch_bounds__(TPB) k_hash(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                              const int64_t* __restrict__ cbeg, int64_t n, int64_t n_tasks, unsigned long long* h) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t i = owner_of(cbeg, n, t), c = t - cbeg[i];
        const int64_t L = len[i], nw = (L + 7) >> 3, q = L >> 3;
        const int r = (int)(L & 7);
        const uint32_t* R = W + woff[i];
        uint64_t flo = 0, fhi = 0, rlo = 0, rhi = 0;
        const int64_t j1 = min(nw, (c + 1) * HASH_CHUNK);
        for (int64_t j = c * HASH_CHUNK + 4 * lane; j < j1; j += 256) {
            const uint4 v = *(const uint4*)(R + j);
            const uint32_t x[5] = { v.x, v.y, v.z, v.w, (r && j + 4 <= q) ? R[j + 4] : 0u };
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t k = j + u;
                if (k < nw) term((uint64_t)k, x[u], flo, fhi);
                if (k < q) term((uint64_t)(q - 1 - k), rc_word(x[u + 1], x[u], r), rlo, rhi);
            }
            if (j == 0 && r) term((uint64_t)q, rc_word(x[0], 0u, r), rlo, rhi);
        }
        flo = wave_sum64(flo); fhi = wave_sum64(fhi); rlo = wave_sum64(rlo); rhi = wave_sum64(rhi);
        if (lane == 0) {
            atomicAdd(h + 4 * i, (unsigned long long)flo); atomicAdd(h + 4 * i + 1, (unsigned long long)fhi);
            atomicAdd(h + 4 * i + 2, (unsigned long long)rlo); atomicAdd(h + 4 * i + 3, (unsigned long long)rhi);
        }
    }
}

// key of record i: (length, min(fw, rc)) with the hash cut to its low `bits` bits; ori[i] = 1 when rc < fw
__global__ void k_keys(const unsigned long long* h, const int64_t* len, int64_t n, int bits, uint64_t* klo, uint64_t* khi,
                       uint64_t* klen, uint8_t* ori, int32_t* idx) {
    const uint64_t mlo = bits >= 64 ? ~0ull : (1ull << bits) - 1, mhi = bits >= 128 ? ~0ull : bits <= 64 ? 0ull : (1ull << (bits - 64)) - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t flo = h[4 * i], fhi = h[4 * i + 1], rlo = h[4 * i + 2], rhi = h[4 * i + 3];
        const bool o = rhi < fhi || (rhi == fhi && rlo < flo);
        klo[i] = (o ? rlo : flo) & mlo; khi[i] = (o ? rhi : fhi) & mhi; klen[i] = (uint64_t)len[i];
        ori[i] = o ? 1 : 0; idx[i] = (int32_t)i;
    }
}
__global__ void k_gather(const uint64_t* key, const int32_t* perm, int64_t n, uint64_t* out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) out[p] = key[perm[p]];
}

// ---------------------------------------------------------------- device: verification rounds
__device__ __forceinline__ bool same_key(const uint64_t* klo, const uint64_t* khi, const uint64_t* klen, int32_t a, int32_t b) {
    return klo[a] == klo[b] && khi[a] == khi[b] && klen[a] == klen[b];
}
// hp[p] = p at the start of a run of equal keys, else 0 (an inclusive max-scan then gives every position its run's head)
__global__ void k_runs(const int32_t* A, int64_t na, const uint64_t* klo, const uint64_t* khi, const uint64_t* klen, int64_t* hp) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < na; p += (int64_t)gridDim.x * blockDim.x)
        hp[p] = (p == 0 || !same_key(klo, khi, klen, A[p], A[p - 1])) ? p : 0;
}
// verification tasks per position: ceil(words / VERIFY_CHUNK) for a member, 0 for a head; cnt[na] = 0 (the total's slot)
__global__ void k_tasks(const int32_t* A, int64_t na, const int64_t* hp, const int64_t* len, int64_t* cnt, uint8_t* diff) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= na; p += (int64_t)gridDim.x * blockDim.x) {
        if (p == na) { cnt[p] = 0; continue; }
        const int64_t nw = (len[A[p]] + 7) >> 3;
        cnt[p] = hp[p] == p ? 0 : (nw + VERIFY_CHUNK - 1) / VERIFY_CHUNK;
        diff[p] = 0;
    }
}
// one wave per (member, chunk): the member's words against the head's, forward or reverse-complement as the orientation
// bits say (equal bits: the member equals the head itself; different bits: the head's reverse complement)
__global__ void __launch_bounds__(TPB) k_verify(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                                const uint8_t* __restrict__ ori, const int32_t* __restrict__ A, int64_t na,
                                                const int64_t* __restrict__ hp, const int64_t* __restrict__ tbeg, int64_t n_tasks, uint8_t* diff) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t p = owner_of(tbeg, na, t), c = t - tbeg[p];
        const int32_t m = A[p], hd = A[hp[p]];
        const int64_t L = len[m], nw = (L + 7) >> 3, q = L >> 3;
        const int r = (int)(L & 7);
        const uint32_t* M = W + woff[m]; const uint32_t* H = W + woff[hd];
        const bool fw = ori[m] == ori[hd];
        bool bad = false;
        for (int64_t k = c * VERIFY_CHUNK + lane, k1 = min(nw, (c + 1) * VERIFY_CHUNK); k < k1; k += 64) {
            uint32_t b;
            if (fw) b = H[k];
            else if (k < q) { const int64_t s = q - 1 - k; b = rc_word(r ? H[s + 1] : 0u, H[s], r); }
            else b = rc_word(H[0], 0u, r);                   // (k == q, r > 0)
            bad |= M[k] != b;
        }
        if (__ballot(bad) && lane == 0) diff[p] = 1;
    }
}
// heads keep themselves, equal members join their head, differing members stay (keep[p] = 1)
__global__ void k_resolve(const int32_t* A, int64_t na, const int64_t* hp, const uint8_t* diff, const uint8_t* ori,
                          int32_t* rep, int8_t* strand, int32_t* keep, unsigned long long* n_diff) {
    int c = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < na; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = A[p], hd = A[hp[p]];
        int32_t k = 0;
        if (hp[p] == p) { rep[i] = i; strand[i] = 0; }
        else if (!diff[p]) { rep[i] = hd; strand[i] = ori[i] != ori[hd] ? 1 : 0; }
        else { k = 1; ++c; }
        keep[p] = k;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_diff, (unsigned long long)c);
}
__global__ void k_compact(const int32_t* A, int64_t na, const int32_t* keep, const int32_t* at, int32_t* out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < na; p += (int64_t)gridDim.x * blockDim.x)
        if (keep[p]) out[at[p]] = A[p];
}

// ---------------------------------------------------------------- device: circular mode
__device__ __forceinline__ uint32_t sym_at(const uint32_t* R, int64_t pos) { return (R[pos >> 3] >> (4 * (int)(pos & 7))) & 15u; }
// n (<= 16) cyclic symbols of a record of L >= 1 symbols starting at b < L, one by one (the wrap point and short records)
__device__ __forceinline__ uint64_t gather(const uint32_t* R, int64_t L, int64_t b, int n) {
    uint64_t w = 0;
    for (int j = 0; j < n; ++j) { w |= (uint64_t)sym_at(R, b) << (4 * j); if (++b == L) b = 0; }
    return w;
}
// word k >= q of the record continued behind its end by its own start (q = L / 8, r = L % 8, L >= 16)
__device__ __forceinline__ uint32_t ext_word(const uint32_t* R, int64_t q, int r, int64_t k) {
    const int64_t m = k - q;
    if (r == 0) return R[m];
    if (m == 0) return R[q] | (R[0] << (4 * r));
    return __builtin_amdgcn_alignbit(R[m], R[m - 1], (uint32_t)(32 - 4 * r));
}
// f(valid, i, window) for every start i of chunk c of a record of L >= 1 symbols, window = the 16 cyclic symbols from i (the
// first in the low bits).  Every lane makes the same calls (f may hold ballots); valid says whether i < L.  A lane takes
// the 32 starts of its 16-byte load and needs the two words behind it; behind the record's end these are its first words,
// re-framed by L % 8.  Below 16 symbols a window wraps more than once: lane i gathers window i.
template <class F>
__device__ __forceinline__ void for_windows(const uint32_t* R, int64_t L, int64_t c, int lane, F&& f) {
    if (L < 16) {
        const bool valid = lane < L;
        f(valid, (int64_t)lane, valid ? gather(R, L, lane, 16) : 0ull);
        return;
    }
    const int64_t nw = (L + 7) >> 3, q = L >> 3;
    const int r = (int)(L & 7);
    for (int64_t base = c * HASH_CHUNK, j1 = min(nw, (c + 1) * HASH_CHUNK); base < j1; base += 256) {
        const int64_t j = base + 4 * lane;
        uint32_t x[6] = { 0u, 0u, 0u, 0u, 0u, 0u };
        if (j < nw) {
            const uint4 v = *(const uint4*)(R + j);
            const uint32_t own[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int64_t k = j + u;
                x[u] = k < q ? (u < 4 ? own[u & 3] : R[k]) : k <= nw + 1 ? ext_word(R, q, r, k) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int64_t i = 8 * (j + u) + t;
                const uint32_t lo = __builtin_amdgcn_alignbit(x[u + 1], x[u], (uint32_t)(4 * t));
                const uint32_t hi = __builtin_amdgcn_alignbit(x[u + 2], x[u + 1], (uint32_t)(4 * t));
                f(i < L, i, (uint64_t)lo | ((uint64_t)hi << 32));
            }
    }
}
// the reverse complement of a window of 16 symbols
__device__ __forceinline__ uint64_t rc_window(uint64_t w) { return __builtin_bitreverse64(w); }

// h[2 i], h[2 i + 1]: the sums of the two mixes of min(window, reverse complement) over all cyclic windows of record i
__global__ void __launch_bounds__(TPB) k_chash(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                               const int64_t* __restrict__ cbeg, int64_t n, int64_t n_tasks, unsigned long long* h) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t i = owner_of(cbeg, n, t), c = t - cbeg[i];
        const int64_t L = len[i];
        if (L == 0) continue;
        uint64_t lo = 0, hi = 0;
        for_windows(W + woff[i], L, c, lane, [&](bool valid, int64_t, uint64_t w) {
            const uint64_t rc = rc_window(w);
            const uint64_t a = fmix64((w < rc ? w : rc) ^ 0x9e3779b97f4a7c15ull);
            lo += valid ? a : 0ull;
            hi += valid ? (a ^ (a >> 29)) * 0xbf58476d1ce4e5b9ull : 0ull;
        });
        lo = wave_sum64(lo); hi = wave_sum64(hi);
        if (lane == 0) { atomicAdd(h + 2 * i, (unsigned long long)lo); atomicAdd(h + 2 * i + 1, (unsigned long long)hi); }
    }
}
// key of record i: (length, the sum cut to its low `bits` bits); no orientation
__global__ void k_ckeys(const unsigned long long* h, const int64_t* len, int64_t n, int bits, uint64_t* klo, uint64_t* khi,
                        uint64_t* klen, int32_t* idx) {
    const uint64_t mlo = bits >= 64 ? ~0ull : (1ull << bits) - 1, mhi = bits >= 128 ? ~0ull : bits <= 64 ? 0ull : (1ull << (bits - 64)) - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        klo[i] = h[2 * i] & mlo; khi[i] = h[2 * i + 1] & mhi; klen[i] = (uint64_t)len[i]; idx[i] = (int32_t)i;
    }
}
static_assert(HASH_CHUNK == VERIFY_CHUNK, "the candidate pass cuts a record as for_windows does");
__device__ __forceinline__ int64_t chunks_of(int64_t L) { return max((int64_t)1, (((L + 7) >> 3) + VERIFY_CHUNK - 1) / VERIFY_CHUNK); }

// ---------------------------------------------------------------- device: the candidate engine
// Circular mode and the terminal repeats share it.  An owner (a sort position p of a round; a record i of the repeat pass)
// has nch[owner] compare chunks (0: it takes no part), candidates (owner, code) in one list, and a result res[owner]: the
// smallest code whose compare finds no difference, NO_OFFSET while there is none.  A mode brings its candidate kernel
// (which windows are candidates) and its compare functor (which two words a lane XORs); everything else is below.
constexpr unsigned long long NO_OFFSET = ~0ull;
struct cand_slots { unsigned long long cap; uint64_t* owner; uint64_t* code; unsigned long long* ccnt; unsigned long long* total; };
// Slot hand-out, called by every lane of a wave with hits = __ballot(hit): lane 0 adds the hits to the list's total and to
// the owner's counter, every hit takes the next slot in lane order.  What lies past `cap` is counted and not written (the
// host grows the list and repeats the pass).
__device__ __forceinline__ void put_candidates(const cand_slots& to, uint64_t hits, bool hit, int64_t owner, uint64_t code, int lane) {
    if (!hits) return;
    unsigned long long at = 0;
    if (lane == 0) { at = atomicAdd(to.total, (unsigned long long)__popcll(hits)); atomicAdd(to.ccnt + owner, (unsigned long long)__popcll(hits)); }
    const unsigned long long slot = __shfl(at, 0) + (unsigned long long)__popcll(hits & ((1ull << lane) - 1));
    if (hit && slot < to.cap) { to.owner[slot] = (uint64_t)owner; to.code[slot] = code; }
}
// compare tasks of a batch per owner: (its candidates of rank lo .. hi - 1) x chunks; none for owners without chunks and for
// those that have their result; cnt[n_own] = 0 (the total's slot)
__global__ void k_batch(int64_t n_own, const int64_t* nch, const unsigned long long* res, const int64_t* ccnt, int64_t lo, int64_t hi,
                        int64_t* cnt) {
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o <= n_own; o += (int64_t)gridDim.x * blockDim.x) {
        if (o == n_own) { cnt[o] = 0; continue; }
        const bool open = nch[o] != 0 && res[o] == NO_OFFSET;
        cnt[o] = open ? max((int64_t)0, min(ccnt[o], hi) - lo) * nch[o] : 0;
    }
}
// the valid symbols of a compared word of which `left` symbols (>= 1) are left
__device__ __forceinline__ uint32_t word_mask(int64_t left) { return left >= 8 ? ~0u : (1u << (4 * left)) - 1; }
// One wave per (owner, candidate, chunk).  pair.of(owner, code) is the candidate's compare: nw words, and words(k, x, y,
// mask) gives the two words at k and the mask of their valid symbols.  A mismatch sets the candidate's flag; a set flag ends
// the other chunks of that candidate early.
template <class Pair>
__global__ void __launch_bounds__(TPB) k_compare(const Pair pair, const int64_t* __restrict__ nch, int64_t n_own, const int64_t* __restrict__ tbeg,
                                                 int64_t n_tasks, const int64_t* __restrict__ cbeg, int64_t lo,
                                                 const uint64_t* __restrict__ cand_code, uint8_t* bad) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t o = owner_of(tbeg, n_own, t), local = t - tbeg[o];
        const int64_t g = cbeg[o] + lo + local / nch[o], c = local % nch[o];
        if (bad[g]) continue;
        const auto cand = pair.of(o, cand_code[g]);
        bool diff = false;
        for (int64_t base = c * VERIFY_CHUNK, k1 = min(cand.nw, (c + 1) * VERIFY_CHUNK); base < k1; base += 64) {
            const int64_t k = base + lane;
            if (k < k1) {
                uint32_t x, y, mask;
                cand.words(k, x, y, mask);
                diff = ((x ^ y) & mask) != 0;
            }
            if (__ballot(diff)) break;
        }
        if (__ballot(diff) && lane == 0) bad[g] = 1;
    }
}
// the smallest code of the batch without a mismatch is the owner's result; count (may be null): count[0] += candidates of
// the batch, count[1] += the equal ones
__global__ void k_pick(const int64_t* nch, int64_t n_own, const int64_t* tbeg, int64_t n_tasks, const int64_t* cbeg, int64_t lo,
                       const uint64_t* cand_code, const uint8_t* bad, unsigned long long* res, unsigned long long* count) {
    int nc = 0, ne = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tasks; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = owner_of(tbeg, n_own, t), local = t - tbeg[o];
        if (local % nch[o]) continue;
        const int64_t g = cbeg[o] + lo + local / nch[o];
        ++nc;
        if (!bad[g]) { atomicMin(res + o, (unsigned long long)cand_code[g]); ++ne; }
    }
    if (!count) return;
    for (int o = 32; o > 0; o >>= 1) { nc += __shfl_xor(nc, o); ne += __shfl_xor(ne, o); }
    if ((threadIdx.x & 63) == 0 && nc) { atomicAdd(count, (unsigned long long)nc); atomicAdd(count + 1, (unsigned long long)ne); }
}

// ---------------------------------------------------------------- device: circular mode's candidates and compare
// owners of a round: nch[p] = the chunks of a member (one for an empty record), 0 for a head: its candidate tasks and the
// chunks of each compare; nch[na] = 0 (the total's slot); res[p] = no offset yet
__global__ void k_ctasks(const int32_t* A, int64_t na, const int64_t* hp, const int64_t* len, int64_t* nch, unsigned long long* res) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= na; p += (int64_t)gridDim.x * blockDim.x) {
        if (p == na) { nch[p] = 0; continue; }
        nch[p] = hp[p] == p ? 0 : chunks_of(len[A[p]]);
        res[p] = NO_OFFSET;
    }
}
// One wave per (member, chunk of the head).  removed == rot(Y, s) needs Y's window at s to equal the member's window at 0.
// Y = head: s = u for every u whose window equals it.  Y = revcomp(head): Y's window at s is the reverse complement of the
// head's window at (L - 16 - s) mod L, so s = (L - 16 - u) mod L for every u whose window equals the reverse complement of
// the member's.  Code of a candidate: strand << sbits | s.
__global__ void __launch_bounds__(TPB) k_ccand(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                               const int32_t* __restrict__ A, int64_t na, const int64_t* __restrict__ hp,
                                               const int64_t* __restrict__ tbeg, int64_t n_tasks, int sbits, const cand_slots to) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t p = owner_of(tbeg, na, t), c = t - tbeg[p];
        const int32_t m = A[p], hd = A[hp[p]];
        const int64_t L = len[m];
        const uint32_t* M = W + woff[m];
        if (L == 0) {          // (all empty records are equal: offset 0 on the forward strand)
            put_candidates(to, 1ull, lane == 0, p, 0ull, lane);
            continue;
        }
        const uint64_t m0 = L < 16 ? gather(M, L, 0, 16) : ((uint64_t)M[0] | ((uint64_t)M[1] << 32)), r0 = rc_window(m0);
        for_windows(W + woff[hd], L, c, lane, [&](bool valid, int64_t u, uint64_t w) {
            const bool mf = valid && w == m0, mr = valid && w == r0;
            const uint64_t bf = __ballot(mf), br = __ballot(mr);
            if (bf | br) {     // (one branch per window without a hit; a hand-out per strand inside it)
                put_candidates(to, bf, mf, p, (uint64_t)u, lane);
                put_candidates(to, br, mr, p, mr ? (1ull << sbits) | (uint64_t)((L - (16 + u) % L) % L) : 0ull, lane);
            }
        });
    }
}
// 8 cyclic symbols of a record from b < L: one re-framed pair of words, or symbol by symbol across the wrap point
__device__ __forceinline__ uint32_t cyc8(const uint32_t* R, int64_t L, int64_t b) {
    if (b + 8 <= L) { const int64_t w = b >> 3; return __builtin_amdgcn_alignbit(R[w + 1], R[w], (uint32_t)(4 * (b & 7))); }
    return (uint32_t)gather(R, L, b, 8);
}
// The compare of position p's member with Y rotated by s (code = strand << sbits | s): member word k against the 8 symbols
// of Y from (8 k + s) mod L; for Y = revcomp(head) these are the bit reversal of the head's 8 symbols from (L - 8 - pos) mod L.
struct rotation_words {
    const uint32_t* W; const int64_t* woff; const int64_t* len; const int32_t* A; const int64_t* hp; int sbits;
    struct cand {
        const uint32_t* M; const uint32_t* H; int64_t L, s, nw; bool rcs;
        __device__ __forceinline__ void words(int64_t k, uint32_t& x, uint32_t& y, uint32_t& mask) const {
            int64_t pos = 8 * k + s; if (pos >= L) pos -= L;
            if (rcs) { int64_t b = (L - 8 - pos) % L; if (b < 0) b += L; y = __builtin_bitreverse32(cyc8(H, L, b)); }
            else y = cyc8(H, L, pos);
            x = M[k]; mask = word_mask(L - 8 * k);
        }
    };
    __device__ __forceinline__ cand of(int64_t p, uint64_t code) const {
        const int32_t m = A[p];
        const int64_t L = len[m];
        return { W + woff[m], W + woff[A[hp[p]]], L, (int64_t)(code & ((1ull << sbits) - 1)), (L + 7) >> 3, (code >> sbits) != 0 };
    }
};
// heads keep themselves, members with an offset join their head, the others stay (keep[p] = 1)
__global__ void k_cresolve(const int32_t* A, int64_t na, const int64_t* hp, const unsigned long long* res, int sbits,
                           int32_t* rep, int8_t* strand, int64_t* off, int32_t* keep, unsigned long long* n_diff) {
    int c = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < na; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = A[p];
        int32_t k = 0;
        if (hp[p] == p) { rep[i] = i; strand[i] = 0; off[i] = 0; }
        else if (res[p] != NO_OFFSET) { rep[i] = A[hp[p]]; strand[i] = (int8_t)(res[p] >> sbits); off[i] = (int64_t)(res[p] & ((1ull << sbits) - 1)); }
        else { k = 1; ++c; }
        keep[p] = k;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_diff, (unsigned long long)c);
}

// ---------------------------------------------------------------- device: terminal repeats
// tr(X): the largest t in [m, L / 2] with X[0 : t) == X[u : L), u = L - t.  The starts u are ceil(L / 2) .. L - m.
__device__ __forceinline__ int64_t tr_first_start(int64_t L) { return L - (L >> 1); }
// owners of the pass: every record; a repeat has at most L / 2 symbols: the chunks of each compare; res[i] = no start yet
__global__ void k_ttasks(int64_t n, const int64_t* len, int64_t* nch, unsigned long long* res) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        nch[i] = chunks_of(len[i] >> 1);
        res[i] = NO_OFFSET;
    }
}
// One wave per (record, chunk).  X[0 : t) == X[u : L) needs the w = min(16, m) symbols from u to equal the record's first w
// symbols; u + w <= L, so the low w symbols of the window at u lie inside the record.  Every such u is a candidate; its code is u.
__global__ void __launch_bounds__(TPB) k_tcand(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                               const int64_t* __restrict__ cbeg, int64_t n, int64_t n_tasks, int64_t m, const cand_slots to) {
    const int lane = threadIdx.x & 63;
    const int w = (int)min((int64_t)16, m);
    const uint64_t wmask = w == 16 ? ~0ull : (1ull << (4 * w)) - 1;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t i = owner_of(cbeg, n, t), c = t - cbeg[i];
        const int64_t L = len[i], u0 = tr_first_start(L), u1 = L - m;         // (candidate starts u0 .. u1)
        if ((L >> 1) < m) continue;
        if (L >= 16 && (8 * (c + 1) * HASH_CHUNK <= u0 || 8 * c * HASH_CHUNK > u1)) continue;
        const uint32_t* R = W + woff[i];
        const uint64_t m0 = (L < 16 ? gather(R, L, 0, 16) : ((uint64_t)R[0] | ((uint64_t)R[1] << 32))) & wmask;
        for_windows(R, L, c, lane, [&](bool valid, int64_t u, uint64_t win) {
            const bool hit = valid && u >= u0 && u <= u1 && (win & wmask) == m0;
            put_candidates(to, __ballot(hit), hit, i, (uint64_t)u, lane);
        });
    }
}
// The compare of record i's prefix with its symbols from u (code = u): word k of the prefix against the 8 symbols from
// u + 8 k, two neighbouring words re-framed by u mod 8 symbols (the word behind the record's last is read and shifted out or
// masked: the packed buffer ends with zero words).  The last word is masked to t mod 8 symbols.
struct repeat_words {
    const uint32_t* W; const int64_t* woff; const int64_t* len;
    struct cand {
        const uint32_t* R; const uint32_t* S; int64_t tl, nw; uint32_t sh;
        __device__ __forceinline__ void words(int64_t k, uint32_t& x, uint32_t& y, uint32_t& mask) const {
            x = R[k]; y = __builtin_amdgcn_alignbit(S[k + 1], S[k], sh); mask = word_mask(tl - 8 * k);
        }
    };
    __device__ __forceinline__ cand of(int64_t i, uint64_t code) const {
        const int64_t u = (int64_t)code, tl = len[i] - u;
        const uint32_t* R = W + woff[i];
        return { R, R + (u >> 3), tl, (tl + 7) >> 3, (uint32_t)(4 * (u & 7)) };
    }
};
// repeat[i] = L - (the start found), 0 without one; eff[i] = L - repeat[i]
__global__ void k_trepeat(int64_t n, const int64_t* len, const unsigned long long* res, int64_t* repeat, int64_t* eff) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t L = len[i], t = res[i] == NO_OFFSET ? 0 : L - (int64_t)res[i];
        repeat[i] = t; eff[i] = L - t;
    }
}
// One wave per (record, chunk): every symbol at or past the effective length becomes zero in the record's words, so that the
// circle is padded as a packed record is (for_windows and ext_word rely on zero nibbles behind the end).
__global__ void __launch_bounds__(TPB) k_trim(uint32_t* W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                              const int64_t* __restrict__ eff, const int64_t* __restrict__ cbeg, int64_t n, int64_t n_tasks) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t i = owner_of(cbeg, n, t), c = t - cbeg[i];
        const int64_t L = len[i], E = eff[i], nw = (L + 7) >> 3, k0 = E >> 3;
        if (E == L) continue;
        uint32_t* R = W + woff[i];
        for (int64_t k = max(k0, c * HASH_CHUNK) + lane, k1 = min(nw, (c + 1) * HASH_CHUNK); k < k1; k += 64)
            R[k] = k == k0 ? R[k] & ((1u << (4 * (int)(E & 7))) - 1) : 0u;
    }
}

// ---------------------------------------------------------------- device: contained mode
// the 16 symbols of a record of L symbols from b < L, the first in the low bits; zero behind the record's end (three words
// are read: the packed buffer ends with four zero words)
__device__ __forceinline__ uint64_t window_at(const uint32_t* R, int64_t L, int64_t b) {
    const int64_t k = b >> 3;
    const uint32_t sh = (uint32_t)(4 * (b & 7)), x0 = R[k], x1 = R[k + 1], x2 = R[k + 2];
    const uint64_t w = (uint64_t)__builtin_amdgcn_alignbit(x1, x0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(x2, x1, sh) << 32);
    const int64_t nv = L - b;
    return nv >= 16 ? w : w & ((1ull << (4 * nv)) - 1);
}
// Index entry t of a pass: position pos0 + t of the concatenated records (pbeg = the records' first positions).  The key is
// the bit reversal of the window: symbol k of the window sits in nibble 15 - k as its complement's code, so keys that share
// their top 4 w bits are the windows that share their first w symbols.
__global__ void k_sub_windows(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                           const int64_t* __restrict__ pbeg, int64_t n, int64_t pos0, int64_t np, uint64_t* key, int64_t* val) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < np; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = pos0 + t, j = owner_of(pbeg, n, g);
        key[t] = __builtin_bitreverse64(window_at(W + woff[j], len[j], g - pbeg[j]));
        val[t] = g;
    }
}
// Query q = 2 i + strand: the sorted keys that start with the anchor, hlo[q] .. hlo[q] + hcnt[q] - 1.  Forward anchor: the
// first w = min(anchor, L) symbols of X.  Reverse anchor: the first w symbols of revcomp(X), whose key is X's last w symbols
// as they are packed, moved to the top bits (revcomp(X) lies in Y exactly when X lies in revcomp(Y)).  hcnt[2 n] = 0.
__global__ void k_sub_lookup(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len, int64_t n,
                          int anchor, const uint64_t* __restrict__ key, int64_t np, int64_t* hlo, int64_t* hcnt) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= 2 * n; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = q >> 1, L = q < 2 * n ? len[i] : 0;
        if (L == 0) { hlo[q] = 0; hcnt[q] = 0; continue; }
        const int w = (int)min((int64_t)anchor, L);
        const uint64_t rest = w == 16 ? 0ull : (1ull << (64 - 4 * w)) - 1;
        const uint32_t* R = W + woff[i];
        const uint64_t a = ((q & 1) ? window_at(R, L, L - w) << (64 - 4 * w) : __builtin_bitreverse64(window_at(R, L, 0))) & ~rest;
        int64_t lo = 0, hi = np;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] < a) lo = mid + 1; else hi = mid; }
        const int64_t first = lo;
        hi = np;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[mid] <= (a | rest)) lo = mid + 1; else hi = mid; }
        hlo[q] = first; hcnt[q] = lo - first;
    }
}
// Hits h0 .. h1 - 1 of the pass (hoff = the queries' first hits): hit (i, strand) at position s of record j is a candidate
// when j is longer and holds the whole record from s, or j is an earlier record of the same length and s = 0.  The queue has
// room for every hit of the slice.
__global__ void __launch_bounds__(TPB) k_sub_cands(const int64_t* __restrict__ len, const int64_t* __restrict__ pbeg, int64_t n,
                                                   const int64_t* __restrict__ hoff, const int64_t* __restrict__ hlo, const int64_t* __restrict__ val,
                                                   int64_t h0, int64_t h1, uint32_t* cq, int32_t* cj, int64_t* cs, unsigned long long* n_cand) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1;
    for (int64_t h = h0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;; h += (int64_t)gridDim.x * blockDim.x) {
        if (!__ballot(h < h1)) break;
        bool ok = false;
        int64_t q = 0, j = 0, s = 0;
        if (h < h1) {
            q = owner_of(hoff, 2 * n, h);
            const int64_t g = val[hlo[q] + (h - hoff[q])], i = q >> 1;
            j = owner_of(pbeg, n, g); s = g - pbeg[j];
            const int64_t Li = len[i], Lj = len[j];
            ok = (Lj > Li && s + Li <= Lj) || (Lj == Li && s == 0 && j < i);
        }
        const uint64_t b = __ballot(ok);
        if (!b) continue;
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(n_cand, (unsigned long long)__popcll(b));
        at = __shfl(at, 0) + (unsigned long long)__popcll(b & below);
        if (ok) { cq[at] = (uint32_t)q; cj[at] = (int32_t)j; cs[at] = s; }
    }
}
// verification tasks per candidate: the chunks of the record; bad[c] = 0; cnt[nc] = 0 (the total's slot)
__global__ void k_sub_tasks(const uint32_t* cq, int64_t nc, const int64_t* len, int64_t* cnt, uint32_t* bad) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= nc; c += (int64_t)gridDim.x * blockDim.x) {
        if (c == nc) { cnt[c] = 0; continue; }
        cnt[c] = chunks_of(len[cq[c] >> 1]);
        bad[c] = 0;
    }
}
// One wave per (candidate, chunk): word k of X (forward) or of revcomp(X) (reverse: only the record is reversed) against
// the 8 symbols of the container from s + 8 k, two neighbouring words re-framed by s mod 8 symbols.  The padding of the last
// word is masked.  A mismatch sets the candidate's flag; a set flag ends the candidate's other chunks early.
__global__ void __launch_bounds__(TPB) k_sub_verify(const uint32_t* __restrict__ W, const int64_t* __restrict__ woff, const int64_t* __restrict__ len,
                                                    const uint32_t* __restrict__ cq, const int32_t* __restrict__ cj, const int64_t* __restrict__ cs,
                                                    int64_t nc, const int64_t* __restrict__ tbeg, int64_t n_tasks, uint32_t* bad) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < n_tasks; t += (int64_t)gridDim.x * WAVES) {
        const int64_t c = owner_of(tbeg, nc, t), ch = t - tbeg[c];
        if (bad[c]) continue;
        const int64_t i = cq[c] >> 1, s = cs[c];
        const bool rcs = (cq[c] & 1u) != 0;
        const int64_t L = len[i], nw = (L + 7) >> 3, qd = L >> 3;
        const int r = (int)(L & 7);
        const uint32_t sh = (uint32_t)(4 * (s & 7));
        const uint32_t* M = W + woff[i]; const uint32_t* H = W + woff[cj[c]] + (s >> 3);
        bool diff = false;
        for (int64_t base = ch * VERIFY_CHUNK, k1 = min(nw, (ch + 1) * VERIFY_CHUNK); base < k1; base += 64) {
            const int64_t k = base + lane;
            if (k < k1) {
                uint32_t x;
                if (!rcs) x = M[k];
                else if (k < qd) { const int64_t f = qd - 1 - k; x = rc_word(r ? M[f + 1] : 0u, M[f], r); }
                else x = rc_word(M[0], 0u, r);                   // (k == qd, r > 0)
                const uint32_t y = __builtin_amdgcn_alignbit(H[k + 1], H[k], sh);
                const int64_t nv = min((int64_t)8, L - 8 * k);
                const uint32_t mask = nv == 8 ? ~0u : (1u << (4 * nv)) - 1;
                diff = ((x ^ y) & mask) != 0;
            }
            if (__ballot(diff)) break;
        }
        if (__ballot(diff) && lane == 0) atomicOr(bad + c, 1u);
    }
}
// best[i] = the largest key over the candidates without a flag: the container's rank from the end of the order (length
// descending, index ascending), then '+' before '-', then the smallest offset.  The offset of a reverse hit is counted in
// revcomp(container): revcomp(X) at s of Y is X at L_Y - L_X - s of revcomp(Y).  Keys are above 0 (an offset is below 2^sbits - 1).
__global__ void k_sub_pick(const int64_t* len, const int32_t* rnk, int64_t n, const uint32_t* cq, const int32_t* cj, const int64_t* cs, int64_t nc,
                        const uint32_t* bad, int sbits, unsigned long long* best, unsigned long long* n_equal) {
    int e = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
        if (bad[c]) continue;
        const int64_t i = cq[c] >> 1, j = cj[c];
        const uint64_t rcs = cq[c] & 1u, off = (uint64_t)(rcs ? len[j] - len[i] - cs[c] : cs[c]), m = (1ull << sbits) - 1;
        atomicMax(best + i, (unsigned long long)(((uint64_t)(n - 1 - rnk[j]) << (sbits + 1)) | ((rcs ^ 1u) << sbits) | (m - off)));
        ++e;
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    if ((threadIdx.x & 63) == 0 && e) atomicAdd(n_equal, (unsigned long long)e);
}

// ---------------------------------------------------------------- host: the device side of a call
enum dedup_mode { MODE_PLAIN, MODE_CIRCULAR, MODE_CONTAINED };
// blocks of a grid-stride launch with one item per thread, and with one task per wave
int blocks(int64_t n) { return grid_for(n, TPB, 16384); }
int wave_blocks(int64_t n) { return grid_for(n, WAVES, 65536); }

template <class K, class V>
void sort_pairs(dbuf<K>& keys, dbuf<K>& keys2, dbuf<V>& vals, dbuf<V>& vals2, int64_t n, unsigned bits, hipStream_t s) {
    with_temp_storage([&](void* tmp, size_t& tb) {
        return rocprim::radix_sort_pairs(tmp, tb, keys.p, keys2.p, vals.p, vals2.p, (size_t)n, 0u, bits, s); });
    std::swap(keys.p, keys2.p); std::swap(vals.p, vals2.p);
}
template <class T, class Op>
void scan(const T* in, T* out, int64_t n, bool inclusive, Op op, hipStream_t s) {
    with_temp_storage([&](void* tmp, size_t& tb) {
        return inclusive ? rocprim::inclusive_scan(tmp, tb, in, out, (size_t)n, op, s)
                         : rocprim::exclusive_scan(tmp, tb, in, out, (T)0, (size_t)n, op, s); });
}
// one counter of the device on the host: a copy and a synchronise
template <class T> T read_back(const T* at, hipStream_t s) {
    T v = 0;
    vg_download_bytes(&v, at, sizeof v, s);
    VG_HIP(hipStreamSynchronize(s));
    return v;
}
// beg[0 .. n] = the exclusive scan of the counts cnt[0 .. n) (slot n is only scanned over: beg[n] is the total) -> the total
int64_t scan_total(const int64_t* cnt, int64_t* beg, int64_t n, hipStream_t s) {
    scan(cnt, beg, n + 1, false, rocprim::plus<int64_t>(), s);
    return read_back(beg + n, s);
}
// the (record, chunk of HASH_CHUNK words) tasks of records of len[i] symbols: cbeg[i] = record i's first task (an empty record has one)
struct chunk_tasks { std::vector<int64_t> cbeg; int64_t n_tasks = 0, max_len = 0, total_words = 0; };
chunk_tasks chunk_tasks_of(const std::vector<int64_t>& len) {
    chunk_tasks ct;
    ct.cbeg.assign(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) {
        const int64_t nw = (len[i] + 7) >> 3;
        ct.cbeg[i + 1] = ct.cbeg[i] + std::max<int64_t>(1, (nw + HASH_CHUNK - 1) / HASH_CHUNK);
        ct.max_len = std::max(ct.max_len, len[i]); ct.total_words += nw;
    }
    ct.n_tasks = ct.cbeg.back();
    return ct;
}
// the per-record arrays of the packed set on the device: record i's first word, its symbols (ps.len, or the circles' lengths
// once the repeats are off) and beg[0 .. n]: its first hash task (cbeg) or its first index position (pbeg).  Three copies.
struct record_table {
    dbuf<int64_t> woff, len, beg;
    record_table(const packed_set& ps, const std::vector<int64_t>& len_, const std::vector<int64_t>& beg_, hipStream_t s)
        : woff((size_t)ps.n), len((size_t)ps.n), beg((size_t)ps.n + 1) {
        woff.upload(ps.woff.data(), (size_t)ps.n, s); len.upload(len_.data(), (size_t)ps.n, s); beg.upload(beg_.data(), (size_t)ps.n + 1, s);
    }
};

// the candidate engine's list: the candidates (owner, code) of every owner, sorted by (owner, code) once order() has run,
// and their flags
struct cand_list {
    dbuf<uint64_t> owner, code, owner2, code2;
    dbuf<uint8_t> bad;
    dbuf<int64_t> cnt, beg, nch;             // per owner (n + 1): its candidates, where they start, its compare chunks
    dbuf<unsigned long long> total;
    void alloc_owners(int64_t n) { cnt.alloc((size_t)n + 1); beg.alloc((size_t)n + 1); nch.alloc((size_t)n + 1); total.alloc(1); }
};
// Fills the list: produce(slots) launches the mode's candidate kernel over the n_own owners.  A list of cap0 slots (or the
// one it has, if larger) is tried first; when more candidates were counted than it holds, nothing of it is used: it grows to
// the count and the pass runs again.  -> the candidates
template <class F>
int64_t collect(cand_list& cl, int64_t n_own, size_t cap0, hipStream_t s, F produce) {
    unsigned long long n_cand = 0;
    for (size_t cap = cap0;; cap = (size_t)n_cand) {
        if (cl.owner.n < cap) { cl.owner.alloc(cap); cl.code.alloc(cap); cl.owner2.alloc(cap); cl.code2.alloc(cap); cl.bad.alloc(cap); }
        VG_HIP(hipMemsetAsync(cl.cnt.p, 0, (size_t)(n_own + 1) * sizeof(int64_t), s));
        cl.total.zero(s);
        produce(cand_slots{ (unsigned long long)cl.owner.n, cl.owner.p, cl.code.p, (unsigned long long*)cl.cnt.p, cl.total.p });
        n_cand = read_back(cl.total.p, s);
        if (n_cand <= cl.owner.n) return (int64_t)n_cand;
    }
}
// sorts the n_cand candidates by (owner, code), gives every owner its segment and clears the flags
void order(cand_list& cl, int64_t n_own, int64_t n_cand, unsigned code_bits, unsigned owner_bits, hipStream_t s) {
    sort_pairs(cl.code, cl.code2, cl.owner, cl.owner2, n_cand, code_bits, s);
    sort_pairs(cl.owner, cl.owner2, cl.code, cl.code2, n_cand, owner_bits, s);
    scan(cl.cnt.p, cl.beg.p, n_own + 1, false, rocprim::plus<int64_t>(), s);
    VG_HIP(hipMemsetAsync(cl.bad.p, 0, (size_t)n_cand, s));
}
// Compares the candidates of rank [lo, lo + width) of every owner still without a result; the width doubles, so the first
// batch with an equal candidate holds the owner's smallest equal code.  One read-back per batch.  cnt, tbeg: n_own + 1
// each; count: k_pick's counters, or null.  -> the batches launched
template <class Pair>
int64_t verify_batches(cand_list& cl, int64_t n_own, const Pair& pair, dbuf<int64_t>& cnt, dbuf<int64_t>& tbeg, unsigned long long* res,
                       unsigned long long* count, hipStream_t s) {
    for (int64_t batches = 0, lo = 0, width = 1;; ++batches, lo += width, width *= 2) {
        hipLaunchKernelGGL(k_batch, dim3(blocks(n_own + 1)), dim3(TPB), 0, s, n_own, cl.nch.p, res, cl.cnt.p, lo, lo + width, cnt.p);
        const int64_t n_vt = scan_total(cnt.p, tbeg.p, n_own, s);
        if (n_vt == 0) return batches;
        hipLaunchKernelGGL(k_compare<Pair>, dim3(wave_blocks(n_vt)), dim3(TPB), 0, s, pair, cl.nch.p, n_own, tbeg.p, n_vt, cl.beg.p, lo, cl.code.p, cl.bad.p);
        hipLaunchKernelGGL(k_pick, dim3(blocks(n_vt)), dim3(TPB), 0, s, cl.nch.p, n_own, tbeg.p, n_vt, cl.beg.p, lo, cl.code.p, cl.bad.p, res, count);
    }
}

// The terminal repeats of the packed records (resident): repeat_out[i] = tr(record i) for the minimum m >= 1.  Candidate
// starts in increasing order per record: the smallest equal start is the largest repeat.  trim: the device copy of every
// record is cut to its circle (symbols at or past L - tr become zero); the host copy stays.
void repeats_device(const packed_set& ps, int64_t m, int64_t* repeat_out, vg_dedup_repeat_stats& rst, bool trim) {
    const int64_t n = ps.n;
    if (n == 0) return;
    hipStream_t s = vg_stream();
    const chunk_tasks ct = chunk_tasks_of(ps.len);
    record_table rt(ps, ps.len, ct.cbeg, s);
    dbuf<int64_t> d_rep((size_t)n), d_eff((size_t)n);
    dbuf<unsigned long long> res((size_t)n), d_count(2);
    cand_list cl;
    cl.alloc_owners(n);
    hipLaunchKernelGGL(k_ttasks, dim3(blocks(n)), dim3(TPB), 0, s, n, rt.len.p, cl.nch.p, res.p);
    d_count.zero(s);
    {
        vg_prof_scope ps_("dedup_trepeat", (double)ct.total_words * 2.0);
        const int64_t n_cand = collect(cl, n, (size_t)(2 * n + 1024), s, [&](const cand_slots& to) {
            hipLaunchKernelGGL(k_tcand, dim3(wave_blocks(ct.n_tasks)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, rt.beg.p, n, ct.n_tasks, m, to); });
        if (n_cand > 0) {
            dbuf<int64_t> cnt((size_t)n + 1), tbeg((size_t)n + 1);
            order(cl, n, n_cand, bit_width((uint64_t)ct.max_len, 1), bit_width((uint64_t)n, 1), s);
            rst.batches += verify_batches(cl, n, repeat_words{ ps.d_words.p, rt.woff.p, rt.len.p }, cnt, tbeg, res.p, d_count.p, s);
        }
    }
    {
        vg_prof_scope ps_("dedup_trim", (double)n * 32.0);
        hipLaunchKernelGGL(k_trepeat, dim3(blocks(n)), dim3(TPB), 0, s, n, rt.len.p, res.p, d_rep.p, d_eff.p);
        if (trim)
            hipLaunchKernelGGL(k_trim, dim3(wave_blocks(ct.n_tasks)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, d_eff.p, rt.beg.p, n, ct.n_tasks);
    }
    unsigned long long count[2] = { 0, 0 };
    d_rep.download(repeat_out, (size_t)n, s);
    d_count.download(count, 2, s);
    VG_HIP(hipStreamSynchronize(s));
    rst.candidates = (int64_t)count[0]; rst.equal = (int64_t)count[1];
    for (int64_t i = 0; i < n; ++i) { rst.with_repeat += repeat_out[i] > 0; rst.repeat_symbols += repeat_out[i]; }
}

// What the rounds of the plain and the circular mode share, in the order it is allocated: the keys per record, the unresolved
// records A[0 .. na) in key order, the labels, the run heads hp per position, a count / scan pair, the members that differ.
struct round_bufs {
    dbuf<uint64_t> klo, khi, klen;
    dbuf<int32_t> A, A2, d_rep, keep, at;
    dbuf<int8_t> d_strand;
    dbuf<int64_t> hp, hp2, cnt, tbeg;
    dbuf<unsigned long long> d_ndiff;
    void alloc_keys(size_t n) { klo.alloc(n); khi.alloc(n); klen.alloc(n); A.alloc(n); A2.alloc(n); }
    void alloc_rounds(size_t n) {
        d_rep.alloc(n); keep.alloc(n); at.alloc(n); d_strand.alloc(n); hp.alloc(n); hp2.alloc(n); cnt.alloc(n + 1); tbeg.alloc(n + 1); d_ndiff.alloc(1);
    }
};
// each mode's own, allocated by that mode alone.  Plain: which strand gave a record's key; whether a member differs from its head.
// Circular: the bits of an offset (it is below the length), the offsets, a member's smallest equal (strand << sbits | offset), the list.
struct plain_state { dbuf<uint8_t> ori, diff; };
struct circular_state { int sbits = 1; dbuf<int64_t> d_off; dbuf<unsigned long long> res; cand_list cl; };

// the three stable passes over the keys (low hash half, high half, length): equal keys end up adjacent, in index order
void sort_by_key(round_bufs& r, int64_t n, int bits, unsigned len_bits, hipStream_t s) {
    vg_prof_scope ps_("dedup_sort", (double)n * 48.0);
    dbuf<uint64_t> kg((size_t)n), ks((size_t)n);
    const unsigned pass_bits[3] = { (unsigned)std::min(bits, 64), (unsigned)std::max(bits - 64, 0), len_bits };
    const uint64_t* src[3] = { r.klo.p, r.khi.p, r.klen.p };
    for (int pass = 0; pass < 3; ++pass) {
        if (!pass_bits[pass]) continue;
        hipLaunchKernelGGL(k_gather, dim3(blocks(n)), dim3(TPB), 0, s, src[pass], r.A.p, n, kg.p);
        sort_pairs(kg, ks, r.A, r.A2, n, pass_bits[pass], s);
    }
}
// hp[p] = the position of the head of p's run of equal keys among A[0 .. na): the start of either mode's dedup_runs scope
void run_heads(round_bufs& r, int64_t na, hipStream_t s) {
    hipLaunchKernelGGL(k_runs, dim3(blocks(na)), dim3(TPB), 0, s, r.A.p, na, r.klo.p, r.khi.p, r.klen.p, r.hp2.p);
    scan(r.hp2.p, r.hp.p, na, true, rocprim::maximum<int64_t>(), s);
}
// One round of the plain mode: every member against its head in the orientation the two bits imply; the members that differ are kept.
void plain_round(const packed_set& ps, const record_table& rt, round_bufs& r, plain_state& pl, int64_t na, hipStream_t s) {
    {
        vg_prof_scope ps_("dedup_runs", (double)na * 60.0);
        run_heads(r, na, s);
        hipLaunchKernelGGL(k_tasks, dim3(blocks(na + 1)), dim3(TPB), 0, s, r.A.p, na, r.hp.p, rt.len.p, r.cnt.p, pl.diff.p);
        scan(r.cnt.p, r.tbeg.p, na + 1, false, rocprim::plus<int64_t>(), s);
    }
    const int64_t n_vt = read_back(r.tbeg.p + na, s);        // (the element at na: the total; outside the scope, which times the group's kernels)
    if (n_vt > 0) {
        vg_prof_scope ps_("dedup_verify", (double)n_vt * VERIFY_CHUNK * 8.0);
        hipLaunchKernelGGL(k_verify, dim3(wave_blocks(n_vt)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, pl.ori.p, r.A.p, na, r.hp.p, r.tbeg.p, n_vt, pl.diff.p);
    }
    vg_prof_scope ps_("dedup_labels", (double)na * 24.0);
    hipLaunchKernelGGL(k_resolve, dim3(blocks(na)), dim3(TPB), 0, s, r.A.p, na, r.hp.p, pl.diff.p, pl.ori.p, r.d_rep.p, r.d_strand.p, r.keep.p, r.d_ndiff.p);
}
// One round of the circular mode: res[p] = strand << sbits | offset of every member equal to its head in some rotation of one of
// the head's strands, NO_OFFSET for the others, which are kept for the next round.  Candidates sorted by (position, strand, offset).
void circular_round(const packed_set& ps, const record_table& rt, round_bufs& r, circular_state& ci, int64_t na, hipStream_t s) {
    {
        vg_prof_scope ps_("dedup_runs", (double)na * 60.0);
        run_heads(r, na, s);
    }
    int64_t n_cand = 0;
    {
        vg_prof_scope ps_("dedup_ccand", (double)na * 16.0);
        hipLaunchKernelGGL(k_ctasks, dim3(blocks(na + 1)), dim3(TPB), 0, s, r.A.p, na, r.hp.p, rt.len.p, ci.cl.nch.p, ci.res.p);
        const int64_t n_ct = scan_total(ci.cl.nch.p, r.tbeg.p, na, s);        // (0: heads only)
        if (n_ct > 0) n_cand = collect(ci.cl, na, std::max(ci.cl.owner.n, (size_t)(4 * na + 1024)), s, [&](const cand_slots& to) {
            hipLaunchKernelGGL(k_ccand, dim3(wave_blocks(n_ct)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, r.A.p, na, r.hp.p, r.tbeg.p, n_ct, ci.sbits, to); });
        if (n_cand > 0) order(ci.cl, na, n_cand, (unsigned)ci.sbits + 1, bit_width((uint64_t)na, 1), s);
    }
    if (n_cand > 0) {
        vg_prof_scope ps_("dedup_cverify", 0.0);
        verify_batches(ci.cl, na, rotation_words{ ps.d_words.p, rt.woff.p, rt.len.p, r.A.p, r.hp.p, ci.sbits }, r.cnt, r.tbeg, ci.res.p, nullptr, s);
    }
    vg_prof_scope ps_("dedup_labels", (double)na * 32.0);
    hipLaunchKernelGGL(k_cresolve, dim3(blocks(na)), dim3(TPB), 0, s, r.A.p, na, r.hp.p, ci.res.p, ci.sbits, r.d_rep.p, r.d_strand.p, ci.d_off.p, r.keep.p, r.d_ndiff.p);
}

// The plain and the circular mode on the device: packed records (resident, of len[i] symbols each: the circles after repeats_device has
// trimmed them, else ps.len) -> representative / strand (circular: and offset) on the host.  Hash and keys by mode, one sort, the mode's rounds.
void dedup_device(const packed_set& ps, const std::vector<int64_t>& len, dedup_mode mode, int32_t* rep_out, int8_t* strand_out, int64_t* off_out, vg_dedup_stats& st) {
    const int64_t n = ps.n;
    if (n == 0) return;
    const bool circular = mode == MODE_CIRCULAR;
    hipStream_t s = vg_stream();
    const int bits = g_hash_bits.load();
    const chunk_tasks ct = chunk_tasks_of(len);
    const unsigned len_bits = bit_width((uint64_t)ct.max_len, 0);
    record_table rt(ps, len, ct.cbeg, s);
    round_bufs r;
    plain_state pl;                          // (each allocated by its mode alone)
    circular_state ci;
    dbuf<unsigned long long> d_h((size_t)n * 4);
    d_h.zero(s);
    {
        vg_prof_scope ps_(circular ? "dedup_chash" : "dedup_hash", (double)ct.total_words * 4.0);
        hipLaunchKernelGGL((circular ? k_chash : k_hash), dim3(wave_blocks(ct.n_tasks)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, rt.beg.p, n, ct.n_tasks, d_h.p);
    }
    rt.beg.release();
    r.alloc_keys((size_t)n);
    if (!circular) pl.ori.alloc((size_t)n);
    {
        vg_prof_scope ps_("dedup_keys", (double)n * 66.0);
        if (circular) hipLaunchKernelGGL(k_ckeys, dim3(blocks(n)), dim3(TPB), 0, s, d_h.p, rt.len.p, n, bits, r.klo.p, r.khi.p, r.klen.p, r.A.p);
        else hipLaunchKernelGGL(k_keys, dim3(blocks(n)), dim3(TPB), 0, s, d_h.p, rt.len.p, n, bits, r.klo.p, r.khi.p, r.klen.p, pl.ori.p, r.A.p);
    }
    d_h.release();
    sort_by_key(r, n, bits, len_bits, s);
    r.alloc_rounds((size_t)n);
    if (circular) {
        ci.sbits = (int)std::max(1u, len_bits);
        ci.d_off.alloc((size_t)n); ci.res.alloc((size_t)n); ci.cl.alloc_owners(n);
    }
    else pl.diff.alloc((size_t)n);
    for (int64_t na = n; na > 0;) {
        ++st.rounds;
        r.d_ndiff.zero(s);
        circular ? circular_round(ps, rt, r, ci, na, s) : plain_round(ps, rt, r, pl, na, s);
        const unsigned long long nd = read_back(r.d_ndiff.p, s);
        if (nd == 0) break;
        st.collisions += (int64_t)nd;
        {
            vg_prof_scope ps_("dedup_compact", (double)na * 12.0);
            scan(r.keep.p, r.at.p, na, false, rocprim::plus<int32_t>(), s);
            hipLaunchKernelGGL(k_compact, dim3(blocks(na)), dim3(TPB), 0, s, r.A.p, na, r.keep.p, r.at.p, r.A2.p);
        }
        std::swap(r.A.p, r.A2.p);
        na = (int64_t)nd;
    }
    r.d_rep.download(rep_out, (size_t)n, s);
    r.d_strand.download(strand_out, (size_t)n, s);
    if (circular) ci.d_off.download(off_out, (size_t)n, s);
    VG_HIP(hipStreamSynchronize(s));
}

// The contained mode's plan, computed before anything is allocated: the index positions (pbeg[i] = record i's first, one per
// symbol), the bits of an offset and the order by (length descending, index ascending) of the result key, the positions per pass.
struct contained_plan {
    std::vector<int64_t> pbeg;
    int64_t total_pos = 0, per_pass = 0;
    int sbits = 1, anchor = 16;
    std::vector<int32_t> order, rnk;         // order[rank] = record, rnk[record] = rank
};
contained_plan plan_contained(const packed_set& ps) {
    const int64_t n = ps.n;
    contained_plan pl;
    pl.pbeg.assign((size_t)n + 1, 0);
    int64_t max_len = 0;
    for (int64_t i = 0; i < n; ++i) { pl.pbeg[(size_t)i + 1] = pl.pbeg[(size_t)i] + ps.len[(size_t)i]; max_len = std::max(max_len, ps.len[(size_t)i]); }
    pl.total_pos = pl.pbeg[(size_t)n];
    // (bit_width(x, 1) is what two hand-written loops gave here: their stops at 63 and 32 bits are out of reach of a length < 2^63 and of n - 1 < 2^31)
    pl.sbits = (int)bit_width((uint64_t)max_len, 1);
    if ((int)bit_width((uint64_t)(n - 1), 1) + 1 + pl.sbits > 64)
        throw vg_error(VG_EOVERFLOW, "vg_deduplicate_contained: record count and longest record together exceed the 64-bit result key");
    pl.order.resize((size_t)n); pl.rnk.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) pl.order[(size_t)i] = (int32_t)i;
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](int32_t a, int32_t b) { return ps.len[(size_t)a] > ps.len[(size_t)b]; });
    for (int64_t r = 0; r < n; ++r) pl.rnk[(size_t)pl.order[(size_t)r]] = (int32_t)r;
    if (pl.total_pos == 0) return pl;        // (nothing to index: no device call at all)
    pl.anchor = g_anchor_symbols.load();
    pl.per_pass = g_index_positions.load();
    if (pl.per_pass <= 0) {
        size_t fr = 0, tot = 0;
        VG_HIP(hipMemGetInfo(&fr, &tot));
        pl.per_pass = std::max<int64_t>(1 << 20, (int64_t)(fr / 2) / INDEX_BYTES);
    }
    pl.per_pass = std::min(std::min(pl.per_pass, pl.total_pos), MAX_PASS_POSITIONS);
    return pl;
}
// The device side of a contained call: its buffers in the order they are allocated, one index pass, one slice of its hits.
struct contained_run {
    const packed_set& ps; const contained_plan& pl; vg_dedup_contained_stats& cst; hipStream_t s;
    const int64_t n = ps.n, nq = 2 * ps.n;   // records; queries (record, strand)
    record_table rt{ ps, ps.len, pl.pbeg, s };
    dbuf<int32_t> d_rnk{ (size_t)n };
    dbuf<unsigned long long> d_best{ (size_t)n }, d_count{ 2 };            // d_count: [0] candidates of a slice, [1] equal candidates
    dbuf<int64_t> hlo{ (size_t)nq + 1 }, hcnt{ (size_t)nq + 1 }, hoff{ (size_t)nq + 1 };       // per query: first hit key, hits, first hit of the pass
    dbuf<uint32_t> cq{ (size_t)CAND_SLICE }, bad{ (size_t)CAND_SLICE };    // the candidate queue of a slice: query, flag,
    dbuf<int32_t> cj{ (size_t)CAND_SLICE };                                //   container,
    dbuf<int64_t> cs{ (size_t)CAND_SLICE }, cnt{ (size_t)CAND_SLICE + 1 }, tbeg{ (size_t)CAND_SLICE + 1 };      //   position; tasks per candidate, their scan
    dbuf<uint64_t> key; dbuf<int64_t> val;   // the sorted index of the pass
    // the positions [pos0, pos0 + np): windows, sort, and the lookup of every query, which leaves the hit ranges -> the hits of the pass
    int64_t index_pass(int64_t pos0, int64_t np) {
        val.release(); key.release();        // (the pass before)
        key.alloc((size_t)np); val.alloc((size_t)np);
        {
            vg_prof_scope ps_("dedupc_windows", (double)np * 16.5);
            hipLaunchKernelGGL(k_sub_windows, dim3(grid_for(np, TPB, 65536)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, rt.beg.p, n, pos0, np, key.p, val.p);
        }
        {
            vg_prof_scope ps_("dedupc_sort", (double)np * 64.0);
            dbuf<uint64_t> key2((size_t)np);
            dbuf<int64_t> val2((size_t)np);
            sort_pairs(key, key2, val, val2, np, 64u, s);
        }
        vg_prof_scope ps_("dedupc_lookup", (double)nq * 40.0);
        hipLaunchKernelGGL(k_sub_lookup, dim3(blocks(nq + 1)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, n, pl.anchor, key.p, np, hlo.p, hcnt.p);
        return scan_total(hcnt.p, hoff.p, nq, s);
    }
    // the hits h0 .. h1 - 1 of the pass: candidates, verification tasks, verify, pick into d_best
    void verify_slice(int64_t h0, int64_t h1) {
        int64_t nc = 0;
        {
            vg_prof_scope ps_("dedupc_lookup", (double)(h1 - h0) * 32.0);
            VG_HIP(hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL(k_sub_cands, dim3(blocks(h1 - h0)), dim3(TPB), 0, s, rt.len.p, rt.beg.p, n, hoff.p, hlo.p, val.p, h0, h1, cq.p, cj.p, cs.p, d_count.p);
            nc = (int64_t)read_back(d_count.p, s);
        }
        if (nc == 0) return;
        cst.candidates += nc;
        {
            vg_prof_scope ps_("dedupc_verify", 0.0);
            hipLaunchKernelGGL(k_sub_tasks, dim3(blocks(nc + 1)), dim3(TPB), 0, s, cq.p, nc, rt.len.p, cnt.p, bad.p);
            const int64_t n_vt = scan_total(cnt.p, tbeg.p, nc, s);
            hipLaunchKernelGGL(k_sub_verify, dim3(wave_blocks(n_vt)), dim3(TPB), 0, s, ps.d_words.p, rt.woff.p, rt.len.p, cq.p, cj.p, cs.p, nc, tbeg.p, n_vt, bad.p);
        }
        vg_prof_scope ps_("dedupc_pick", (double)nc * 24.0);
        hipLaunchKernelGGL(k_sub_pick, dim3(blocks(nc)), dim3(TPB), 0, s, rt.len.p, d_rnk.p, n, cq.p, cj.p, cs.p, nc, bad.p, pl.sbits, d_best.p, d_count.p + 1);
    }
};
// the host decode of best[]: the container's rank, '+' before '-', the offset; the empty records form one group
void contained_labels(const packed_set& ps, const contained_plan& pl, const std::vector<unsigned long long>& best, int32_t* rep_out, int8_t* strand_out, int64_t* off_out) {
    const int64_t n = ps.n;
    int64_t first_empty = -1;
    const unsigned long long m = (1ull << pl.sbits) - 1;
    for (int64_t i = 0; i < n; ++i) {
        rep_out[i] = (int32_t)i; strand_out[i] = 0; off_out[i] = 0;
        if (ps.len[(size_t)i] == 0) { if (first_empty < 0) first_empty = i; else rep_out[i] = (int32_t)first_empty; continue; }
        const unsigned long long b = best[(size_t)i];
        if (!b) continue;
        rep_out[i] = pl.order[(size_t)(n - 1 - (int64_t)(b >> (pl.sbits + 1)))];
        strand_out[i] = ((b >> pl.sbits) & 1ull) ? 0 : 1;
        off_out[i] = (int64_t)(m - (b & m));
    }
}

// Contained mode on the device: packed records (resident) -> representative / strand / offset on the host.  Every equal
// candidate is a container of its record, and the largest key among them names a kept record: were the longest, earliest
// container removed, its own container (longer, or equal and earlier) would contain the record too and have a larger key.
// So one reduction over all candidates of all passes gives the representative; no second phase over the kept records.
void contained_device(const packed_set& ps, int32_t* rep_out, int8_t* strand_out, int64_t* off_out, vg_dedup_stats& st, vg_dedup_contained_stats& cst) {
    const int64_t n = ps.n;
    if (n == 0) return;
    hipStream_t s = vg_stream();
    const contained_plan pl = plan_contained(ps);
    std::vector<unsigned long long> best((size_t)n, 0ull);
    if (pl.total_pos > 0) {
        contained_run run{ ps, pl, cst, s };
        run.d_rnk.upload(pl.rnk.data(), (size_t)n, s);
        run.d_best.zero(s); run.d_count.zero(s);
        for (int64_t pos0 = 0; pos0 < pl.total_pos; pos0 += pl.per_pass) {
            const int64_t np = std::min(pl.per_pass, pl.total_pos - pos0);
            ++cst.passes; cst.positions += np;
            const int64_t n_hits = run.index_pass(pos0, np);
            cst.hits += n_hits;
            for (int64_t h0 = 0; h0 < n_hits; h0 += CAND_SLICE, ++cst.slices) run.verify_slice(h0, std::min(n_hits, h0 + CAND_SLICE));
        }
        run.d_best.download(best.data(), (size_t)n, s);
        cst.verified = (int64_t)read_back(run.d_count.p + 1, s);
    }
    st.rounds = cst.passes; st.collisions = cst.candidates - cst.verified;
    contained_labels(ps, pl, best, rep_out, strand_out, off_out);
}

// a deduplicate call on the packed set, whatever the entry point: the mode's device part (min_repeat > 0: after the terminal repeats), the counts
void run_mode(const packed_set& ps, dedup_mode mode, int64_t min_repeat, int32_t* rep, int8_t* strand, int64_t* offset, int64_t* repeat, vg_dedup_stats& st,
              vg_dedup_contained_stats& cst, vg_dedup_repeat_stats& rst) {
    const int64_t n = ps.n;
    if (mode == MODE_CONTAINED) contained_device(ps, rep, strand, offset, st, cst);
    else if (min_repeat > 0) {
        repeats_device(ps, min_repeat, repeat, rst, true);
        std::vector<int64_t> eff((size_t)n);
        for (int64_t i = 0; i < n; ++i) eff[(size_t)i] = ps.len[(size_t)i] - repeat[i];
        dedup_device(ps, eff, mode, rep, strand, offset, st);
    }
    else dedup_device(ps, ps.len, mode, rep, strand, offset, st);
    st.records = n; st.unique = 0; st.reverse = 0;
    for (int64_t i = 0; i < n; ++i) { st.unique += rep[i] == (int32_t)i; st.reverse += rep[i] != (int32_t)i && strand[i]; }
    st.removed = n - st.unique;
}

// ---------------------------------------------------------------- host: the writer
std::string first_token(const char* b, const char* e) {
    const char* q = b; while (q < e && *q != ' ' && *q != '\t' && *q != '\r') ++q;
    return std::string(b, q);
}
// offset: nullptr, or (circular and contained mode) the fourth column; repeat: nullptr, or (terminal repeats) the fifth and
// sixth: the removed record's and the kept record's
void write_duplicates(const char* path, const vg_fasta_text& in, const std::vector<std::string>& prefix, const int32_t* rep, const int8_t* strand,
                      const int64_t* offset, const int64_t* repeat) {
    const int64_t n = (int64_t)in.recs.size();
    auto id = [&](int64_t i) { const vg_fasta_rec& r = in.recs[(size_t)i]; return prefix[(size_t)r.file] + first_token(r.hdr, r.hdr_end); };
    std::string out = repeat ? "representative\tduplicate\tstrand\toffset\trepeat\trepresentative_repeat\n"
                    : offset ? "representative\tduplicate\tstrand\toffset\n" : "representative\tduplicate\tstrand\n";
    for (int64_t i = 0; i < n; ++i) {
        if (rep[i] == (int32_t)i) continue;
        out += id(rep[i]); out += '\t'; out += id(i); out += '\t'; out += strand[i] ? '-' : '+';
        if (offset) { out += '\t'; out += std::to_string(offset[i]); }
        if (repeat) { out += '\t'; out += std::to_string(repeat[i]); out += '\t'; out += std::to_string(repeat[rep[i]]); }
        out += '\n';
    }
    vg_write_file(path, { out });
}
// the array arguments of an array-level call, before anything is packed: fn names the call in the messages, outputs: its output arrays are all there
void check_seq_arrays(const std::string& fn, const char* ascii, const int64_t* offsets, int64_t n, bool outputs) {
    if (n < 0) throw vg_error(VG_EINVAL, fn + ": negative count");
    if (n >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, fn + ": 2^31 or more records (record indices are int32)");
    if (n && (!offsets || !outputs)) throw vg_error(VG_EINVAL, fn + ": null argument");
    if (n && offsets[n] > offsets[0] && !ascii) throw vg_error(VG_EINVAL, fn + ": null sequence buffer");
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) throw vg_error(VG_EINVAL, fn + ": offsets must not decrease");
}
// packs and uploads the n > 0 sequences of an array-level call; a byte outside the alphabet is the error, named by its record
void pack_seqs(const char* ascii, const int64_t* offsets, int64_t n, packed_set& ps) {
    std::vector<std::pair<const char*, const char*>> seq((size_t)n);
    for (int64_t i = 0; i < n; ++i) seq[(size_t)i] = { ascii + offsets[i], ascii + offsets[i + 1] };
    pack_and_upload(seq, vg_host_threads(), ps);
    if (ps.bad_rec >= 0)
        throw vg_error(VG_EINVAL, "record " + std::to_string(ps.bad_rec) + ": '" + quote_byte(*ps.bad_at) + "' is not an IUPAC nucleotide code");
}

// the caller's stats struct, zeroed, or the local one where the caller passed none
template <class T> T& cleared(T* p, T& local) {
    if (p) *p = T{};
    return p ? *p : local;
}
// min_repeat > 0 (circular mode only): terminal repeats of at least that many symbols are taken off first; repeat[n] gets them
int dedup_seqs(const char* ascii, const int64_t* offsets, int64_t n, dedup_mode mode, int32_t* representative, int8_t* strand, int64_t* offset,
               vg_dedup_stats* stats, vg_dedup_contained_stats* cstats, int64_t min_repeat = 0, int64_t* repeat = nullptr,
               vg_dedup_repeat_stats* rstats = nullptr) {
    VG_API_BEGIN
    if (n > 0 && min_repeat > 0 && !repeat) throw vg_error(VG_EINVAL, "vg_dedup_seqs_circular_tr: the repeat array is required");
    if (n > 0 && mode == MODE_CIRCULAR && !offset) throw vg_error(VG_EINVAL, "vg_dedup_seqs_ex: circular mode needs the offset array");
    if (n > 0 && mode == MODE_CONTAINED && !offset) throw vg_error(VG_EINVAL, "vg_dedup_seqs_contained: the offset array is required");
    check_seq_arrays("vg_dedup_seqs", ascii, offsets, n, representative && strand);
    vg_dedup_stats st_local{}; vg_dedup_stats& st = cleared(stats, st_local);
    vg_dedup_contained_stats cst_local{}; vg_dedup_contained_stats& cst = cleared(cstats, cst_local);
    vg_dedup_repeat_stats rst_local{}; vg_dedup_repeat_stats& rst = cleared(rstats, rst_local);
    if (n == 0) return VG_OK;
    packed_set ps;
    pack_seqs(ascii, offsets, n, ps);
    if (offset) std::fill(offset, offset + n, (int64_t)0);
    run_mode(ps, mode, min_repeat, representative, strand, offset, repeat, st, cst, rst);
    VG_API_END
}

int deduplicate_files(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path, const char* dup_path,
                      const vg_dedup_params* p, dedup_mode mode, int64_t min_repeat = 0) {
    VG_API_BEGIN
    if (!paths || n_paths <= 0 || !out_path || !dup_path || !p) throw vg_error(VG_EINVAL, "vg_deduplicate: null argument");
    if (p->gzip_level < 0 || p->gzip_level > 9) throw vg_error(VG_EINVAL, "vg_deduplicate: gzip_level must be 0 (plain) or 1..9");
    for (int i = 0; i < n_paths; ++i) {
        struct stat sb;
        if (!paths[i]) throw vg_error(VG_EINVAL, "vg_deduplicate: null path");
        if (stat(paths[i], &sb) == 0 && S_ISDIR(sb.st_mode)) throw vg_error(VG_EINVAL, std::string(paths[i]) + " is a directory, not a FASTA file");
    }
    const int T = p->num_threads > 0 ? p->num_threads : vg_host_threads();
    std::vector<std::string> prefix((size_t)n_paths);
    if (prefixes) for (int i = 0; i < n_paths; ++i) prefix[(size_t)i] = prefixes[i] ? prefixes[i] : "";
    vg_host_mark("vg_deduplicate: enter");
    vg_fasta_text in;
    vg_fasta_read(paths, n_paths, T, in);
    const int64_t n = (int64_t)in.recs.size();
    if (n >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, "vg_deduplicate: 2^31 or more records (record indices are int32)");
    vg_host_mark("dedup: records found");
    std::vector<std::pair<const char*, const char*>> seq((size_t)n);
    for (int64_t i = 0; i < n; ++i) seq[(size_t)i] = { in.recs[(size_t)i].seq, in.recs[(size_t)i].end };
    packed_set ps;
    pack_and_upload(seq, T, ps);
    if (ps.bad_rec >= 0) {
        const vg_fasta_rec& r = in.recs[(size_t)ps.bad_rec];
        const char* f0 = in.file_data[(size_t)r.file];
        const int64_t line = 1 + (int64_t)std::count(f0, ps.bad_at, '\n');
        throw vg_error(VG_EINVAL, std::string(paths[r.file]) + ":" + std::to_string(line) + ": '" + quote_byte(*ps.bad_at) +
                                  "' is not an IUPAC nucleotide code");
    }
    vg_require_device();
    const bool with_offset = mode != MODE_PLAIN;
    std::vector<int32_t> rep((size_t)std::max<int64_t>(n, 1));
    std::vector<int8_t> strand((size_t)std::max<int64_t>(n, 1));
    std::vector<int64_t> offset(with_offset ? (size_t)std::max<int64_t>(n, 1) : 0);
    vg_dedup_stats st{};
    vg_dedup_contained_stats cst{};
    vg_dedup_repeat_stats rst{};
    std::vector<int64_t> repeat(min_repeat > 0 ? (size_t)std::max<int64_t>(n, 1) : 0);
    run_mode(ps, mode, min_repeat, rep.data(), strand.data(), offset.data(), repeat.data(), st, cst, rst);
    ps.d_words.release();
    vg_host_mark("dedup: groups computed");
    vg_fasta_write_kept(out_path, in, prefix, rep.data(), p->gzip_level, T);
    write_duplicates(dup_path, in, prefix, rep.data(), strand.data(), with_offset ? offset.data() : nullptr,
                     min_repeat > 0 ? repeat.data() : nullptr);
    vg_host_mark("dedup: written");
    if (p->verbosity >= 1) {
        auto N = [](int64_t v) { return std::to_string(v); };
        std::string line = "vg_deduplicate: " + N(st.records) + " records, " + N(st.unique) + " unique, " + N(st.removed) + " removed (" + N(st.reverse);
        if (mode == MODE_CONTAINED)
            line += " on the reverse strand), " + N(cst.hits) + " anchor hits, " + N(cst.candidates) + " candidates, " + N(cst.verified) +
                    " of them equal, " + N(cst.passes) + " index passes";
        else line += " as reverse complements), " + N(st.collisions) + " hash collisions in " + N(st.rounds) + " rounds";
        if (mode != MODE_CONTAINED && min_repeat > 0) line += ", " + N(rst.with_repeat) + " records with a terminal repeat (" + N(rst.repeat_symbols) + " symbols)";
        fprintf(stderr, "%s\n", line.c_str());
    }
    VG_API_END
}
}  // namespace

extern "C" void vg_dedup_set_hash_bits(int bits) { g_hash_bits.store(std::max(0, std::min(bits, 128))); }
extern "C" void vg_dedup_set_anchor_symbols(int w) { g_anchor_symbols.store(std::max(1, std::min(w, 16))); }
extern "C" void vg_dedup_set_index_positions(int64_t n) { g_index_positions.store(std::max<int64_t>(0, n)); }

extern "C" int vg_dedup_seqs_ex(const char* ascii, const int64_t* offsets, int64_t n, const vg_dedup_options* options,
                                int32_t* representative, int8_t* strand, int64_t* offset, vg_dedup_stats* stats) {
    return dedup_seqs(ascii, offsets, n, options && options->circular ? MODE_CIRCULAR : MODE_PLAIN, representative, strand, offset, stats, nullptr);
}

extern "C" int vg_dedup_seqs(const char* ascii, const int64_t* offsets, int64_t n, int32_t* representative, int8_t* strand,
                             vg_dedup_stats* stats) {
    return dedup_seqs(ascii, offsets, n, MODE_PLAIN, representative, strand, nullptr, stats, nullptr);
}

extern "C" int vg_dedup_seqs_contained(const char* ascii, const int64_t* offsets, int64_t n, int32_t* representative, int8_t* strand,
                                       int64_t* offset, vg_dedup_stats* stats, vg_dedup_contained_stats* contained_stats) {
    return dedup_seqs(ascii, offsets, n, MODE_CONTAINED, representative, strand, offset, stats, contained_stats);
}

extern "C" int vg_deduplicate_ex(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                                 const char* dup_path, const vg_dedup_params* p, const vg_dedup_options* options) {
    return deduplicate_files(paths, n_paths, prefixes, out_path, dup_path, p, options && options->circular ? MODE_CIRCULAR : MODE_PLAIN);
}

extern "C" int vg_deduplicate(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                              const char* dup_path, const vg_dedup_params* p) {
    return deduplicate_files(paths, n_paths, prefixes, out_path, dup_path, p, MODE_PLAIN);
}

extern "C" int vg_deduplicate_contained(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                                        const char* dup_path, const vg_dedup_params* p) {
    return deduplicate_files(paths, n_paths, prefixes, out_path, dup_path, p, MODE_CONTAINED);
}

extern "C" int vg_dedup_terminal_repeats(const char* ascii, const int64_t* offsets, int64_t n, int64_t min_repeat, int64_t* repeat) {
    VG_API_BEGIN
    if (min_repeat < 1) throw vg_error(VG_EINVAL, "vg_dedup_terminal_repeats: min_repeat must be at least 1");
    check_seq_arrays("vg_dedup_terminal_repeats", ascii, offsets, n, repeat != nullptr);
    if (n == 0) return VG_OK;
    packed_set ps;
    pack_seqs(ascii, offsets, n, ps);
    vg_dedup_repeat_stats rst{};
    repeats_device(ps, min_repeat, repeat, rst, false);
    VG_API_END
}

extern "C" int vg_dedup_seqs_circular_tr(const char* ascii, const int64_t* offsets, int64_t n, int64_t min_repeat, int32_t* representative,
                                         int8_t* strand, int64_t* offset, int64_t* repeat, vg_dedup_stats* stats,
                                         vg_dedup_repeat_stats* repeat_stats) {
    if (min_repeat < 1) { vg_set_error("vg_dedup_seqs_circular_tr: min_repeat must be at least 1"); return VG_EINVAL; }
    return dedup_seqs(ascii, offsets, n, MODE_CIRCULAR, representative, strand, offset, stats, nullptr, min_repeat, repeat, repeat_stats);
}

extern "C" int vg_deduplicate_circular_tr(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                                          const char* dup_path, const vg_dedup_params* p, int64_t min_repeat) {
    if (min_repeat < 1) { vg_set_error("vg_deduplicate_circular_tr: min_repeat must be at least 1"); return VG_EINVAL; }
    return deduplicate_files(paths, n_paths, prefixes, out_path, dup_path, p, MODE_CIRCULAR, min_repeat);
}
