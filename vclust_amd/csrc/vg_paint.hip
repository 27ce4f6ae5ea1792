// vg_paint.hip — mosaic painting (tests/paint_restatement.py is the sequential statement): rows
// (q, r, qstart, qend, n_match) in; per position of every object the best-ranked row that covers it wins, and out come the maximal runs
// of one winning row (vg_paint_segment), per object the record vg_paint_stat and per (object, winning partner) a vg_paint_donor.
//
// Everything between the upload of the rows and the download of the records runs on the device, in exact integers:
//   paint_rank      the rows of every object from worst to best: three stable radix sorts, least significant part first
//                   ((r, qstart) descending, (identity key, span) ascending, object with the self rows last); a row's priority is its
//                   place in that order, from 1 -- unique, and larger is better
//   paint_breaks    the distinct (object, position) of every qstart, qend + 1, 0 and len: one radix sort, one flag scan; every row
//                   finds the ranks a < b of its two ends by bisection and covers the elementary segments [a, b)
//   paint_max       the winner of every elementary segment: a sparse table run backwards.  With k = floor(log2(b - a)) a row raises
//                   T[k][a] and T[k][b - 2^k] to its priority (32-bit atomicMax); from the top level down, T[k-1][j] takes the maximum
//                   of T[k][j] and T[k][j - 2^(k-1)] -- a gather over the breakpoints without atomics -- and then the raises of the
//                   rows of level k - 1.  Two level buffers in turn; T[0][j] is the winner of elementary segment j.  T[k][a] speaks
//                   for [a, a + 2^k) only, which lies inside the row: nothing crosses an object boundary.
//   paint_segments  an elementary segment starts a segment when its winner differs from its left neighbour's or it is the object's
//                   first: flag scan, scatter, and one segmented scan whose value at an object's last segment is its record
//   paint_donors    the painted segments keyed (object, partner): one radix sort, one scan that sums and numbers the runs, and a
//                   segmented scan over the donor records for donors, top_partner and top_painted
// No kernel adds to a per-object counter: every per-object figure is read off a scan at the object's last element, and the atomicMax
// of paint_max is spread over the breakpoints by the rows' own ends, so an object with 10^6 rows costs what 10^6 objects with one
// row cost.  Every hand-off between workgroups is a kernel boundary.  A row whose bisection misses its breakpoint, or an output
// beyond its buffer, is not written: it sets a flag that the next read-back turns into an internal error.
#include "vg_scan.h"
#include <climits>

namespace {
// ---------------------------------------------------------------- what the host reads back between the stages
struct paint_ctl { int64_t total[2]; int64_t bad; int64_t pad[5]; int64_t beg[64], end[64]; };   // beg / end: the rows of every level

// ---------------------------------------------------------------- the scanned values
struct count2 { int64_t a, b; };
struct count2_op { __device__ count2 operator()(const count2& x, const count2& y) const { return { x.a + y.a, x.b + y.b }; } };
// per segment, starting again at every object's first segment; n_painted runs through
struct pstat_acc { int64_t painted, painted_in, painted_out, switches, segments, n_painted; uint32_t head, pad; };
struct pstat_op { __device__ pstat_acc operator()(const pstat_acc& a, const pstat_acc& b) const {
    if (b.head) return { b.painted, b.painted_in, b.painted_out, b.switches, b.segments, a.n_painted + b.n_painted, b.head, 0 };
    return { a.painted + b.painted, a.painted_in + b.painted_in, a.painted_out + b.painted_out, a.switches + b.switches, a.segments + b.segments,
             a.n_painted + b.n_painted, a.head, 0 }; } };
// per painted segment in (object, partner) order, starting again at every run; n_runs runs through
struct donor_acc { int64_t painted, segments, n_runs; uint32_t head, pad; };
struct donor_op { __device__ donor_acc operator()(const donor_acc& a, const donor_acc& b) const {
    if (b.head) return { b.painted, b.segments, a.n_runs + b.n_runs, b.head, 0 };
    return { a.painted + b.painted, a.segments + b.segments, a.n_runs + b.n_runs, a.head, 0 }; } };
// per donor record, starting again at every object: the maximum by (painted, -partner), and a count
struct top_acc { int64_t painted; int32_t partner; uint32_t head; int64_t count; };
struct top_op { __device__ top_acc operator()(const top_acc& a, const top_acc& b) const {
    if (b.head) return b;
    const bool keep = a.painted > b.painted || (a.painted == b.painted && a.partner < b.partner);
    return { keep ? a.painted : b.painted, keep ? a.partner : b.partner, a.head, a.count + b.count }; } };

// ---------------------------------------------------------------- element-wise kernels
// first sort: smaller r, then smaller qstart, is better -- the key falls with both
__global__ __launch_bounds__(TPB) void k_key_partner_start(const uint32_t* __restrict__ r, const int32_t* __restrict__ qs, int64_t n, unsigned pos_bits,
                                                           uint64_t r_mask, uint64_t pos_mask, uint64_t* key) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
        key[i] = ((r_mask - r[i]) << pos_bits) | (pos_mask - (uint64_t)qs[i]);
}
// second sort: the identity key I = floor(n_match * 2^32 / span) (33 bits) above the span (31 bits)
__global__ __launch_bounds__(TPB) void k_key_identity_span(const uint32_t* __restrict__ order, const int32_t* __restrict__ qs, const int32_t* __restrict__ qe,
                                                           const int32_t* __restrict__ nm, int64_t n, uint64_t* key) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint32_t i = order[j];
        const uint64_t span = (uint64_t)(qe[i] - qs[i]) + 1;
        key[j] = ((((uint64_t)nm[i]) << 32) / span) << 31 | span;
    }
}
// third sort: the object; a self row gets `self`, above every object
__global__ __launch_bounds__(TPB) void k_key_object(const uint32_t* __restrict__ order, const uint32_t* __restrict__ q, const uint32_t* __restrict__ r, int64_t n,
                                                    uint32_t self, uint32_t* key) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint32_t i = order[j];
        key[j] = q[i] == r[i] ? self : q[i];
    }
}
__global__ __launch_bounds__(TPB) void k_gather_ranked(const uint32_t* __restrict__ order, const uint32_t* __restrict__ r, const int32_t* __restrict__ qs,
                                                       const int32_t* __restrict__ qe, const int32_t* __restrict__ nm, int64_t n, int32_t* sr, int32_t* sqs,
                                                       int32_t* sqe, int32_t* snm) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint32_t i = order[j];
        sr[j] = (int32_t)r[i]; sqs[j] = qs[i]; sqe[j] = qe[i]; snm[j] = nm[i];
    }
}
// the candidates of the breakpoints: the two ends of every kept row ...
__global__ __launch_bounds__(TPB) void k_row_candidates(const uint32_t* __restrict__ obj, const int32_t* __restrict__ sqs, const int32_t* __restrict__ sqe, int64_t n,
                                                        unsigned pos_bits, uint64_t* cand) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint64_t o = (uint64_t)obj[j] << pos_bits;
        cand[2 * j] = o | (uint64_t)sqs[j];
        cand[2 * j + 1] = o | ((uint64_t)sqe[j] + 1);
    }
}
// ... and 0 and len of every object with len > 0; an object without a position gets two keys that sort behind every object
__global__ __launch_bounds__(TPB) void k_object_candidates(const int32_t* __restrict__ len, int64_t n, unsigned pos_bits, uint64_t* cand) {
    for (int64_t o = (int64_t)blockIdx.x * TPB + threadIdx.x; o < n; o += (int64_t)gridDim.x * TPB) {
        const bool live = len[o] > 0;
        cand[2 * o] = live ? (uint64_t)o << pos_bits : (uint64_t)n << pos_bits;
        cand[2 * o + 1] = live ? ((uint64_t)o << pos_bits) | (uint64_t)len[o] : (uint64_t)n << pos_bits;
    }
}
__global__ __launch_bounds__(TPB) void k_init_records(const int32_t* __restrict__ len, int64_t n, vg_paint_stat* rec) {
    for (int64_t o = (int64_t)blockIdx.x * TPB + threadIdx.x; o < n; o += (int64_t)gridDim.x * TPB)
        rec[o] = vg_paint_stat{ len[o], 0, 0, 0, 0, -1, 0, 0, 0 };
}
// the first index in [0, n) whose key is not below `want` (n: none)
__device__ __forceinline__ int64_t lower_bound_key(const uint64_t* __restrict__ key, int64_t n, uint64_t want) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// per kept row the ranks a < b of its ends among the breakpoints, as the two cells it raises (a and b - 2^k) and its level k; a row
// that misses a breakpoint raises nothing (lo = -1) and sets the flag
__global__ __launch_bounds__(TPB) void k_row_ranks(const uint32_t* __restrict__ obj, const int32_t* __restrict__ sqs, const int32_t* __restrict__ sqe, int64_t n,
                                                   unsigned pos_bits, const uint64_t* __restrict__ ukey, int64_t n_breaks, int64_t* lo, int64_t* hi, uint8_t* level,
                                                   int64_t* bad) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint64_t o = (uint64_t)obj[j] << pos_bits, ka = o | (uint64_t)sqs[j], kb = o | ((uint64_t)sqe[j] + 1);
        const int64_t a = lower_bound_key(ukey, n_breaks, ka), b = lower_bound_key(ukey, n_breaks, kb);
        if (!(a < b && b < n_breaks && ukey[a] == ka && ukey[b] == kb)) {
            lo[j] = -1; hi[j] = -1; level[j] = 0;
            *bad = 1;
            continue;
        }
        const int k = 63 - __clzll((long long)(b - a));
        lo[j] = a; hi[j] = b - (1ll << k); level[j] = (uint8_t)k;
    }
}
// where the rows of every level begin and end in level order
__global__ __launch_bounds__(TPB) void k_level_bounds(const uint8_t* __restrict__ level, int64_t n, paint_ctl* ctl) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const int k = level[i] & 63;
        if (i == 0 || level[i - 1] != level[i]) ctl->beg[k] = i;
        if (i == n - 1 || level[i + 1] != level[i]) ctl->end[k] = i + 1;
    }
}
// the rows of one level raise their two cells to their priority (their place in rank order, from 1)
__global__ __launch_bounds__(TPB) void k_raise(const uint32_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                               int64_t n_breaks, uint32_t* T) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const uint32_t j = rows[i];
        const int64_t a = lo[j], b = hi[j];
        if (a < 0 || b < a || b >= n_breaks) continue;
        atomicMax(&T[a], j + 1);
        if (b != a) atomicMax(&T[b], j + 1);
    }
}
// one level down: cell j of the next level is covered by cell j and by cell j - half of this one
__global__ __launch_bounds__(TPB) void k_push_down(const uint32_t* __restrict__ T, int64_t n, int64_t half, uint32_t* next) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        uint32_t v = T[j];
        if (j >= half) { const uint32_t w = T[j - half]; v = w > v ? w : v; }
        next[j] = v;
    }
}
// breakpoint j opens an elementary segment unless it is the object's len; that one starts a segment when it is the object's first
// or its winner is not its left neighbour's
__device__ __forceinline__ bool starts_segment(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ win, const int32_t* __restrict__ len, int64_t j,
                                               unsigned pos_bits, uint64_t pos_mask) {
    const uint64_t key = ukey[j], pos = key & pos_mask;
    if (pos >= (uint64_t)len[key >> pos_bits]) return false;
    return pos == 0 || win[j] != win[j - 1];
}
__global__ __launch_bounds__(TPB) void k_scatter_segments(const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ win, const int32_t* __restrict__ len,
                                                          const int64_t* __restrict__ slot, int64_t n_breaks, unsigned pos_bits, uint64_t pos_mask,
                                                          const int32_t* __restrict__ sr, const int32_t* __restrict__ sqs, const int32_t* __restrict__ sqe,
                                                          const int32_t* __restrict__ snm, int64_t n_rows, int64_t n_seg, vg_paint_segment* seg, int64_t* bad) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n_breaks; j += (int64_t)gridDim.x * TPB) {
        if (!starts_segment(ukey, win, len, j, pos_bits, pos_mask)) continue;
        const int64_t x = slot[j];
        const uint32_t w = win[j];
        if (x < 0 || x >= n_seg || (int64_t)w > n_rows) { *bad = 1; continue; }
        const int32_t o = (int32_t)(ukey[j] >> pos_bits), pos = (int32_t)(ukey[j] & pos_mask);
        seg[x] = w ? vg_paint_segment{ o, pos, 0, sr[w - 1], sqs[w - 1], sqe[w - 1], snm[w - 1] } : vg_paint_segment{ o, pos, 0, -1, -1, -1, 0 };
    }
}

// (a copy of vg_cover.hip's: the smallest i in [0, n) with bad(i), or -1; the chunks of the host threads each stop at their first)
template <class Bad> int64_t first_bad(int64_t n, Bad bad) {
    const int n_thr = vg_host_threads();
    std::vector<int64_t> found((size_t)std::max(1, n_thr), -1);
    vg_parallel_chunks(n, n_thr, [&](int64_t lo, int64_t hi, int t) {
        for (int64_t i = lo; i < hi; ++i) if (bad(i)) { found[(size_t)t] = i; return; }
    });
    for (const int64_t k : found) if (k >= 0) return k;
    return -1;
}

// what the host has checked and counted
struct paint_input {
    int64_t n; const int32_t* len; const int32_t* label; int64_t n_empty, max_len;
    const uint32_t* q; const uint32_t* r; const int32_t* qs; const int32_t* qe; const int32_t* nm; int64_t n_rows, n_kept;
};

paint_ctl read_ctl(const dbuf<paint_ctl>& ctl, hipStream_t s, const char* where) {
    const paint_ctl c = read_back((const paint_ctl*)ctl.p, s);
    if (c.bad) throw vg_error(VG_EHIP, std::string("vg_paint_rows: ") + where + " (internal error)");
    return c;
}
// a host copy of `count` device records that the caller releases with vg_free
template <class T> T* download_owned(const dbuf<T>& d, int64_t count, hipStream_t s) {
    T* h = (T*)malloc(sizeof(T) * (size_t)std::max<int64_t>(1, count));
    if (!h) throw vg_error(VG_ENOMEM, "out of host memory");
    struct guard { void* p; ~guard() { free(p); } } g{ h };
    if (count) d.download(h, (size_t)count, s);
    VG_HIP(hipStreamSynchronize(s));
    g.p = nullptr;
    return h;
}

void paint_on_device(const paint_input& in, vg_paint_stat* out, vg_paint_segment** segments, int64_t* n_segments, vg_paint_donor** donors, int64_t* n_donors,
                     vg_paint_run_stats& st) {
    hipStream_t s = vg_stream();
    const int64_t n = in.n, R = in.n_rows, K = in.n_kept;
    // partners below objects in a donor key; positions up to max_len (a breakpoint at len is legal) below the object in a breakpoint key,
    // where the object may be n (the keys of the objects without a position)
    const unsigned r_bits = bit_width((uint64_t)(n - 1), 1), q_bits = bit_width((uint64_t)n, 1), pos_bits = bit_width((uint64_t)in.max_len, 1);
    const uint64_t pos_mask = (1ull << pos_bits) - 1, r_mask = (1ull << r_bits) - 1;

    dbuf<int32_t> len((size_t)n), label((size_t)n);
    dbuf<vg_paint_stat> d_out((size_t)n);
    dbuf<paint_ctl> ctl(1);
    len.upload(in.len, (size_t)n, s);
    if (in.label) label.upload(in.label, (size_t)n, s); else label.zero(s);
    ctl.zero(s);
    const int32_t* d_len = len.p; const int32_t* d_label = label.p;
    paint_ctl* d_ctl = ctl.p; int64_t* d_bad = &ctl.p->bad;
    hipLaunchKernelGGL(k_init_records, dim3(blocks(n)), dim3(TPB), 0, s, d_len, n, d_out.p);

    // the kept rows from worst to best inside every object: row j has the priority j + 1
    dbuf<uint32_t> sobj((size_t)R); dbuf<int32_t> sr((size_t)K), sqs((size_t)K), sqe((size_t)K), snm((size_t)K);
    if (K > 0) {
        vg_prof_scope ps("paint_rank", (double)R * (20.0 + 2.0 * 2.0 * 12.0 + 2.0 * 8.0 + 8.0 + 16.0 + 8.0 + 32.0));
        dbuf<uint32_t> q((size_t)R), r((size_t)R); dbuf<int32_t> qs((size_t)R), qe((size_t)R), nm((size_t)R);
        q.upload(in.q, (size_t)R, s); r.upload(in.r, (size_t)R, s); qs.upload(in.qs, (size_t)R, s); qe.upload(in.qe, (size_t)R, s); nm.upload(in.nm, (size_t)R, s);
        dbuf<uint32_t> ord_a((size_t)R), ord_b((size_t)R);
        {
            dbuf<uint64_t> key((size_t)R), key_sorted((size_t)R);
            hipLaunchKernelGGL(k_iota, dim3(blocks(R)), dim3(TPB), 0, s, ord_a.p, R);
            hipLaunchKernelGGL(k_key_partner_start, dim3(blocks(R)), dim3(TPB), 0, s, (const uint32_t*)r.p, (const int32_t*)qs.p, R, pos_bits, r_mask, pos_mask, key.p);
            sort_pairs((const uint64_t*)key.p, key_sorted.p, (const uint32_t*)ord_a.p, ord_b.p, R, r_bits + pos_bits, s);
            hipLaunchKernelGGL(k_key_identity_span, dim3(blocks(R)), dim3(TPB), 0, s, (const uint32_t*)ord_b.p, (const int32_t*)qs.p, (const int32_t*)qe.p,
                               (const int32_t*)nm.p, R, key.p);
            sort_pairs((const uint64_t*)key.p, key_sorted.p, (const uint32_t*)ord_b.p, ord_a.p, R, 64u, s);
        }
        dbuf<uint32_t> okey((size_t)R);
        hipLaunchKernelGGL(k_key_object, dim3(blocks(R)), dim3(TPB), 0, s, (const uint32_t*)ord_a.p, (const uint32_t*)q.p, (const uint32_t*)r.p, R, (uint32_t)n, okey.p);
        sort_pairs((const uint32_t*)okey.p, sobj.p, (const uint32_t*)ord_a.p, ord_b.p, R, q_bits, s);
        hipLaunchKernelGGL(k_gather_ranked, dim3(blocks(K)), dim3(TPB), 0, s, (const uint32_t*)ord_b.p, (const uint32_t*)r.p, (const int32_t*)qs.p,
                           (const int32_t*)qe.p, (const int32_t*)nm.p, K, sr.p, sqs.p, sqe.p, snm.p);
        VG_HIP(hipGetLastError());
    }
    st.rows_kept = K;

    // the breakpoints (object, pos) ascending, and per kept row the two cells it raises and its level
    const int64_t n_cand = 2 * K + 2 * (n - in.n_empty);
    dbuf<uint64_t> ukey((size_t)n_cand);
    dbuf<int64_t> cell_lo((size_t)K), cell_hi((size_t)K);
    dbuf<uint32_t> by_level((size_t)K);
    int64_t n_breaks = 0;
    paint_ctl lv{};
    {
        vg_prof_scope ps("paint_breaks", (double)(n_cand + 2 * in.n_empty) * (8.0 + 2.0 * 8.0 * 2.0) + (double)n_cand * 16.0 + (double)K * (12.0 + 17.0 + 2.0 * 5.0 * 2.0));
        if (n_cand > 0) {
            const int64_t C = 2 * K + 2 * n;
            dbuf<uint64_t> cand((size_t)C), sorted((size_t)C);
            if (K) hipLaunchKernelGGL(k_row_candidates, dim3(blocks(K)), dim3(TPB), 0, s, (const uint32_t*)sobj.p, (const int32_t*)sqs.p, (const int32_t*)sqe.p, K, pos_bits, cand.p);
            hipLaunchKernelGGL(k_object_candidates, dim3(blocks(n)), dim3(TPB), 0, s, d_len, n, pos_bits, cand.p + 2 * K);
            with_temp_storage([&](void* tmp, size_t& tb) {
                return rocprim::radix_sort_keys(tmp, tb, (const uint64_t*)cand.p, sorted.p, (size_t)C, 0u, pos_bits + q_bits, s); });
            const uint64_t* d_sorted = sorted.p; uint64_t* d_ukey = ukey.p;
            scan_tiles(n_cand, (int64_t)0, [] __device__(int64_t a, int64_t b) { return a + b; },
                [=] __device__(int64_t i) { return (int64_t)(i == 0 || d_sorted[i] != d_sorted[i - 1]); },
                [=] __device__(int64_t i, const int64_t& inc, const int64_t& ex) {
                    if (i == 0 || d_sorted[i] != d_sorted[i - 1]) d_ukey[ex] = d_sorted[i];
                    if (i == n_cand - 1) d_ctl->total[0] = inc;
                }, s);
            n_breaks = read_ctl(ctl, s, "the breakpoints").total[0];
        }
        if (K > 0) {
            dbuf<uint8_t> level((size_t)K), level_sorted((size_t)K);
            dbuf<uint32_t> iota((size_t)K);
            hipLaunchKernelGGL(k_row_ranks, dim3(blocks(K)), dim3(TPB), 0, s, (const uint32_t*)sobj.p, (const int32_t*)sqs.p, (const int32_t*)sqe.p, K, pos_bits,
                               (const uint64_t*)ukey.p, n_breaks, cell_lo.p, cell_hi.p, level.p, d_bad);
            hipLaunchKernelGGL(k_iota, dim3(blocks(K)), dim3(TPB), 0, s, iota.p, K);
            sort_pairs((const uint8_t*)level.p, level_sorted.p, (const uint32_t*)iota.p, by_level.p, K, 6u, s);
            hipLaunchKernelGGL(k_level_bounds, dim3(blocks(K)), dim3(TPB), 0, s, (const uint8_t*)level_sorted.p, K, d_ctl);
            VG_HIP(hipGetLastError());
            lv = read_ctl(ctl, s, "a row's end is not among the breakpoints");
        }
    }
    st.breakpoints = n_breaks;
    int top = -1;
    for (int k = 0; k < 64; ++k) if (lv.end[k] > lv.beg[k]) top = k;
    st.levels = top + 1;

    // the winner of every elementary segment: T[0] of the sparse table run backwards
    dbuf<uint32_t> win((size_t)n_breaks);
    {
        vg_prof_scope ps("paint_max", (double)n_breaks * 4.0 + (double)std::max(0, top) * (double)n_breaks * 12.0 + (double)K * (4.0 + 16.0 + 8.0));
        dbuf<uint32_t> other((size_t)(top > 0 ? n_breaks : 0));
        win.zero(s);
        for (int k = top; k >= 0; --k) {
            const int64_t rows = lv.end[k] - lv.beg[k];
            if (rows > 0)
                hipLaunchKernelGGL(k_raise, dim3(blocks(rows)), dim3(TPB), 0, s, (const uint32_t*)by_level.p + lv.beg[k], rows, (const int64_t*)cell_lo.p,
                                   (const int64_t*)cell_hi.p, n_breaks, win.p);
            if (k > 0) {
                hipLaunchKernelGGL(k_push_down, dim3(blocks(n_breaks)), dim3(TPB), 0, s, (const uint32_t*)win.p, n_breaks, (int64_t)1 << (k - 1), other.p);
                std::swap(win, other);
            }
        }
        VG_HIP(hipGetLastError());
    }
    cell_lo.release(); cell_hi.release(); by_level.release();

    // the segments, and the record of every object off a scan over them
    const uint64_t* d_ukey = ukey.p; const uint32_t* d_win = win.p;
    int64_t S = 0, P = 0;
    dbuf<vg_paint_segment> seg;
    dbuf<uint64_t> dkey; dbuf<int64_t> dwidth;
    {
        vg_prof_scope ps("paint_segments", (double)n_breaks * (2.0 * 16.0 + 8.0 + 24.0) + 0.0);
        dbuf<int64_t> slot((size_t)n_breaks);
        int64_t* d_slot = slot.p;
        scan_tiles(n_breaks, count2{ 0, 0 }, count2_op(),
            [=] __device__(int64_t j) {
                const bool start = starts_segment(d_ukey, d_win, d_len, j, pos_bits, pos_mask);
                return count2{ start ? 1ll : 0ll, start && d_win[j] ? 1ll : 0ll };
            },
            [=] __device__(int64_t j, const count2& inc, const count2& ex) {
                d_slot[j] = ex.a;
                if (j == n_breaks - 1) { d_ctl->total[0] = inc.a; d_ctl->total[1] = inc.b; }
            }, s);
        if (n_breaks) { const paint_ctl c = read_ctl(ctl, s, "the segment count"); S = c.total[0]; P = c.total[1]; }
        seg.alloc((size_t)S); dkey.alloc((size_t)P); dwidth.alloc((size_t)P);
        if (S) {
            hipLaunchKernelGGL(k_scatter_segments, dim3(blocks(n_breaks)), dim3(TPB), 0, s, d_ukey, d_win, d_len, (const int64_t*)slot.p, n_breaks, pos_bits, pos_mask,
                               (const int32_t*)sr.p, (const int32_t*)sqs.p, (const int32_t*)sqe.p, (const int32_t*)snm.p, K, S, seg.p, d_bad);
            VG_HIP(hipGetLastError());
        }
        vg_paint_segment* d_seg = seg.p; vg_paint_stat* d_rec = d_out.p; uint64_t* d_dkey = dkey.p; int64_t* d_dwidth = dwidth.p;
        auto segment_end = [=] __device__(int64_t x) { return x + 1 < S && d_seg[x + 1].object == d_seg[x].object ? d_seg[x + 1].start - 1 : d_len[d_seg[x].object] - 1; };
        scan_tiles(S, pstat_acc{ 0, 0, 0, 0, 0, 0, 0, 0 }, pstat_op(),
            [=] __device__(int64_t x) {
                const vg_paint_segment g = d_seg[x];
                const bool head = x == 0 || d_seg[x - 1].object != g.object, painted = g.partner >= 0;
                const bool in_group = painted && d_label[g.partner] == d_label[g.object];
                const int64_t width = painted ? (int64_t)segment_end(x) - g.start + 1 : 0;
                const bool sw = painted && !head && d_seg[x - 1].partner >= 0 && d_seg[x - 1].partner != g.partner;
                return pstat_acc{ width, in_group ? width : 0, in_group ? 0 : width, sw ? 1ll : 0ll, 1, painted ? 1ll : 0ll, (uint32_t)head, 0 };
            },
            [=] __device__(int64_t x, const pstat_acc& inc, const pstat_acc&) {
                const vg_paint_segment g = d_seg[x];
                const int32_t end = segment_end(x);
                d_seg[x].end = end;                                  // (no other element's load or store reads this field)
                if (g.partner >= 0) {
                    const int64_t p = inc.n_painted - 1;
                    if (p < 0 || p >= P) *d_bad = 1;
                    else { d_dkey[p] = ((uint64_t)g.object << r_bits) | (uint64_t)g.partner; d_dwidth[p] = (int64_t)end - g.start + 1; }
                }
                if (x + 1 < S && d_seg[x + 1].object == g.object) return;
                vg_paint_stat& rec = d_rec[g.object];
                rec.painted = inc.painted; rec.painted_in = inc.painted_in; rec.painted_out = inc.painted_out; rec.switches = inc.switches; rec.segments = inc.segments;
            }, s);
    }
    st.segments = S;

    // the donor records, and donors / top_partner / top_painted of every object off a scan over them
    int64_t D = 0;
    dbuf<vg_paint_donor> donor((size_t)P);
    if (P > 0) {
        vg_prof_scope ps("paint_donors", (double)P * (2.0 * 16.0 * 2.0 + 2.0 * 16.0 + 24.0 + 2.0 * 24.0));
        dbuf<uint64_t> dkey2((size_t)P); dbuf<int64_t> dwidth2((size_t)P);
        sort_pairs((const uint64_t*)dkey.p, dkey2.p, (const int64_t*)dwidth.p, dwidth2.p, P, 2 * r_bits, s);
        const uint64_t* d_key = dkey2.p; const int64_t* d_width = dwidth2.p; vg_paint_donor* d_donor = donor.p; vg_paint_stat* d_rec = d_out.p;
        scan_tiles(P, donor_acc{ 0, 0, 0, 0, 0 }, donor_op(),
            [=] __device__(int64_t i) {
                const bool head = i == 0 || d_key[i] != d_key[i - 1];
                return donor_acc{ d_width[i], 1, head ? 1ll : 0ll, (uint32_t)head, 0 };
            },
            [=] __device__(int64_t i, const donor_acc& inc, const donor_acc&) {
                if (i == P - 1) d_ctl->total[0] = inc.n_runs;
                if (i + 1 < P && d_key[i + 1] == d_key[i]) return;
                const int64_t at = inc.n_runs - 1;
                if (at < 0 || at >= P) { *d_bad = 1; return; }
                d_donor[at] = vg_paint_donor{ (int32_t)(d_key[i] >> r_bits), (int32_t)(d_key[i] & r_mask), inc.painted, inc.segments };
            }, s);
        D = read_ctl(ctl, s, "a segment or a donor record beyond its buffer").total[0];
        scan_tiles(D, top_acc{ -1, INT_MAX, 0, 0 }, top_op(),
            [=] __device__(int64_t i) {
                const vg_paint_donor d = d_donor[i];
                return top_acc{ d.painted, d.partner, (uint32_t)(i == 0 || d_donor[i - 1].object != d.object), 1 };
            },
            [=] __device__(int64_t i, const top_acc& inc, const top_acc&) {
                const int32_t o = d_donor[i].object;
                if (i + 1 < D && d_donor[i + 1].object == o) return;
                vg_paint_stat& rec = d_rec[o];
                rec.donors = inc.count; rec.top_partner = inc.partner; rec.top_painted = inc.painted;
            }, s);
    }
    st.donor_records = D;
    d_out.download(out, (size_t)n, s);
    VG_HIP(hipStreamSynchronize(s));
    read_ctl(ctl, s, "a segment beyond its buffer");
    // (both copies are made before either pointer is handed over: an error leaves the caller nothing to release)
    vg_paint_segment* h_seg = segments ? download_owned(seg, S, s) : nullptr;
    struct guard { void* p; ~guard() { free(p); } } g{ h_seg };
    vg_paint_donor* h_donor = donors ? download_owned(donor, D, s) : nullptr;
    g.p = nullptr;
    if (segments) { *segments = h_seg; *n_segments = S; }
    if (donors) { *donors = h_donor; *n_donors = D; }
}
}  // namespace

extern "C" int vg_paint_rows(int64_t n_objects, const int64_t* len, const int32_t* label, int64_t n_groups, const uint32_t* q, const uint32_t* r,
                             const int32_t* qstart, const int32_t* qend, const int32_t* n_match, int64_t n_rows, vg_paint_stat* out,
                             vg_paint_segment** segments, int64_t* n_segments, vg_paint_donor** donors, int64_t* n_donors, vg_paint_run_stats* st) {
    VG_API_BEGIN
    const std::string fn = "vg_paint_rows: ";
    if (n_objects < 0 || n_rows < 0) throw vg_error(VG_EINVAL, fn + "negative count");
    if (n_objects >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, fn + "2^31 or more objects");
    if (n_rows >= (1LL << 32)) throw vg_error(VG_EOVERFLOW, fn + "2^32 or more rows");
    if ((segments == nullptr) != (n_segments == nullptr)) throw vg_error(VG_EINVAL, fn + "segments and n_segments go together (both or neither)");
    if ((donors == nullptr) != (n_donors == nullptr)) throw vg_error(VG_EINVAL, fn + "donors and n_donors go together (both or neither)");
    if ((n_objects && (!len || !out)) || (n_rows && (!q || !r || !qstart || !qend || !n_match))) throw vg_error(VG_EINVAL, fn + "null argument");
    if (label && (n_groups < 1 || n_groups >= (1LL << 31)) && n_objects) throw vg_error(VG_EINVAL, fn + "n_groups = " + std::to_string(n_groups) + " outside 1..2^31-1");
    const int64_t n = n_objects;
    int64_t bad = first_bad(n, [&](int64_t i) { return len[i] < 0 || len[i] >= (1LL << 31); });
    if (bad >= 0) throw vg_error(VG_EINVAL, fn + "len[" + std::to_string(bad) + "] = " + std::to_string(len[bad]) + (len[bad] < 0 ? " is negative" : " is 2^31 or more"));
    if (label) {
        bad = first_bad(n, [&](int64_t i) { return label[i] < 0 || label[i] >= n_groups; });
        if (bad >= 0) throw vg_error(VG_EINVAL, fn + "label[" + std::to_string(bad) + "] = " + std::to_string(label[bad]) + " outside 0.." + std::to_string(n_groups - 1));
    }
    bad = first_bad(n_rows, [&](int64_t i) {
        return q[i] >= (uint64_t)n || r[i] >= (uint64_t)n || qstart[i] < 0 || qstart[i] > qend[i] || qend[i] >= len[q[i]] || n_match[i] < 0 ||
               (int64_t)n_match[i] > (int64_t)qend[i] - qstart[i] + 1; });
    if (bad >= 0) {
        const std::string row = fn + "row " + std::to_string(bad) + ": ";
        if (q[bad] >= (uint64_t)n || r[bad] >= (uint64_t)n)
            throw vg_error(VG_EINVAL, row + "index " + std::to_string(q[bad] >= (uint64_t)n ? q[bad] : r[bad]) + " outside 0.." + std::to_string(n - 1));
        if (qstart[bad] < 0) throw vg_error(VG_EINVAL, row + "qstart " + std::to_string(qstart[bad]) + " is negative");
        if (qstart[bad] > qend[bad]) throw vg_error(VG_EINVAL, row + "qstart " + std::to_string(qstart[bad]) + " > qend " + std::to_string(qend[bad]));
        if (qend[bad] >= len[q[bad]])
            throw vg_error(VG_EINVAL, row + "qend " + std::to_string(qend[bad]) + " >= len[" + std::to_string(q[bad]) + "] = " + std::to_string(len[q[bad]]));
        if (n_match[bad] < 0) throw vg_error(VG_EINVAL, row + "n_match " + std::to_string(n_match[bad]) + " is negative");
        throw vg_error(VG_EINVAL, row + "n_match " + std::to_string(n_match[bad]) + " > span " + std::to_string((int64_t)qend[bad] - qstart[bad] + 1));
    }
    vg_paint_run_stats local{};
    if (segments) { *segments = nullptr; *n_segments = 0; }
    if (donors) { *donors = nullptr; *n_donors = 0; }
    if (n == 0) {
        if (st) *st = local;
        return VG_OK;
    }
    vg_require_device();
    std::vector<int32_t> len32((size_t)n);
    int64_t max_len = 0, n_empty = 0;
    for (int64_t i = 0; i < n; ++i) { len32[(size_t)i] = (int32_t)len[i]; max_len = std::max(max_len, len[i]); n_empty += len[i] == 0; }
    int64_t n_self = 0;
    for (int64_t i = 0; i < n_rows; ++i) n_self += q[i] == r[i];
    const paint_input in{ n, len32.data(), label, n_empty, max_len, q, r, qstart, qend, n_match, n_rows, n_rows - n_self };
    paint_on_device(in, out, segments, n_segments, donors, n_donors, local);
    if (st) *st = local;
    VG_API_END
}
