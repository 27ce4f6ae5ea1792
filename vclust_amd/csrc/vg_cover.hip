// vg_cover.hip — coverage map (tests/cover_restatement.py is the sequential statement): rows
// (q, r, qstart, qend) in, per object the record vg_cover_stat and the run-length depth profile (vg_cover_segment) out.
//
// Everything between the upload of the rows and the download of the records and segments runs on the device, in exact integers:
//   cover_sort     rows by (q, r, qstart): two stable radix sorts (rocPRIM), self rows under a key that sorts last
//   cover_merge    running maximum of qend inside every (q, r) run (a segmented scan) -> the heads and tails of the disjoint
//                  intervals of C(q, r); a second scan numbers the intervals, emits their two events and leaves partners_* and sum_*
//   cover_events   events sorted by (q, pos), deltas of equal (q, pos) summed (rocPRIM radix sort + reduce_by_key)
//   cover_depth    inclusive scan of the deltas = the depths behind every breakpoint; segment starts counted, placed and written
//   cover_stats    segment ends, and a segmented scan over the segments whose value at an object's last segment is its record
// No kernel here uses an atomic on a per-object counter: every per-object figure is read off a scan at the object's first and last
// element, so an object with 10^6 events costs what 10^6 objects with one event cost.  (The one atomic is the label histogram's, one
// add per distinct label per wave.)  Every hand-off between workgroups is a kernel boundary: the scans are three launches (tile
// totals, one workgroup over the totals, tiles again with their carry), tiles of TILE = 1024 elements.
#include "vg_scan.h"
#include <climits>

namespace {
// ---------------------------------------------------------------- the scanned values
// running maximum that starts again at every element with head set
struct seg_max { int32_t mx; uint32_t head; };
struct seg_max_op { __device__ seg_max operator()(const seg_max& a, const seg_max& b) const { return b.head ? b : seg_max{ a.mx > b.mx ? a.mx : b.mx, a.head }; } };
// per sorted row: run heads (in the low, out in the high 32 bits), covered lengths by channel, interval heads
struct merge_acc { int64_t partners, sum_in, sum_out, n_int; };
struct merge_op { __device__ merge_acc operator()(const merge_acc& a, const merge_acc& b) const {
    return { a.partners + b.partners, a.sum_in + b.sum_in, a.sum_out + b.sum_out, a.n_int + b.n_int }; } };
// per breakpoint: the packed depths (in + (out << 32)) and the segment starts so far
struct depth_acc { int64_t depth, n_start; };
struct depth_op { __device__ depth_acc operator()(const depth_acc& a, const depth_acc& b) const { return { a.depth + b.depth, a.n_start + b.n_start }; } };
struct plus_op { __device__ int64_t operator()(int64_t a, int64_t b) const { return a + b; } };
// per segment, starting again at every object's first segment
struct stat_acc { int64_t covered, covered_in, covered_out, core; int32_t max_depth; uint32_t head; };
struct stat_op { __device__ stat_acc operator()(const stat_acc& a, const stat_acc& b) const {
    if (b.head) return b;
    return { a.covered + b.covered, a.covered_in + b.covered_in, a.covered_out + b.covered_out, a.core + b.core,
             a.max_depth > b.max_depth ? a.max_depth : b.max_depth, a.head }; } };

// ---------------------------------------------------------------- element-wise kernels
// members per label: the lanes of a wave that hold the same label add once
__global__ __launch_bounds__(TPB) void k_label_hist(const int32_t* __restrict__ label, int64_t n, unsigned long long* size) {
    const int lane = threadIdx.x & (WAVE - 1);
    for (int64_t base = (int64_t)blockIdx.x * TPB; base < n; base += (int64_t)gridDim.x * TPB) {
        const int64_t i = base + threadIdx.x;
        bool live = i < n;
        const int32_t g = live ? label[i] : -1;
        unsigned long long todo = __ballot(live);
        while (todo) {                      // (todo is the same in every lane)
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t lg = __shfl(g, leader, WAVE);
            const unsigned long long same = __ballot(live && g == lg);
            if (lane == leader) atomicAdd(&size[lg], (unsigned long long)__popcll(same));
            if (g == lg) live = false;
            todo &= ~same;
        }
    }
}
// the (q, r) key of the rows in qstart order; a self row gets `self`, above every other key
__global__ __launch_bounds__(TPB) void k_pair_keys(const uint32_t* __restrict__ order, const uint32_t* __restrict__ q, const uint32_t* __restrict__ r,
                                                   int64_t n, unsigned r_bits, uint64_t self, uint64_t* key) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint32_t i = order[j];
        key[j] = q[i] == r[i] ? self : ((uint64_t)q[i] << r_bits) | r[i];
    }
}
__global__ __launch_bounds__(TPB) void k_gather_rows(const uint32_t* __restrict__ order, const int32_t* __restrict__ qs, const int32_t* __restrict__ qe,
                                                     int64_t n, int32_t* sqs, int32_t* sqe) {
    for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < n; j += (int64_t)gridDim.x * TPB) {
        const uint32_t i = order[j];
        sqs[j] = qs[i]; sqe[j] = qe[i];
    }
}
// segments per object: the leading zero-depth run unless a breakpoint sits at 0, and the starts among its breakpoints
__global__ __launch_bounds__(TPB) void k_object_segments(const int32_t* __restrict__ len, const uint8_t* __restrict__ at0, const int64_t* __restrict__ first,
                                                         const int64_t* __restrict__ last, int64_t n, int64_t* n_seg) {
    for (int64_t o = (int64_t)blockIdx.x * TPB + threadIdx.x; o < n; o += (int64_t)gridDim.x * TPB)
        n_seg[o] = (len[o] > 0 && !at0[o] ? 1 : 0) + (last[o] - first[o]);
}
__global__ __launch_bounds__(TPB) void k_lead_segments(const int32_t* __restrict__ len, const uint8_t* __restrict__ at0, const int64_t* __restrict__ seg_beg,
                                                       int64_t n, vg_cover_segment* seg) {
    for (int64_t o = (int64_t)blockIdx.x * TPB + threadIdx.x; o < n; o += (int64_t)gridDim.x * TPB)
        if (len[o] > 0 && !at0[o]) seg[seg_beg[o]] = vg_cover_segment{ (int32_t)o, 0, 0, 0, 0 };
}
__device__ __forceinline__ bool starts_segment(int64_t delta, int64_t pos, int32_t len) { return delta != 0 && pos < len; }
__global__ __launch_bounds__(TPB) void k_break_segments(const uint64_t* __restrict__ ukey, const int64_t* __restrict__ udelta, const int64_t* __restrict__ depth,
                                                        const int64_t* __restrict__ starts_before, int64_t n_breaks, unsigned pos_bits,
                                                        const int32_t* __restrict__ len, const uint8_t* __restrict__ at0, const int64_t* __restrict__ first,
                                                        const int64_t* __restrict__ seg_beg, vg_cover_segment* seg) {
    for (int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x; k < n_breaks; k += (int64_t)gridDim.x * TPB) {
        const int64_t o = (int64_t)(ukey[k] >> pos_bits), pos = (int64_t)(ukey[k] & ((1ull << pos_bits) - 1));
        if (!starts_segment(udelta[k], pos, len[o])) continue;
        const int64_t slot = seg_beg[o] + (at0[o] ? 0 : 1) + (starts_before[k] - first[o]);
        seg[slot] = vg_cover_segment{ (int32_t)o, (int32_t)pos, 0, (int32_t)(depth[k] & 0xffffffffll), (int32_t)(depth[k] >> 32) };
    }
}


// what the host has checked and counted
struct cover_input {
    int64_t n; const int32_t* len; const int32_t* label; int64_t n_groups; int64_t max_len;
    const uint32_t* q; const uint32_t* r; const int32_t* qs; const int32_t* qe; int64_t n_rows, n_kept;
};

void cover_on_device(const cover_input& in, vg_cover_stat* out, vg_cover_segment** segments, int64_t* n_segments, vg_cover_run_stats& st) {
    hipStream_t s = vg_stream();
    const int64_t n = in.n, R = in.n_rows, K = in.n_kept;
    // (q, r) keys: r below q; positions up to max_len (a breakpoint at len is legal) below the object in an event key
    const unsigned r_bits = bit_width((uint64_t)(n - 1), 1), q_bits = bit_width((uint64_t)n, 1), pos_bits = bit_width((uint64_t)in.max_len, 1);
    const uint64_t pos_mask = (1ull << pos_bits) - 1, r_mask = (1ull << r_bits) - 1;

    dbuf<int32_t> len((size_t)n), label((size_t)n);
    dbuf<unsigned long long> group_size((size_t)in.n_groups);
    dbuf<merge_acc> obj_first((size_t)n), obj_last((size_t)n);           // the merge scan in front of and behind every object's rows
    dbuf<int64_t> brk_first((size_t)n), brk_last((size_t)n), n_seg((size_t)n), seg_beg((size_t)n), total(1);
    dbuf<uint8_t> at0((size_t)n);                                         // the object has a breakpoint at position 0
    dbuf<vg_cover_stat> d_out((size_t)n);
    len.upload(in.len, (size_t)n, s);
    if (in.label) label.upload(in.label, (size_t)n, s); else label.zero(s);
    group_size.zero(s); obj_first.zero(s); obj_last.zero(s); brk_first.zero(s); brk_last.zero(s); at0.zero(s); d_out.zero(s); total.zero(s);
    const int32_t* d_len = len.p; const int32_t* d_label = label.p;

    dbuf<uint64_t> ukey; dbuf<int64_t> udelta;                            // the breakpoints: (object, pos) ascending, net packed delta
    int64_t n_breaks = 0;
    if (K > 0) {
        dbuf<uint64_t> skey((size_t)R); dbuf<int32_t> sqs((size_t)K), sqe((size_t)K);     // the kept rows by (q, r, qstart)
        {
            vg_prof_scope ps("cover_sort", (double)R * (16.0 + 2.0 * 8.0 * 2.0 + 2.0 * 12.0 * 2.0 + 24.0));
            dbuf<uint32_t> q((size_t)R), r((size_t)R); dbuf<int32_t> qs((size_t)R), qe((size_t)R);
            q.upload(in.q, (size_t)R, s); r.upload(in.r, (size_t)R, s); qs.upload(in.qs, (size_t)R, s); qe.upload(in.qe, (size_t)R, s);
            dbuf<uint32_t> by_start((size_t)R), order((size_t)R);
            {
                dbuf<uint32_t> iota((size_t)R), start_sorted((size_t)R);
                hipLaunchKernelGGL(k_iota, dim3(blocks(R)), dim3(TPB), 0, s, iota.p, R);
                sort_pairs((const uint32_t*)qs.p, start_sorted.p, (const uint32_t*)iota.p, by_start.p, R, pos_bits, s);
            }
            dbuf<uint64_t> key((size_t)R);
            hipLaunchKernelGGL(k_pair_keys, dim3(blocks(R)), dim3(TPB), 0, s, (const uint32_t*)by_start.p, (const uint32_t*)q.p, (const uint32_t*)r.p, R, r_bits,
                               (uint64_t)n << r_bits, key.p);
            sort_pairs((const uint64_t*)key.p, skey.p, (const uint32_t*)by_start.p, order.p, R, r_bits + q_bits, s);
            hipLaunchKernelGGL(k_gather_rows, dim3(blocks(K)), dim3(TPB), 0, s, (const uint32_t*)order.p, (const int32_t*)qs.p, (const int32_t*)qe.p, K, sqs.p, sqe.p);
            VG_HIP(hipGetLastError());
        }
        const uint64_t* d_key = skey.p; const int32_t* d_qs = sqs.p; const int32_t* d_qe = sqe.p;
        dbuf<uint64_t> ekey((size_t)(2 * K)); dbuf<int64_t> edelta((size_t)(2 * K));      // two events per interval, at most per row
        {
            vg_prof_scope ps("cover_merge", (double)K * (2.0 * 16.0 + 5.0 + 2.0 * 21.0 + 32.0));
            dbuf<int32_t> reach((size_t)K); dbuf<uint8_t> head((size_t)K);               // the running maximum of qend; the row opens an interval
            int32_t* d_reach = reach.p; uint8_t* d_head = head.p;
            scan_tiles(K, seg_max{ INT_MIN, 0 }, seg_max_op(),
                [=] __device__(int64_t i) { return seg_max{ d_qe[i], (uint32_t)(i == 0 || d_key[i] != d_key[i - 1]) }; },
                [=] __device__(int64_t i, const seg_max& inc, const seg_max& ex) {
                    d_reach[i] = inc.mx;
                    d_head[i] = (uint8_t)(i == 0 || d_key[i] != d_key[i - 1] || d_qs[i] > ex.mx + 1);       // (touching rows are one interval)
                }, s);
            uint64_t* d_ekey = ekey.p; int64_t* d_edelta = edelta.p; merge_acc* d_first = obj_first.p; merge_acc* d_last = obj_last.p; int64_t* d_total = total.p;
            auto row = [=] __device__(int64_t i, bool& in_group, bool& run_head, bool& opens, bool& closes) {
                const uint64_t key = d_key[i];
                in_group = d_label[key >> r_bits] == d_label[key & r_mask];
                run_head = i == 0 || d_key[i - 1] != key;
                opens = d_head[i] != 0;
                closes = i == K - 1 || d_head[i + 1] != 0;
            };
            scan_tiles(K, merge_acc{ 0, 0, 0, 0 }, merge_op(),
                [=] __device__(int64_t i) {
                    bool in_group, run_head, opens, closes;
                    row(i, in_group, run_head, opens, closes);
                    const int64_t covered = (closes ? (int64_t)d_reach[i] + 1 : 0) - (opens ? (int64_t)d_qs[i] : 0);
                    return merge_acc{ run_head ? (in_group ? 1ll : 1ll << 32) : 0ll, in_group ? covered : 0ll, in_group ? 0ll : covered, opens ? 1ll : 0ll };
                },
                [=] __device__(int64_t i, const merge_acc& inc, const merge_acc& ex) {
                    bool in_group, run_head, opens, closes;
                    row(i, in_group, run_head, opens, closes);
                    const uint64_t q = d_key[i] >> r_bits;
                    const int64_t delta = in_group ? 1ll : 1ll << 32;
                    if (opens) { d_ekey[2 * ex.n_int] = (q << pos_bits) | (uint64_t)d_qs[i]; d_edelta[2 * ex.n_int] = delta; }
                    if (closes) { d_ekey[2 * inc.n_int - 1] = (q << pos_bits) | (uint64_t)(d_reach[i] + 1); d_edelta[2 * inc.n_int - 1] = -delta; }
                    if (i == 0 || (d_key[i - 1] >> r_bits) != q) d_first[q] = ex;
                    if (i == K - 1 || (d_key[i + 1] >> r_bits) != q) d_last[q] = inc;
                    if (i == K - 1) *d_total = inc.n_int;
                }, s);
            st.intervals = read_back(total.p, s);
        }
        skey.release(); sqs.release(); sqe.release();                    // (the events carry all that is left of the rows)
        const int64_t n_events = 2 * st.intervals;
        {
            vg_prof_scope ps("cover_events", (double)n_events * (2.0 * 16.0 * 2.0 + 32.0));
            dbuf<uint64_t> ekey2((size_t)n_events); dbuf<int64_t> edelta2((size_t)n_events);
            sort_pairs((const uint64_t*)ekey.p, ekey2.p, (const int64_t*)edelta.p, edelta2.p, n_events, pos_bits + r_bits, s);
            with_temp_storage([&](void* tmp, size_t& tb) {
                return rocprim::reduce_by_key(tmp, tb, (const uint64_t*)ekey2.p, (const int64_t*)edelta2.p, (size_t)n_events, ekey.p, edelta.p, total.p,
                                              rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), s); });
            n_breaks = read_back(total.p, s);
        }
        ukey = std::move(ekey); udelta = std::move(edelta);
    }
    st.rows_kept = K; st.breakpoints = n_breaks;

    dbuf<int64_t> depth((size_t)n_breaks), starts_before((size_t)n_breaks);
    const uint64_t* d_ukey = ukey.p; const int64_t* d_udelta = udelta.p;
    int64_t n_seg_total = 0;
    dbuf<vg_cover_segment> seg;
    {
        vg_prof_scope ps("cover_depth", (double)n_breaks * (2.0 * 16.0 + 16.0 + 36.0 + 20.0) + (double)n * (2.0 * 8.0 + 40.0));
        int64_t* d_depth = depth.p; int64_t* d_before = starts_before.p; int64_t* d_bfirst = brk_first.p; int64_t* d_blast = brk_last.p; uint8_t* d_at0 = at0.p;
        scan_tiles(n_breaks, depth_acc{ 0, 0 }, depth_op(),
            [=] __device__(int64_t k) {
                const uint64_t key = d_ukey[k];
                return depth_acc{ d_udelta[k], starts_segment(d_udelta[k], (int64_t)(key & pos_mask), d_len[key >> pos_bits]) ? 1ll : 0ll };
            },
            [=] __device__(int64_t k, const depth_acc& inc, const depth_acc& ex) {
                const uint64_t o = d_ukey[k] >> pos_bits;
                d_depth[k] = inc.depth; d_before[k] = ex.n_start;
                if (k == 0 || (d_ukey[k - 1] >> pos_bits) != o) { d_bfirst[o] = ex.n_start; d_at0[o] = (uint8_t)((d_ukey[k] & pos_mask) == 0); }
                if (k == n_breaks - 1 || (d_ukey[k + 1] >> pos_bits) != o) d_blast[o] = inc.n_start;
            }, s);
        hipLaunchKernelGGL(k_object_segments, dim3(blocks(n)), dim3(TPB), 0, s, d_len, (const uint8_t*)at0.p, (const int64_t*)brk_first.p, (const int64_t*)brk_last.p, n, n_seg.p);
        const int64_t* d_nseg = n_seg.p; int64_t* d_beg = seg_beg.p; int64_t* d_total = total.p;
        scan_tiles(n, (int64_t)0, plus_op(), [=] __device__(int64_t o) { return d_nseg[o]; },
            [=] __device__(int64_t o, const int64_t& inc, const int64_t& ex) { d_beg[o] = ex; if (o == n - 1) *d_total = inc; }, s);
        n_seg_total = read_back(total.p, s);
        seg.alloc((size_t)n_seg_total);
        if (n_seg_total) {
            hipLaunchKernelGGL(k_lead_segments, dim3(blocks(n)), dim3(TPB), 0, s, d_len, (const uint8_t*)at0.p, (const int64_t*)seg_beg.p, n, seg.p);
            if (n_breaks)
                hipLaunchKernelGGL(k_break_segments, dim3(blocks(n_breaks)), dim3(TPB), 0, s, d_ukey, d_udelta, (const int64_t*)depth.p, (const int64_t*)starts_before.p,
                                   n_breaks, pos_bits, d_len, (const uint8_t*)at0.p, (const int64_t*)brk_first.p, (const int64_t*)seg_beg.p, seg.p);
        }
        VG_HIP(hipGetLastError());
    }
    st.segments = n_seg_total;
    {
        vg_prof_scope ps("cover_stats", (double)n_seg_total * (2.0 * 40.0 + 4.0) + (double)n * 180.0);
        hipLaunchKernelGGL(k_label_hist, dim3(blocks(n)), dim3(TPB), 0, s, d_label, n, group_size.p);
        vg_cover_segment* d_seg = seg.p; vg_cover_stat* d_rec = d_out.p;
        const unsigned long long* d_gsize = group_size.p; const merge_acc* d_first = obj_first.p; const merge_acc* d_last = obj_last.p; const int64_t* d_nseg = n_seg.p;
        const int64_t S = n_seg_total;
        auto segment_end = [=] __device__(int64_t x) { return x + 1 < S && d_seg[x + 1].object == d_seg[x].object ? d_seg[x + 1].start - 1 : d_len[d_seg[x].object] - 1; };
        scan_tiles(S, stat_acc{ 0, 0, 0, 0, 0, 0 }, stat_op(),
            [=] __device__(int64_t x) {
                const vg_cover_segment g = d_seg[x];
                const int64_t width = (int64_t)segment_end(x) - g.start + 1, members = (int64_t)d_gsize[d_label[g.object]];
                return stat_acc{ g.depth_in + g.depth_out >= 1 ? width : 0, g.depth_in >= 1 ? width : 0, g.depth_out >= 1 ? width : 0,
                                 members >= 2 && g.depth_in == members - 1 ? width : 0, g.depth_in + g.depth_out,
                                 (uint32_t)(x == 0 || d_seg[x - 1].object != g.object) };
            },
            [=] __device__(int64_t x, const stat_acc& inc, const stat_acc&) {
                const int32_t o = d_seg[x].object;
                d_seg[x].end = segment_end(x);                       // (no other element's load or store reads this field)
                if (x + 1 < S && d_seg[x + 1].object == o) return;
                const merge_acc a = d_first[o], b = d_last[o];
                const int64_t partners = b.partners - a.partners;
                d_rec[o] = vg_cover_stat{ d_len[o], partners & 0xffffffffll, partners >> 32, inc.covered, inc.covered_in, inc.covered_out, inc.core,
                                          b.sum_in - a.sum_in, b.sum_out - a.sum_out, inc.max_depth, d_nseg[o] };
            }, s);
    }
    d_out.download(out, (size_t)n, s);
    if (segments) {
        vg_cover_segment* h = (vg_cover_segment*)malloc(sizeof(vg_cover_segment) * (size_t)std::max<int64_t>(1, n_seg_total));
        if (!h) throw vg_error(VG_ENOMEM, "out of host memory");
        struct guard { void* p; ~guard() { free(p); } } g{ h };
        if (n_seg_total) seg.download(h, (size_t)n_seg_total, s);
        VG_HIP(hipStreamSynchronize(s));
        g.p = nullptr;
        *segments = h; *n_segments = n_seg_total;
    }
    VG_HIP(hipStreamSynchronize(s));
}

// the smallest i in [0, n) with bad(i), or -1 (the chunks of the host threads each stop at their first)
template <class Bad> int64_t first_bad(int64_t n, Bad bad) {
    const int n_thr = vg_host_threads();
    std::vector<int64_t> found((size_t)std::max(1, n_thr), -1);
    vg_parallel_chunks(n, n_thr, [&](int64_t lo, int64_t hi, int t) {
        for (int64_t i = lo; i < hi; ++i) if (bad(i)) { found[(size_t)t] = i; return; }
    });
    for (const int64_t k : found) if (k >= 0) return k;
    return -1;
}
}  // namespace

extern "C" int vg_cover_rows(int64_t n_objects, const int64_t* len, const int32_t* label, int64_t n_groups, const uint32_t* q, const uint32_t* r,
                             const int32_t* qstart, const int32_t* qend, int64_t n_rows, vg_cover_stat* out, vg_cover_segment** segments,
                             int64_t* n_segments, vg_cover_run_stats* st) {
    VG_API_BEGIN
    const std::string fn = "vg_cover_rows: ";
    if (n_objects < 0 || n_rows < 0) throw vg_error(VG_EINVAL, fn + "negative count");
    if (n_objects >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, fn + "2^31 or more objects");
    if (n_rows >= (1LL << 32)) throw vg_error(VG_EOVERFLOW, fn + "2^32 or more rows");
    if ((segments == nullptr) != (n_segments == nullptr)) throw vg_error(VG_EINVAL, fn + "segments and n_segments go together (both or neither)");
    if ((n_objects && (!len || !out)) || (n_rows && (!q || !r || !qstart || !qend))) throw vg_error(VG_EINVAL, fn + "null argument");
    if (label && (n_groups < 1 || n_groups >= (1LL << 31)) && n_objects) throw vg_error(VG_EINVAL, fn + "n_groups = " + std::to_string(n_groups) + " outside 1..2^31-1");
    const int64_t n = n_objects;
    int64_t bad = first_bad(n, [&](int64_t i) { return len[i] < 0 || len[i] >= (1LL << 31); });
    if (bad >= 0) throw vg_error(VG_EINVAL, fn + "len[" + std::to_string(bad) + "] = " + std::to_string(len[bad]) + (len[bad] < 0 ? " is negative" : " is 2^31 or more"));
    if (label) {
        bad = first_bad(n, [&](int64_t i) { return label[i] < 0 || label[i] >= n_groups; });
        if (bad >= 0) throw vg_error(VG_EINVAL, fn + "label[" + std::to_string(bad) + "] = " + std::to_string(label[bad]) + " outside 0.." + std::to_string(n_groups - 1));
    }
    bad = first_bad(n_rows, [&](int64_t i) { return q[i] >= (uint64_t)n || r[i] >= (uint64_t)n || qstart[i] < 0 || qstart[i] > qend[i] || qend[i] >= len[q[i]]; });
    if (bad >= 0) {
        const std::string row = fn + "row " + std::to_string(bad) + ": ";
        if (q[bad] >= (uint64_t)n || r[bad] >= (uint64_t)n)
            throw vg_error(VG_EINVAL, row + "index " + std::to_string(q[bad] >= (uint64_t)n ? q[bad] : r[bad]) + " outside 0.." + std::to_string(n - 1));
        if (qstart[bad] < 0) throw vg_error(VG_EINVAL, row + "qstart " + std::to_string(qstart[bad]) + " is negative");
        if (qstart[bad] > qend[bad]) throw vg_error(VG_EINVAL, row + "qstart " + std::to_string(qstart[bad]) + " > qend " + std::to_string(qend[bad]));
        throw vg_error(VG_EINVAL, row + "qend " + std::to_string(qend[bad]) + " >= len[" + std::to_string(q[bad]) + "] = " + std::to_string(len[q[bad]]));
    }
    vg_cover_run_stats local{};
    if (segments) { *segments = nullptr; *n_segments = 0; }
    if (n == 0) {
        if (st) *st = local;
        return VG_OK;
    }
    vg_require_device();
    std::vector<int32_t> len32((size_t)n);
    int64_t max_len = 0;
    for (int64_t i = 0; i < n; ++i) { len32[(size_t)i] = (int32_t)len[i]; max_len = std::max(max_len, len[i]); }
    int64_t n_self = 0;
    for (int64_t i = 0; i < n_rows; ++i) n_self += q[i] == r[i];
    const cover_input in{ n, len32.data(), label, label ? n_groups : 1, max_len, q, r, qstart, qend, n_rows, n_rows - n_self };
    cover_on_device(in, out, segments, n_segments, local);
    if (st) *st = local;
    VG_API_END
}
