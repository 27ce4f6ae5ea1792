// vg_common.h — shared host-side declarations of libvclust_gpu (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdlib>
#include <stdint.h>
#include <string>
#include <string_view>
#include <atomic>
#include <algorithm>
#include <functional>
#include <vector>
#include <stdexcept>
#include <thread>
#include <exception>
#include <memory>
#include "../../include/vclust_gpu.h"

// ---------------------------------------------------------------- errors
void vg_set_error(const char* fmt, ...);
struct vg_error : std::runtime_error {
    int code;
    vg_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
#define VG_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    throw vg_error(VG_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// wraps a C-ABI body: exceptions -> error code + vg_last_error()
#define VG_API_BEGIN try {
#define VG_API_END } catch (const vg_error& e) { vg_set_error("%s", e.what()); return e.code; } \
    catch (const std::bad_alloc&) { vg_set_error("out of host memory"); return VG_ENOMEM; } \
    catch (const std::exception& e) { vg_set_error("%s", e.what()); return VG_EINVAL; } \
    return VG_OK;

void vg_require_device();        // throws VG_ENODEV when no HIP device is usable
hipStream_t vg_stream();         // the library's compute stream on the current device
hipStream_t vg_side_stream();                     // a second queue of the same device (created on first use)
void* vg_dev_alloc(size_t bytes); // caching device allocator (throws vg_error)
void  vg_dev_free(void* p);
// while one lives, a failing allocation of this thread throws VG_ENOMEM at once: no trim of the cache, no wait for another
// process's memory (for buffers that are an optimisation only)
struct vg_dev_try_scope { vg_dev_try_scope(); ~vg_dev_try_scope(); };
// copies between a caller's (pageable) buffer and the device on stream s, staged through the library's pinned buffers
// (vg_core.cpp); a download of 32 KiB or more has completed when the call returns
void  vg_upload_bytes(void* dst, const void* src, size_t bytes, hipStream_t s);
void  vg_download_bytes(void* dst, const void* src, size_t bytes, hipStream_t s);
// one empty launch out of the translation unit (loads its code object): for the warm-up thread of the whole-stage calls
void  vg_warm_prefilter(hipStream_t s);
void  vg_warm_align(hipStream_t s);
void  vg_dev_trim();             // return all cached blocks to the driver
// placement trials: set the cached blocks aside (the next allocations are fresh ones beside them); then either restore them
// (the newer cache goes back to the driver) or free them
void  vg_dev_park_cache();
void  vg_dev_unpark(bool restore_parked);
size_t vg_dev_cached_bytes();
// Clean-up work that takes the address-space lock for long (unmapping GBs of FASTA): a whole-stage call parks it
// (vg_defer_mode) until the main thread sits in a long wait for the GPU (vg_deferred_start); otherwise it runs at once
// on a helper thread.
void  vg_defer_mode(bool on);
void  vg_defer(std::function<void()> fn);
void  vg_deferred_start();
// a cold one-shot call (vg_prefilter / vg_align, the CLI): the library keeps its device footprint small for its duration
// (the first use of device memory is what such a process may have to wait for, vg_core.cpp)
void  vg_one_shot_begin(); void vg_one_shot_end(); bool vg_one_shot();
struct vg_one_shot_scope { vg_one_shot_scope() { vg_one_shot_begin(); } ~vg_one_shot_scope() { vg_one_shot_end(); } };

// ---------------------------------------------------------------- device buffers
template <class T> struct dbuf {
    T* p = nullptr; size_t n = 0; bool owned = true;
    dbuf() {}
    explicit dbuf(size_t count) { alloc(count); }
    dbuf(const dbuf&) = delete; dbuf& operator=(const dbuf&) = delete;
    dbuf(dbuf&& o) noexcept : p(o.p), n(o.n), owned(o.owned) { o.p = nullptr; o.n = 0; o.owned = true; }
    dbuf& operator=(dbuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; owned = o.owned; o.p = nullptr; o.n = 0; o.owned = true; } return *this; }
    ~dbuf() { release(); }
    // blocks come from a caching allocator (vg_core.cpp): every kernel and copy of the library is
    // issued on one in-order stream, so a released block can be handed out again without a
    // device synchronisation and the hot path never calls hipMalloc/hipFree.
    void alloc(size_t count) {
        release(); n = count;
        if (count) p = (T*)vg_dev_alloc(count * sizeof(T));
    }
    void release() { if (p && owned) vg_dev_free(p); p = nullptr; n = 0; owned = true; }
    // non-owning window into another buffer (the owner must outlive it)
    void view(T* ptr, size_t count) { release(); p = ptr; n = count; owned = false; }
    size_t bytes() const { return n * sizeof(T); }
    void zero(hipStream_t s) { if (n) VG_HIP(hipMemsetAsync(p, 0, bytes(), s)); }
    void upload(const T* h, size_t count, hipStream_t s) { vg_upload_bytes(p, h, count * sizeof(T), s); }
    void download(T* h, size_t count, hipStream_t s) const { vg_download_bytes(h, p, count * sizeof(T), s); }
};

// rocPRIM's two-call convention: call(nullptr, bytes) is the size query, then the call runs with that much temporary storage
template <class F> void with_temp_storage(F call) {
    size_t tb = 0;
    VG_HIP(call((void*)nullptr, tb));
    dbuf<char> tmp(tb ? tb : 1);
    VG_HIP(call((void*)tmp.p, tb));
}
// blocks of a grid-stride launch over n items: one item per thread, at least one block and at most max_blocks
inline int grid_for(int64_t n, int block = 256, int max_blocks = 256 * 16) {
    int64_t b = (n + block - 1) / block; if (b < 1) b = 1;
    return (int)(b < max_blocks ? b : max_blocks);
}
// the smallest b >= from (at most 64) with x < 2^b: the bits of a radix sort over keys up to x
inline unsigned bit_width(uint64_t x, unsigned from) {
    unsigned b = from;
    while (b < 64 && (x >> b)) ++b;
    return b;
}
#if defined(__HIPCC__) || defined(__HIP__)
// workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() also drains the wave's global
// stores (s_waitcnt vmcnt(0)), which serialises "store the tile" with "prepare the next one"; the kernels that use
// it order nothing but LDS contents between their phases, so their stores stay in flight across the barrier.
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#endif

// ---------------------------------------------------------------- profiling (HIP events on vg_stream)
struct vg_prof_scope {
    const char* name; double bytes; hipEvent_t e0 = nullptr, e1 = nullptr; bool on; hipStream_t stream;
    vg_prof_scope(const char* name, double algorithmic_bytes = 0, hipStream_t on_stream = nullptr);   // nullptr: the library stream
    ~vg_prof_scope();
};
bool vg_profile_on();

// ---------------------------------------------------------------- genome set
// Layout (host and HBM): bases 2-bit packed, 16 per uint32 word, little end first
// (base i of the padded stream sits in word i/16, bits 2*(i%16)..+1); N mask 1 bit per base,
// 32 per word.  Every genome starts at a multiple of VG_ALIGN bases of the padded stream;
// padding bases are A with mask bit 1, and every genome is followed by at least one (a k-mer window that
// leaves its genome therefore always contains a masked base).
constexpr int64_t VG_ALIGN = 64;        // minimum alignment; the set's block size is 1 << align_shift
// std::vector storage without the value-initialising fill (resize() leaves new elements untouched):
// the 2-bit arrays of a big set are zeroed / written by many threads, not by one
template <class T> struct no_init_alloc : std::allocator<T> {
    template <class U> struct rebind { using other = no_init_alloc<U>; };
    template <class U> void construct(U* p) noexcept { ::new ((void*)p) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new ((void*)p) U(std::forward<A>(a)...); }
};

inline uint64_t vg_genomes_next_uid() { static std::atomic<uint64_t> last{0}; return ++last; }
struct vg_genomes {
    int n = 0;
    int align_shift = 6;                 // genomes start at multiples of (1 << align_shift) bases
    std::vector<uint32_t> blk2g;         // block (1 << align_shift bases) -> genome id
    std::vector<std::string> names;
    std::vector<int64_t> len;        // n
    std::vector<int32_t> n_parts;    // n
    std::vector<int64_t> base_off;   // n+1, padded base offsets
    std::vector<uint8_t> has_n;      // n
    std::vector<uint32_t, no_init_alloc<uint32_t>> packed;    // base_off[n]/16 words (+ slack)
    std::vector<uint32_t, no_init_alloc<uint32_t>> nmask;     // base_off[n]/32 words (+ slack)
    // device residency
    int device = -1;
    bool device_only = false;            // a subset gathered on the device (vg_subset.hip): packed / nmask above stay empty
    dbuf<uint32_t> d_packed, d_nmask;
    mutable dbuf<uint32_t> d_planes;     // the bases once more as bit planes ((lo, hi) word pair per 32 bases): what the LZ parse reads; made on first use (vg_align.hip)
    dbuf<int64_t> d_base_off, d_len;
    dbuf<uint8_t> d_has_n;
    dbuf<uint32_t> d_blk2g;
    // a device-only set is extended and truncated in place (vg_genomes_extend / vg_genomes_truncate, vg_subset.hip): its memory belongs
    // to the cap_* buffers, which may be larger than what is used, and the d_* arrays above are windows of exactly the used part
    dbuf<uint32_t> cap_packed, cap_nmask, cap_blk2g;
    dbuf<int64_t> cap_base_off, cap_len;
    dbuf<uint8_t> cap_has_n;
    uint64_t uid = vg_genomes_next_uid();       // this set among all sets the process ever made (an address comes back after a free)
    uint64_t parent_uid = 0;                    // device-only: the set it was gathered from ...
    std::vector<int32_t> parent_id;             // ... and, per genome, the id there
    int64_t padded_total() const { return base_off.empty() ? 0 : base_off.back(); }
    // L1 order (stable sort by length, descending), computed once: order[rank] = input id, rank[id]
    mutable std::vector<int32_t> len_order, len_rank;
};
// The layout rule, stated once (the loaders of vg_genomes.cpp, the device-only sets of vg_subset.hip).  A genome of len bases takes
// its length rounded up to the set's block with at least one masked base behind it: no k-mer window reaches the next genome.
inline int64_t vg_padded_len(int64_t len, int align_shift) { const int64_t al = 1LL << align_shift; return (len / al + 1) * al; }
// genome g->n (the caller counts it) of len bases appended to the layout: its blk2g run and the next base_off; returns its offset
inline int64_t vg_layout_append(vg_genomes* g, int64_t len) {
    if (g->base_off.empty()) g->base_off.push_back(0);
    const int64_t off = g->base_off.back(), padded = vg_padded_len(len, g->align_shift);
    g->blk2g.insert(g->blk2g.end(), (size_t)(padded >> g->align_shift), (uint32_t)g->n);
    g->base_off.push_back(off + padded);
    return off;
}
// the layout closed: the entry behind the last block, which a kernel that reads a few words past the last genome looks up
inline void vg_layout_close(vg_genomes* g) { g->blk2g.push_back(g->n > 0 ? (uint32_t)(g->n - 1) : 0u); }
void vg_length_order(const vg_genomes* g);        // fills g->len_order / g->len_rank on first use
int  vg_align_tasks_perm(const vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs, vg_task** tasks, int64_t* n_tasks, uint32_t* perm /* n_pairs entries, or null */);
const uint32_t* vg_genome_planes(const vg_genomes* g, hipStream_t s);   // g->d_planes, made from the resident 2-bit codes on first use (queued on s; vg_align.hip)
void vg_lz_drop_prepared(const vg_genomes* g);    // forget the index plan vg_lz_prepare left for g (nullptr: whatever it left)

// vg_genomes_load with the upload to the library's device overlapped with the packing (vg_genomes.cpp; whole-stage calls)
int vg_genomes_load_resident(const char* const* paths, int n_paths, int multisample, int n_threads, vg_genomes** out);
int vg_genomes_load_db_new_resident(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, int multisample,
                                    int n_threads, vg_genomes** out, int* n_db_genomes);      // (the same for vg_genomes_load_db_new)
// RANGE shards held by several ranks (vg_prefilter.hip, k_slice_scan): every rank scans 1/world of the BASES and the kept
// masks + level-1 counts of each rank's digit range travel to it.  The exchange is an all-to-all of device memory:
// for every part, block d of `send` (bytes send_off[d] .. send_off[d + 1]) goes to rank d and block s of `recv` (bytes
// recv_off[s] .. recv_off[s + 1]) arrives from rank s.  `status` is the caller's status so far: the implementation
// agrees on it with all ranks BEFORE anything travels and throws on every rank when one of them failed.
struct vg_xpart { const void* send; const int64_t* send_off; void* recv; const int64_t* recv_off; };
struct vg_slice_exchange {
    int rank = 0, world = 1;
    bool emulate = false;       // developer / tests: no peers -- their slices are scanned by this process (one GPU stands in for `world`)
    std::function<void(int status, const vg_xpart* parts, int n_parts)> alltoallv;
};
// whether a shard pass of (g, k, fraction) over `world` ranks takes the sliced scan: a pure function of its arguments
bool vg_slice_exchange_applies(const vg_genomes* g, int k, double fraction, int world);
int vg_kmer_shard_mode(const vg_genomes* g, double fraction, int n_shards);      // 1 = RANGE shards, 2 = HASH shards (what a rank of an n_shards-way call would do)
// one k-mer range shard of vg_kmer_shared with the (a, b, shared) records left in HBM (vg_prefilter.hip; used by vg_dist.hip)
void vg_kmer_shared_device(vg_genomes* g, int k, double fraction, int shard, int n_shards, uint32_t min_shared,
                           int64_t* set_sizes, dbuf<vg_pair_count>& pairs, int64_t* n_pairs, vg_slice_exchange* xs = nullptr,
                           int* mode_out = nullptr /* how the k-mers were cut: 1 = RANGE shards, 2 = HASH shards */);

// ---------------------------------------------------------------- host threads
// fn(lo, hi, t) over [0, n) cut into contiguous chunks, one per thread (the library's host loops over
// 10^5..10^6 pairs / tasks: a few threads are enough; an exception in a chunk is rethrown on the caller)
int vg_host_threads();
const char* vg_dev_getenv(const char* name);      // a developer switch: read only when VG_DEV_SWITCHES=1 is set
// developer aid: with VG_HOST_TRACE=1 prints the wall time since the previous mark (host-side phases of a call)
void vg_host_mark(const char* what);
double vg_alloc_wait_ms();            // wall time this process has spent inside the driver's device-allocation calls
template <class F> void vg_parallel_chunks(int64_t n, int n_thr, F fn);
// fn(i) for every i in [0, n): the items are handed out by a shared counter to n_threads threads, the caller one of them (work
// items of uneven cost; at most n threads).  Every thread is joined; an exception ends the hand-out, and the first one (by
// thread index) is rethrown on the caller.
template <class F> void vg_parallel_for(int64_t n, int n_threads, F fn);
// the file `path` made of `parts` in order; closed on every way out, VG_EIO "cannot write <path>" / "write error on <path>" (vg_io.cpp)
void vg_write_file(const char* path, const std::vector<std::string_view>& parts);
// append one genome given codes (0..3, >3 = N); used by the FASTA reader and vg_genomes_from_codes
void vg_genomes_append(vg_genomes* g, const std::string& name, const uint8_t* codes, int64_t len, int n_parts);
void vg_genomes_finish(vg_genomes* g);
// block size for a set of n genomes with total_len bases: ~mean/16, power of two in [64, 4096]
int vg_choose_align_shift(int64_t total_len, int64_t n);

// ---------------------------------------------------------------- host-side helpers shared by writers
int  vg_fmt_num(double x, char* buf);                 // LZ-ANI number format
int  vg_fmt_len_ratio(int64_t a, int64_t b, char* buf);
double vg_ani_shorter(int64_t shared, int64_t na, int64_t nb, int k);
// One row of ani.tsv as numbers (vg_io.cpp).  vg_ani_row_values: what vg_write_ani computes for the task (q, r) from the integers of
// the task (x) and of its reverse (rev) and the two lengths.  vg_ani_row_printed: those values as a reader of the file gets them --
// each through the writer's formatter and the cluster parser's from_chars.  vg_cluster_row_passes: the filters of
// vg_cluster_read_rows on such a row (minimums > 0 hold with >=, num_alns <= the maximum when that is > 0); *w = the metric's value.
struct vg_ani_row { double tani, gani, ani, qcov, rcov, len_ratio; uint32_t num_alns; };
void vg_ani_row_values(int64_t lq, int64_t lr, const vg_pair_stat& x, const vg_pair_stat& rev, vg_ani_row& row);
void vg_ani_row_printed(int64_t lq, int64_t lr, const vg_ani_row& row, vg_ani_row& printed);
bool vg_cluster_row_passes(const vg_cluster_params* p, const vg_ani_row& printed, double* w);
// the records of FASTA files as the deduplicate stage reads them, and `which` of them written verbatim, in that order (vg_io.cpp)
struct vg_fasta_text;
void vg_fasta_write_records(const char* path, const vg_fasta_text& text, const std::vector<int64_t>& which);
// the deduplicate stage's output (vg_io.cpp): the records with rep[i] == i, each header behind its file's prefix, in input order; level 0
// = plain, 1..9 = gzip members of 4 MiB of text compressed on n_threads threads (the bytes do not depend on n_threads)
void vg_fasta_write_kept(const char* path, const vg_fasta_text& in, const std::vector<std::string>& prefix, const int32_t* rep, int level, int n_threads);
// cluster stage (vg_io.cpp): the first column of the ids file; the passing rows of ani.tsv (VG_EINVAL with file:line on a
// missing column, an index outside the ids file or a malformed number); clusters.tsv
// (seq_len, if given: also the column of that header name, one non-negative integer below 2^31 per id; VG_EINVAL with file:line)
void vg_cluster_read_ids(const char* path, std::vector<std::string>& ids, std::vector<int64_t>* seq_len = nullptr);
void vg_cluster_read_rows(const char* path, int64_t n_objects, const vg_cluster_params* p,
                          std::vector<uint32_t>& q, std::vector<uint32_t>& r, std::vector<double>& w);
void vg_cluster_write(const char* path, const std::vector<std::string>& ids, const int32_t* label, const int32_t* rep, bool representatives);
// a prior clusters.tsv against the ids (vg_io.cpp): prior_rep[i] = -1 for an object without a line, else the index of its cluster's
// representative -- the earliest member of the cluster number, or (is_repr) the object named in column 2; VG_EINVAL with file:line
void vg_cluster_read_prior(const char* path, const std::vector<std::string>& ids, bool is_repr, std::vector<int32_t>& prior_rep);
// cluster report.  The label columns of a clusters.tsv against the ids (vg_io.cpp): every id exactly once, a label a non-negative
// integer or (is_repr) the id of a member of its cluster; VG_EINVAL with file:line.  The clusters of a column are numbered 0.. by
// their earliest member: label[c][i] is that number, text[c][k] the label of cluster k as the file writes it.
struct vg_label_columns { std::vector<std::string> names; std::vector<std::vector<int32_t>> label; std::vector<std::vector<std::string>> text; };
void vg_cluster_read_columns(const char* path, const std::vector<std::string>& ids, bool is_repr, vg_label_columns& out);
// the records of n_cols labellings of one graph (vg_cluster.hip): host checks (errors name fn), one graph build, three passes per
// labelling; own_max / other_max / other (each may be null) are the per-object values of labelling 0
void vg_cluster_stats_run(const char* fn, int64_t n, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows, int n_cols,
                          const int32_t* const* label, const int64_t* n_clusters, vg_cluster_stat* const* out, uint64_t* own_max,
                          uint64_t* other_max, int32_t* other);
// the report file (vg_io.cpp): one block per column, one line per cluster in the order of the records (by earliest member)
void vg_cluster_stats_write(const char* path, const char* metric, const std::vector<std::string>& ids, const vg_label_columns& cols,
                            const std::vector<std::vector<vg_cluster_stat>>& stats);
// coverage stage (vg_io.cpp).  The alignment table against the ids: the columns query, reference, qstart, qend by header name, names
// matched to ids, positions 1-based inclusive in the file and 0-based in the arrays; VG_EINVAL with file:line on a missing column,
// an unknown name, a malformed number or a range outside 1..len.  The rows are in file order whatever n_threads is.  nm (the painting
// stage): also the column nt_match into *nm, after the checks alnlen == qend - qstart + 1, nt_match <= alnlen and, if the table has
// the column, nt_match + nt_mismatch == alnlen.
void vg_cover_read_rows(const char* path, const std::vector<std::string>& ids, const std::vector<int64_t>& len, int n_threads,
                        std::vector<uint32_t>& q, std::vector<uint32_t>& r, std::vector<int32_t>& qs, std::vector<int32_t>& qe,
                        std::vector<int32_t>* nm = nullptr);
// the per-object summary (group / group_text null: one group, printed `-`; group_size per group) and the depth profile
void vg_cover_write(const char* path, const std::vector<std::string>& ids, const int32_t* group, const std::vector<std::string>* group_text,
                    const std::vector<int64_t>& group_size, const vg_cover_stat* stats, int n_threads);
void vg_cover_write_segments(const char* path, const std::vector<std::string>& ids, const vg_cover_segment* seg, int64_t n_segments, int n_threads);
// painting stage (vg_io.cpp): the per-object summary (group / group_text null: printed `-`), the segments with the pident of their
// winning row, and the donor table with painted / len[object]
void vg_paint_write(const char* path, const std::vector<std::string>& ids, const int32_t* group, const std::vector<std::string>* group_text,
                    const vg_paint_stat* stats, int n_threads);
void vg_paint_write_segments(const char* path, const std::vector<std::string>& ids, const vg_paint_segment* seg, int64_t n_segments, int n_threads);
void vg_paint_write_donors(const char* path, const std::vector<std::string>& ids, const std::vector<int64_t>& len, const vg_paint_donor* donor, int64_t n_donors,
                           int n_threads);
// merge table (vg_cluster.hip): the forest edges of the rows in merge order (a < b, weights non-increasing) -- checks the rows
// (errors name fn), then the device; the node numbering of the table and the labels of a cut are host loops over those records.
// algorithm: VG_CLUSTER_SINGLE (the maximum spanning forest), VG_CLUSTER_COMPLETE (the worst edge of every complete-linkage merge)
// or VG_CLUSTER_AVERAGE: (a, b) are the two cluster ids merged, w the rounded average, and sum / pairs hold the exact (S, P) of every
// record (empty for the other two); floor is read by VG_CLUSTER_AVERAGE alone, which also wants every weight in [0, 1]
struct vg_forest { std::vector<int32_t> a, b; std::vector<double> w; std::vector<uint64_t> sum, pairs; vg_linkage_stats stats{}; };
void vg_cluster_forest(const char* fn, int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows, vg_forest& f,
                       int algorithm = VG_CLUSTER_SINGLE, double floor = 0.0);
void vg_forest_table(int64_t n, const vg_forest& f, int64_t* node_a, int64_t* node_b, int64_t* size);
void vg_forest_cut(int64_t n, const vg_forest& f, double level, int32_t* label, int32_t* rep);
// clusters.tsv with further columns (vg_io.cpp): column c has the header names[c] and the labels / representatives label[c], rep[c]
void vg_cluster_write_columns(const char* path, const std::vector<std::string>& ids, const std::vector<std::string>& names,
                              const std::vector<const int32_t*>& label, const std::vector<const int32_t*>& rep, bool representatives);
void vg_linkage_write(const char* path, const vg_forest& f, const int64_t* node_a, const int64_t* node_b, const int64_t* size);

// deduplicate stage (vg_genomes.cpp): the input files whole in memory (plain files mapped, gzip / BGZF inflated) and every
// record in command-line and file order; a record is its header line [hdr, hdr_end) without '>' and its sequence lines [seq, end)
struct vg_fasta_rec { const char* hdr; const char* hdr_end; const char* seq; const char* end; int file; };
struct vg_fasta_text {
    std::shared_ptr<void> bufs;                 // owns the mappings / inflated text
    std::vector<const char*> file_data; std::vector<size_t> file_len;
    std::vector<vg_fasta_rec> recs;
};
void vg_fasta_read(const char* const* paths, int n_paths, int n_threads, vg_fasta_text& out);

template <class F> void vg_parallel_chunks(int64_t n, int n_thr, F fn) {
    if (n_thr < 1) n_thr = 1;
    if (n < 4096 || n_thr == 1) { fn((int64_t)0, n, 0); return; }
    std::vector<std::thread> th; std::vector<std::exception_ptr> err((size_t)n_thr);
    for (int t = 0; t < n_thr; ++t) th.emplace_back([&, t]() {
        try { fn(n * t / n_thr, n * (t + 1) / n_thr, t); } catch (...) { err[(size_t)t] = std::current_exception(); } });
    for (auto& x : th) x.join();
    for (auto& e : err) if (e) std::rethrow_exception(e);
}
template <class F> void vg_parallel_for(int64_t n, int n_threads, F fn) {
    std::atomic<int64_t> next(0);
    std::vector<std::exception_ptr> err((size_t)std::max(1, n_threads));
    auto work = [&](int t) {
        try { for (;;) { const int64_t i = next.fetch_add(1); if (i >= n) break; fn(i); } }
        catch (...) { err[(size_t)t] = std::current_exception(); next.store(n); }
    };
    std::vector<std::thread> th;
    struct joiner { std::vector<std::thread>& th; ~joiner() { for (auto& x : th) x.join(); } };
    {
        joiner j{ th };                  // (a thread that cannot be started leaves the started ones joined)
        for (int t = 1; t < std::min<int64_t>(n_threads, n); ++t) th.emplace_back(work, t);
        work(0);
    }
    for (auto& e : err) if (e) std::rethrow_exception(e);
}
