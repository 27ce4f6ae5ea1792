// vg_cluster.hip — the cluster stage on the GPU: single linkage, cd-hit, uclust, greedy set cover and Markov clustering over the edge graph
// of ani.tsv (in place of Clusty, cmd_clusty, vclust.py:1184-1278).  DESIGN.md section 9 states the contract and the design.
//   edges     rows -> both directions -> radix sort on (src, dst) -> duplicates merged to the max weight -> CSR (int64 offsets)
//   single    hook (atomicMin on the parent array) + pointer jumping, one launch each per round: label = min member
//   cd-hit /  parallel rounds over UNDECIDED -> REP | MEMBER(rep) using edges to earlier objects, then a one-workgroup
//   uclust    sweep in index order once a round decides too little
//   set-cover rounds of 2-hop local maxima of (unassigned-neighbour count, -index), then a one-workgroup greedy sweep
//   labels    min member per cluster, multi-member clusters numbered by earliest member, then singletons
//   update    a prior clustering taken as given (vg_cluster_update_graph): objects renumbered to visit ranks (prior first), rows
//             between two prior objects dropped at the emit, the states / parents seeded from the prior clusters, then the rounds,
//             the sweep and the hooking above unchanged, and the labels after mapping back
//   linkage   the single-linkage merge table: edges ranked by (w descending, a, b) with one more radix sort, Boruvka rounds on
//             the ranks (find + hook + jump + relabel), the marked forest edges compacted in rank order; node numbering on the host
//   rounds    the loop of the two contraction-based hierarchies (agglomerate): rounds that merge every pair of mutually nearest
//             clusters (find + match), one read-back, then a contraction of the cluster graph (relabel, radix sort, reduce-by-key,
//             compaction, CSR).  A linkage is a small policy struct that supplies what differs:
//   complete  the complete-linkage merge table on the ranks of the single-linkage table: the smallest rank of a row, a reduction to
//             the worst rank that keeps a cluster pair only while every object pair between the two is an edge (select); the merge
//             records go the forest's way
//   average   the average-linkage (UPGMA) merge table in exact integer arithmetic: 64-bit sums of quantised weights, candidates
//             compared as fractions (128-bit products), a reduction that adds the sums of a cluster pair
//   report    the cohesion / separation figures of a GIVEN labelling: a row pass per object, a reduction of the objects sorted by
//             label (segments inside a wave by shuffles, one atomic group per segment piece), a second row pass for the nearest cluster
//   mcl       Markov clustering in integers of 2^-30 (its own section at the end of the file): per iteration a plan pass, the row
//             expansion in an LDS hash table (a wave or a workgroup per row) with a sorted spill path, one finish for both
// Every cross-workgroup hand-off is a kernel boundary.  Inside a round, reads of other objects' state may be stale: states
// only move from UNDECIDED to final, so a stale read delays a decision and never changes one.  The sweeps are one workgroup:
// their stores are agent-scope (sc1) and drained before the barrier, their loads of state agent-scope (not L1-served).
#include "vg_common.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <type_traits>

namespace {
constexpr int32_t UND = -1;             // an undecided / unassigned object (state arrays are cleared with 0xff bytes)
constexpr int TPB = 256;
constexpr int SWEEP_TPB = 256;          // cd-hit / uclust sweep: 4 waves, two barriers per object
constexpr int SC_TPB = 1024;            // set-cover sweep: one key block per thread block of the argmax index
constexpr int SC_BLK = 1024;            // objects per block of the set-cover argmax index
constexpr int SC_DIRTY_CAP = 2048;      // dirty blocks listed per pick (more: every block is recomputed)

int grid_of(int64_t n, int cap = 8192) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + TPB - 1) / TPB, cap)); }
// bits of an object or cluster id, the sentinel n included: the low half of an edge's sort key, both halves of a contraction's
int id_bits(int64_t n) { int bits = 1; while ((1LL << bits) <= n) ++bits; return bits; }

__device__ __forceinline__ int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t ld64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one workgroup: every store / atomic this thread issued has completed before any thread of the workgroup goes on
__device__ __forceinline__ void drain_sync() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// per-thread decision counts of a grid-stride kernel -> one atomic per wave (every lane reaches this point)
__device__ __forceinline__ void add_count(unsigned long long* counter, int c) {
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(counter, (unsigned long long)c);
}
#define GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---------------------------------------------------------------- edge graph
// both directions of every row; a self row becomes two sentinel keys (src = n) that sort behind every edge.  MAPPED (the update of
// a prior clustering): both ends become visit ranks, and a row whose ends are both prior objects (rank < n_prior) is dropped the
// same way
template <bool MAPPED>
__global__ void k_emit(const uint32_t* q, const uint32_t* r, const double* w, int64_t rows, uint32_t n, const int32_t* visit, uint32_t n_prior,
                       uint64_t* keys, double* vals) {
    GRID_STRIDE(k, rows) {
        uint64_t a = q[k], b = r[k];
        bool self = a == b;
        if (MAPPED) { a = (uint64_t)visit[a]; b = (uint64_t)visit[b]; self = self || (a < n_prior && b < n_prior); }
        keys[2 * k] = self ? (uint64_t)n << 32 : a << 32 | b;
        keys[2 * k + 1] = self ? (uint64_t)n << 32 : b << 32 | a;
        vals[2 * k] = vals[2 * k + 1] = w[k];
    }
}
// CSR of the sorted unique keys: off[s] = first edge of source s (off[n] = m), adj = destinations (ascending per row)
__global__ void k_csr(const uint64_t* keys, int64_t m, int64_t n, int64_t* off, int32_t* adj) {
    GRID_STRIDE(e, m + 1) {
        const int64_t prev = e > 0 ? (int64_t)(keys[e - 1] >> 32) : -1;
        const int64_t cur = e < m ? (int64_t)(keys[e] >> 32) : n;
        for (int64_t s = prev + 1; s <= cur; ++s) off[s] = e;
        if (e < m) adj[e] = (int32_t)(uint32_t)keys[e];
    }
}
__global__ void k_iota(int32_t* a, int64_t n) { GRID_STRIDE(i, n) a[i] = (int32_t)i; }
__global__ void k_fill(int32_t* a, int64_t n, int32_t v) { GRID_STRIDE(i, n) a[i] = v; }

// ---------------------------------------------------------------- single linkage
// every undirected edge once (dst < src): hook the larger of the two roots under the smaller; parent[x] <= x always
__global__ void k_hook(const uint64_t* keys, int64_t m, int32_t* parent, int32_t* changed) {
    int c = 0;
    GRID_STRIDE(e, m) {
        const int32_t s = (int32_t)(keys[e] >> 32), d = (int32_t)(uint32_t)keys[e];
        if (d >= s) continue;
        const int32_t ps = ld(parent + s), pd = ld(parent + d);
        if (ps != pd) { atomicMin(parent + (ps > pd ? ps : pd), ps < pd ? ps : pd); c = 1; }
    }
    if (c) st(changed, 1);
}
// pointer jumping to the root (roots do not move inside the kernel; a stale read is an older ancestor)
__device__ __forceinline__ void jump_to_root(int32_t* parent, int64_t i) {
    int32_t x = ld(parent + i);
    for (;;) { const int32_t y = ld(parent + x); if (y == x) break; x = y; }
    st(parent + i, x);
}
__global__ void k_compress(int32_t* parent, int64_t n) { GRID_STRIDE(i, n) jump_to_root(parent, i); }

// ---------------------------------------------------------------- cd-hit / uclust
// state[i]: UND, i (REP) or j < i (MEMBER of REP j).  Object i looks at its earlier neighbours only (the row prefix < i).
//   cd-hit: the first REP in index order, provided every earlier neighbour before it is decided; REP when all are MEMBERs
//   uclust: the REP of highest weight (ties: earliest), provided no undecided neighbour could outrank it
__device__ __forceinline__ bool outranks(double w1, int32_t j1, double w2, int32_t j2) { return w1 > w2 || (w1 == w2 && j1 < j2); }

template <bool UCLUST>
__global__ void k_greedy_round(int64_t n, const int64_t* off, const int32_t* adj, const double* wts, int32_t* state,
                               unsigned long long* decided) {
    int c = 0;
    GRID_STRIDE(i64, n) {
        const int32_t i = (int32_t)i64;
        if (ld(state + i) != UND) continue;
        int32_t rep = -1, und = -1; double wrep = 0, wund = 0; bool wait = false;
        for (int64_t k = off[i], e = off[i + 1]; k < e; ++k) {
            const int32_t j = adj[k];
            if (j >= i) break;
            const int32_t s = ld(state + j);
            if (!UCLUST) {
                if (s == UND) { wait = true; break; }
                if (s == j) { rep = j; break; }
            } else {
                const double wj = wts[k];
                if (s == j) { if (rep < 0 || outranks(wj, j, wrep, rep)) { rep = j; wrep = wj; } }
                else if (s == UND) { if (und < 0 || outranks(wj, j, wund, und)) { und = j; wund = wj; } }
            }
        }
        if (UCLUST) wait = und >= 0 && (rep < 0 || outranks(wund, und, wrep, rep));
        if (wait) continue;
        st(state + i, rep >= 0 ? rep : i);
        ++c;
    }
    add_count(decided, c);
}

template <bool UCLUST>
__device__ __forceinline__ void wave_best(double& w, int32_t& j) {
    for (int o = 32; o > 0; o >>= 1) {
        const double w2 = __shfl_xor(w, o); const int32_t j2 = __shfl_xor(j, o);
        if (UCLUST) { if (j2 >= 0 && (j < 0 || outranks(w2, j2, w, j))) { w = w2; j = j2; } }
        else if (j2 >= 0 && (j < 0 || j2 < j)) j = j2;
    }
}
// The tail: the remaining undecided objects in index order, one at a time (every earlier object is decided by then), each
// neighbour list scanned by the whole workgroup.  One workgroup, launched once.
template <bool UCLUST>
__global__ void __launch_bounds__(SWEEP_TPB) k_greedy_sweep(int64_t n, const int64_t* off, const int32_t* adj, const double* wts,
                                                            int32_t* state, int64_t first) {
    __shared__ uint64_t und_mask[SWEEP_TPB / 64];
    __shared__ double red_w[SWEEP_TPB / 64];
    __shared__ int32_t red_j[SWEEP_TPB / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int64_t base = first; base < n; base += SWEEP_TPB) {
        const int64_t mine = base + t;
        const bool u = mine < n && ld(state + mine) == UND;
        const uint64_t bal = __ballot(u);
        if (lane == 0) und_mask[wv] = bal;
        __syncthreads();
        for (int w = 0; w < SWEEP_TPB / 64; ++w) {
            for (uint64_t bits = und_mask[w]; bits; bits &= bits - 1) {
                const int32_t i = (int32_t)(base + w * 64 + __builtin_ctzll(bits));
                double bw = 0; int32_t bj = -1;
                for (int64_t k = off[i] + t, e = off[i + 1]; k < e; k += SWEEP_TPB) {
                    const int32_t j = adj[k];
                    if (j >= i) break;
                    if (ld(state + j) != j) continue;
                    if (UCLUST) { const double wj = wts[k]; if (bj < 0 || outranks(wj, j, bw, bj)) { bw = wj; bj = j; } }
                    else if (bj < 0) bj = j;        // (ascending: this thread's first REP is its smallest)
                }
                wave_best<UCLUST>(bw, bj);
                if (lane == 0) { red_w[wv] = bw; red_j[wv] = bj; }
                __syncthreads();
                if (t == 0) {
                    for (int x = 1; x < SWEEP_TPB / 64; ++x) {
                        const int32_t j2 = red_j[x]; const double w2 = red_w[x];
                        if (UCLUST) { if (j2 >= 0 && (bj < 0 || outranks(w2, j2, bw, bj))) { bw = w2; bj = j2; } }
                        else if (j2 >= 0 && (bj < 0 || j2 < bj)) bj = j2;
                    }
                    st(state + i, bj >= 0 ? bj : i);
                }
                drain_sync();
            }
        }
        __syncthreads();      // (und_mask is rewritten by the next chunk)
    }
}

// ---------------------------------------------------------------- set cover
// key of an unassigned object: (unassigned-neighbour count, -index), packed so that a larger key wins; assigned: 0
__device__ __forceinline__ uint64_t sc_key(uint32_t cnt, int64_t i) { return (uint64_t)cnt << 32 | (uint64_t)(0xffffffffu - (uint32_t)i); }

__global__ void k_sc_key(int64_t n, const int64_t* off, const int32_t* adj, const int32_t* asg, uint64_t* key) {
    GRID_STRIDE(i, n) {
        uint64_t kv = 0;
        if (asg[i] == UND) {
            uint32_t cnt = 0;
            for (int64_t k = off[i], e = off[i + 1]; k < e; ++k) cnt += asg[adj[k]] == UND;
            kv = sc_key(cnt, i);
        }
        key[i] = kv;
    }
}
// out[i] = max over i and its neighbours (assigned objects too: 2-hop paths may pass through them)
__global__ void k_sc_max(int64_t n, const int64_t* off, const int32_t* adj, const uint64_t* in, uint64_t* out) {
    GRID_STRIDE(i, n) {
        uint64_t v = in[i];
        for (int64_t k = off[i], e = off[i + 1]; k < e; ++k) v = umax64(v, in[adj[k]]);
        out[i] = v;
    }
}
// an unassigned object whose key is the maximum within 2 hops is picked (asg = itself)
__global__ void k_sc_pick(int64_t n, const int64_t* off, const int32_t* adj, const uint64_t* key, const uint64_t* m1, int32_t* asg,
                          unsigned long long* decided) {
    int c = 0;
    GRID_STRIDE(i, n) {
        if (asg[i] != UND) continue;
        uint64_t v = m1[i];
        for (int64_t k = off[i], e = off[i + 1]; k < e; ++k) v = umax64(v, m1[adj[k]]);
        if (key[i] == v) { asg[i] = (int32_t)i; ++c; }
    }
    add_count(decided, c);
}
// an unassigned object next to a REP joins it: a REP of an earlier round has claimed all its neighbours already, and two picks
// of one round are > 2 hops apart, so at most one neighbour qualifies
__global__ void k_sc_claim(int64_t n, const int64_t* off, const int32_t* adj, int32_t* asg, unsigned long long* decided) {
    int c = 0;
    GRID_STRIDE(i, n) {
        if (ld(asg + i) != UND) continue;
        for (int64_t k = off[i], e = off[i + 1]; k < e; ++k) {
            const int32_t j = adj[k];
            if (ld(asg + j) == j) { st(asg + i, j); ++c; break; }
        }
    }
    add_count(decided, c);
}
// the argmax index of the sweep: bmax[b] = max key of objects [b * SC_BLK, (b + 1) * SC_BLK)
__device__ __forceinline__ uint64_t block_max(uint64_t v, uint64_t* red) {
    for (int o = 32; o > 0; o >>= 1) v = umax64(v, (uint64_t)__shfl_xor((unsigned long long)v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int x = 0; x < (int)(blockDim.x >> 6); ++x) v = umax64(v, red[x]);
    __syncthreads();
    return v;
}
__global__ void __launch_bounds__(SC_TPB) k_sc_block_max(int64_t n, const uint64_t* key, uint64_t* bmax) {
    __shared__ uint64_t red[SC_TPB / 64];
    const int64_t i = (int64_t)blockIdx.x * SC_BLK + threadIdx.x;
    const uint64_t v = block_max(i < n ? key[i] : 0, red);
    if (threadIdx.x == 0) bmax[blockIdx.x] = v;
}
// The tail: the sequential greedy itself.  Each step takes the global maximum key (argmax over bmax), assigns the pick and its
// unassigned neighbours, lowers the keys of their unassigned neighbours (one count each) and recomputes the blocks it touched.
__global__ void __launch_bounds__(SC_TPB) k_sc_sweep(int64_t n, int64_t nb, const int64_t* off, const int32_t* adj, int32_t* asg,
                                                     uint64_t* key, uint64_t* bmax, int32_t* dirty) {
    __shared__ uint64_t red[SC_TPB / 64];
    __shared__ int32_t dlist[SC_DIRTY_CAP];
    __shared__ int32_t dcount;
    const int t = threadIdx.x;
    auto mark = [&](int64_t obj) {
        const int32_t b = (int32_t)(obj / SC_BLK);
        if (atomicExch(dirty + b, 1) == 0) { const int32_t s = atomicAdd(&dcount, 1); if (s < SC_DIRTY_CAP) dlist[s] = b; }
    };
    for (;;) {
        uint64_t v = 0;
        for (int64_t b = t; b < nb; b += SC_TPB) v = umax64(v, ld64(bmax + b));
        const uint64_t best = block_max(v, red);
        if (best == 0) break;                                    // every object is assigned
        const int32_t p = (int32_t)(0xffffffffu - (uint32_t)best);
        if (t == 0) dcount = 0;
        __syncthreads();
        const int64_t p0 = off[p], p1 = off[p + 1];
        for (int64_t k = p0 + t; k < p1; k += SC_TPB) {
            const int32_t j = adj[k];
            if (ld(asg + j) == UND) { st(asg + j, p); st64(key + j, 0); mark(j); }
        }
        if (t == 0) { st(asg + p, p); st64(key + p, 0); mark(p); }
        drain_sync();
        for (int64_t k = p0 + t; k < p1; k += SC_TPB) {
            const int32_t x = adj[k];
            if (ld(asg + x) != p) continue;                      // (assigned before this step)
            for (int64_t kk = off[x], e = off[x + 1]; kk < e; ++kk) {
                const int32_t y = adj[kk];
                if (ld(asg + y) == UND) { atomicSub((unsigned long long*)(key + y), 1ull << 32); mark(y); }
            }
        }
        drain_sync();
        const int32_t nd = dcount;
        const bool all = nd > SC_DIRTY_CAP;
        for (int64_t d = 0, e = all ? nb : nd; d < e; ++d) {
            const int64_t b = all ? d : dlist[d];
            const int64_t i = b * SC_BLK + t;                    // (SC_BLK == SC_TPB: one key per thread)
            const uint64_t m = block_max(i < n ? ld64(key + i) : 0, red);
            if (t == 0) { st64(bmax + b, m); st(dirty + b, 0); }
        }
        drain_sync();
    }
}

// ---------------------------------------------------------------- single-linkage merge table (maximum spanning forest)
// Edge {a, b} (a < b) of weight w has the key (-w, a, b); its rank is its position in that order.  Ranks are unique, so the
// forest and everything derived from it is, whatever ties the weights have.
constexpr uint64_t NO_RANK = ~0ull;     // (rank arrays are cleared with 0xff bytes)
constexpr int ROW_LANES = 16;           // lanes that scan one object's CSR row in k_bor_find
// doubles as unsigned keys that sort ascending where the weights sort descending; -0.0 is +0.0 (NaN never gets here)
__device__ __forceinline__ uint64_t desc_key(double w) {
    uint64_t b = (uint64_t)__double_as_longlong(w + 0.0);
    b = (b >> 63) ? ~b : b | (1ull << 63);      // ascending order of the doubles
    return ~b;
}
struct forward_edge {                   // the directed edges a -> b with a < b: every undirected edge once, in (a, b) order
    const uint64_t* keys;
    __device__ bool operator()(int64_t k) const { const uint64_t x = keys[k]; return (uint32_t)(x >> 32) < (uint32_t)x; }
};
__global__ void k_rank_keys(const int64_t* pos, const double* vals, int64_t mu, uint64_t* wkey) {
    GRID_STRIDE(j, mu) wkey[j] = desc_key(vals[pos[j]]);
}
// pos[p] = the directed position of the forward edge of rank p: both directions of the edge learn the rank (the reverse one
// is found by bisection of the other end's row, which is ascending)
__global__ void k_rank_scatter(const int64_t* pos, int64_t mu, const uint64_t* keys, const int64_t* off, const int32_t* adj,
                               uint64_t* rank, int32_t* bad) {
    GRID_STRIDE(p, mu) {
        const int64_t k = pos[p];
        const int32_t a = (int32_t)(keys[k] >> 32), b = (int32_t)(uint32_t)keys[k];
        rank[k] = (uint64_t)p;
        int64_t lo = off[b], hi = off[b + 1];
        while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (adj[mid] < a) lo = mid + 1; else hi = mid; }
        if (lo < off[b + 1] && adj[lo] == a) rank[lo] = (uint64_t)p; else st(bad, 1);
    }
}
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
// Boruvka, step 1: every object (ROW_LANES lanes each) looks for its lowest-rank edge that leaves its component and hands it to
// the component's root.  comp[] is not written here.  An object without a leaving edge never gets one again (components only
// grow): it is skipped from then on.
__global__ void k_bor_find(int64_t n, const int64_t* off, const int32_t* adj, const uint64_t* rank, const int32_t* comp,
                           uint8_t* inner, unsigned long long* cmin) {
    const int lane = threadIdx.x % ROW_LANES;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / ROW_LANES;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ROW_LANES; i < n; i += groups) {
        if (inner[i]) continue;
        const int32_t c = comp[i];
        uint64_t best = NO_RANK;
        for (int64_t k = off[i] + lane, e = off[i + 1]; k < e; k += ROW_LANES)
            if (comp[adj[k]] != c) best = umin64(best, rank[k]);
        for (int o = ROW_LANES / 2; o > 0; o >>= 1) best = umin64(best, (uint64_t)__shfl_xor((unsigned long long)best, o));
        if (lane == 0) { if (best == NO_RANK) inner[i] = 1; else atomicMin(cmin + c, (unsigned long long)best); }
    }
}
// step 2: every root with a leaving edge marks it as a forest edge and hooks under the root at its other end.  Along such hooks
// the ranks of the chosen edges fall, except where two roots chose each other -- then they chose the same edge (ranks are
// unique), and the larger root hooks under the smaller.  Reads comp[] and cmin[] (fixed in this kernel), writes parent[own].
__global__ void k_bor_hook(int64_t n, const int32_t* comp, const unsigned long long* cmin, const int64_t* pos, const uint64_t* keys,
                           uint8_t* forest, int32_t* parent, unsigned long long* active) {
    int c = 0;
    GRID_STRIDE(i64, n) {
        const int32_t i = (int32_t)i64;
        if (comp[i] != i) continue;
        const uint64_t p = cmin[i];
        if (p == NO_RANK) continue;
        forest[p] = 1;
        const uint64_t key = keys[pos[p]];
        const int32_t ca = comp[(int32_t)(key >> 32)], o = ca == i ? comp[(int32_t)(uint32_t)key] : ca;
        if (!(cmin[o] == p && i < o)) parent[i] = o;
        ++c;
    }
    add_count(active, c);
}
// step 3: pointer jumping over the roots of this round (parent[] of a current root is itself; a stale read is an older ancestor)
__global__ void k_bor_jump(int64_t n, const int32_t* comp, int32_t* parent) {
    GRID_STRIDE(i, n) if (comp[i] == (int32_t)i) jump_to_root(parent, i);
}
// step 4: every root of this round now points at its final root
__global__ void k_bor_relabel(int64_t n, const int32_t* parent, int32_t* comp) { GRID_STRIDE(i, n) comp[i] = parent[comp[i]]; }
__global__ void k_forest_gather(const int64_t* frank, int64_t nf, const int64_t* pos, const uint64_t* keys, const double* vals,
                                int32_t* a, int32_t* b, double* w) {
    GRID_STRIDE(j, nf) {
        const int64_t k = pos[frank[j]];
        a[j] = (int32_t)(keys[k] >> 32); b[j] = (int32_t)(uint32_t)keys[k]; w[j] = vals[k] + 0.0;
    }
}

// ---------------------------------------------------------------- cluster graph (complete and average linkage)
// Both hierarchies run on a cluster graph: directed records (src cluster << 32 | dst cluster, value), sorted by key, with row
// offsets; a cluster's id is its minimum member; initially these are the object graph.  A round is the linkage's find + match over
// it, then a contraction whose first step is the same for both:
// every record under the new cluster ids, keyed on 2 * bits bits for the sort, its value shifted up by count_bits with a count of 1
// below it (complete linkage counts the records merged into one; average linkage has no count bits and keeps the value); the
// record of a merged pair itself becomes the sentinel (src = n) that sorts last.  One hop of parent[] is enough: the merges are a
// matching.
__global__ void k_relabel(const uint64_t* keys, const uint64_t* val, int64_t m, const int32_t* parent, int64_t n, int bits, int count_bits,
                          uint64_t* okey, uint64_t* oval) {
    GRID_STRIDE(e, m) {
        const uint64_t s = (uint64_t)parent[keys[e] >> 32], d = (uint64_t)parent[(uint32_t)keys[e]];
        okey[e] = s == d ? (uint64_t)n << bits : s << bits | d;
        oval[e] = val[e] << count_bits | (count_bits ? 1 : 0);
    }
}

// ---------------------------------------------------------------- complete linkage
// The value of a record is a rank: K of the cluster pair, the largest rank over the object edges between the two, and there is a
// record only while EVERY object pair between them is an edge.  Initially these are the ranks of the object graph.
constexpr int COUNT_BITS = 3;           // contraction: a record's value is rank << 3 | records merged into it (<= 4 per cluster pair)
// round, step 1: every cluster (ROW_LANES lanes each) finds the smallest rank of its row and the cluster at that record's other
// end.  The ranks of a row are distinct (each is another object edge), so one lane holds the minimum.  A cluster with an empty
// row is final: it only gets "no rank".  mult[] (members of the matching merged into a cluster this round) starts at 1.
__global__ void k_cl_find(int64_t n, const int64_t* off, const uint64_t* keys, const uint64_t* rank, unsigned long long* best,
                          int32_t* bdst, int32_t* mult) {
    const int lane = threadIdx.x % ROW_LANES;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / ROW_LANES;
    for (int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ROW_LANES; c < n; c += groups) {
        const int64_t lo = off[c], hi = off[c + 1];
        if (lo == hi) { if (lane == 0) { best[c] = NO_RANK; mult[c] = 1; } continue; }
        uint64_t mine = NO_RANK; int64_t at = lo;
        for (int64_t k = lo + lane; k < hi; k += ROW_LANES) { const uint64_t p = rank[k]; if (p < mine) { mine = p; at = k; } }
        uint64_t low = mine;
        for (int o = ROW_LANES / 2; o > 0; o >>= 1) low = umin64(low, (uint64_t)__shfl_xor((unsigned long long)low, o));
        if (mine == low) { best[c] = low; bdst[c] = (int32_t)(uint32_t)keys[at]; mult[c] = 1; }
    }
}
// step 2: the record (c, d), c < d, is a merge when its rank is the smallest of both rows.  Ranks are unique, so the merges of a
// round are a matching, and the smallest rank of the whole graph is always one of them.  Reads only what k_cl_find wrote; the
// merge list is filled in any order (it is sorted at the end), `total` counts the merges of all rounds so far.
__global__ void k_cl_match(int64_t n, const unsigned long long* best, const int32_t* bdst, int32_t* parent, int32_t* mult,
                           int64_t* merged, int64_t cap, unsigned long long* total) {
    GRID_STRIDE(c, n) {
        const uint64_t p = best[c];
        if (p == NO_RANK) continue;
        const int64_t d = bdst[c];
        if (d <= c || d >= n || best[d] != p) continue;
        const unsigned long long slot = atomicAdd(total, 1ull);
        if (slot < (unsigned long long)cap) merged[slot] = (int64_t)p;
        parent[d] = (int32_t)c; mult[c] = 2;
    }
}
// contraction (after k_relabel with COUNT_BITS and the sort): the reduce-by-key operator
struct max_rank_add_count {             // (rank, count) + (rank, count) of one cluster pair: the worst rank, the records seen
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
        const uint64_t ra = a >> COUNT_BITS, rb = b >> COUNT_BITS, lowbits = (1ull << COUNT_BITS) - 1;
        return (ra > rb ? ra : rb) << COUNT_BITS | (((a & lowbits) + (b & lowbits)) & lowbits);
    }
};
// step 2 (after sort and reduce-by-key): the pair (S, D) stays only if all mult(S) * mult(D) pairs of its constituents had a record
struct surviving_pair {
    const uint64_t* gkey; const uint64_t* gval; const unsigned long long* n_groups; const int32_t* mult; int64_t n; int bits;
    __device__ bool operator()(int64_t k) const {
        if ((unsigned long long)k >= *n_groups) return false;
        const uint64_t s = gkey[k] >> bits, d = gkey[k] & ((1ull << bits) - 1);
        return s < (uint64_t)n && d < (uint64_t)n && (gval[k] & ((1ull << COUNT_BITS) - 1)) == (uint64_t)(mult[s] * mult[d]);
    }
};
// step 3: the survivors, in key order, are the new records; the tail of the old list is filled with the sentinel, so that k_csr
// over the old length gives the new offsets (off[n] = the new length) without the host knowing it yet
__global__ void k_cl_compact(const int64_t* idx, const unsigned long long* m_new, int64_t m_old, const uint64_t* gkey, const uint64_t* gval,
                             int64_t n, int bits, uint64_t* keys, uint64_t* rank) {
    const int64_t mn = (int64_t)*m_new < m_old ? (int64_t)*m_new : m_old;
    GRID_STRIDE(e, m_old) {
        if (e < mn) {
            const uint64_t k = gkey[idx[e]];
            keys[e] = (k >> bits) << 32 | (k & ((1ull << bits) - 1)); rank[e] = gval[idx[e]] >> COUNT_BITS;
        } else keys[e] = (uint64_t)n << 32;
    }
}

// ---------------------------------------------------------------- average linkage (UPGMA)
// A weight w is the integer u = llrint(ldexp(w, 32)).  The cluster graph: directed records (src cluster << 32 | dst cluster, S) with
// S the sum of u over the object edges between the two clusters, sorted by key, with row offsets; size[c] = members of cluster c.
// sim(A, B) = S / (|A| |B| 2^32): a pair of objects without an edge adds nothing to S, and a cluster pair without a record is no
// candidate.  A candidate has the key (-sim, lo, hi), lo < hi the two cluster ids; no floating-point sum exists anywhere.
struct av_cand { uint64_t S, P; uint32_t lo, hi; };         // P: the object pairs |A| |B| (inside one row: the other cluster's size)
// < 0 when x has the smaller key (the larger similarity; ties: the smaller (lo, hi)), 0 for equal keys.  S1 / P1 against S2 / P2 is
// S1 * P2 against S2 * P1 in 128 bits: S < 2^64 and P < 2^64, and a 64-bit product of the two would wrap.
__host__ __device__ inline int av_compare(const av_cand& x, const av_cand& y) {
    const unsigned __int128 l = (unsigned __int128)x.S * y.P, r = (unsigned __int128)y.S * x.P;
    if (l != r) return l > r ? -1 : 1;
    if (x.lo != y.lo) return x.lo < y.lo ? -1 : 1;
    return x.hi < y.hi ? -1 : x.hi > y.hi ? 1 : 0;
}
// sim >= T / 2^32, exactly: S >= T * P (T <= 2^32 + 1 and P < 2^62: the product needs more than 64 bits)
__host__ __device__ inline bool av_reaches(uint64_t S, uint64_t P, uint64_t T) { return (unsigned __int128)S >= (unsigned __int128)T * P; }

__global__ void k_av_quantise(const double* vals, int64_t m, uint64_t* sum) { GRID_STRIDE(e, m) sum[e] = (uint64_t)llrint(ldexp(vals[e], 32)); }
// round, step 1: every cluster (ROW_LANES lanes each) finds the record of its row with the smallest key.  Inside a row the
// cluster's own size cancels: the candidates carry the other cluster's size as P.  The key order is total, so after the butterfly
// every lane of the group holds the same candidate.  A cluster with an empty row is final: it gets no destination.
__global__ void k_av_find(int64_t n, const int64_t* off, const uint64_t* keys, const uint64_t* sum, const int32_t* size,
                          unsigned long long* bsum, int32_t* bdst) {
    const int lane = threadIdx.x % ROW_LANES;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / ROW_LANES;
    for (int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ROW_LANES; c < n; c += groups) {
        const int64_t lo = off[c], hi = off[c + 1];
        if (lo == hi) { if (lane == 0) bdst[c] = UND; continue; }
        // the candidate held by this lane: (S, P = the other cluster's size, d); d == UND: none yet.  Three scalars updated by
        // selects, on purpose: as one av_cand assigned under a branch, the 64-bit P of the running best was left stale after a
        // take by the compiler (seen in the ISA and as wrong merges on the device)
        uint64_t bs = 0; uint32_t bp = 1; int32_t bd = UND;
        const uint32_t uc = (uint32_t)c;
        auto better = [&](uint64_t S2, uint32_t P2, int32_t d2) {   // is (S2, P2, d2) a candidate, with a smaller key than the lane's?
            const uint32_t u1 = (uint32_t)bd, u2 = (uint32_t)d2;
            const av_cand x{ S2, (uint64_t)P2, u2 < uc ? u2 : uc, u2 < uc ? uc : u2 }, y{ bs, (uint64_t)bp, u1 < uc ? u1 : uc, u1 < uc ? uc : u1 };
            return d2 != UND && (bd == UND || av_compare(x, y) < 0);
        };
        for (int64_t k = lo + lane; k < hi; k += ROW_LANES) {
            const int32_t d = (int32_t)(uint32_t)keys[k];
            const uint64_t S = sum[k]; const uint32_t P = (uint32_t)size[d];
            const bool take = better(S, P, d);
            bs = take ? S : bs; bp = take ? P : bp; bd = take ? d : bd;
        }
        for (int o = ROW_LANES / 2; o > 0; o >>= 1) {           // the whole candidate travels: (S, P, d)
            const uint64_t S2 = (uint64_t)__shfl_xor((unsigned long long)bs, o);
            const uint32_t P2 = __shfl_xor(bp, o);
            const int32_t d2 = __shfl_xor(bd, o);
            const bool take = better(S2, P2, d2);
            bs = take ? S2 : bs; bp = take ? P2 : bp; bd = take ? d2 : bd;
        }
        if (lane == 0) { bsum[c] = bs; bdst[c] = bd; }
    }
}
// step 2: (c, d), c < d, is a merge when each is the other's choice and sim >= floor (S >= F * P); a record of S == 0 never merges
// here (see average_linkage).  The key order is total and symmetric, so the merges of a round are a matching.  Reads only what
// k_av_find wrote, size[] (which grows in the contraction, after these reads) and, in the zero phase, the first record: then the
// one merge of the round is the record of smallest (c, d), which is keys[0].  The merge list is filled in any order.
__global__ void k_av_match(int64_t n, const unsigned long long* bsum, const int32_t* bdst, const int32_t* size, uint64_t F, int zero_phase,
                           const uint64_t* keys, int32_t* parent, uint64_t* msum, uint64_t* mpairs, int32_t* mc, int32_t* md, int64_t cap,
                           unsigned long long* total) {
    GRID_STRIDE(c, n) {
        const int64_t d = bdst[c];
        if (d <= c || d >= n || bdst[d] != (int32_t)c) continue;            // (no destination is -1)
        const uint64_t S = bsum[c], P = (uint64_t)size[c] * (uint64_t)size[d];
        if (zero_phase ? keys[0] != ((uint64_t)c << 32 | (uint64_t)d) : (S == 0 || !av_reaches(S, P, F))) continue;
        const unsigned long long slot = atomicAdd(total, 1ull);
        if (slot < (unsigned long long)cap) { msum[slot] = S; mpairs[slot] = P; mc[slot] = (int32_t)c; md[slot] = (int32_t)d; }
        parent[d] = (int32_t)c;
    }
}
// before the contraction: the merges [from, to) of this round are a matching, so every size[] entry has one writer
__global__ void k_av_grow(const int32_t* mc, const int32_t* md, int64_t from, int64_t to, int32_t* size) {
    GRID_STRIDE(j, to - from) size[mc[from + j]] += size[md[from + j]];
}
// contraction (after k_relabel without count bits, the sort and reduce-by-key with plus): the groups, in key order, are the new
// records -- all but the sentinel group, which is the last one; the tail of the old list is filled with the sentinel, so that
// k_csr over the old length gives the new offsets.  *m_new = the new length, for the round's read-back.
__global__ void k_av_compact(const unsigned long long* n_groups, int64_t m_old, const uint64_t* gkey, const uint64_t* gsum, int64_t n, int bits,
                             uint64_t* keys, uint64_t* sum, unsigned long long* m_new) {
    const int64_t ng = (int64_t)*n_groups < m_old ? (int64_t)*n_groups : m_old;
    GRID_STRIDE(e, m_old) {
        const bool live = e < ng && (gkey[e] >> bits) < (uint64_t)n;
        if (live) { keys[e] = (gkey[e] >> bits) << 32 | (gkey[e] & ((1ull << bits) - 1)); sum[e] = gsum[e]; }
        else keys[e] = (uint64_t)n << 32;
        if (e == 0) *m_new = (unsigned long long)(ng - (ng > 0 && (gkey[ng - 1] >> bits) >= (uint64_t)n ? 1 : 0));
    }
}
__global__ void k_av_order(const uint64_t* S, const uint32_t* sc, const uint32_t* sd, const uint32_t* c, const uint32_t* d, int64_t n, int8_t* out) {
    GRID_STRIDE(i, n - 1) {
        const av_cand x{ S[i], (uint64_t)sc[i] * sd[i], c[i] < d[i] ? c[i] : d[i], c[i] < d[i] ? d[i] : c[i] };
        const av_cand y{ S[i + 1], (uint64_t)sc[i + 1] * sd[i + 1], c[i + 1] < d[i + 1] ? c[i + 1] : d[i + 1], c[i + 1] < d[i + 1] ? d[i + 1] : c[i + 1] };
        out[i] = (int8_t)av_compare(x, y);
    }
}

// ---------------------------------------------------------------- labels
// every object must carry a cluster id in [0, n) before the label kernels index with it
__global__ void k_check_roots(const int32_t* root, int64_t n, int32_t* bad) { GRID_STRIDE(i, n) if ((uint32_t)root[i] >= (uint64_t)n) st(bad, 1); }
__global__ void k_min_member(const int32_t* root, int64_t n, int32_t* minm) { GRID_STRIDE(i, n) atomicMin(minm + root[i], (int32_t)i); }
__global__ void k_rep_size(const int32_t* root, const int32_t* minm, int64_t n, int32_t* rep, int32_t* size) {
    GRID_STRIDE(i, n) { const int32_t r = minm[root[i]]; rep[i] = r; atomicAdd(size + r, 1); }
}
__global__ void k_flags(const int32_t* rep, const int32_t* size, int64_t n, int32_t* fm, int32_t* fs) {
    GRID_STRIDE(i, n) { const bool head = rep[i] == (int32_t)i; fm[i] = head && size[i] >= 2; fs[i] = head && size[i] == 1; }
}
// label of a cluster head: multi-member clusters 0.. by earliest member, then singletons in object order
__global__ void k_head_labels(const int32_t* fm, const int32_t* fs, const int32_t* sm, const int32_t* ss, int64_t n, int32_t* lab) {
    const int32_t n_multi = sm[n - 1] + fm[n - 1];
    GRID_STRIDE(i, n) { if (fm[i]) lab[i] = sm[i]; else if (fs[i]) lab[i] = n_multi + ss[i]; }
}
__global__ void k_gather(const int32_t* rep, const int32_t* lab, int64_t n, int32_t* label) { GRID_STRIDE(i, n) label[i] = lab[rep[i]]; }

// ---------------------------------------------------------------- update of a prior clustering ("Update")
// prior[i]: -1 for a new object, else the index of the representative of i's prior cluster.  Visit rank: the prior objects in
// index order, then the new ones in index order; everything between the edge emit and the labels runs on visit ranks.
__global__ void k_new_flags(const int32_t* prior, int64_t n, int32_t* flag) { GRID_STRIDE(i, n) flag[i] = prior[i] < 0; }
// before[] = the exclusive scan of flag[]: the new objects ahead of i.  visit[] and its inverse, and the number of prior objects
__global__ void k_visit_rank(const int32_t* flag, const int32_t* before, int64_t n, int32_t* visit, int32_t* inv, int32_t* n_prior_out) {
    const int32_t n_prior = (int32_t)n - (before[n - 1] + flag[n - 1]);
    GRID_STRIDE(i, n) {
        const int32_t v = flag[i] ? n_prior + before[i] : (int32_t)i - before[i];
        visit[i] = v; inv[v] = (int32_t)i;
        if (i == 0) *n_prior_out = n_prior;
    }
}
// cd-hit / uclust: a prior representative is REP, a prior member MEMBER(its representative), whichever of the two comes first
__global__ void k_seed_greedy(const int32_t* prior, const int32_t* visit, int64_t n, int32_t* state) {
    GRID_STRIDE(i, n) { const int32_t p = prior[i]; if (p >= 0) state[visit[i]] = visit[p]; }
}
// single: the parent of a prior object is the smallest visit rank of its prior cluster, so that parent[x] <= x holds whichever
// member the prior file calls the representative.  minv[] is indexed by the representative's rank and starts as the identity (a
// representative is a member of its cluster), so only a member that comes before its representative has anything to lower: none
// does where the representative is the earliest member, and a large prior cluster does not serialise its members on one word
__global__ void k_seed_min(const int32_t* prior, const int32_t* visit, int64_t n, int32_t* minv) {
    GRID_STRIDE(i, n) {
        const int32_t p = prior[i];
        if (p < 0) continue;
        const int32_t vp = visit[p], v = visit[i];
        if (v < vp) atomicMin(minv + vp, v);
    }
}
__global__ void k_seed_single(const int32_t* prior, const int32_t* visit, const int32_t* minv, int64_t n, int32_t* parent) {
    GRID_STRIDE(i, n) { const int32_t p = prior[i], v = visit[i]; parent[v] = p >= 0 ? minv[visit[p]] : v; }
}
// back to object ids: the cluster id of object i as an object (greedy: its representative; single: some member of its component)
__global__ void k_unmap(const int32_t* root, const int32_t* visit, const int32_t* inv, int64_t n, int32_t* out) {
    GRID_STRIDE(i, n) out[i] = inv[root[visit[i]]];
}
// c[0..2]: new objects that joined a cluster with a prior object / joined a new representative / founded (single: lie in a
// component without a prior object); c[3]: prior clusters; c[4]: prior objects that are still a cluster id (greedy: all the prior
// representatives; single: one per component that holds a prior object)
__global__ void k_update_counts(const int32_t* root, const int32_t* prior, const int32_t* visit, int64_t n, int32_t n_prior, bool single,
                                unsigned long long* c) {
    int jp = 0, jn = 0, fd = 0, pc = 0, pk = 0;
    GRID_STRIDE(i, n) {
        const int32_t v = visit[i], s = root[v];
        if (prior[i] >= 0) { pc += prior[i] == (int32_t)i; pk += s == v; }
        else if (s < n_prior) ++jp;
        else if (single || s == v) ++fd;
        else ++jn;
    }
    add_count(c + 0, jp); add_count(c + 1, jn); add_count(c + 2, fd); add_count(c + 3, pc); add_count(c + 4, pk);
}

// ---------------------------------------------------------------- cohesion / separation report ("Cluster report")
// A given labelling label[i] in [0, n_clusters) over the edge graph, every weight the integer u of average linkage.  Three passes:
//   rows     every object (ROW_LANES lanes each, row-strided as k_cl_find) reduces its row: count / sum / minimum of its own-cluster
//            edges (each undirected edge at its smaller end), count of its external edges, own_max, the best external (u, label)
//   reduce   the objects sorted by label (one radix sort); a wave reduces 64 sorted positions by segment with shuffles and the
//            first lane of every segment piece adds it to the cluster's record: one atomic group per cluster per 64 members
//   nearest  the rows once more for the sum over the edges to each cluster's nearest one and the misfit flags, reduced the same way
// Every sum is an integer sum and every choice the maximum / minimum of a total order: the result does not depend on launch order.
// the best external neighbour as one key: u (<= 2^32: 33 bits) above the complement of the label (31 bits), so that the maximum is the
// largest u and, among equals, the smallest label.  "None" is not a key value: the count of external edges says so.
constexpr uint64_t ST_LABEL_MASK = 0x7fffffffull;
__host__ __device__ inline uint64_t st_key(uint64_t u, int32_t label) { return u << 31 | (ST_LABEL_MASK - (uint64_t)label); }
__host__ __device__ inline int32_t st_key_label(uint64_t key) { return (int32_t)(ST_LABEL_MASK - (key & ST_LABEL_MASK)); }
__host__ __device__ inline uint64_t st_key_u(uint64_t key) { return key >> 31; }
// what a row or a piece of a cluster adds to the cluster's record; the identity is { 0, 0, 0, ~0, 0 }
struct st_part { uint64_t cnt, sum, ext, mn, key; };
__device__ __forceinline__ void st_combine(st_part& x, const st_part& y) {
    x.cnt += y.cnt; x.sum += y.sum; x.ext += y.ext; x.mn = umin64(x.mn, y.mn); x.key = umax64(x.key, y.key);
}
__device__ __forceinline__ st_part st_shfl(const st_part& x, int o, bool down) {
    auto mv = [&](uint64_t v) { return (uint64_t)(down ? __shfl_down((unsigned long long)v, o) : __shfl_xor((unsigned long long)v, o)); };
    return st_part{ mv(x.cnt), mv(x.sum), mv(x.ext), mv(x.mn), mv(x.key) };
}
// rows.  NEAR = false: the partials of the record and own_max; NEAR = true: part.sum = the sum of u over the edges into the nearest
// cluster of the object's own (rec_ext / rec_key of its cluster say which), part.cnt = 1 for a misfit (other_max > own_max).
template <bool NEAR>
__global__ void k_st_rows(int64_t n, const int64_t* off, const int32_t* adj, const uint64_t* u, const int32_t* label,
                          const uint64_t* rec_ext, const uint64_t* rec_key, uint64_t* p_cnt, uint64_t* p_sum, uint64_t* p_ext, uint64_t* p_mn,
                          uint64_t* p_key, uint64_t* own_max) {
    const int lane = threadIdx.x % ROW_LANES;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / ROW_LANES;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ROW_LANES; i < n; i += groups) {
        const int32_t c = label[i];
        const int32_t near = NEAR && rec_ext[c] ? st_key_label(rec_key[c]) : -1;
        st_part v{ 0, 0, 0, ~0ull, 0 }; uint64_t own = 0;
        for (int64_t k = off[i] + lane, e = off[i + 1]; k < e; k += ROW_LANES) {
            const int32_t j = adj[k], d = label[j]; const uint64_t x = u[k];
            if (NEAR) { if (d == near) v.sum += x; continue; }
            if (d == c) { own = umax64(own, x); if (j > i) { ++v.cnt; v.sum += x; v.mn = umin64(v.mn, x); } }
            else { ++v.ext; v.key = umax64(v.key, st_key(x, d)); }
        }
        for (int o = ROW_LANES / 2; o > 0; o >>= 1) {
            st_combine(v, st_shfl(v, o, false));
            own = umax64(own, (uint64_t)__shfl_xor((unsigned long long)own, o));
        }
        if (lane) continue;
        if (NEAR) { p_sum[i] = v.sum; p_cnt[i] = (p_ext[i] ? st_key_u(p_key[i]) : 0) > own_max[i]; }
        else { p_cnt[i] = v.cnt; p_sum[i] = v.sum; p_ext[i] = v.ext; p_mn[i] = v.mn; p_key[i] = v.key; own_max[i] = own; }
    }
}
// reduce.  slabel[p] / order[p]: the label and the object at sorted position p (ascending label, then index).  A wave takes 64
// positions per trip; after the segmented butterfly the first lane of every run of equal labels holds the run's total and adds it to
// the record.  NEAR = false also notes where a cluster begins and ends in the sorted order (its size and its earliest member, without
// atomics); NEAR = true adds (misfits, nearest_sum) only.
template <bool NEAR>
__global__ void k_st_reduce(int64_t n, const int32_t* slabel, const int32_t* order, const uint64_t* p_cnt, const uint64_t* p_sum,
                            const uint64_t* p_ext, const uint64_t* p_mn, const uint64_t* p_key, unsigned long long* r_cnt,
                            unsigned long long* r_sum, unsigned long long* r_ext, unsigned long long* r_mn, unsigned long long* r_key,
                            int64_t* r_begin, int64_t* r_end, int32_t* r_rep) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; base < n; base += stride) {      // (wave-uniform)
        const int64_t p = base + lane;
        const bool live = p < n;
        const int32_t lb = live ? slabel[p] : -1;               // (no label is -1: a dead lane joins no run of a live one)
        st_part v{ 0, 0, 0, ~0ull, 0 };
        if (live) {
            const int32_t i = order[p];
            v.cnt = p_cnt[i]; v.sum = p_sum[i];
            if (!NEAR) {
                v.ext = p_ext[i]; v.mn = p_mn[i]; v.key = p_key[i];
                if (p == 0 || slabel[p - 1] != lb) { r_begin[lb] = p; r_rep[lb] = i; }
                if (p == n - 1 || slabel[p + 1] != lb) r_end[lb] = p + 1;
            }
        }
        for (int o = 1; o < 64; o <<= 1) {                      // lane l: the total over [l, l + 2o) cut at the end of its run
            const st_part w = st_shfl(v, o, true);
            const int32_t lb2 = __shfl_down(lb, o);
            const bool take = lane + o < 64 && lb2 == lb;       // (selects, not a branch around the struct: see k_av_find)
            st_part t = v;
            st_combine(t, w);
            v.cnt = take ? t.cnt : v.cnt; v.sum = take ? t.sum : v.sum; v.ext = take ? t.ext : v.ext;
            v.mn = take ? t.mn : v.mn; v.key = take ? t.key : v.key;
        }
        const int32_t before = __shfl_up(lb, 1);
        if (!live || (lane && before == lb)) continue;
        if (v.cnt) atomicAdd(r_cnt + lb, (unsigned long long)v.cnt);
        if (v.sum) atomicAdd(r_sum + lb, (unsigned long long)v.sum);
        if (NEAR) continue;
        if (v.cnt) atomicMin(r_mn + lb, (unsigned long long)v.mn);
        if (v.ext) { atomicAdd(r_ext + lb, (unsigned long long)v.ext); atomicMax(r_key + lb, (unsigned long long)v.key); }
    }
}
// the records as the caller's structs; a label without members: size 0, rep and nearest -1, the rest 0
__global__ void k_st_finish(int64_t n_clusters, const int64_t* r_begin, const int64_t* r_end, const int32_t* r_rep, const unsigned long long* r_cnt,
                            const unsigned long long* r_sum, const unsigned long long* r_ext, const unsigned long long* r_mn,
                            const unsigned long long* r_key, const unsigned long long* r_mis, const unsigned long long* r_nsum, vg_cluster_stat* out) {
    GRID_STRIDE(c, n_clusters) {
        vg_cluster_stat o{};
        o.rep = -1; o.nearest = -1;
        if (r_begin[c] >= 0) {
            o.size = r_end[c] - r_begin[c]; o.rep = r_rep[c];
            o.pairs = (uint64_t)o.size * (uint64_t)(o.size - 1) / 2;
            o.linked = r_cnt[c]; o.sum = r_sum[c]; o.min = o.linked ? r_mn[c] : 0; o.external = r_ext[c];
            if (o.external) { o.nearest = st_key_label(r_key[c]); o.nearest_max = st_key_u(r_key[c]); o.nearest_sum = r_nsum[c]; }
            o.misfits = (int64_t)r_mis[c];
        }
        out[c] = o;
    }
}

// a round that decides fewer objects than this (and < 1 % of those left) hands the rest to the one-workgroup sweep
constexpr int64_t LOW_PROGRESS = 4096;
bool low_progress(int64_t decided, int64_t left) { return decided < LOW_PROGRESS && decided * 100 < left; }

int64_t read_counter(dbuf<unsigned long long>& c, hipStream_t s) {
    unsigned long long v = 0;
    c.download(&v, 1, s);
    VG_HIP(hipStreamSynchronize(s));
    return (int64_t)v;
}

void exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, hipStream_t s) {
    with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::exclusive_scan(tmp, tb, in, out, 0, (size_t)n, rocprim::plus<int32_t>(), s); });
}
// ---------------------------------------------------------------- the opening of the array-level entries
struct row_list { int64_t n; const uint32_t *q, *r; const double* w; int64_t n_rows; };    // the rows of a call over n objects
// The argument checks of every array-level entry, before any device use.  The order in which an entry raises its errors is part of
// its behaviour, so the opening comes in steps an entry calls around its own checks: check_call, check_row_values and, where sums
// of weights are taken, check_unit_weights.
// check_call: the sizes and the row pointers, then the entry's own null condition and its algorithm set -- null_error and
// algorithm_error are the texts behind "<fn>: " of the one that failed, nullptr where it holds
void check_call(const char* fn, const row_list& in, const char* null_error = nullptr, const char* algorithm_error = nullptr) {
    const std::string name(fn);
    if (in.n < 0 || in.n_rows < 0) throw vg_error(VG_EINVAL, name + ": negative size");
    if (in.n >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, name + ": 2^31 or more objects (object indices are int32)");
    if (in.n_rows && (!in.q || !in.r || !in.w)) throw vg_error(VG_EINVAL, name + ": null rows");
    if (null_error) throw vg_error(VG_EINVAL, name + ": " + null_error);
    if (algorithm_error) throw vg_error(VG_EINVAL, name + ": " + algorithm_error);
}
// the first row for which is_bad(row) holds, or -1: a parallel scan, every thread stops at the first of its chunk
template <class Bad> int64_t first_bad_row(int64_t n_rows, Bad is_bad) {
    std::vector<int64_t> bad((size_t)std::max(1, vg_host_threads()), -1);
    vg_parallel_chunks(n_rows, vg_host_threads(), [&](int64_t lo, int64_t hi, int t) {
        for (int64_t k = lo; k < hi; ++k) if (is_bad(k)) { bad[(size_t)t] = k; return; }
    });
    for (int64_t k : bad) if (k >= 0) return k;
    return -1;
}
void check_row_values(const char* fn, const row_list& in) {
    const int64_t k = first_bad_row(in.n_rows, [&](int64_t i) { return in.q[i] >= (uint64_t)in.n || in.r[i] >= (uint64_t)in.n || std::isnan(in.w[i]); });
    if (k >= 0)
        throw vg_error(VG_EINVAL, std::string(fn) + ": row " + std::to_string(k) + ": " +
                       (std::isnan(in.w[k]) ? std::string("weight is NaN") : "object index outside 0.." + std::to_string(in.n - 1)));
}
// the quantum 2^-32 and the 64-bit sums (average linkage, the report, Markov clustering) stand on weights in [0, 1] ...
void check_unit_weights(const char* fn, const row_list& in, const char* what = nullptr) {      // what: named in parentheses behind the text
    const int64_t k = first_bad_row(in.n_rows, [&](int64_t i) { return !(in.w[i] >= 0 && in.w[i] <= 1); });
    if (k >= 0)
        throw vg_error(VG_EINVAL, std::string(fn) + ": row " + std::to_string(k) + ": weight " + std::to_string(in.w[k]) + " outside [0, 1]" +
                       (what ? " (" + std::string(what) + ")" : std::string()));
}
// ... and on fewer than 2^32 of them
void check_edge_sums(const std::string& fn, int64_t n_edges) {
    if (n_edges >= (1LL << 32)) throw vg_error(VG_EOVERFLOW, fn + ": 2^32 or more edges (a sum of weights must fit 64 bits)");
}
// the stats of a call, cleared: the caller's, or a local one if it wants none
template <class Stats> Stats& cleared(Stats* stats, Stats& local) { Stats& st = stats ? *stats : local; st = Stats{}; return st; }

// the edge graph of the rows on the device: the m directed edges sorted by (src, dst) with their weights, and the CSR.  With a
// visit_map (the update of a prior clustering) the graph is over visit ranks and holds no edge between two prior objects.
struct edge_graph { dbuf<uint64_t> ukeys; dbuf<double> uvals; int64_t m = 0; dbuf<int64_t> off; dbuf<int32_t> adj; };
struct visit_map { const int32_t* visit = nullptr; int64_t n_prior = 0; };      // visit[object] = visit rank (device); ranks < n_prior are prior
void build_edge_graph(const row_list& in, hipStream_t s, edge_graph& g, visit_map vm) {
    const int64_t n = in.n, n_rows = in.n_rows; const uint32_t *q = in.q, *r = in.r; const double* w = in.w;
    dbuf<uint64_t>& ukeys = g.ukeys; dbuf<double>& uvals = g.uvals; int64_t& m = g.m;
    const int bits = id_bits(n);

    // ---- edges: sort both directions by (src, dst), merge duplicates to the max weight, CSR
    if (n_rows) {
        const int64_t nd = 2 * n_rows;
        dbuf<uint64_t> keys((size_t)nd), keys2((size_t)nd); dbuf<double> vals((size_t)nd), vals2((size_t)nd);
        {
            dbuf<uint32_t> dq((size_t)n_rows), dr((size_t)n_rows); dbuf<double> dw((size_t)n_rows);
            dq.upload(q, (size_t)n_rows, s); dr.upload(r, (size_t)n_rows, s); dw.upload(w, (size_t)n_rows, s);
            vg_prof_scope ps("cluster_edges_emit", (double)n_rows * 48.0);
            if (vm.visit)
                hipLaunchKernelGGL(k_emit<true>, dim3(grid_of(n_rows)), dim3(TPB), 0, s, dq.p, dr.p, dw.p, n_rows, (uint32_t)n, vm.visit, (uint32_t)vm.n_prior, keys.p, vals.p);
            else
                hipLaunchKernelGGL(k_emit<false>, dim3(grid_of(n_rows)), dim3(TPB), 0, s, dq.p, dr.p, dw.p, n_rows, (uint32_t)n, (const int32_t*)nullptr, 0u, keys.p, vals.p);
        }
        {
            vg_prof_scope ps("cluster_edges_sort", (double)nd * 32.0 * 2.0);
            with_temp_storage([&](void* tmp, size_t& tb) {
                return rocprim::radix_sort_pairs(tmp, tb, keys.p, keys2.p, vals.p, vals2.p, (size_t)nd, 0u, 32u + (unsigned)bits, s); });
        }
        keys.release(); vals.release();
        ukeys.alloc((size_t)nd); uvals.alloc((size_t)nd);
        dbuf<unsigned long long> d_cnt(1);
        {
            vg_prof_scope ps("cluster_edges_merge", (double)nd * 32.0);
            with_temp_storage([&](void* tmp, size_t& tb) {
                return rocprim::reduce_by_key(tmp, tb, keys2.p, vals2.p, (size_t)nd, ukeys.p, uvals.p, d_cnt.p, rocprim::maximum<double>(),
                                              rocprim::equal_to<uint64_t>(), s); });
        }
        m = read_counter(d_cnt, s);
        if (m > 0) {                                             // the self-row sentinel, if any, is the last unique key
            uint64_t last = 0;
            vg_download_bytes(&last, ukeys.p + (m - 1), sizeof last, s);
            VG_HIP(hipStreamSynchronize(s));
            if ((int64_t)(last >> 32) == n) --m;
        }
    }
    g.off.alloc((size_t)n + 1); g.adj.alloc((size_t)std::max<int64_t>(m, 1));
    {
        vg_prof_scope ps("cluster_csr", (double)m * 12.0 + (double)n * 8.0);
        hipLaunchKernelGGL(k_csr, dim3(grid_of(m + 1)), dim3(TPB), 0, s, (const uint64_t*)ukeys.p, m, n, g.off.p, g.adj.p);
    }
}
// From checked rows to their graph on the device, the step behind the opening of every entry: nobody else builds a graph.
// -> the library's stream, on which the graph is complete in stream order (eg.m / 2 = the undirected edges)
hipStream_t graph_on_device(const row_list& in, edge_graph& eg, visit_map vm = {}) {
    vg_require_device();
    hipStream_t s = vg_stream();
    build_edge_graph(in, s, eg, vm);
    return s;
}

// rank: forward edges in (a, b) order, then ONE stable sort by the weight key -> (w descending, a, b).  pos[p] = the directed
// position of the forward edge of rank p (mu = m / 2 of them), rank[k] = the rank of the directed edge k
void rank_edges(const edge_graph& eg, hipStream_t s, dbuf<int64_t>& pos, dbuf<uint64_t>& rank) {
    const int64_t m = eg.m, mu = m / 2;
    pos.alloc((size_t)mu); rank.alloc((size_t)m);
    {
        vg_prof_scope ps("cluster_rank", (double)m * 8.0 + (double)mu * (16.0 + 32.0 * 2.0 + 40.0));
        dbuf<int64_t> pos0((size_t)mu); dbuf<uint64_t> wkey((size_t)mu), wkey2((size_t)mu);
        dbuf<unsigned long long> d_cnt(1);
        rocprim::counting_iterator<int64_t> iota(0);
        const forward_edge fwd{ eg.ukeys.p };
        with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::select(tmp, tb, iota, pos0.p, d_cnt.p, (size_t)m, fwd, s); });
        if (read_counter(d_cnt, s) != mu) throw vg_error(VG_EHIP, "vg_cluster_linkage: the edge list is not symmetric (internal error)");
        hipLaunchKernelGGL(k_rank_keys, dim3(grid_of(mu)), dim3(TPB), 0, s, (const int64_t*)pos0.p, (const double*)eg.uvals.p, mu, wkey.p);
        with_temp_storage([&](void* tmp, size_t& tb) {
            return rocprim::radix_sort_pairs(tmp, tb, wkey.p, wkey2.p, pos0.p, pos.p, (size_t)mu, 0u, 64u, s); });
        dbuf<int32_t> bad(1); bad.zero(s);
        hipLaunchKernelGGL(k_rank_scatter, dim3(grid_of(mu)), dim3(TPB), 0, s, (const int64_t*)pos.p, mu, (const uint64_t*)eg.ukeys.p,
                           (const int64_t*)eg.off.p, (const int32_t*)eg.adj.p, rank.p, bad.p);
        int32_t b = 0; bad.download(&b, 1, s);
        VG_HIP(hipStreamSynchronize(s));
        if (b) throw vg_error(VG_EHIP, "vg_cluster_linkage: an edge without its reverse (internal error)");
    }
}
// the merge records of the ranks frank[0 .. nf) (ascending = merge order): their ends and weights; only these leave the device
void download_forest(const dbuf<int64_t>& frank, int64_t nf, const dbuf<int64_t>& pos, const edge_graph& eg, hipStream_t s, vg_forest& f) {
    dbuf<int32_t> da((size_t)nf), db((size_t)nf); dbuf<double> dw((size_t)nf);
    hipLaunchKernelGGL(k_forest_gather, dim3(grid_of(nf)), dim3(TPB), 0, s, (const int64_t*)frank.p, nf, (const int64_t*)pos.p,
                       (const uint64_t*)eg.ukeys.p, (const double*)eg.uvals.p, da.p, db.p, dw.p);
    VG_HIP(hipGetLastError());
    f.a.resize((size_t)nf); f.b.resize((size_t)nf); f.w.resize((size_t)nf);
    da.download(f.a.data(), (size_t)nf, s); db.download(f.b.data(), (size_t)nf, s); dw.download(f.w.data(), (size_t)nf, s);
    VG_HIP(hipStreamSynchronize(s));
    f.stats.n_merges = nf;
}

// The forest edges of the graph in merge order (ascending rank), computed on the device; only these records come back.
void forest_on_device(int64_t n, const edge_graph& eg, hipStream_t s, vg_forest& f) {
    const int64_t m = eg.m, mu = m / 2;
    f.stats.n_edges = mu;
    if (mu == 0) return;
    dbuf<int64_t> pos; dbuf<uint64_t> rank;
    rank_edges(eg, s, pos, rank);
    // ---- Boruvka rounds on the ranks: find, hook, jump, relabel; one counter read back per round
    dbuf<uint8_t> forest((size_t)mu);
    {
        dbuf<int32_t> comp((size_t)n), parent((size_t)n); dbuf<uint8_t> inner((size_t)n); dbuf<unsigned long long> cmin((size_t)n), active(1);
        forest.zero(s); inner.zero(s);
        hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, comp.p, n);
        hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, parent.p, n);
        for (;;) {
            {
                vg_prof_scope ps("cluster_boruvka", (double)m * 16.0 + (double)n * 32.0);
                VG_HIP(hipMemsetAsync(cmin.p, 0xff, cmin.bytes(), s));
                active.zero(s);
                hipLaunchKernelGGL(k_bor_find, dim3(grid_of(n * ROW_LANES)), dim3(TPB), 0, s, n, (const int64_t*)eg.off.p, (const int32_t*)eg.adj.p,
                                   (const uint64_t*)rank.p, (const int32_t*)comp.p, inner.p, cmin.p);
                hipLaunchKernelGGL(k_bor_hook, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int32_t*)comp.p, (const unsigned long long*)cmin.p,
                                   (const int64_t*)pos.p, (const uint64_t*)eg.ukeys.p, forest.p, parent.p, active.p);
                hipLaunchKernelGGL(k_bor_jump, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int32_t*)comp.p, parent.p);
                hipLaunchKernelGGL(k_bor_relabel, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int32_t*)parent.p, comp.p);
            }
            ++f.stats.rounds;
            if (read_counter(active, s) == 0) break;           // no component has a leaving edge
            if (f.stats.rounds > 64) throw vg_error(VG_EHIP, "vg_cluster_linkage: the rounds do not end (internal error)");
        }
    }
    VG_HIP(hipGetLastError());
    // ---- forest: the marked ranks, ascending = merge order, with their ends and weights
    vg_prof_scope ps("cluster_forest", (double)mu + (double)n * 40.0);
    const int64_t cap = std::min<int64_t>(mu, n - 1);
    dbuf<int64_t> frank((size_t)mu); dbuf<unsigned long long> d_cnt(1);
    rocprim::counting_iterator<int64_t> iota(0);
    with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::select(tmp, tb, iota, forest.p, frank.p, d_cnt.p, (size_t)mu, s); });
    const int64_t nf = read_counter(d_cnt, s);
    if (nf < 1 || nf > cap) throw vg_error(VG_EHIP, "vg_cluster_linkage: the marked edges are no forest (internal error)");
    download_forest(frank, nf, pos, eg, s, f);
}

// ---------------------------------------------------------------- agglomeration rounds (complete and average linkage)
// The state of the loop.  The cluster graph (keys, val, eg.off) starts as the object graph; t* / s* are the contraction's work arrays.
struct cluster_rounds {
    const int64_t n, m0, cap; const int bits; const hipStream_t s; edge_graph& eg;     // m0 directed edges, at most cap merges
    dbuf<uint64_t> keys, val, tkey, tval, skey, sval;
    dbuf<int32_t> parent, bdst;
    dbuf<unsigned long long> cnt, n_groups;                     // cnt: merges of all rounds so far, records of the cluster graph
    int64_t rounds = 0, total = 0, m = 0;                       // total, m: the two counters as last read back
};
// The rounds of a hierarchy on the edge graph (which they consume: the row offsets are rebuilt per contraction): find + match, one
// read-back of two counters, contraction; f receives the merge records in merge order.  The Linkage supplies only what differs:
//   name, contract_scope, count_bits, reduce_op    the name in notes and error texts, the profile scope of the contraction, the
//                             count bits k_relabel puts below a value, the reduce-by-key operator on such values
//   begin(st)                 its checks, its own arrays, and st.val: the values of the object graph's records
//   find_and_match(st)        the round's two launches under its scope name -> bdst, parent[d] = c, its merge list, cnt[0]
//   round_limit(n), idle_round(st)    more rounds are an internal error; after a round without merges, true for another round
//   before_contraction(st, merges)    what the round's merges change beside the cluster graph
//   compact(st)               the reduced groups (tkey, tval, n_groups) -> the surviving records in keys / val, the tail of the old
//                             list filled with the sentinel, cnt[1] = the new length
//   finish(st, f)             the merge records leave the device
template <class Linkage>
void agglomerate(int64_t n, edge_graph& eg, hipStream_t s, Linkage& lk, vg_forest& f) {
    const int64_t m0 = eg.m, mu = m0 / 2;
    f.stats.n_edges = mu;
    if (mu == 0) return;
    const std::string fn = std::string("vg_cluster_") + Linkage::name + "_linkage";
    cluster_rounds st{ n, m0, std::min<int64_t>(mu, n - 1), id_bits(n), s, eg };     // two ids are a sort key of the contraction
    lk.begin(st);
    for (dbuf<uint64_t>* b : { &st.keys, &st.tkey, &st.tval, &st.skey, &st.sval }) b->alloc((size_t)m0);
    st.parent.alloc((size_t)n); st.bdst.alloc((size_t)n); st.cnt.alloc(2); st.n_groups.alloc(1);
    VG_HIP(hipMemcpyAsync(st.keys.p, eg.ukeys.p, (size_t)m0 * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, st.parent.p, n);
    const unsigned long long cnt0[2] = { 0, (unsigned long long)m0 };
    st.cnt.upload(cnt0, 2, s);
    st.m = m0;
    char note[96];
    for (;;) {
        lk.find_and_match(st);
        ++st.rounds;
        unsigned long long now[2] = { 0, 0 };                   // the one read-back of the round: both counters
        st.cnt.download(now, 2, s);
        VG_HIP(hipStreamSynchronize(s));
        const int64_t merges = (int64_t)now[0] - st.total, m = (int64_t)now[1];
        st.total = (int64_t)now[0]; st.m = m;
        if (st.total > st.cap || m < 0 || m > m0 || (m & 1)) throw vg_error(VG_EHIP, fn + ": the merges are no hierarchy (internal error)");
        snprintf(note, sizeof note, "%s round %lld: %lld merges, %lld records", Linkage::name, (long long)st.rounds, (long long)merges, (long long)m);
        vg_host_mark(note);
        // (a round without merges cannot be what passes the limit: every round before it merged, and total <= cap < n)
        if (st.rounds > lk.round_limit(n)) throw vg_error(VG_EHIP, fn + ": the rounds do not end (internal error)");
        if (merges == 0) { if (lk.idle_round(st)) continue; break; }
        vg_prof_scope ps(Linkage::contract_scope, (double)m * (32.0 + 32.0 * 2.0 + 32.0 + 24.0) + (double)n * 16.0);
        lk.before_contraction(st, merges);
        hipLaunchKernelGGL(k_relabel, dim3(grid_of(m)), dim3(TPB), 0, s, (const uint64_t*)st.keys.p, (const uint64_t*)st.val.p, m,
                           (const int32_t*)st.parent.p, n, st.bits, Linkage::count_bits, st.tkey.p, st.tval.p);
        with_temp_storage([&](void* tmp, size_t& tb) {
            return rocprim::radix_sort_pairs(tmp, tb, st.tkey.p, st.skey.p, st.tval.p, st.sval.p, (size_t)m, 0u, 2u * (unsigned)st.bits, s); });
        with_temp_storage([&](void* tmp, size_t& tb) {           // -> (cluster pair, reduced value) in tkey / tval
            return rocprim::reduce_by_key(tmp, tb, st.skey.p, st.sval.p, (size_t)m, st.tkey.p, st.tval.p, st.n_groups.p,
                                          typename Linkage::reduce_op(), rocprim::equal_to<uint64_t>(), s); });
        lk.compact(st);
        hipLaunchKernelGGL(k_csr, dim3(grid_of(m + 1)), dim3(TPB), 0, s, (const uint64_t*)st.keys.p, m, n, eg.off.p, eg.adj.p);
    }
    VG_HIP(hipGetLastError());
    f.stats.rounds = st.rounds;
    lk.finish(st, f);
}

// Complete linkage: the values are the ranks of rank_edges.  comp[i] = the cluster of object i after every merge (its minimum
// member); the merge records, if wanted, are the merge ranks sorted on the device and fetched the forest's way.
struct complete_linkage {
    static constexpr const char *name = "complete", *contract_scope = "cluster_complete_contract";
    static constexpr int count_bits = COUNT_BITS; using reduce_op = max_rank_add_count;
    dbuf<int32_t>& comp; const bool want_records;
    dbuf<int64_t> pos, idx, merged; dbuf<int32_t> mult; dbuf<unsigned long long> best;
    void begin(cluster_rounds& st) {
        rank_edges(st.eg, st.s, pos, st.val);
        idx.alloc((size_t)st.m0); merged.alloc((size_t)st.cap); mult.alloc((size_t)st.n); best.alloc((size_t)st.n);
    }
    void find_and_match(cluster_rounds& st) {
        vg_prof_scope ps("cluster_complete_best", (double)st.m * 16.0 + (double)st.n * 40.0);
        hipLaunchKernelGGL(k_cl_find, dim3(grid_of(st.n * ROW_LANES)), dim3(TPB), 0, st.s, st.n, (const int64_t*)st.eg.off.p, (const uint64_t*)st.keys.p,
                           (const uint64_t*)st.val.p, best.p, st.bdst.p, mult.p);
        hipLaunchKernelGGL(k_cl_match, dim3(grid_of(st.n)), dim3(TPB), 0, st.s, st.n, (const unsigned long long*)best.p, (const int32_t*)st.bdst.p,
                           st.parent.p, mult.p, merged.p, st.cap, st.cnt.p);
    }
    int64_t round_limit(int64_t n) const { return n; }
    bool idle_round(const cluster_rounds&) { return false; }    // no finite K is left
    void before_contraction(cluster_rounds& st, int64_t) {
        hipLaunchKernelGGL(k_bor_relabel, dim3(grid_of(st.n)), dim3(TPB), 0, st.s, st.n, (const int32_t*)st.parent.p, comp.p);
    }
    void compact(cluster_rounds& st) {                          // (cluster pair, worst rank << 3 | records): select the full pairs
        const surviving_pair alive{ st.tkey.p, st.tval.p, st.n_groups.p, mult.p, st.n, st.bits };
        rocprim::counting_iterator<int64_t> iota(0);
        with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::select(tmp, tb, iota, idx.p, st.cnt.p + 1, (size_t)st.m, alive, st.s); });
        hipLaunchKernelGGL(k_cl_compact, dim3(grid_of(st.m)), dim3(TPB), 0, st.s, (const int64_t*)idx.p, (const unsigned long long*)(st.cnt.p + 1), st.m,
                           (const uint64_t*)st.tkey.p, (const uint64_t*)st.tval.p, st.n, st.bits, st.keys.p, st.val.p);
    }
    void finish(cluster_rounds& st, vg_forest& f) {             // the merge ranks, ascending = merge order
        if (!want_records || st.total == 0) return;
        vg_prof_scope ps("cluster_forest", (double)st.total * 16.0 + (double)st.n * 40.0);
        dbuf<int64_t> frank((size_t)st.total);
        with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::radix_sort_keys(tmp, tb, merged.p, frank.p, (size_t)st.total, 0u, 64u, st.s); });
        download_forest(frank, st.total, pos, st.eg, st.s, f);
    }
};
void complete_on_device(int64_t n, edge_graph& eg, hipStream_t s, dbuf<int32_t>& comp, bool want_records, vg_forest& f) {
    comp.alloc((size_t)n);
    hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, comp.p, n);
    VG_HIP(hipGetLastError());
    complete_linkage lk{ comp, want_records };
    agglomerate(n, eg, s, lk, f);
}

// the level t as a count of quanta: sim >= t is S >= T * P.  Below 0 every merge passes, above 1 none does (sim <= 1).
uint64_t av_quanta(double t) { return t <= 0 ? 0 : t > 1 ? (1ull << 32) + 1 : (uint64_t)llrint(ldexp(t, 32)); }
// the double nearest to S / (P * 2^32), ties to even: both operands shifted to 64 significant bits, one 128-by-64-bit division to a
// 62- or 63-bit quotient whose lowest bit also takes the remainder (sticky), one conversion (which rounds once) and an exact ldexp
double av_similarity(uint64_t S, uint64_t P) {
    if (P == 0) return NAN;
    if (S == 0) return 0.0;
    const int zs = __builtin_clzll(S), zp = __builtin_clzll(P);
    const unsigned __int128 num = (unsigned __int128)(S << zs) << 62;
    const uint64_t den = P << zp;
    const uint64_t quot = (uint64_t)(num / den) | (num % den ? 1u : 0u);
    return ldexp((double)quot, zp - zs - 62 - 32);
}

// Average linkage: the values are the 64-bit sums; the merge records (c, d, S, P) leave the device and are sorted on the host.  With
// floor 0 a record of S == 0 may merge too, but a cluster pair WITHOUT a record has the same similarity 0 and becomes a candidate
// when a merge gives it a record: among such ties the parallel rounds are not the sequential rule.  So records of S == 0 wait until
// a round finds no other merge (then every record left has S == 0) and merge one per round from there, the smallest (c, d) first --
// the sequential rule itself, whose order the host keeps for those records instead of sorting them.
struct average_linkage {
    static constexpr const char *name = "average", *contract_scope = "cluster_average_contract";
    static constexpr int count_bits = 0; using reduce_op = rocprim::plus<uint64_t>;
    const uint64_t F;                                           // the floor in quanta
    dbuf<uint64_t> msum, mpairs; dbuf<int32_t> mc, md, size; dbuf<unsigned long long> bsum;
    int64_t in_key_order = -1;                                  // the merges before the zero phase (-1: it never began)
    void begin(cluster_rounds& st) {
        check_edge_sums("vg_cluster_average_linkage", st.m0 / 2);
        st.val.alloc((size_t)st.m0); msum.alloc((size_t)st.cap); mpairs.alloc((size_t)st.cap); mc.alloc((size_t)st.cap); md.alloc((size_t)st.cap);
        size.alloc((size_t)st.n); bsum.alloc((size_t)st.n);
        hipLaunchKernelGGL(k_av_quantise, dim3(grid_of(st.m0)), dim3(TPB), 0, st.s, (const double*)st.eg.uvals.p, st.m0, st.val.p);
        hipLaunchKernelGGL(k_fill, dim3(grid_of(st.n)), dim3(TPB), 0, st.s, size.p, st.n, 1);
    }
    void find_and_match(cluster_rounds& st) {
        vg_prof_scope ps("cluster_average_best", (double)st.m * 20.0 + (double)st.n * 40.0);
        hipLaunchKernelGGL(k_av_find, dim3(grid_of(st.n * ROW_LANES)), dim3(TPB), 0, st.s, st.n, (const int64_t*)st.eg.off.p, (const uint64_t*)st.keys.p,
                           (const uint64_t*)st.val.p, (const int32_t*)size.p, bsum.p, st.bdst.p);
        hipLaunchKernelGGL(k_av_match, dim3(grid_of(st.n)), dim3(TPB), 0, st.s, st.n, (const unsigned long long*)bsum.p, (const int32_t*)st.bdst.p,
                           (const int32_t*)size.p, F, in_key_order >= 0 ? 1 : 0, (const uint64_t*)st.keys.p, st.parent.p, msum.p, mpairs.p, mc.p,
                           md.p, st.cap, st.cnt.p);
    }
    int64_t round_limit(int64_t n) const { return 2 * n + 2; }    // (n - 1 merging rounds and two that find nothing, with room)
    bool idle_round(const cluster_rounds& st) {                 // only records of S == 0 are left: the zero phase begins, once
        if (!(F == 0 && st.m > 0 && in_key_order < 0)) return false;
        in_key_order = st.total;
        return true;
    }
    void before_contraction(cluster_rounds& st, int64_t merges) {
        hipLaunchKernelGGL(k_av_grow, dim3(grid_of(merges)), dim3(TPB), 0, st.s, (const int32_t*)mc.p, (const int32_t*)md.p, st.total - merges, st.total, size.p);
    }
    void compact(cluster_rounds& st) {                          // (cluster pair, sum): every group but the sentinel's, no select pass
        hipLaunchKernelGGL(k_av_compact, dim3(grid_of(st.m)), dim3(TPB), 0, st.s, (const unsigned long long*)st.n_groups.p, st.m, (const uint64_t*)st.tkey.p,
                           (const uint64_t*)st.tval.p, st.n, st.bits, st.keys.p, st.val.p, st.cnt.p + 1);
    }
    // the <= n - 1 merge records leave the device; their order is the key order (keys are distinct: d disappears when absorbed)
    void finish(cluster_rounds& st, vg_forest& f) {
        const int64_t total = st.total;
        f.stats.n_merges = total;
        if (total == 0) return;
        std::vector<uint64_t> hs((size_t)total), hp((size_t)total); std::vector<int32_t> hc((size_t)total), hd((size_t)total);
        msum.download(hs.data(), (size_t)total, st.s); mpairs.download(hp.data(), (size_t)total, st.s);
        mc.download(hc.data(), (size_t)total, st.s); md.download(hd.data(), (size_t)total, st.s);
        VG_HIP(hipStreamSynchronize(st.s));
        std::vector<int64_t> order((size_t)total);
        for (int64_t k = 0; k < total; ++k) order[(size_t)k] = k;
        std::stable_sort(order.begin(), order.begin() + (in_key_order >= 0 ? in_key_order : total), [&](int64_t x, int64_t y) {
            return av_compare(av_cand{ hs[(size_t)x], hp[(size_t)x], (uint32_t)hc[(size_t)x], (uint32_t)hd[(size_t)x] },
                              av_cand{ hs[(size_t)y], hp[(size_t)y], (uint32_t)hc[(size_t)y], (uint32_t)hd[(size_t)y] }) < 0; });
        f.a.resize((size_t)total); f.b.resize((size_t)total); f.w.resize((size_t)total); f.sum.resize((size_t)total); f.pairs.resize((size_t)total);
        for (int64_t k = 0; k < total; ++k) {
            const size_t j = (size_t)order[(size_t)k];
            f.a[(size_t)k] = hc[j]; f.b[(size_t)k] = hd[j]; f.sum[(size_t)k] = hs[j]; f.pairs[(size_t)k] = hp[j];
            f.w[(size_t)k] = av_similarity(hs[j], hp[j]);
        }
    }
};
void average_on_device(int64_t n, edge_graph& eg, double floor, hipStream_t s, vg_forest& f) {
    average_linkage lk{ av_quanta(floor) };
    agglomerate(n, eg, s, lk, f);
}

// ---------------------------------------------------------------- the algorithms of vg_cluster_graph: root[i] = the cluster id of i
// hook + compress, one launch each per round; the changed word is read back every 4 rounds (of the last)
// (seeded: root[] already holds a forest of depth one with parent[x] <= x -- the prior clusters of an update -- in place of k_iota)
void single_on_device(int64_t n, const edge_graph& eg, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& sts, bool seeded = false) {
    if (!seeded) hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, root.p, n);
    dbuf<int32_t> changed(1);
    for (;;) {
        for (int k = 0; k < 4; ++k) {
            if (k == 3) changed.zero(s);
            { vg_prof_scope ps("cluster_hook", (double)eg.m * 8.0); hipLaunchKernelGGL(k_hook, dim3(grid_of(eg.m)), dim3(TPB), 0, s, (const uint64_t*)eg.ukeys.p, eg.m, root.p, changed.p); }
            { vg_prof_scope ps("cluster_compress", (double)n * 8.0); hipLaunchKernelGGL(k_compress, dim3(grid_of(n)), dim3(TPB), 0, s, root.p, n); }
            ++sts.rounds;
        }
        int32_t c = 0;
        changed.download(&c, 1, s);
        VG_HIP(hipStreamSynchronize(s));
        if (!c) break;
    }
}
// f(std::true_type) for uclust, f(std::false_type) for cd-hit: a launch of either instantiation is written once
template <class F> void with_uclust(bool uclust, F f) { if (uclust) f(std::true_type{}); else f(std::false_type{}); }
// cd-hit, uclust and set cover: rounds that decide objects (round(counter) launches one, counting its decisions) until none is
// left; a round of low progress hands the rest to the one-workgroup sweep().  seed() (the update of a prior clustering) writes the
// final states of the n - undecided objects that are decided before the first round.
template <class Round, class Sweep, class Seed>
void decide_in_rounds(int64_t undecided, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& sts, Round round, Sweep sweep, Seed seed) {
    dbuf<unsigned long long> d_dec(1);
    VG_HIP(hipMemsetAsync(root.p, 0xff, root.bytes(), s));
    seed();
    for (int64_t left = undecided; left > 0;) {
        d_dec.zero(s);
        round(d_dec.p);
        ++sts.rounds;
        const int64_t dec = read_counter(d_dec, s);
        left -= dec;
        if (left > 0 && low_progress(dec, left + dec)) { sweep(); sts.sweep_objects = left; left = 0; }
    }
}
template <class Round, class Sweep>
void decide_in_rounds(int64_t n, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& sts, Round round, Sweep sweep) {
    decide_in_rounds(n, s, root, sts, round, sweep, [] {});
}
// seed / n_prior (the update of a prior clustering): the first n_prior objects get their states from seed() and are never
// undecided, so the rounds pass over them and the sweep starts behind them
template <class Seed>
void greedy_on_device(bool uclust, int64_t n, const edge_graph& eg, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& sts, int64_t n_prior, Seed seed) {
    const int64_t* off = eg.off.p; const int32_t* adj = eg.adj.p; const double* wts = eg.uvals.p;
    decide_in_rounds(n - n_prior, s, root, sts, [&](unsigned long long* decided) {
        vg_prof_scope ps(uclust ? "cluster_uclust_round" : "cluster_cdhit_round", (double)eg.m * 12.0 + (double)n * 12.0);
        with_uclust(uclust, [&](auto uc) {
            hipLaunchKernelGGL(k_greedy_round<decltype(uc)::value>, dim3(grid_of(n)), dim3(TPB), 0, s, n, off, adj, wts, root.p, decided); });
    }, [&] {
        // every object before the first undecided one is decided: the sweep may start at the lowest undecided index,
        // which the host does not know -- it starts at 0 (behind the prior objects of an update) and skips decided chunks 256 at a time
        vg_prof_scope ps(uclust ? "cluster_uclust_sweep" : "cluster_cdhit_sweep", (double)eg.m * 12.0);
        with_uclust(uclust, [&](auto uc) {
            hipLaunchKernelGGL(k_greedy_sweep<decltype(uc)::value>, dim3(1), dim3(SWEEP_TPB), 0, s, n, off, adj, wts, root.p, n_prior); });
    }, seed);
}
void greedy_on_device(bool uclust, int64_t n, const edge_graph& eg, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& sts) {
    greedy_on_device(uclust, n, eg, s, root, sts, 0, [] {});
}
void set_cover_on_device(int64_t n, const edge_graph& eg, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& sts) {
    const int64_t* off = eg.off.p; const int32_t* adj = eg.adj.p;
    dbuf<uint64_t> key((size_t)n), m1((size_t)n);
    decide_in_rounds(n, s, root, sts, [&](unsigned long long* decided) {
        vg_prof_scope ps("cluster_setcover_round", (double)eg.m * 4.0 * 12.0);
        hipLaunchKernelGGL(k_sc_key, dim3(grid_of(n)), dim3(TPB), 0, s, n, off, adj, (const int32_t*)root.p, key.p);
        hipLaunchKernelGGL(k_sc_max, dim3(grid_of(n)), dim3(TPB), 0, s, n, off, adj, (const uint64_t*)key.p, m1.p);
        hipLaunchKernelGGL(k_sc_pick, dim3(grid_of(n)), dim3(TPB), 0, s, n, off, adj, (const uint64_t*)key.p, (const uint64_t*)m1.p, root.p, decided);
        hipLaunchKernelGGL(k_sc_claim, dim3(grid_of(n)), dim3(TPB), 0, s, n, off, adj, root.p, decided);
    }, [&] {
        const int64_t nb = (n + SC_BLK - 1) / SC_BLK;
        dbuf<uint64_t> bmax((size_t)nb); dbuf<int32_t> dirty((size_t)nb);
        dirty.zero(s);
        vg_prof_scope ps("cluster_setcover_sweep", (double)eg.m * 12.0);
        hipLaunchKernelGGL(k_sc_key, dim3(grid_of(n)), dim3(TPB), 0, s, n, off, adj, (const int32_t*)root.p, key.p);
        hipLaunchKernelGGL(k_sc_block_max, dim3((unsigned)nb), dim3(SC_TPB), 0, s, n, (const uint64_t*)key.p, bmax.p);
        hipLaunchKernelGGL(k_sc_sweep, dim3(1), dim3(SC_TPB), 0, s, n, nb, off, adj, root.p, key.p, bmax.p, dirty.p);
    });
}
void check_roots(int64_t n, const dbuf<int32_t>& root, hipStream_t s) {
    dbuf<int32_t> bad(1); bad.zero(s);
    hipLaunchKernelGGL(k_check_roots, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)root.p, n, bad.p);
    int32_t b = 0; bad.download(&b, 1, s);
    VG_HIP(hipStreamSynchronize(s));
    if (b) throw vg_error(VG_EHIP, "vg_cluster_graph: an object was left without a cluster (internal error)");
}
// labels: cluster id -> earliest member -> numbering.  by_min_member: a cluster id need not be its cluster's earliest member (a
// set-cover pick; the other algorithms' ids are)
void labels_on_device(int64_t n, const dbuf<int32_t>& root, bool by_min_member, hipStream_t s, dbuf<int32_t>& label, dbuf<int32_t>& rep) {
    dbuf<int32_t> size((size_t)n), fm((size_t)n), fs((size_t)n), sm((size_t)n), ss((size_t)n), lab((size_t)n);
    dbuf<int32_t>& minm = label;                                // (the earliest members, then the labels)
    minm.alloc((size_t)n); rep.alloc((size_t)n);
    vg_prof_scope ps("cluster_labels", (double)n * 4.0 * 14.0);
    size.zero(s);
    if (by_min_member) {
        hipLaunchKernelGGL(k_fill, dim3(grid_of(n)), dim3(TPB), 0, s, minm.p, n, INT32_MAX);
        hipLaunchKernelGGL(k_min_member, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)root.p, n, minm.p);
    } else hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, minm.p, n);
    hipLaunchKernelGGL(k_rep_size, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)root.p, (const int32_t*)minm.p, n, rep.p, size.p);
    hipLaunchKernelGGL(k_flags, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)rep.p, (const int32_t*)size.p, n, fm.p, fs.p);
    exclusive_scan_i32(fm.p, sm.p, n, s);
    exclusive_scan_i32(fs.p, ss.p, n, s);
    hipLaunchKernelGGL(k_head_labels, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)fm.p, (const int32_t*)fs.p, (const int32_t*)sm.p, (const int32_t*)ss.p, n, lab.p);
    hipLaunchKernelGGL(k_gather, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)rep.p, (const int32_t*)lab.p, n, minm.p);
}
// The labelling exit of every call that returns a partition: root[] is checked, ids(): the cluster ids to number -- root[] itself,
// or what the update makes of the checked root[] -- go through labels_on_device, and label[] and representative[] (a cluster's
// earliest member, or with rep_is_id its id) leave the device under one synchronise, behind what also() downloads with them.
template <class Ids, class Also>
void labels_to_host(int64_t n, const dbuf<int32_t>& root, bool by_min_member, bool rep_is_id, hipStream_t s, int32_t* label, int32_t* representative,
                    Ids ids, Also also) {
    VG_HIP(hipGetLastError());
    check_roots(n, root, s);
    const dbuf<int32_t>& id = ids();
    dbuf<int32_t> d_label, d_rep;
    labels_on_device(n, id, by_min_member, s, d_label, d_rep);
    VG_HIP(hipGetLastError());
    also();
    d_label.download(label, (size_t)n, s);
    (rep_is_id ? id : d_rep).download(representative, (size_t)n, s);
    VG_HIP(hipStreamSynchronize(s));
}
void labels_to_host(int64_t n, const dbuf<int32_t>& root, bool by_min_member, hipStream_t s, int32_t* label, int32_t* representative) {
    labels_to_host(n, root, by_min_member, false, s, label, representative, [&]() -> const dbuf<int32_t>& { return root; }, [] {});
}

// The report of one labelling: what the three passes share, the partial results per object (k_st_rows writes them: st_part's fields,
// own_max, and from the nearest pass the misfit flags and the sums into the nearest cluster) and per cluster (k_st_reduce adds them
// up over the objects sorted by label: slabel[p] = the label at sorted position p, order[p] = its object)
struct st_labelling { int64_t n, n_clusters; const edge_graph& eg; const dbuf<uint64_t>& u; hipStream_t s; dbuf<int32_t> label, slabel, order; };
struct st_object_parts {
    dbuf<uint64_t> cnt, sum, ext, mn, key, own, mis, nsum;
    explicit st_object_parts(size_t n) : cnt(n), sum(n), ext(n), mn(n), key(n), own(n), mis(n), nsum(n) {}
};
struct st_cluster_parts {
    dbuf<unsigned long long> cnt, sum, ext, mn, key, mis, nsum; dbuf<int64_t> begin, end; dbuf<int32_t> rep;
    explicit st_cluster_parts(size_t nc) : cnt(nc), sum(nc), ext(nc), mn(nc), key(nc), mis(nc), nsum(nc), begin(nc), end(nc), rep(nc) {}
};
void stats_rows_pass(const st_labelling& L, st_object_parts& p) {
    vg_prof_scope ps("cluster_stats_rows", (double)L.eg.m * 16.0 + (double)L.n * 60.0);
    hipLaunchKernelGGL(k_st_rows<false>, dim3(grid_of(L.n * ROW_LANES)), dim3(TPB), 0, L.s, L.n, (const int64_t*)L.eg.off.p, (const int32_t*)L.eg.adj.p,
                       (const uint64_t*)L.u.p, (const int32_t*)L.label.p, (const uint64_t*)nullptr, (const uint64_t*)nullptr, p.cnt.p, p.sum.p, p.ext.p,
                       p.mn.p, p.key.p, p.own.p);
}
void stats_reduce_pass(st_labelling& L, const st_object_parts& p, st_cluster_parts& r) {
    const int64_t n = L.n; hipStream_t s = L.s;
    dbuf<int32_t> iota((size_t)n);
    vg_prof_scope ps("cluster_stats_reduce", (double)n * (16.0 * 2.0 + 52.0) + (double)L.n_clusters * 64.0);
    hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, iota.p, n);
    with_temp_storage([&](void* tmp, size_t& tb) {
        return rocprim::radix_sort_pairs(tmp, tb, (const uint32_t*)L.label.p, (uint32_t*)L.slabel.p, iota.p, L.order.p, (size_t)n, 0u,
                                         (unsigned)id_bits(L.n_clusters), s); });
    for (dbuf<unsigned long long>* b : { &r.cnt, &r.sum, &r.ext, &r.key, &r.mis, &r.nsum }) b->zero(s);
    VG_HIP(hipMemsetAsync(r.mn.p, 0xff, r.mn.bytes(), s));
    VG_HIP(hipMemsetAsync(r.begin.p, 0xff, r.begin.bytes(), s));
    hipLaunchKernelGGL(k_st_reduce<false>, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int32_t*)L.slabel.p, (const int32_t*)L.order.p,
                       (const uint64_t*)p.cnt.p, (const uint64_t*)p.sum.p, (const uint64_t*)p.ext.p, (const uint64_t*)p.mn.p,
                       (const uint64_t*)p.key.p, r.cnt.p, r.sum.p, r.ext.p, r.mn.p, r.key.p, r.begin.p, r.end.p, r.rep.p);
}
void stats_nearest_pass(const st_labelling& L, st_object_parts& p, st_cluster_parts& r, dbuf<vg_cluster_stat>& out) {
    const int64_t n = L.n; hipStream_t s = L.s;
    vg_prof_scope ps("cluster_stats_nearest", (double)L.eg.m * 16.0 + (double)n * 72.0 + (double)L.n_clusters * 176.0);
    hipLaunchKernelGGL(k_st_rows<true>, dim3(grid_of(n * ROW_LANES)), dim3(TPB), 0, s, n, (const int64_t*)L.eg.off.p, (const int32_t*)L.eg.adj.p,
                       (const uint64_t*)L.u.p, (const int32_t*)L.label.p, (const uint64_t*)r.ext.p, (const uint64_t*)r.key.p, p.mis.p, p.nsum.p, p.ext.p,
                       p.mn.p, p.key.p, p.own.p);
    hipLaunchKernelGGL(k_st_reduce<true>, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int32_t*)L.slabel.p, (const int32_t*)L.order.p,
                       (const uint64_t*)p.mis.p, (const uint64_t*)p.nsum.p, (const uint64_t*)nullptr, (const uint64_t*)nullptr,
                       (const uint64_t*)nullptr, r.mis.p, r.nsum.p, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                       (unsigned long long*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_st_finish, dim3(grid_of(L.n_clusters)), dim3(TPB), 0, s, L.n_clusters, (const int64_t*)r.begin.p, (const int64_t*)r.end.p,
                       (const int32_t*)r.rep.p, (const unsigned long long*)r.cnt.p, (const unsigned long long*)r.sum.p,
                       (const unsigned long long*)r.ext.p, (const unsigned long long*)r.mn.p, (const unsigned long long*)r.key.p,
                       (const unsigned long long*)r.mis.p, (const unsigned long long*)r.nsum.p, out.p);
}
// The report of one labelling on the edge graph (u: its quantised weights): the three passes, then the records and, if wanted,
// the per-object values leave the device.  label[] has been checked on the host.
void stats_on_device(int64_t n, const edge_graph& eg, const dbuf<uint64_t>& u, hipStream_t s, const int32_t* label, int64_t n_clusters,
                     vg_cluster_stat* out, uint64_t* own_max, uint64_t* other_max, int32_t* other) {
    st_labelling L{ n, n_clusters, eg, u, s, dbuf<int32_t>((size_t)n), dbuf<int32_t>((size_t)n), dbuf<int32_t>((size_t)n) };
    st_object_parts p((size_t)n);
    st_cluster_parts r((size_t)n_clusters);
    dbuf<vg_cluster_stat> d_out((size_t)n_clusters);
    L.label.upload(label, (size_t)n, s);
    stats_rows_pass(L, p);
    stats_reduce_pass(L, p, r);
    stats_nearest_pass(L, p, r, d_out);
    VG_HIP(hipGetLastError());
    d_out.download(out, (size_t)n_clusters, s);
    if (own_max) p.own.download(own_max, (size_t)n, s);
    if (other_max || other) {                                   // the best external key of every object, decoded here
        std::vector<uint64_t> key((size_t)n), ext((size_t)n);
        p.key.download(key.data(), (size_t)n, s); p.ext.download(ext.data(), (size_t)n, s);
        VG_HIP(hipStreamSynchronize(s));
        for (int64_t i = 0; i < n; ++i) {
            if (other_max) other_max[i] = ext[(size_t)i] ? st_key_u(key[(size_t)i]) : 0;
            if (other) other[i] = ext[(size_t)i] ? st_key_label(key[(size_t)i]) : -1;
        }
    }
    VG_HIP(hipStreamSynchronize(s));
}
}  // namespace

// The cluster report of n_cols labellings of one graph (vg_cluster_stats_graph: one; vg_cluster_stats_file: one per label column):
// the checks on the host, one graph build, one quantisation, then the passes per labelling.  The per-object arrays belong to
// labelling 0 and may be null.
void vg_cluster_stats_run(const char* fn, int64_t n, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows, int n_cols,
                          const int32_t* const* label, const int64_t* n_clusters, vg_cluster_stat* const* out, uint64_t* own_max,
                          uint64_t* other_max, int32_t* other) {
    const std::string name(fn);
    const row_list in{ n, q, r, w, n_rows };
    check_call(fn, in);
    for (int c = 0; c < n_cols; ++c) {
        if (n_clusters[c] < 0) throw vg_error(VG_EINVAL, name + ": negative number of clusters");
        if (n_clusters[c] >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, name + ": 2^31 or more clusters (labels are int32)");
        if ((n && !label[c]) || (n_clusters[c] && !out[c])) throw vg_error(VG_EINVAL, name + ": null argument");
    }
    check_row_values(fn, in);
    check_unit_weights(fn, in);
    for (int c = 0; c < n_cols; ++c) {
        const int64_t bad = first_bad_row(n, [&](int64_t i) { return label[c][i] < 0 || label[c][i] >= n_clusters[c]; });
        if (bad >= 0)
            throw vg_error(VG_EINVAL, name + ": label[" + std::to_string(bad) + "] = " + std::to_string(label[c][bad]) + " outside 0.." + std::to_string(n_clusters[c] - 1));
    }
    if (n == 0) {                                               // no member anywhere
        for (int c = 0; c < n_cols; ++c)
            for (int64_t x = 0; x < n_clusters[c]; ++x) { out[c][x] = vg_cluster_stat{}; out[c][x].rep = out[c][x].nearest = -1; }
        return;
    }
    edge_graph eg;
    hipStream_t s = graph_on_device(in, eg);
    check_edge_sums(name, eg.m / 2);
    dbuf<uint64_t> u((size_t)eg.m);
    hipLaunchKernelGGL(k_av_quantise, dim3(grid_of(eg.m)), dim3(TPB), 0, s, (const double*)eg.uvals.p, eg.m, u.p);
    VG_HIP(hipGetLastError());
    for (int c = 0; c < n_cols; ++c)
        stats_on_device(n, eg, u, s, label[c], n_clusters[c], out[c], c ? nullptr : own_max, c ? nullptr : other_max, c ? nullptr : other);
}

extern "C" int vg_cluster_stats_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                      const int32_t* label, int64_t n_clusters, vg_cluster_stat* out, uint64_t* own_max,
                                      uint64_t* other_max, int32_t* other) {
    VG_API_BEGIN
    vg_cluster_stats_run("vg_cluster_stats_graph", n_objects, q, r, w, n_rows, 1, &label, &n_clusters, &out, own_max, other_max, other);
    VG_API_END
}

extern "C" int vg_cluster_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                int algorithm, int32_t* label, int32_t* representative, vg_cluster_stats* stats) {
    VG_API_BEGIN
    const char* fn = "vg_cluster_graph";
    const row_list in{ n_objects, q, r, w, n_rows };
    check_call(fn, in, n_objects && (!label || !representative) ? "null output" : nullptr,
               algorithm < VG_CLUSTER_SINGLE || algorithm > VG_CLUSTER_COMPLETE ? "unknown algorithm" : nullptr);
    check_row_values(fn, in);
    vg_cluster_stats local; vg_cluster_stats& sts = cleared(stats, local);
    if (n_objects == 0) return VG_OK;
    const int64_t n = n_objects;
    edge_graph eg;
    hipStream_t s = graph_on_device(in, eg);
    sts.n_edges = eg.m / 2;
    dbuf<int32_t> root((size_t)n);
    switch (algorithm) {
        case VG_CLUSTER_SINGLE: single_on_device(n, eg, s, root, sts); break;
        case VG_CLUSTER_COMPLETE: { vg_forest f; complete_on_device(n, eg, s, root, false, f); sts.rounds = f.stats.rounds; } break;    // the floor cut: every merge
        case VG_CLUSTER_SET_COVER: set_cover_on_device(n, eg, s, root, sts); break;
        default: greedy_on_device(algorithm == VG_CLUSTER_UCLUST, n, eg, s, root, sts);
    }
    labels_to_host(n, root, algorithm == VG_CLUSTER_SET_COVER, s, label, representative);
    VG_API_END
}

// ---------------------------------------------------------------- update of a prior clustering
namespace {
// the prior array on the device and the visit ranks made of it: visit[object], its inverse, the number of prior objects
struct update_ranks { dbuf<int32_t> prior, visit, inv; int32_t n_prior = 0; };
void visit_ranks(const char* fn, int64_t n, const int32_t* prior_rep, hipStream_t s, update_ranks& vr) {
    for (dbuf<int32_t>* b : { &vr.prior, &vr.visit, &vr.inv }) b->alloc((size_t)n);
    dbuf<int32_t> flag((size_t)n), before((size_t)n), d_np(1);
    vr.prior.upload(prior_rep, (size_t)n, s);
    {
        vg_prof_scope ps("cluster_update_map", (double)n * 4.0 * 7.0);
        hipLaunchKernelGGL(k_new_flags, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)vr.prior.p, n, flag.p);
        exclusive_scan_i32(flag.p, before.p, n, s);
        hipLaunchKernelGGL(k_visit_rank, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)flag.p, (const int32_t*)before.p, n, vr.visit.p, vr.inv.p, d_np.p);
        d_np.download(&vr.n_prior, 1, s);
        VG_HIP(hipStreamSynchronize(s));
    }
    if (vr.n_prior < 0 || vr.n_prior > n) throw vg_error(VG_EHIP, std::string(fn) + ": the visit ranks are inconsistent (internal error)");
}
// the algorithm on the kept edges from the seeded state -> root[] on visit ranks
void seeded_on_device(int algorithm, int64_t n, const edge_graph& eg, const update_ranks& vr, hipStream_t s, dbuf<int32_t>& root, vg_cluster_stats& cs) {
    const int32_t *prior = vr.prior.p, *visit = vr.visit.p;
    if (algorithm == VG_CLUSTER_SINGLE) {
        {
            dbuf<int32_t> minv((size_t)n);
            vg_prof_scope ps("cluster_update_seed", (double)n * 4.0 * 8.0);
            hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(TPB), 0, s, minv.p, n);
            hipLaunchKernelGGL(k_seed_min, dim3(grid_of(n)), dim3(TPB), 0, s, prior, visit, n, minv.p);
            hipLaunchKernelGGL(k_seed_single, dim3(grid_of(n)), dim3(TPB), 0, s, prior, visit, (const int32_t*)minv.p, n, root.p);
        }
        single_on_device(n, eg, s, root, cs, true);
    } else
        greedy_on_device(algorithm == VG_CLUSTER_UCLUST, n, eg, s, root, cs, vr.n_prior, [&] {
            vg_prof_scope ps("cluster_update_seed", (double)n * 4.0 * 4.0);
            hipLaunchKernelGGL(k_seed_greedy, dim3(grid_of(n)), dim3(TPB), 0, s, prior, visit, n, root.p);
        });
}
// the outcome counts of the checked root[] -> d_cnt, and cid[] = the cluster ids back on object indices
void update_outcome(int64_t n, const dbuf<int32_t>& root, const update_ranks& vr, bool single, hipStream_t s, dbuf<unsigned long long>& d_cnt,
                    dbuf<int32_t>& cid) {
    d_cnt.zero(s);
    hipLaunchKernelGGL(k_update_counts, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)root.p, (const int32_t*)vr.prior.p, (const int32_t*)vr.visit.p, n,
                       vr.n_prior, single, d_cnt.p);
    hipLaunchKernelGGL(k_unmap, dim3(grid_of(n)), dim3(TPB), 0, s, (const int32_t*)root.p, (const int32_t*)vr.visit.p, (const int32_t*)vr.inv.p, n, cid.p);
}
}  // namespace

extern "C" int vg_cluster_update_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                       int algorithm, const int32_t* prior_rep, int32_t* label, int32_t* representative,
                                       vg_cluster_update_stats* stats) {
    VG_API_BEGIN
    const char* fn = "vg_cluster_update_graph";
    const row_list in{ n_objects, q, r, w, n_rows };
    const int64_t n = n_objects;
    const bool single = algorithm == VG_CLUSTER_SINGLE;
    check_call(fn, in, n && (!prior_rep || !label || !representative) ? "null argument" : nullptr,
               !single && algorithm != VG_CLUSTER_CDHIT && algorithm != VG_CLUSTER_UCLUST ? "the update of a prior clustering is single, cd-hit or uclust" : nullptr);
    check_row_values(fn, in);
    int64_t bad = first_bad_row(n, [&](int64_t i) { return prior_rep[i] < -1 || prior_rep[i] >= n; });
    if (bad >= 0) throw vg_error(VG_EINVAL, std::string(fn) + ": prior_rep[" + std::to_string(bad) + "] = " + std::to_string(prior_rep[bad]) + " outside -1.." + std::to_string(n - 1));
    bad = first_bad_row(n, [&](int64_t i) { return prior_rep[i] >= 0 && prior_rep[prior_rep[i]] != prior_rep[i]; });
    if (bad >= 0) throw vg_error(VG_EINVAL, std::string(fn) + ": prior_rep[" + std::to_string(bad) + "] = " + std::to_string(prior_rep[bad]) + " is not its own representative");
    vg_cluster_update_stats local; vg_cluster_update_stats& sts = cleared(stats, local);
    if (n == 0) return VG_OK;
    // visit ranks, the kept edges on them, the algorithm from the seeded state
    update_ranks vr;
    visit_ranks(fn, n, prior_rep, vg_stream(), vr);
    sts.n_prior = vr.n_prior; sts.n_new = n - vr.n_prior;
    edge_graph eg;
    hipStream_t s = graph_on_device(in, eg, visit_map{ vr.visit.p, vr.n_prior });
    sts.n_edges = eg.m / 2;
    dbuf<int32_t> root((size_t)n);
    vg_cluster_stats cs{};
    seeded_on_device(algorithm, n, eg, vr, s, root, cs);
    sts.rounds = cs.rounds; sts.sweep_objects = cs.sweep_objects;
    // outcome counts, then labels on object ids: numbering by earliest member; the representative is the frozen or founding one
    // (greedy: the cluster id itself) or the earliest member (single)
    dbuf<unsigned long long> d_cnt(5); dbuf<int32_t> cid((size_t)n);
    unsigned long long cnt[5] = {};
    labels_to_host(n, root, true, !single, s, label, representative,
                   [&]() -> const dbuf<int32_t>& { update_outcome(n, root, vr, single, s, d_cnt, cid); return cid; }, [&] { d_cnt.download(cnt, 5, s); });
    sts.joined_prior = (int64_t)cnt[0]; sts.joined_new = (int64_t)cnt[1]; sts.founded = (int64_t)cnt[2];
    sts.prior_merged = (int64_t)cnt[3] - (int64_t)cnt[4];
    VG_API_END
}

// ---------------------------------------------------------------- merge table and cuts (host numbering of <= n - 1 records)
void vg_cluster_forest(const char* fn, int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows, vg_forest& f,
                       int algorithm, double floor) {
    const row_list in{ n_objects, q, r, w, n_rows };
    check_call(fn, in);
    check_row_values(fn, in);
    if (algorithm != VG_CLUSTER_SINGLE && algorithm != VG_CLUSTER_COMPLETE && algorithm != VG_CLUSTER_AVERAGE)
        throw vg_error(VG_EINVAL, std::string(fn) + ": the merge table is single, complete or average linkage");
    if (algorithm == VG_CLUSTER_AVERAGE) {
        if (!(floor >= 0 && floor <= 1)) throw vg_error(VG_EINVAL, std::string(fn) + ": the floor must lie in [0, 1]");
        check_unit_weights(fn, in, "average linkage");
    }
    f = vg_forest{};
    if (n_objects == 0) return;
    edge_graph eg;
    hipStream_t s = graph_on_device(in, eg);
    dbuf<int32_t> comp;
    switch (algorithm) {
        case VG_CLUSTER_SINGLE: forest_on_device(n_objects, eg, s, f); break;
        case VG_CLUSTER_AVERAGE: average_on_device(n_objects, eg, floor, s, f); break;
        default: complete_on_device(n_objects, eg, s, comp, true, f);
    }
}

namespace {
// union-find over the forest records; the root of a set is its minimum member
struct min_sets {
    std::vector<int32_t> up;
    explicit min_sets(int64_t n) : up((size_t)n) { for (int64_t i = 0; i < n; ++i) up[(size_t)i] = (int32_t)i; }
    int32_t find(int32_t x) { while (up[(size_t)x] != x) { up[(size_t)x] = up[(size_t)up[(size_t)x]]; x = up[(size_t)x]; } return x; }
    int32_t join(int32_t a, int32_t b) { a = find(a); b = find(b); if (a > b) std::swap(a, b); up[(size_t)b] = a; return a; }
};
}  // namespace

void vg_forest_table(int64_t n, const vg_forest& f, int64_t* node_a, int64_t* node_b, int64_t* size) {
    min_sets sets(n);
    std::vector<int64_t> node((size_t)n), members((size_t)n, 1);        // of a set's root: its current node and its size
    for (int64_t i = 0; i < n; ++i) node[(size_t)i] = i;
    for (size_t k = 0; k < f.a.size(); ++k) {
        const int32_t ra = sets.find(f.a[k]), rb = sets.find(f.b[k]);
        if (ra == rb) throw vg_error(VG_EHIP, "vg_cluster_linkage: a forest edge inside one cluster (internal error)");
        node_a[k] = std::min(node[(size_t)ra], node[(size_t)rb]); node_b[k] = std::max(node[(size_t)ra], node[(size_t)rb]);
        const int64_t sz = members[(size_t)ra] + members[(size_t)rb];
        const int32_t root = sets.join(ra, rb);
        node[(size_t)root] = n + (int64_t)k; members[(size_t)root] = sz; size[k] = sz;
    }
}

void vg_forest_cut(int64_t n, const vg_forest& f, double level, int32_t* label, int32_t* rep) {
    min_sets sets(n);
    if (f.sum.empty()) { for (size_t k = 0; k < f.a.size() && f.w[k] >= level; ++k) sets.join(f.a[k], f.b[k]); }    // (the weights are non-increasing)
    else {                                                      // average linkage: on the exact (S, P), not on the rounded double
        const uint64_t T = av_quanta(level);
        for (size_t k = 0; k < f.a.size(); ++k) if (av_reaches(f.sum[k], f.pairs[k], T)) sets.join(f.a[k], f.b[k]);
    }
    std::vector<int32_t> members((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) { rep[i] = sets.find((int32_t)i); ++members[(size_t)rep[i]]; }
    // multi-member clusters 0.. by earliest member, then singletons in object order (as k_head_labels)
    std::vector<int32_t> head((size_t)n, 0);
    int32_t next = 0;
    for (int64_t i = 0; i < n; ++i) if (rep[i] == i && members[(size_t)i] >= 2) head[(size_t)i] = next++;
    for (int64_t i = 0; i < n; ++i) if (rep[i] == i && members[(size_t)i] == 1) head[(size_t)i] = next++;
    for (int64_t i = 0; i < n; ++i) label[i] = head[(size_t)rep[i]];
}

namespace {
void linkage_graph(const char* fn, int algorithm, int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                   int32_t* object_a, int32_t* object_b, double* weight, int64_t* node_a, int64_t* node_b,
                   int64_t* size, int64_t* n_merges, vg_linkage_stats* stats, double floor = 0.0, uint64_t* sum = nullptr, uint64_t* pairs = nullptr) {
    const bool average = algorithm == VG_CLUSTER_AVERAGE;
    check_call(fn, { n_objects, q, r, w, n_rows },
               !n_merges || (n_objects > 1 && (!object_a || !object_b || !weight || !node_a || !node_b || !size || (average && (!sum || !pairs)))) ? "null output" : nullptr);
    *n_merges = 0;
    if (stats) *stats = vg_linkage_stats{};
    vg_forest f;
    vg_cluster_forest(fn, n_objects, q, r, w, n_rows, f, algorithm, floor);
    const size_t nf = f.a.size();
    if (nf) {
        memcpy(object_a, f.a.data(), nf * sizeof(int32_t)); memcpy(object_b, f.b.data(), nf * sizeof(int32_t));
        memcpy(weight, f.w.data(), nf * sizeof(double));
        if (average) { memcpy(sum, f.sum.data(), nf * sizeof(uint64_t)); memcpy(pairs, f.pairs.data(), nf * sizeof(uint64_t)); }
        vg_forest_table(n_objects, f, node_a, node_b, size);
    }
    *n_merges = (int64_t)nf;
    if (stats) *stats = f.stats;
}
void levels_graph(const char* fn, int algorithm, int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                  const double* levels, int n_levels, int32_t* label, int32_t* representative, vg_linkage_stats* stats, double floor = 0.0) {
    const std::string name(fn);
    check_call(fn, { n_objects, q, r, w, n_rows });
    if (n_levels < 0 || (n_levels && !levels)) throw vg_error(VG_EINVAL, name + ": null levels");
    for (int l = 0; l < n_levels; ++l) if (std::isnan(levels[l])) throw vg_error(VG_EINVAL, name + ": a level is NaN");
    if (algorithm == VG_CLUSTER_AVERAGE)                        // (the hierarchy stops at the floor: there is nothing to cut below it)
        for (int l = 0; l < n_levels; ++l) if (levels[l] < floor) throw vg_error(VG_EINVAL, name + ": level " + std::to_string(levels[l]) + " is below the floor");
    if (n_objects && n_levels && (!label || !representative)) throw vg_error(VG_EINVAL, name + ": null output");
    if (stats) *stats = vg_linkage_stats{};
    vg_forest f;
    vg_cluster_forest(fn, n_objects, q, r, w, n_rows, f, algorithm, floor);
    for (int l = 0; l < n_levels; ++l) vg_forest_cut(n_objects, f, levels[l], label + (int64_t)l * n_objects, representative + (int64_t)l * n_objects);
    if (stats) *stats = f.stats;
}
}  // namespace

extern "C" int vg_cluster_linkage_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                        int32_t* object_a, int32_t* object_b, double* weight, int64_t* node_a, int64_t* node_b,
                                        int64_t* size, int64_t* n_merges, vg_linkage_stats* stats) {
    VG_API_BEGIN
    linkage_graph("vg_cluster_linkage_graph", VG_CLUSTER_SINGLE, n_objects, q, r, w, n_rows, object_a, object_b, weight, node_a, node_b, size, n_merges, stats);
    VG_API_END
}
extern "C" int vg_cluster_complete_linkage_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                                 int32_t* object_a, int32_t* object_b, double* weight, int64_t* node_a, int64_t* node_b,
                                                 int64_t* size, int64_t* n_merges, vg_linkage_stats* stats) {
    VG_API_BEGIN
    linkage_graph("vg_cluster_complete_linkage_graph", VG_CLUSTER_COMPLETE, n_objects, q, r, w, n_rows, object_a, object_b, weight, node_a, node_b, size, n_merges, stats);
    VG_API_END
}

extern "C" int vg_cluster_levels_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                       const double* levels, int n_levels, int32_t* label, int32_t* representative,
                                       vg_linkage_stats* stats) {
    VG_API_BEGIN
    levels_graph("vg_cluster_levels_graph", VG_CLUSTER_SINGLE, n_objects, q, r, w, n_rows, levels, n_levels, label, representative, stats);
    VG_API_END
}
extern "C" int vg_cluster_complete_levels_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                                const double* levels, int n_levels, int32_t* label, int32_t* representative,
                                                vg_linkage_stats* stats) {
    VG_API_BEGIN
    levels_graph("vg_cluster_complete_levels_graph", VG_CLUSTER_COMPLETE, n_objects, q, r, w, n_rows, levels, n_levels, label, representative, stats);
    VG_API_END
}

extern "C" int vg_cluster_average_linkage_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                                double floor, int32_t* object_a, int32_t* object_b, double* similarity, uint64_t* sum,
                                                uint64_t* pairs, int64_t* node_a, int64_t* node_b, int64_t* size, int64_t* n_merges,
                                                vg_linkage_stats* stats) {
    VG_API_BEGIN
    linkage_graph("vg_cluster_average_linkage_graph", VG_CLUSTER_AVERAGE, n_objects, q, r, w, n_rows, object_a, object_b, similarity, node_a, node_b, size,
                  n_merges, stats, floor, sum, pairs);
    VG_API_END
}
extern "C" int vg_cluster_average_levels_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                               double floor, const double* levels, int n_levels, int32_t* label, int32_t* representative,
                                               vg_linkage_stats* stats) {
    VG_API_BEGIN
    levels_graph("vg_cluster_average_levels_graph", VG_CLUSTER_AVERAGE, n_objects, q, r, w, n_rows, levels, n_levels, label, representative, stats, floor);
    VG_API_END
}

// ---------------------------------------------------------------- test entries of the average-linkage arithmetic
extern "C" double vg_cluster_average_similarity(uint64_t sum, uint64_t pairs) { return av_similarity(sum, pairs); }

extern "C" int vg_cluster_average_order_selftest(const uint64_t* sum, const uint32_t* size_c, const uint32_t* size_d, const uint32_t* c,
                                                 const uint32_t* d, int64_t n, int on_device, int8_t* out) {
    VG_API_BEGIN
    if (n < 0 || (n > 0 && (!sum || !size_c || !size_d || !c || !d)) || (n > 1 && !out))
        throw vg_error(VG_EINVAL, "vg_cluster_average_order_selftest: null argument");
    if (n < 2) return VG_OK;
    if (!on_device) {
        auto cand = [&](int64_t i) { return av_cand{ sum[i], (uint64_t)size_c[i] * size_d[i], std::min(c[i], d[i]), std::max(c[i], d[i]) }; };
        for (int64_t i = 0; i + 1 < n; ++i) out[i] = (int8_t)av_compare(cand(i), cand(i + 1));
        return VG_OK;
    }
    vg_require_device();
    hipStream_t s = vg_stream();
    dbuf<uint64_t> ds((size_t)n); dbuf<uint32_t> dsc((size_t)n), dsd((size_t)n), dc((size_t)n), dd((size_t)n); dbuf<int8_t> dout((size_t)n - 1);
    ds.upload(sum, (size_t)n, s); dsc.upload(size_c, (size_t)n, s); dsd.upload(size_d, (size_t)n, s); dc.upload(c, (size_t)n, s); dd.upload(d, (size_t)n, s);
    hipLaunchKernelGGL(k_av_order, dim3(grid_of(n - 1)), dim3(TPB), 0, s, (const uint64_t*)ds.p, (const uint32_t*)dsc.p, (const uint32_t*)dsd.p,
                       (const uint32_t*)dc.p, (const uint32_t*)dd.p, n, dout.p);
    VG_HIP(hipGetLastError());
    dout.download(out, (size_t)n - 1, s);
    VG_HIP(hipStreamSynchronize(s));
    VG_API_END
}

// ---------------------------------------------------------------- Markov clustering ("Markov clustering")
// The flow matrix in integers: an entry is col << 32 | p, p a uint32 in units of 2^-30; row i is ent[off[i] .. off[i] + cnt[i]) in
// any order (every step below is a sum, a maximum or a choice by a unique key, so the order never shows).  One iteration:
//   plan      the candidate bound of every row (the sum of nnz over the rows it names, and no more than n: its columns are
//             objects), its kernel by that bound -- a wave or a workgroup --, the storage of the next matrix (min(max_row, bound)
//             per row, one scan); one read-back
//   expand    a row per wave / workgroup: (column, value) pairs of the named rows gathered 16 lanes a row, products added into an
//             open-addressing hash table in LDS (column claimed by compare-and-swap, 64-bit sums by LDS atomics), then the finish
//   spill     rows whose bound exceeds the table and whose distinct columns, tried in it, fill more than 3/4 of it: (row, column,
//             product) records, one radix sort, reduce-by-key, the same finish over the row's segment of the reduced records, in
//             place in global memory
//   finish    inflation, normalisation, pruning (cut, then a radix select of the max_row largest keys p << 32 | ~column),
//             normalisation, the row's chaos; it touches the candidate array a[0 .. L) (0 = no entry) only at a thread's own strided
//             positions, so LDS table and global segment are the same code
namespace {
constexpr uint64_t MCL_ONE = 1ull << 30;
constexpr uint32_t MCL_EMPTY = 0xffffffffu;        // (no column: columns are < 2^31)
constexpr int MCL_WAVE_SLOTS = 512;                 // 6 KiB of table: a one-wave workgroup per row
constexpr int MCL_GROUP_SLOTS = 4096;               // 48 KiB of table: three 256-thread workgroups on a CU's 160 KiB
constexpr int MCL_SUB = 16;                         // lanes that read one named row: 16 pairs = 128 bytes
constexpr int64_t MCL_SPILL_BATCH = 1ll << 25;      // spill records sorted at once (a row above it is a batch of its own)
// the counters of one iteration: MC_WAVE .. MC_STORAGE are the plan's (MC_TRY: group rows whose bound exceeds the table), MC_SPILL
// counts the rows the group kernel hands on
enum { MC_CHAOS, MC_BAD, MC_WAVE, MC_GROUP, MC_TRY, MC_STORAGE, MC_SPILL, MC_N };
std::atomic<int> g_mcl_slots{ 0 };

struct mcl_matrix { dbuf<int64_t> off; dbuf<int32_t> cnt; dbuf<uint64_t> ent; };
struct mcl_dev { int a; uint32_t cut; int max_row; };       // inflation = a / 2, cut = floor(prune * ONE)
struct mcl_scratch { uint32_t hist[256]; uint64_t red[4]; uint32_t n_out, n_keys, full; };

// floor(sqrt(x)), x <= 2^60: the double root is off by a few units at most, integer compares settle it
__device__ __forceinline__ uint64_t mcl_isqrt(uint64_t x) {
    uint64_t s = (uint64_t)sqrt((double)x);
    while (s * s > x) --s;
    while ((s + 1) * (s + 1) <= x) ++s;
    return s;
}
// y^(a / 2), y <= ONE: every intermediate is <= ONE and every product <= 2^60
__device__ __forceinline__ uint64_t mcl_power(uint64_t y, int a) {
    uint64_t t = (a & 1) ? mcl_isqrt(y << 30) : MCL_ONE;
    for (int k = a >> 1; k > 0; --k) t = (t * y) >> 30;
    return t;
}
// the candidate of value p in column col: larger p first, then the smaller column; no entry is 0 (a key has p >= 1)
__device__ __forceinline__ uint64_t mcl_key(uint64_t p, uint32_t col) { return p ? p << 32 | (uint32_t)~col : 0; }

template <int T> __device__ __forceinline__ uint64_t mcl_sum(uint64_t v, mcl_scratch& sc) {
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    if (T == 64) return v;
    if ((threadIdx.x & 63) == 0) sc.red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int x = 0; x < T / 64; ++x) v += sc.red[x];
    __syncthreads();
    return v;
}
template <int T> __device__ __forceinline__ uint64_t mcl_max(uint64_t v, mcl_scratch& sc) {
    for (int o = 32; o > 0; o >>= 1) v = umax64(v, (uint64_t)__shfl_xor((unsigned long long)v, o));
    if (T == 64) return v;
    if ((threadIdx.x & 63) == 0) sc.red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int x = 0; x < T / 64; ++x) v = umax64(v, sc.red[x]);
    __syncthreads();
    return v;
}

// The finish of one row by a workgroup of T threads.  a[0 .. L), L >= 1: mcl_key(inflated value, column) or 0, in LDS or in global
// memory; out[0 .. cap): the row's storage in the next matrix.  Steps 2 (its end) to 6 of the definition.
template <int T>
__device__ __forceinline__ void mcl_finish(uint64_t* a, int L, int32_t row, const mcl_dev P, mcl_scratch& sc, uint64_t* out, int64_t cap,
                                           int32_t* out_cnt, unsigned long long* ctr) {
    const int t = threadIdx.x;
    uint64_t s = 0;
    for (int x = t; x < L; x += T) s += a[x] >> 32;
    uint64_t S = mcl_sum<T>(s, sc);
    if (S == 0) { if (t == 0) a[0] = mcl_key(MCL_ONE, (uint32_t)row); S = MCL_ONE; }      // nothing survived inflation: the loop alone
    // normalise, then the cut; `best` is the largest normalised candidate, kept if none passes
    uint64_t best = 0, kept = 0;
    for (int x = t; x < L; x += T) {
        const uint64_t k = a[x];
        if (!k) continue;
        const uint64_t p = ((k >> 32) << 30) / S;
        uint64_t nk = p ? p << 32 | (uint32_t)k : 0;
        best = umax64(best, nk);
        if (p < P.cut) nk = 0;
        a[x] = nk; kept += nk != 0;
    }
    best = mcl_max<T>(best, sc); kept = mcl_sum<T>(kept, sc);
    if (kept == 0) { if (t == 0) a[0] = best; kept = 1; }
    if (kept > (uint64_t)P.max_row) {
        // radix select, 8 bits a pass from the top: `prefix` becomes the max_row-th largest key (keys are unique)
        uint64_t prefix = 0; uint32_t need = (uint32_t)P.max_row;
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int x = t; x < 256; x += T) sc.hist[x] = 0;
            __syncthreads();
            for (int x = t; x < L; x += T) {
                const uint64_t k = a[x];
                if (k && (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&sc.hist[(k >> shift) & 255], 1u);
            }
            __syncthreads();
            int d = 255; uint32_t above = 0;                    // every thread walks the histogram down (broadcast reads)
            for (; d > 0; --d) { const uint32_t h = sc.hist[d]; if (above + h >= need) break; above += h; }
            need -= above; prefix |= (uint64_t)d << shift;
            __syncthreads();
        }
        for (int x = t; x < L; x += T) if (a[x] < prefix) a[x] = 0;
    }
    uint64_t s2 = 0;
    for (int x = t; x < L; x += T) s2 += a[x] >> 32;
    const uint64_t S2 = mcl_sum<T>(s2, sc);
    if (t == 0) sc.n_out = 0;
    __syncthreads();
    uint64_t mx = 0, sq = 0; bool over = false;
    for (int x = t; x < L; x += T) {
        const uint64_t k = a[x];
        if (!k) continue;
        const uint64_t p = ((k >> 32) << 30) / S2;
        if (!p) continue;
        const uint32_t slot = atomicAdd(&sc.n_out, 1u);
        if ((int64_t)slot < cap) out[slot] = (uint64_t)(~(uint32_t)k) << 32 | p; else over = true;
        mx = umax64(mx, p); sq += p * p;
    }
    if (over) atomicMax(ctr + MC_BAD, 1ull);
    mx = mcl_max<T>(mx, sc); sq = mcl_sum<T>(sq, sc);
    __syncthreads();
    if (t == 0) {
        out_cnt[row] = (int32_t)((int64_t)sc.n_out < cap ? (int64_t)sc.n_out : cap);
        atomicMax(ctr + MC_CHAOS, (unsigned long long)(mx - (sq >> 30)));
    }
    __syncthreads();
}

// start: one pass over the CSR and the quantised weights u; row i gets the deg(i) + 1 slots behind off[i] = eoff[i] + i.  (A row
// whose weights all quantise to 0 gets the loop of an object without edges: there is nothing to normalise by otherwise.)
__global__ void k_mcl_start(int64_t n, const int64_t* eoff, const int32_t* adj, const uint64_t* u, int64_t* off, int32_t* cnt, uint64_t* ent) {
    GRID_STRIDE(i, n) {
        const int64_t lo = eoff[i], hi = eoff[i + 1], base = lo + i;
        uint64_t mx = 0, sum = 0;
        for (int64_t k = lo; k < hi; ++k) { mx = umax64(mx, u[k]); sum += u[k]; }
        const uint64_t loop = mx ? mx : MCL_ONE, S = sum + loop;
        int32_t c = 0;
        for (int64_t k = lo; k < hi; ++k) {
            const uint64_t p = u[k] * MCL_ONE / S;
            if (p) ent[base + c++] = (uint64_t)(uint32_t)adj[k] << 32 | p;
        }
        const uint64_t p = loop * MCL_ONE / S;
        if (p) ent[base + c++] = (uint64_t)i << 32 | p;
        off[i] = base; cnt[i] = c;
    }
}
// plan, step 1: bound[i] = the sum of nnz over the rows that row i names (ROW_LANES lanes a row)
__global__ void k_mcl_bound(int64_t n, const int64_t* off, const int32_t* cnt, const uint64_t* ent, int64_t* bound) {
    const int lane = threadIdx.x % ROW_LANES;
    const int64_t groups = (int64_t)gridDim.x * blockDim.x / ROW_LANES;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / ROW_LANES; i < n; i += groups) {
        const int64_t o = off[i];
        uint64_t b = 0;
        for (int32_t e = lane, c = cnt[i]; e < c; e += ROW_LANES) b += (uint64_t)cnt[ent[o + e] >> 32];
        for (int x = ROW_LANES / 2; x > 0; x >>= 1) b += (uint64_t)__shfl_xor((unsigned long long)b, x);
        if (lane == 0) bound[i] = (int64_t)b;
    }
}
// plan, step 2: the row lists of the two kernels (one atomic per wave and class), the rows among the workgroup's whose bound exceeds
// the table counted, and the storage bound of every row with its total
__global__ void k_mcl_classify(int64_t n, const int64_t* bound, int64_t wave_cap, int64_t group_cap, int64_t max_row, int32_t* wave_rows,
                               int32_t* group_rows, int64_t* store, unsigned long long* ctr) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {      // (whole waves stay together for the ballots)
        const int64_t i = base + threadIdx.x;
        const bool live = i < n;
        const int64_t b = live ? bound[i] : 0, distinct = b < n ? b : n;       // (a row has no more distinct columns than there are objects)
        const int cls = !live ? -1 : distinct <= wave_cap ? 0 : 1;
        for (int c = 0; c < 2; ++c) {
            const uint64_t mask = __ballot(cls == c);
            if (!mask) continue;
            const int leader = __builtin_ctzll(mask);
            unsigned long long at = 0;
            if (lane == leader) at = atomicAdd(ctr + MC_WAVE + c, (unsigned long long)__builtin_popcountll(mask));
            at = __shfl(at, leader);
            if (cls != c) continue;
            at += (unsigned long long)__builtin_popcountll(mask & ((1ull << lane) - 1));
            if (c == 0) wave_rows[at] = (int32_t)i; else group_rows[at] = (int32_t)i;
        }
        const uint64_t above = __ballot(live && distinct > group_cap);
        if (lane == 0 && above) atomicAdd(ctr + MC_TRY, (unsigned long long)__builtin_popcountll(above));
        uint64_t keep = live ? (uint64_t)(distinct < max_row ? distinct : max_row) : 0;
        if (live) store[i] = (int64_t)keep;
        for (int o = 32; o > 0; o >>= 1) keep += (uint64_t)__shfl_xor((unsigned long long)keep, o);
        if (lane == 0 && keep) atomicAdd(ctr + MC_STORAGE, (unsigned long long)keep);
    }
}
// expand + finish in LDS, one row per workgroup of T threads (T = 64: a wave).  slots <= SLOTS is the table a row may use (the
// developer knob lowers it); a row takes the power of two that holds twice its bound, so clearing and scanning follow the row's size.
// min(bound, n) >= the distinct columns: a row with that <= slots always finds a slot (the probe count is a guard).  A row whose
// bound EXCEEDS the table (only the workgroup kernel gets such rows) is tried all the same -- the bound counts every product, the
// distinct columns of a row inside a family are far fewer -- with its claimed slots counted: once more than 3/4 of the table is
// claimed the row is given up and appended to the spill list.  That happens iff the row has more distinct columns than that, whatever
// the order of the claims, so which rows spill is as fixed as everything else.
template <int T, int SLOTS>
__global__ void __launch_bounds__(T) k_mcl_expand(int64_t n, const int32_t* rows, int64_t n_rows, const int64_t* off, const int32_t* cnt, const uint64_t* ent,
                                                  const int64_t* bound, int slots, const mcl_dev P, const int64_t* off_next, const int64_t* store,
                                                  int32_t* cnt_next, uint64_t* ent_next, int32_t* spill_rows, int64_t* spill_bound,
                                                  unsigned long long* ctr) {
    __shared__ uint32_t keys[SLOTS];
    __shared__ uint64_t acc[SLOTS];
    __shared__ mcl_scratch sc;
    const int t = threadIdx.x, sub = t / MCL_SUB, sl = t % MCL_SUB;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t i = rows[r];
        const int64_t distinct = bound[i] < n ? bound[i] : n;
        int lg = 6;
        while ((1 << lg) < slots && (int64_t)(1 << lg) < 2 * distinct) ++lg;
        if ((1 << lg) > slots) lg = 31 - __builtin_clz((unsigned)slots);
        const int ts = 1 << lg;
        const bool tried = distinct > slots;                    // (then ts == slots)
        const uint32_t limit = (uint32_t)(ts - ts / 4);
        for (int x = t; x < ts; x += T) { keys[x] = MCL_EMPTY; acc[x] = 0; }
        if (t == 0) { sc.n_keys = 0; sc.full = 0; }
        __syncthreads();
        const int64_t o = off[i];
        bool lost = false;
        for (int32_t e = sub, c = cnt[i]; e < c; e += T / MCL_SUB) {
            if (tried && *(volatile uint32_t*)&sc.full) break;
            const uint64_t ik = ent[o + e];
            const uint32_t k = (uint32_t)(ik >> 32);
            const uint64_t p = (uint32_t)ik;
            const int64_t ok = off[k];
            for (int32_t j = sl, ck = cnt[k]; j < ck; j += MCL_SUB) {
                const uint64_t kj = ent[ok + j];
                const uint32_t col = (uint32_t)(kj >> 32);
                uint32_t h = (col * 2654435761u) >> (32 - lg);
                int probe = 0;
                for (; probe < ts; ++probe) {
                    const uint32_t prev = atomicCAS(&keys[h], MCL_EMPTY, col);
                    if (prev == MCL_EMPTY && tried && atomicAdd(&sc.n_keys, 1u) >= limit) *(volatile uint32_t*)&sc.full = 1;
                    if (prev == MCL_EMPTY || prev == col) break;
                    h = (h + 1) & (uint32_t)(ts - 1);
                }
                if (probe < ts) atomicAdd((unsigned long long*)&acc[h], (unsigned long long)(p * (uint32_t)kj));
                else if (tried) *(volatile uint32_t*)&sc.full = 1;       // (claims in flight filled the rest: the count has passed the limit)
                else lost = true;
            }
        }
        if (lost) atomicMax(ctr + MC_BAD, 1ull);
        __syncthreads();
        if (tried && sc.full) {                                 // uniform: the row goes to the spill path
            if (t == 0) { const unsigned long long at = atomicAdd(ctr + MC_SPILL, 1ull); spill_rows[at] = i; spill_bound[at] = bound[i]; }
            __syncthreads();
            continue;
        }
        for (int x = t; x < ts; x += T) {
            const uint32_t col = keys[x];
            acc[x] = col == MCL_EMPTY ? 0 : mcl_key(mcl_power(acc[x] >> 30, P.a), col);
        }
        mcl_finish<T>(acc, ts, i, P, sc, ent_next + off_next[i], store[i], cnt_next, ctr);
    }
}
// spill, step 1: the records of one batch of rows, a workgroup per row; the row's bound records start where the batch's cursor stood
__global__ void __launch_bounds__(TPB) k_mcl_spill_emit(const int32_t* rows, const int64_t* row_bound, int64_t n_rows, const int64_t* off,
                                                        const int32_t* cnt, const uint64_t* ent, unsigned long long* cursor, int64_t rec_cap,
                                                        uint64_t* rkey, uint64_t* rval, unsigned long long* ctr) {
    __shared__ unsigned long long first;
    const int t = threadIdx.x;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t i = rows[r];
        const int64_t b = row_bound[r];
        if (t == 0) first = atomicAdd(cursor, (unsigned long long)b);
        __syncthreads();
        int64_t pos = (int64_t)first;
        __syncthreads();
        if (pos + b > rec_cap) { if (t == 0) atomicMax(ctr + MC_BAD, 1ull); continue; }
        const int64_t o = off[i], end = pos + b;
        for (int32_t e = 0, c = cnt[i]; e < c; ++e) {
            const uint64_t ik = ent[o + e];
            const uint32_t k = (uint32_t)(ik >> 32);
            const uint64_t p = (uint32_t)ik;
            const int64_t ok = off[k];
            const int32_t ck = cnt[k];
            for (int32_t j = t; j < ck && pos + j < end; j += TPB) {
                const uint64_t kj = ent[ok + j];
                rkey[pos + j] = (uint64_t)(uint32_t)i << 32 | (kj >> 32);
                rval[pos + j] = p * (uint32_t)kj;
            }
            pos += ck;
        }
    }
}
// spill, step 2 (after the sort and reduce-by-key): the row's segment of the reduced records becomes its candidate array, in place
__global__ void __launch_bounds__(TPB) k_mcl_spill_finish(const int32_t* rows, int64_t n_rows, const uint64_t* gkey, uint64_t* gval,
                                                          const unsigned long long* n_groups, const mcl_dev P, const int64_t* off_next,
                                                          const int64_t* store, int32_t* cnt_next, uint64_t* ent_next, unsigned long long* ctr) {
    __shared__ mcl_scratch sc;
    const int t = threadIdx.x;
    const int64_t ng = (int64_t)*n_groups;
    auto lower = [&](uint64_t key) { int64_t lo = 0, hi = ng; while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (gkey[mid] < key) lo = mid + 1; else hi = mid; } return lo; };
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int32_t i = rows[r];
        const int64_t lo = lower((uint64_t)(uint32_t)i << 32), hi = lower(((uint64_t)(uint32_t)i + 1) << 32);
        if (hi <= lo) { if (t == 0) atomicMax(ctr + MC_BAD, 1ull); continue; }      // (a row always has candidates)
        for (int64_t x = lo + t; x < hi; x += TPB) gval[x] = mcl_key(mcl_power(gval[x] >> 30, P.a), (uint32_t)gkey[x]);
        mcl_finish<TPB>(gval + lo, (int)(hi - lo), i, P, sc, ent_next + off_next[i], store[i], cnt_next, ctr);
    }
}
// the last matrix: an undirected edge per entry off the diagonal for the hooking (larger end first: k_hook reads those), the
// (row, column) keys of the CSR output if it is wanted, entries and widest row.  Storage between the rows stays as it was filled.
__global__ void k_mcl_last(int64_t n, const int64_t* off, const int32_t* cnt, const uint64_t* ent, uint64_t* hook, uint64_t* ckey, uint32_t* cval,
                           unsigned long long* tally) {
    int nnz = 0; unsigned long long widest = 0;
    GRID_STRIDE(i, n) {
        const int64_t o = off[i];
        const int32_t c = cnt[i];
        for (int32_t e = 0; e < c; ++e) {
            const uint64_t x = ent[o + e], col = x >> 32, row = (uint64_t)i;
            hook[o + e] = col == row ? 0 : (col > row ? col << 32 | row : row << 32 | col);
            if (ckey) { ckey[o + e] = row << 32 | col; cval[o + e] = (uint32_t)x; }
        }
        nnz += c; widest = umax64(widest, (uint64_t)c);
    }
    add_count(tally, nnz);
    if (widest) atomicMax(tally + 1, widest);
}

void check_mcl_params(const std::string& fn, const vg_mcl_params* p) {
    if (!p) throw vg_error(VG_EINVAL, fn + ": null parameters");
    const double twice = 2 * p->inflation;
    if (!(p->inflation >= 1.5 && p->inflation <= 6) || !(std::fabs(twice - (double)llrint(twice)) < 1e-9))
        throw vg_error(VG_EINVAL, fn + ": inflation " + std::to_string(p->inflation) + " must be a multiple of 0.5 in [1.5, 6]");
    if (!(p->prune >= 0 && p->prune <= 0.1)) throw vg_error(VG_EINVAL, fn + ": prune " + std::to_string(p->prune) + " must lie in [0, 0.1]");
    if (p->max_row < 2 || p->max_row > 4096) throw vg_error(VG_EINVAL, fn + ": max_row " + std::to_string(p->max_row) + " must lie in [2, 4096]");
    if (!(p->chaos_eps >= 0 && p->chaos_eps < 1)) throw vg_error(VG_EINVAL, fn + ": chaos_eps " + std::to_string(p->chaos_eps) + " must lie in [0, 1)");
    if (p->max_iterations < 1 || p->max_iterations > 1000)
        throw vg_error(VG_EINVAL, fn + ": max_iterations " + std::to_string(p->max_iterations) + " must lie in [1, 1000]");
}

// The plan of one iteration over M: row lists, the offsets and the storage of the next matrix; h = the read-back (with the chaos of
// the expansion that produced M)
struct mcl_plan {
    dbuf<int64_t> bound, spill_bound, store, off_next; dbuf<int32_t> wave_rows, group_rows, spill_rows;
    unsigned long long h[MC_N] = {};
};
void mcl_make_plan(int64_t n, const mcl_matrix& M, int slots, int max_row, dbuf<unsigned long long>& ctr, hipStream_t s, mcl_plan& pl) {
    vg_prof_scope ps("cluster_mcl_plan", (double)n * 60.0);
    pl.off_next.alloc((size_t)n);
    VG_HIP(hipMemsetAsync(ctr.p + MC_WAVE, 0, (MC_N - MC_WAVE) * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_mcl_bound, dim3(grid_of(n * ROW_LANES)), dim3(TPB), 0, s, n, (const int64_t*)M.off.p, (const int32_t*)M.cnt.p,
                       (const uint64_t*)M.ent.p, pl.bound.p);
    hipLaunchKernelGGL(k_mcl_classify, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int64_t*)pl.bound.p, (int64_t)std::min(MCL_WAVE_SLOTS, slots),
                       (int64_t)std::min(MCL_GROUP_SLOTS, slots), (int64_t)max_row, pl.wave_rows.p, pl.group_rows.p, pl.store.p, ctr.p);
    with_temp_storage([&](void* tmp, size_t& tb) {
        return rocprim::exclusive_scan(tmp, tb, pl.store.p, pl.off_next.p, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), s); });
    VG_HIP(hipGetLastError());
    ctr.download(pl.h, MC_N, s);
    VG_HIP(hipStreamSynchronize(s));
    if (pl.h[MC_BAD]) throw vg_error(VG_EHIP, "vg_cluster_mcl_graph: a row lost candidates (internal error)");
    if ((int64_t)(pl.h[MC_WAVE] + pl.h[MC_GROUP]) != n) throw vg_error(VG_EHIP, "vg_cluster_mcl_graph: the row classes do not add up (internal error)");
}

// the ns spill rows of one iteration (the list the group kernel filled), in batches of at most MCL_SPILL_BATCH records
void mcl_spill(int64_t n, int64_t ns, const mcl_matrix& M, mcl_matrix& N, const mcl_plan& pl, const mcl_dev& P, dbuf<unsigned long long>& ctr,
               hipStream_t s) {
    std::vector<int64_t> hb((size_t)ns);
    pl.spill_bound.download(hb.data(), (size_t)ns, s);
    VG_HIP(hipStreamSynchronize(s));
    dbuf<unsigned long long> cursor(1), n_groups(1);
    const unsigned key_bits = 32u + (unsigned)id_bits(n);
    for (int64_t from = 0; from < ns;) {
        int64_t to = from, recs = 0;
        while (to < ns && (to == from || recs + hb[(size_t)to] <= MCL_SPILL_BATCH)) recs += hb[(size_t)to++];
        const int64_t rows = to - from;
        if (recs >= (1LL << 31)) throw vg_error(VG_EOVERFLOW, "vg_cluster_mcl_graph: one row has 2^31 or more candidates");
        dbuf<uint64_t> rkey((size_t)recs), rval((size_t)recs), skey((size_t)recs), sval((size_t)recs);
        {
            vg_prof_scope ps("cluster_mcl_spill_emit", (double)recs * 24.0);
            cursor.zero(s);
            hipLaunchKernelGGL(k_mcl_spill_emit, dim3((unsigned)std::min<int64_t>(rows, 1 << 20)), dim3(TPB), 0, s, (const int32_t*)pl.spill_rows.p + from,
                               (const int64_t*)pl.spill_bound.p + from, rows, (const int64_t*)M.off.p, (const int32_t*)M.cnt.p, (const uint64_t*)M.ent.p,
                               cursor.p, recs, rkey.p, rval.p, ctr.p);
        }
        {
            vg_prof_scope ps("cluster_mcl_spill_sort", (double)recs * (32.0 * 2.0 + 32.0));
            with_temp_storage([&](void* tmp, size_t& tb) {
                return rocprim::radix_sort_pairs(tmp, tb, rkey.p, skey.p, rval.p, sval.p, (size_t)recs, 0u, key_bits, s); });
            with_temp_storage([&](void* tmp, size_t& tb) {       // -> (row, column, sum of products) in rkey / rval
                return rocprim::reduce_by_key(tmp, tb, skey.p, sval.p, (size_t)recs, rkey.p, rval.p, n_groups.p, rocprim::plus<uint64_t>(),
                                              rocprim::equal_to<uint64_t>(), s); });
        }
        {
            vg_prof_scope ps("cluster_mcl_spill_finish", (double)recs * 16.0);
            hipLaunchKernelGGL(k_mcl_spill_finish, dim3((unsigned)std::min<int64_t>(rows, 1 << 20)), dim3(TPB), 0, s, (const int32_t*)pl.spill_rows.p + from,
                               rows, (const uint64_t*)rkey.p, rval.p, (const unsigned long long*)n_groups.p, P, (const int64_t*)N.off.p,
                               (const int64_t*)pl.store.p, N.cnt.p, N.ent.p, ctr.p);
        }
        VG_HIP(hipGetLastError());
        from = to;
    }
}

// what the stages of one run share: the device parameters, the table size, the counters
struct mcl_run { const int64_t n; const hipStream_t s; const mcl_dev P; const int slots; dbuf<unsigned long long> ctr; };

// the start matrix from the edge graph (released behind it), and the plan of the first iteration
void mcl_start_matrix(mcl_run& R, edge_graph& eg, mcl_matrix& M, mcl_plan& pl) {
    const int64_t n = R.n; hipStream_t s = R.s;
    {
        dbuf<uint64_t> u((size_t)std::max<int64_t>(eg.m, 1));
        M.off.alloc((size_t)n); M.cnt.alloc((size_t)n); M.ent.alloc((size_t)(eg.m + n));
        vg_prof_scope ps("cluster_mcl_start", (double)eg.m * 28.0 + (double)n * 28.0);
        hipLaunchKernelGGL(k_av_quantise, dim3(grid_of(eg.m)), dim3(TPB), 0, s, (const double*)eg.uvals.p, eg.m, u.p);
        hipLaunchKernelGGL(k_mcl_start, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int64_t*)eg.off.p, (const int32_t*)eg.adj.p, (const uint64_t*)u.p,
                           M.off.p, M.cnt.p, M.ent.p);
        VG_HIP(hipGetLastError());
    }
    eg = edge_graph{};
    R.ctr.alloc(MC_N);
    R.ctr.zero(s);
    pl.bound.alloc((size_t)n); pl.spill_bound.alloc((size_t)n); pl.store.alloc((size_t)n);
    pl.wave_rows.alloc((size_t)n); pl.group_rows.alloc((size_t)n); pl.spill_rows.alloc((size_t)n);
    mcl_make_plan(n, M, R.slots, R.P.max_row, R.ctr, s, pl);
}
// the nr rows of one class expanded from M into N, a row per T-thread workgroup with a table of at most SLOTS slots
template <int T, int SLOTS>
void mcl_expand_rows(const char* scope, double bytes, mcl_run& R, const dbuf<int32_t>& rows, int64_t nr, const mcl_matrix& M, mcl_matrix& N, mcl_plan& pl) {
    vg_prof_scope ps(scope, bytes);
    hipLaunchKernelGGL((k_mcl_expand<T, SLOTS>), dim3((unsigned)std::min<int64_t>(nr, 1 << 20)), dim3(T), 0, R.s, R.n, (const int32_t*)rows.p, nr,
                       (const int64_t*)M.off.p, (const int32_t*)M.cnt.p, (const uint64_t*)M.ent.p, (const int64_t*)pl.bound.p,
                       std::min(SLOTS, R.slots), R.P, (const int64_t*)N.off.p, (const int64_t*)pl.store.p, N.cnt.p, N.ent.p,
                       pl.spill_rows.p, pl.spill_bound.p, R.ctr.p);
}
// One iteration: M expanded by its plan (the two LDS kernels, then the rows the table did not hold), M replaced, the plan of the next
// iteration -- whose read-back is also this iteration's chaos
void mcl_iterate(mcl_run& R, mcl_matrix& M, mcl_plan& pl, vg_mcl_stats& sts) {
    const int64_t n = R.n, nw = (int64_t)pl.h[MC_WAVE], ng = (int64_t)pl.h[MC_GROUP]; hipStream_t s = R.s;
    mcl_matrix N;
    N.off = std::move(pl.off_next); N.cnt.alloc((size_t)n); N.ent.alloc((size_t)std::max<int64_t>((int64_t)pl.h[MC_STORAGE], 1));
    VG_HIP(hipMemsetAsync(R.ctr.p, 0, MC_WAVE * sizeof(unsigned long long), s));     // chaos and the guard flag
    if (nw) mcl_expand_rows<64, MCL_WAVE_SLOTS>("cluster_mcl_expand_wave", (double)nw * 512.0, R, pl.wave_rows, nw, M, N, pl);
    if (ng) mcl_expand_rows<TPB, MCL_GROUP_SLOTS>("cluster_mcl_expand_group", (double)ng * 16384.0, R, pl.group_rows, ng, M, N, pl);
    VG_HIP(hipGetLastError());
    int64_t ns = 0;
    if (pl.h[MC_TRY]) {                                         // rows were tried above their bound: how many did the table not hold?
        unsigned long long given_up = 0;
        vg_download_bytes(&given_up, R.ctr.p + MC_SPILL, sizeof given_up, s);
        VG_HIP(hipStreamSynchronize(s));
        ns = (int64_t)given_up;
        if (ns > (int64_t)pl.h[MC_TRY]) throw vg_error(VG_EHIP, "vg_cluster_mcl_graph: more spill rows than rows above the table (internal error)");
    }
    if (ns) mcl_spill(n, ns, M, N, pl, R.P, R.ctr, s);
    M = std::move(N);
    ++sts.iterations; sts.lds_rows += n - ns; sts.spill_rows += ns;
    mcl_make_plan(n, M, R.slots, R.P.max_row, R.ctr, s, pl);
    sts.chaos = pl.h[MC_CHAOS];
    char note[128];
    snprintf(note, sizeof note, "mcl iteration %lld: chaos %llu, %lld + %lld LDS rows, %lld spill rows", (long long)sts.iterations,
             (unsigned long long)sts.chaos, (long long)nw, (long long)(ng - ns), (long long)ns);
    vg_host_mark(note);
}
// the (row, column) keys and the values of the last matrix's entries, for the CSR output
struct mcl_entries { dbuf<uint64_t> key; dbuf<uint32_t> val; };
// The clusters: the components of the last matrix, labelled as single linkage labels them.  want: its entries -> ent too.
void mcl_components(mcl_run& R, const mcl_matrix& M, bool want, int32_t* label, int32_t* representative, vg_mcl_stats& sts, mcl_entries& ent) {
    const int64_t n = R.n, storage = (int64_t)M.ent.n; hipStream_t s = R.s;
    edge_graph hg;
    hg.ukeys.alloc((size_t)storage); hg.m = storage;
    dbuf<uint64_t>& ckey = ent.key; dbuf<uint32_t>& cval = ent.val; dbuf<unsigned long long> tally(2);
    unsigned long long ht[2] = {};
    {
        vg_prof_scope ps("cluster_mcl_last", (double)storage * 28.0);
        hg.ukeys.zero(s); tally.zero(s);
        if (want) {
            ckey.alloc((size_t)storage); cval.alloc((size_t)storage);
            VG_HIP(hipMemsetAsync(ckey.p, 0xff, ckey.bytes(), s));
            cval.zero(s);
        }
        hipLaunchKernelGGL(k_mcl_last, dim3(grid_of(n)), dim3(TPB), 0, s, n, (const int64_t*)M.off.p, (const int32_t*)M.cnt.p, (const uint64_t*)M.ent.p,
                           hg.ukeys.p, ckey.p, cval.p, tally.p);
        VG_HIP(hipGetLastError());
        tally.download(ht, 2, s);
        VG_HIP(hipStreamSynchronize(s));
    }
    sts.nnz = (int64_t)ht[0]; sts.max_row_seen = (int64_t)ht[1];
    if (sts.nnz < n || sts.nnz > storage) throw vg_error(VG_EHIP, "vg_cluster_mcl_graph: the last matrix is inconsistent (internal error)");
    dbuf<int32_t> root((size_t)n);
    vg_cluster_stats cs{};
    single_on_device(n, hg, s, root, cs);
    labels_to_host(n, root, false, s, label, representative);
}
// The CSR output of the last matrix: its nnz entries sorted by (row, column) -- the unused storage (keys of all ones) sorts behind
// them --, then the three arrays, allocated with malloc (the entry frees them if anything throws)
void mcl_export(mcl_run& R, mcl_entries& ent, int64_t nnz, int64_t** m_off, int32_t** m_col, uint32_t** m_val) {
    const int64_t n = R.n, storage = (int64_t)ent.key.n; hipStream_t s = R.s;
    dbuf<uint64_t> key2((size_t)storage); dbuf<uint32_t> val2((size_t)storage);
    vg_prof_scope ps("cluster_mcl_matrix", (double)storage * (12.0 * 2.0 * 2.0));
    with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::radix_sort_pairs(tmp, tb, ent.key.p, key2.p, ent.val.p, val2.p, (size_t)storage, 0u, 64u, s); });
    dbuf<int64_t> d_off((size_t)n + 1); dbuf<int32_t> d_col((size_t)nnz);
    hipLaunchKernelGGL(k_csr, dim3(grid_of(nnz + 1)), dim3(TPB), 0, s, (const uint64_t*)key2.p, nnz, n, d_off.p, d_col.p);
    VG_HIP(hipGetLastError());
    *m_off = (int64_t*)malloc(sizeof(int64_t) * ((size_t)n + 1));
    *m_col = (int32_t*)malloc(sizeof(int32_t) * (size_t)nnz);
    *m_val = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)nnz);
    if (!*m_off || !*m_col || !*m_val) throw vg_error(VG_ENOMEM, "out of host memory");
    d_off.download(*m_off, (size_t)n + 1, s); d_col.download(*m_col, (size_t)nnz, s); val2.download(*m_val, (size_t)nnz, s);
    VG_HIP(hipStreamSynchronize(s));
}
// Markov clustering of the edge graph, which is released once the start matrix stands; m_off null: no matrix output
void mcl_on_device(int64_t n, edge_graph& eg, hipStream_t s, const vg_mcl_params& prm, int32_t* label, int32_t* representative, int64_t** m_off,
                   int32_t** m_col, uint32_t** m_val, vg_mcl_stats& sts) {
    mcl_run R{ n, s, mcl_dev{ (int)llrint(2 * prm.inflation), (uint32_t)(uint64_t)std::floor(prm.prune * (double)MCL_ONE), prm.max_row },
               g_mcl_slots.load() ? g_mcl_slots.load() : MCL_GROUP_SLOTS, {} };
    const uint64_t eps = (uint64_t)std::floor(prm.chaos_eps * (double)MCL_ONE);
    mcl_matrix M; mcl_plan pl;
    mcl_start_matrix(R, eg, M, pl);
    do {
        mcl_iterate(R, M, pl, sts);
        if (sts.chaos <= eps) sts.converged = 1;
    } while (!sts.converged && sts.iterations < prm.max_iterations);
    mcl_entries ent;
    mcl_components(R, M, m_off != nullptr, label, representative, sts, ent);
    if (m_off) mcl_export(R, ent, sts.nnz, m_off, m_col, m_val);
}
}  // namespace

extern "C" void vg_cluster_mcl_set_table_slots(int slots) {
    int v = 0;
    if (slots > 0) { v = 16; while (v < MCL_GROUP_SLOTS && v * 2 <= slots) v *= 2; }      // the power of two below, in 16..4096
    g_mcl_slots.store(v);
}

extern "C" int vg_cluster_mcl_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                    const vg_mcl_params* params, int32_t* label, int32_t* representative, int64_t** m_off, int32_t** m_col,
                                    uint32_t** m_val, vg_mcl_stats* stats) {
    const bool want = m_off || m_col || m_val;
    if (m_off) *m_off = nullptr;
    if (m_col) *m_col = nullptr;
    if (m_val) *m_val = nullptr;
    try {
        const char* fn = "vg_cluster_mcl_graph";
        const row_list in{ n_objects, q, r, w, n_rows };
        check_call(fn, in, n_objects && (!label || !representative) ? "null output" : nullptr);
        if (want && (!m_off || !m_col || !m_val)) throw vg_error(VG_EINVAL, std::string(fn) + ": the matrix outputs are all three or none");
        check_mcl_params(fn, params);
        check_row_values(fn, in);
        check_unit_weights(fn, in, "Markov clustering");
        vg_mcl_stats local; vg_mcl_stats& sts = cleared(stats, local);
        if (n_objects == 0) {
            if (want && !(*m_off = (int64_t*)calloc(1, sizeof(int64_t)))) throw vg_error(VG_ENOMEM, "out of host memory");
            return VG_OK;
        }
        edge_graph eg;
        hipStream_t s = graph_on_device(in, eg);
        sts.n_edges = eg.m / 2;
        mcl_on_device(n_objects, eg, s, *params, label, representative, want ? m_off : nullptr, m_col, m_val, sts);
    } catch (...) {
        // (nothing half-filled leaves the call; the error itself is reported below)
        if (want && m_off && m_col && m_val) { free(*m_off); free(*m_col); free(*m_val); *m_off = nullptr; *m_col = nullptr; *m_val = nullptr; }
        VG_API_BEGIN throw; VG_API_END
    }
    return VG_OK;
}
