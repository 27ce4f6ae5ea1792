// vg_scan.h — the device primitives the interval stages share (vg_cover.hip, vg_paint.hip): the three-launch scan over tiles of
// 1 024 elements, and the thin wrappers of rocPRIM's radix sort and of a one-value read-back.  Everything sits in an anonymous
// namespace: each translation unit that includes the header instantiates its own kernels.
#pragma once
#include "vg_common.h"
#include <rocprim/rocprim.hpp>

namespace {
constexpr int TPB = 256, WAVE = 64, WAVES = TPB / WAVE;
constexpr int IPT = 4;                      // consecutive elements per thread
constexpr int TILE = TPB * IPT;             // elements per workgroup of a scan: 1024

// ---------------------------------------------------------------- scan over tiles
// v of the lane d below (any trivially copyable T of whole dwords)
template <class T> __device__ __forceinline__ T shfl_up_t(const T& v, int d) {
    static_assert(sizeof(T) % 4 == 0, "whole dwords");
    constexpr int W = (int)(sizeof(T) / 4);
    uint32_t w[W];
    memcpy(w, &v, sizeof(T));
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = (uint32_t)__shfl_up((int)w[i], (unsigned)d, WAVE);
    T o;
    memcpy(&o, w, sizeof(T));
    return o;
}
// the fold of `mine` over the threads below this one (op need not commute; id is its identity), and the fold over the whole
// workgroup in *total (may be null): wave64 scan by shuffles, the four wave totals through LDS
template <class T, class Op>
__device__ __forceinline__ T block_exclusive(const T& mine, const T& id, Op op, T* wave_total /* LDS: WAVES */, T* total) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    T incl = mine;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T up = shfl_up_t(incl, d);
        if (lane >= d) incl = op(up, incl);
    }
    T before = shfl_up_t(incl, 1);
    if (lane == 0) before = id;
    if (lane == WAVE - 1) wave_total[wave] = incl;
    __syncthreads();
    T prefix = id, all = id;
    for (int w = 0; w < WAVES; ++w) {
        const T t = wave_total[w];
        if (w < wave) prefix = op(prefix, t);
        all = op(all, t);
    }
    if (total) *total = all;
    __syncthreads();                        // (wave_total may be written again by the caller's next round)
    return op(prefix, before);
}
template <class T, class Op, class Load>
__global__ __launch_bounds__(TPB) void k_tile_reduce(int64_t n, T id, Op op, Load load, T* partial) {
    __shared__ T wave_total[WAVES];
    const int64_t base = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * IPT;
    T mine = id;
#pragma unroll
    for (int j = 0; j < IPT; ++j) if (base + j < n) mine = op(mine, load(base + j));
    T total;
    block_exclusive(mine, id, op, wave_total, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}
// one workgroup: the tile totals -> the carry into every tile (in place)
template <class T, class Op>
__global__ __launch_bounds__(TPB) void k_carry_scan(int64_t n_tiles, T id, Op op, T* partial) {
    __shared__ T wave_total[WAVES];
    T carry = id;
    for (int64_t c = 0; c < n_tiles; c += TPB) {
        const int64_t i = c + threadIdx.x;
        const T mine = i < n_tiles ? partial[i] : id;
        T total;
        const T ex = block_exclusive(mine, id, op, wave_total, &total);
        if (i < n_tiles) partial[i] = op(carry, ex);
        carry = op(carry, total);
    }
}
template <class T, class Op, class Load, class Store>
__global__ __launch_bounds__(TPB) void k_tile_scan(int64_t n, T id, Op op, Load load, Store store, const T* carry) {
    __shared__ T wave_total[WAVES];
    const int64_t base = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * IPT;
    T item[IPT];
    T mine = id;
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        item[j] = base + j < n ? load(base + j) : id;
        mine = op(mine, item[j]);
    }
    T run = block_exclusive(mine, id, op, wave_total, (T*)nullptr);
    if (carry) run = op(carry[blockIdx.x], run);
#pragma unroll
    for (int j = 0; j < IPT; ++j)
        if (base + j < n) {
            const T ex = run;
            run = op(run, item[j]);
            store(base + j, run, ex);
        }
}
// store(i, inclusive, exclusive) for every i in [0, n), the scan of load(i) under op; load may be called twice per element
template <class T, class Op, class Load, class Store>
void scan_tiles(int64_t n, T id, Op op, Load load, Store store, hipStream_t s) {
    if (n <= 0) return;
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    dbuf<T> carry;
    if (n_tiles > 1) {
        carry.alloc((size_t)n_tiles);
        k_tile_reduce<T, Op, Load><<<dim3((unsigned)n_tiles), dim3(TPB), 0, s>>>(n, id, op, load, carry.p);
        k_carry_scan<T, Op><<<dim3(1), dim3(TPB), 0, s>>>(n_tiles, id, op, carry.p);
    }
    k_tile_scan<T, Op, Load, Store><<<dim3((unsigned)n_tiles), dim3(TPB), 0, s>>>(n, id, op, load, store, (const T*)carry.p);
    VG_HIP(hipGetLastError());
}

__global__ __launch_bounds__(TPB) void k_iota(uint32_t* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) out[i] = (uint32_t)i;
}

int blocks(int64_t n) { return grid_for(n, TPB, 16384); }
template <class T> T read_back(const T* at, hipStream_t s) {
    T v{};
    vg_download_bytes(&v, at, sizeof v, s);
    VG_HIP(hipStreamSynchronize(s));
    return v;
}
template <class K, class V>
void sort_pairs(const K* keys, K* keys_out, const V* vals, V* vals_out, int64_t n, unsigned bits, hipStream_t s) {
    with_temp_storage([&](void* tmp, size_t& tb) { return rocprim::radix_sort_pairs(tmp, tb, keys, keys_out, vals, vals_out, (size_t)n, 0u, bits, s); });
}
}  // namespace
