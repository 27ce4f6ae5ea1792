// vg_subset.hip — a subset of a resident genome set, gathered on the device, and the same set extended and truncated in place
// (vg_genomes_subset, vg_genomes_extend, vg_genomes_truncate, vg_genomes_reserve).
// The dereplicate loop compares every batch of genomes with the representatives found so far: the representatives stay where they
// are, the batch is appended behind them and dropped again, the batch's founders are appended for good, and no base travels from
// the host for any of it.
#include "vg_common.h"
#include <numeric>

namespace {
// The unit of the copy is 64 bases: one uint4 of 2-bit codes (16 bytes) and one uint2 of mask bits beside it.  Every genome of either
// set starts at a multiple of its set's block (>= 64 bases), so a unit never straddles two genomes and both sides are aligned.
// Only the units from u0 on are written: those in front are the resident genomes and are neither read nor copied.  Destination unit
// u lies in destination block u >> (align_shift - 6) -> genome s of the subset, the (s - s0)-th appended one; it holds the bases
// [u * 64 - sub_off[s], + 64) of that genome, which the parent holds from par_off[ids[s - s0]] on.  A genome's padding is copied with
// it: the parent's is A with mask bit 1 as well, and never shorter than the subset's (checked on the host).  The units behind the
// last genome are the slack of the arrays (vg_genomes_finish): 16 words of A, 16 words of set mask bits.  With u0 = n_units the
// kernel writes the slack and nothing else (vg_genomes_truncate).
__global__ void __launch_bounds__(256)
k_extend_gather(const uint32_t* __restrict__ par_packed, const uint32_t* __restrict__ par_nmask, const int64_t* __restrict__ par_off,
                const int32_t* __restrict__ ids, const uint32_t* __restrict__ sub_blk2g, const int64_t* __restrict__ sub_off,
                int unit_shift, int64_t u0, uint32_t s0, int64_t n_units, uint32_t* __restrict__ sub_packed, uint32_t* __restrict__ sub_nmask) {
    for (int64_t u = u0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units + 8; u += (int64_t)gridDim.x * blockDim.x) {
        if (u >= n_units) {
            if (u < n_units + 4) *reinterpret_cast<uint4*>(sub_packed + 4 * u) = make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint2*>(sub_nmask + 2 * u) = make_uint2(0xffffffffu, 0xffffffffu);
            continue;
        }
        const uint32_t s = sub_blk2g[u >> unit_shift];
        const int64_t src = (par_off[ids[s - s0]] + (u * 64 - sub_off[s])) >> 6;       // the parent's unit
        const uint4 pk = *reinterpret_cast<const uint4*>(par_packed + 4 * src);
        const uint2 mk = *reinterpret_cast<const uint2*>(par_nmask + 2 * src);
        *reinterpret_cast<uint4*>(sub_packed + 4 * u) = pk;
        *reinterpret_cast<uint2*>(sub_nmask + 2 * u) = mk;
    }
}

// the elements the arrays of a set of n genomes and `total` padded bases hold (vg_genomes_finish: slack behind the bases, one more
// block entry, one more offset)
struct set_sizes {
    size_t packed, nmask, base_off, len, blk2g;
    set_sizes(int64_t total, int64_t n, int align_shift)
        : packed((size_t)(total / 16) + 16), nmask((size_t)(total / 32) + 16), base_off((size_t)n + 1), len((size_t)std::max<int64_t>(1, n)),
          blk2g((size_t)(total >> align_shift) + 1) {}
};
// `cap` holds at least `need` elements, the first `used` of them kept; it grows by half of itself at least (one copy device to device)
template <class T> void grow(dbuf<T>& cap, size_t used, size_t need, hipStream_t s) {
    if (need <= cap.n) return;
    dbuf<T> bigger(std::max(need, cap.n + cap.n / 2));
    if (cap.p && used) VG_HIP(hipMemcpyAsync(bigger.p, cap.p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
    cap = std::move(bigger);      // (the old block goes back to the allocator behind the copy: one in-order stream)
}
void window(vg_genomes* sub);
void grow_all(vg_genomes* sub, const set_sizes& need, hipStream_t s) {
    const set_sizes used(sub->padded_total(), sub->n, sub->align_shift);
    try {
        grow(sub->cap_packed, used.packed, need.packed, s); grow(sub->cap_nmask, used.nmask, need.nmask, s);
        grow(sub->cap_base_off, used.base_off, need.base_off, s); grow(sub->cap_len, used.len, need.len, s);
        grow(sub->cap_has_n, used.len, need.len, s); grow(sub->cap_blk2g, used.blk2g, need.blk2g, s);
    } catch (...) { window(sub); throw; }      // (out of device memory half way: the set is what it was, on the buffers it has now)
}
// the d_* arrays as windows of the used part of the cap_* buffers
void window(vg_genomes* sub) {
    const set_sizes used(sub->padded_total(), sub->n, sub->align_shift);
    sub->d_packed.view(sub->cap_packed.p, used.packed); sub->d_nmask.view(sub->cap_nmask.p, used.nmask);
    sub->d_base_off.view(sub->cap_base_off.p, used.base_off); sub->d_len.view(sub->cap_len.p, used.len);
    sub->d_has_n.view(sub->cap_has_n.p, used.len); sub->d_blk2g.view(sub->cap_blk2g.p, used.blk2g);
}
// what the set keeps of its own contents, remade lazily as for any new set
void drop_caches(vg_genomes* sub) {
    sub->d_planes.release();                              // the bit planes (vg_genome_planes)
    sub->len_order.clear(); sub->len_rank.clear();        // the align order (vg_length_order)
    vg_lz_drop_prepared(sub);                             // the index plans vg_lz_prepare and the last vg_lz_align left for it
    // (the k-mer stage keeps nothing per set: its indexes live for one call)
}
void require_here(const char* fn, const vg_genomes* g, const char* what) {
    vg_require_device();
    int dev = 0; VG_HIP(hipGetDevice(&dev));
    if (dev != g->device)
        throw vg_error(VG_EINVAL, std::string(fn) + ": " + what + " is resident on device " + std::to_string(g->device) + ", the current device is " + std::to_string(dev));
}
// seen[id]: 0 = free, 1 = listed by this call, 2 = in the set already
void check_ids(const char* fn, const vg_genomes* g, const int32_t* ids, int n_ids, std::vector<uint8_t>& seen) {
    for (int i = 0; i < n_ids; ++i) {
        const std::string which = std::string(fn) + ": ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]);
        if (ids[i] < 0 || ids[i] >= g->n) throw vg_error(VG_EINVAL, which + " is outside 0.." + std::to_string(g->n - 1) + " (the genomes of the set)");
        if (seen[(size_t)ids[i]] == 2) throw vg_error(VG_EINVAL, which + " is in the set already");
        if (seen[(size_t)ids[i]] == 1) throw vg_error(VG_EINVAL, which + " is listed twice");
        seen[(size_t)ids[i]] = 1;
    }
}
void check_extendable(const char* fn, const vg_genomes* sub) {
    if (!sub->device_only) throw vg_error(VG_EINVAL, std::string(fn) + ": the set was not made by vg_genomes_subset (a loaded set has a host copy, which would not follow)");
}
// the padded bases of genome id of g by the layout rule (vg_padded_len), which g's own layout must cover
int64_t padded_len(const char* fn, const vg_genomes* g, int32_t id) {
    const int64_t padded = vg_padded_len(g->len[(size_t)id], g->align_shift);
    if (padded > g->base_off[(size_t)id + 1] - g->base_off[(size_t)id])
        throw vg_error(VG_EHIP, std::string(fn) + ": genome " + std::to_string(id) + " has less padding than the loader's rule gives it");
    return padded;
}

// ids[0 .. n_ids) of g appended behind the genomes of sub: the host arrays, the tails of the small device arrays, one gather
// (n_ids = 0: the slack behind the last genome is written and nothing else).  Arguments are checked by the callers.
void append(const char* fn, const char* scope, const char* parent_is, vg_genomes* sub, const vg_genomes* g, const int32_t* ids, int n_ids) {
    const int n0 = sub->n, shift = sub->align_shift;
    const int64_t total0 = sub->padded_total();
    int64_t total = total0;
    for (int i = 0; i < n_ids; ++i) total += padded_len(fn, g, ids[i]);
    if ((int64_t)n0 + n_ids > INT32_MAX) throw vg_error(VG_EINVAL, std::string(fn) + ": more than 2^31 - 1 genomes");
    require_here(fn, g, parent_is);
    hipStream_t s = vg_stream();
    grow_all(sub, set_sizes(total, (int64_t)n0 + n_ids, shift), s);
    drop_caches(sub);
    // layout: the parent's block size, the layout rule
    sub->blk2g.pop_back();                                   // (the entry behind the last block)
    for (int i = 0; i < n_ids; ++i) {
        const size_t id = (size_t)ids[i];
        sub->names.push_back(g->names[id]); sub->len.push_back(g->len[id]); sub->n_parts.push_back(g->n_parts[id]); sub->has_n.push_back(g->has_n[id]);
        sub->parent_id.push_back(ids[i]);
        vg_layout_append(sub, g->len[id]);
        sub->n++;
    }
    vg_layout_close(sub);                                    // (as vg_genomes_finish leaves it)
    window(sub);
    // the device: the new tails of the small arrays, then the bases
    const size_t b0 = (size_t)(total0 >> shift);
    vg_upload_bytes(sub->d_base_off.p + n0, sub->base_off.data() + n0, sizeof(int64_t) * ((size_t)n_ids + 1), s);
    if (n_ids) {
        vg_upload_bytes(sub->d_len.p + n0, sub->len.data() + n0, sizeof(int64_t) * (size_t)n_ids, s);
        vg_upload_bytes(sub->d_has_n.p + n0, sub->has_n.data() + n0, (size_t)n_ids, s);
    }
    vg_upload_bytes(sub->d_blk2g.p + b0, sub->blk2g.data() + b0, sizeof(uint32_t) * (sub->blk2g.size() - b0), s);
    dbuf<int32_t> d_ids(std::max<size_t>(1, (size_t)n_ids));
    if (n_ids) d_ids.upload(ids, (size_t)n_ids, s);
    const int64_t u0 = total0 / 64, n_units = total / 64;
    {
        vg_prof_scope ps(scope, 2.0 * (double)((total - total0) / 4 + (total - total0) / 8));       // read and written once
        hipLaunchKernelGGL(k_extend_gather, dim3(grid_for(n_units - u0 + 8)), dim3(256), 0, s, (const uint32_t*)g->d_packed.p, (const uint32_t*)g->d_nmask.p,
                           (const int64_t*)g->d_base_off.p, (const int32_t*)d_ids.p, (const uint32_t*)sub->d_blk2g.p, (const int64_t*)sub->d_base_off.p,
                           shift - 6, u0, (uint32_t)n0, n_units, sub->d_packed.p, sub->d_nmask.p);
        VG_HIP(hipGetLastError());
    }
    VG_HIP(hipStreamSynchronize(s));      // (ids and the staging of the small uploads are the caller's / this frame's)
}
}  // namespace

extern "C" int vg_genomes_subset(const vg_genomes* g, const int32_t* ids, int n_ids, vg_genomes** out) {
    VG_API_BEGIN
    const char* fn = "vg_genomes_subset";
    if (!g || !out || n_ids < 0 || (!ids && n_ids)) throw vg_error(VG_EINVAL, "vg_genomes_subset: null argument");
    *out = nullptr;
    // the arguments, before any device use
    {
        std::vector<uint8_t> seen((size_t)std::max(g->n, 1), 0);
        check_ids(fn, g, ids, n_ids, seen);
    }
    if (g->device < 0) throw vg_error(VG_EINVAL, "vg_genomes_subset: the set is not resident (vg_genomes_to_device first)");
    // an empty set of g's layout on g's device, then its genomes
    std::unique_ptr<vg_genomes> sub(new vg_genomes());
    sub->align_shift = g->align_shift; sub->device_only = true; sub->parent_uid = g->uid; sub->device = g->device;
    sub->base_off.push_back(0); vg_layout_close(sub.get());
    append(fn, "derep_subset", "the set", sub.get(), g, ids, n_ids);
    *out = sub.release();
    VG_API_END
}

extern "C" int vg_genomes_extend(vg_genomes* sub, const vg_genomes* parent, const int32_t* ids, int n_ids) {
    VG_API_BEGIN
    const char* fn = "vg_genomes_extend";
    if (!sub || !parent || n_ids < 0 || (!ids && n_ids)) throw vg_error(VG_EINVAL, "vg_genomes_extend: null argument");
    // the arguments, before any device use
    {
        std::vector<uint8_t> seen((size_t)std::max(parent->n, 1), 0);
        if (sub->device_only && sub->parent_uid == parent->uid) for (int32_t id : sub->parent_id) seen[(size_t)id] = 2;
        check_ids(fn, parent, ids, n_ids, seen);
    }
    check_extendable(fn, sub);
    if (sub->parent_uid != parent->uid) throw vg_error(VG_EINVAL, "vg_genomes_extend: the set was not gathered from this parent (vg_genomes_subset)");
    if (parent->device < 0) throw vg_error(VG_EINVAL, "vg_genomes_extend: the parent set is not resident (vg_genomes_to_device first)");
    if (sub->device != parent->device)
        throw vg_error(VG_EINVAL, "vg_genomes_extend: the set is resident on device " + std::to_string(sub->device) + ", its parent on device " + std::to_string(parent->device));
    append(fn, "derep_extend", "the parent set", sub, parent, ids, n_ids);
    VG_API_END
}

extern "C" int vg_genomes_truncate(vg_genomes* sub, int n_keep) {
    VG_API_BEGIN
    const char* fn = "vg_genomes_truncate";
    if (!sub) throw vg_error(VG_EINVAL, "vg_genomes_truncate: null argument");
    if (n_keep < 0 || n_keep > sub->n)
        throw vg_error(VG_EINVAL, "vg_genomes_truncate: n_keep = " + std::to_string(n_keep) + " is outside 0.." + std::to_string(sub->n) + " (the genomes of the set)");
    check_extendable(fn, sub);
    require_here(fn, sub, "the set");
    hipStream_t s = vg_stream();
    drop_caches(sub);
    const size_t k = (size_t)n_keep;
    sub->n = n_keep;
    sub->names.resize(k); sub->len.resize(k); sub->n_parts.resize(k); sub->has_n.resize(k); sub->parent_id.resize(k); sub->base_off.resize(k + 1);
    const int64_t total = sub->padded_total();
    sub->blk2g.resize((size_t)(total >> sub->align_shift));
    vg_layout_close(sub);
    window(sub);                                             // (the capacity stays)
    // what a kernel that reads past the end sees: the entry behind the last block, and the slack behind the last genome written afresh
    vg_upload_bytes(sub->d_blk2g.p + (sub->blk2g.size() - 1), &sub->blk2g.back(), sizeof(uint32_t), s);
    {
        vg_prof_scope ps("derep_extend", 64.0 + 64.0);
        hipLaunchKernelGGL(k_extend_gather, dim3(1), dim3(256), 0, s, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const int64_t*)nullptr, (const int32_t*)nullptr,
                           (const uint32_t*)sub->d_blk2g.p, (const int64_t*)sub->d_base_off.p, sub->align_shift - 6, total / 64, (uint32_t)n_keep, total / 64,
                           sub->d_packed.p, sub->d_nmask.p);
        VG_HIP(hipGetLastError());
    }
    VG_HIP(hipStreamSynchronize(s));
    VG_API_END
}

extern "C" int vg_genomes_reserve(vg_genomes* sub, int64_t bases, int64_t genomes) {
    VG_API_BEGIN
    const char* fn = "vg_genomes_reserve";
    if (!sub) throw vg_error(VG_EINVAL, "vg_genomes_reserve: null argument");
    if (bases < 0 || genomes < 0 || genomes > INT32_MAX) throw vg_error(VG_EINVAL, "vg_genomes_reserve: bases and genomes must not be negative (genomes at most 2^31 - 1)");
    check_extendable(fn, sub);
    require_here(fn, sub, "the set");
    // the worst case of the padding rule: a whole block behind every genome
    const int64_t total = std::max(sub->padded_total(), bases + (genomes << sub->align_shift));
    hipStream_t s = vg_stream();
    grow_all(sub, set_sizes(total, std::max<int64_t>(genomes, sub->n), sub->align_shift), s);
    window(sub);
    drop_caches(sub);                                        // (the set may have moved: nothing made of the old buffers is kept)
    VG_HIP(hipStreamSynchronize(s));
    VG_API_END
}
