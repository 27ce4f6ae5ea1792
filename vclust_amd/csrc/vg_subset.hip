// vg_subset.hip — a subset of a resident genome set, gathered on the device (vg_genomes_subset).
// The dereplicate loop compares every batch of genomes with the representatives found so far: the set [representatives | batch]
// is cut out of the resident set once per batch, and no base travels from the host for it.
#include "vg_common.h"
#include <numeric>

namespace {
// The unit of the copy is 64 bases: one uint4 of 2-bit codes (16 bytes) and one uint2 of mask bits beside it.  Every genome of either
// set starts at a multiple of its set's block (>= 64 bases), so a unit never straddles two genomes and both sides are aligned.
// Destination unit u lies in destination block u >> (align_shift - 6) -> genome s of the subset; it holds the bases
// [u * 64 - sub_off[s], + 64) of that genome, which the parent holds from par_off[ids[s]] on.  A genome's padding is copied with it:
// the parent's is A with mask bit 1 as well, and never shorter than the subset's (checked on the host).  The units behind the last
// genome are the slack of the arrays (vg_genomes_finish): 16 words of A, 16 words of set mask bits.
__global__ void __launch_bounds__(256)
k_subset_gather(const uint32_t* __restrict__ par_packed, const uint32_t* __restrict__ par_nmask, const int64_t* __restrict__ par_off,
                const int32_t* __restrict__ ids, const uint32_t* __restrict__ sub_blk2g, const int64_t* __restrict__ sub_off,
                int unit_shift, int64_t n_units, uint32_t* __restrict__ sub_packed, uint32_t* __restrict__ sub_nmask) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_units + 8; u += (int64_t)gridDim.x * blockDim.x) {
        if (u >= n_units) {
            if (u < n_units + 4) *reinterpret_cast<uint4*>(sub_packed + 4 * u) = make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint2*>(sub_nmask + 2 * u) = make_uint2(0xffffffffu, 0xffffffffu);
            continue;
        }
        const uint32_t s = sub_blk2g[u >> unit_shift];
        const int64_t src = (par_off[ids[s]] + (u * 64 - sub_off[s])) >> 6;       // the parent's unit
        const uint4 pk = *reinterpret_cast<const uint4*>(par_packed + 4 * src);
        const uint2 mk = *reinterpret_cast<const uint2*>(par_nmask + 2 * src);
        *reinterpret_cast<uint4*>(sub_packed + 4 * u) = pk;
        *reinterpret_cast<uint2*>(sub_nmask + 2 * u) = mk;
    }
}
}  // namespace

extern "C" int vg_genomes_subset(const vg_genomes* g, const int32_t* ids, int n_ids, vg_genomes** out) {
    VG_API_BEGIN
    if (!g || !out || n_ids < 0 || (!ids && n_ids)) throw vg_error(VG_EINVAL, "vg_genomes_subset: null argument");
    *out = nullptr;
    // the arguments, before any device use
    {
        std::vector<uint8_t> seen((size_t)std::max(g->n, 1), 0);
        for (int i = 0; i < n_ids; ++i) {
            if (ids[i] < 0 || ids[i] >= g->n)
                throw vg_error(VG_EINVAL, "vg_genomes_subset: ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is outside 0.." + std::to_string(g->n - 1) + " (the genomes of the set)");
            if (seen[(size_t)ids[i]]++)
                throw vg_error(VG_EINVAL, "vg_genomes_subset: ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is listed twice");
        }
    }
    if (g->device < 0) throw vg_error(VG_EINVAL, "vg_genomes_subset: the set is not resident (vg_genomes_to_device first)");
    // layout: the parent's block size, the loader's padding rule (vg_genomes_append)
    std::unique_ptr<vg_genomes> sub(new vg_genomes());
    sub->align_shift = g->align_shift; sub->device_only = true;
    const int64_t al = 1LL << g->align_shift;
    sub->base_off.push_back(0);
    for (int i = 0; i < n_ids; ++i) {
        const size_t id = (size_t)ids[i];
        const int64_t off = sub->base_off.back(), padded = (g->len[id] / al + 1) * al;
        if (padded > g->base_off[id + 1] - g->base_off[id])
            throw vg_error(VG_EHIP, "vg_genomes_subset: genome " + std::to_string(ids[i]) + " has less padding than the loader's rule gives it");
        sub->names.push_back(g->names[id]); sub->len.push_back(g->len[id]); sub->n_parts.push_back(g->n_parts[id]); sub->has_n.push_back(g->has_n[id]);
        sub->base_off.push_back(off + padded);
        for (int64_t b = off >> g->align_shift; b < (off + padded) >> g->align_shift; ++b) sub->blk2g.push_back((uint32_t)i);
        sub->n++;
    }
    sub->blk2g.push_back(sub->n > 0 ? (uint32_t)(sub->n - 1) : 0u);       // (as vg_genomes_finish leaves it)
    // the device: small arrays uploaded, bases gathered
    vg_require_device();
    int dev = 0; VG_HIP(hipGetDevice(&dev));
    if (dev != g->device) throw vg_error(VG_EINVAL, "vg_genomes_subset: the set is resident on device " + std::to_string(g->device) + ", the current device is " + std::to_string(dev));
    hipStream_t s = vg_stream();
    const int64_t total = sub->padded_total(), n_units = total / 64;
    sub->d_packed.alloc((size_t)(total / 16) + 16); sub->d_nmask.alloc((size_t)(total / 32) + 16);
    sub->d_base_off.alloc(sub->base_off.size()); sub->d_base_off.upload(sub->base_off.data(), sub->base_off.size(), s);
    sub->d_len.alloc(std::max<size_t>(1, sub->len.size())); if (sub->n) sub->d_len.upload(sub->len.data(), sub->len.size(), s);
    sub->d_has_n.alloc(std::max<size_t>(1, sub->has_n.size())); if (sub->n) sub->d_has_n.upload(sub->has_n.data(), sub->has_n.size(), s);
    sub->d_blk2g.alloc(sub->blk2g.size()); sub->d_blk2g.upload(sub->blk2g.data(), sub->blk2g.size(), s);
    dbuf<int32_t> d_ids(std::max<size_t>(1, (size_t)n_ids));
    if (n_ids) d_ids.upload(ids, (size_t)n_ids, s);
    {
        vg_prof_scope ps("derep_subset", 2.0 * (double)(total / 4 + total / 8));       // read and written once
        hipLaunchKernelGGL(k_subset_gather, dim3(grid_for(n_units + 8)), dim3(256), 0, s, (const uint32_t*)g->d_packed.p, (const uint32_t*)g->d_nmask.p,
                           (const int64_t*)g->d_base_off.p, (const int32_t*)d_ids.p, (const uint32_t*)sub->d_blk2g.p, (const int64_t*)sub->d_base_off.p,
                           g->align_shift - 6, n_units, sub->d_packed.p, sub->d_nmask.p);
        VG_HIP(hipGetLastError());
    }
    VG_HIP(hipStreamSynchronize(s));      // (ids and the staging of the small uploads are the caller's / this frame's)
    sub->device = dev;
    *out = sub.release();
    VG_API_END
}
