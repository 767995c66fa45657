// kernels_spill.hpp -- packs key-major counts rows into the spill block's form (spill_format.hpp) and back.
//
// The on-disk build takes every owner block of a piece off the device (ipkgpu_parts_spill) and brings one batch's blocks back later
// (ipkgpu_spill_merge).  A counts row is mostly zeros, so it travels as occupancy bits plus the non-empty slots' counts as u16 --
// the idea of the compressed tables (mask, then values in slot order).  The entries travel as they are.
//
// Rows are handled a 64-slot word at a time by one wavefront: a row of `slots` slots has W = ceil(slots / 64) words, row r's word w
// is item r * W + w of every per-word array (bits, popcounts, ranks).  All rows of a call go through one launch.
#pragma once
#include "dcla_device.hpp"

namespace ipkgpu {

// Pack, step 1: bits[r * W + w] = ballot(count != 0) over slots [64 w, 64 w + 64) of row r, pops = its popcount.
// A count beyond 65535 raises *too_big (the caller fails the call: never truncated).
__global__ __launch_bounds__(256) void spill_bits_kernel(const uint32_t* __restrict__ counts, uint64_t slots, uint64_t W, uint64_t n_words,
                                                         unsigned long long* __restrict__ bits, uint32_t* __restrict__ pops,
                                                         uint32_t* __restrict__ too_big)
{
    const uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // (wave-uniform)
    if (item >= n_words) return;
    const uint64_t r = item / W, w = item - r * W;
    const uint32_t lane = lane_id();
    const uint64_t q = w * 64 + lane;
    const uint32_t c = q < slots ? counts[r * slots + q] : 0u;
    if (c > 0xFFFFu) atomicOr(too_big, 1u);
    const uint64_t m = __ballot(c != 0u);
    if (lane == 0) { bits[item] = m; pops[item] = (uint32_t)__popcll(m); }
}

// Pack, step 2: rank = exclusive scan of pops over all rows' words; the non-empty slots' counts go to packed[rank + mbcnt] -- the
// rows' u16 runs stand end to end in `packed`, row r's from rank[r * W] on.
__global__ __launch_bounds__(256) void spill_pack_kernel(const uint32_t* __restrict__ counts, uint64_t slots, uint64_t W, uint64_t n_words,
                                                         const uint64_t* __restrict__ rank, uint16_t* __restrict__ packed)
{
    const uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_words) return;
    const uint64_t r = item / W, w = item - r * W;
    const uint64_t q = w * 64 + lane_id();
    const uint32_t c = q < slots ? counts[r * slots + q] : 0u;
    const uint64_t m = __ballot(c != 0u);
    if (c != 0u) packed[rank[item] + mbcnt(m)] = (uint16_t)c;
}

// pops[i] = popcount(bits[i]): the unpack side's scan input (the bits came from a file)
__global__ __launch_bounds__(256) void spill_pops_kernel(const unsigned long long* __restrict__ bits, uint64_t n_words, uint32_t* __restrict__ pops)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) pops[i] = (uint32_t)__popcll(bits[i]);
}

// Unpack: the dense rows u32 [rows][slots] out of bits, ranks and the u16 runs; EVERY slot of every row is written (no memset).
// n_packed bounds the reads of `packed`: the host has checked the bits against it, the kernel still never reads past it.
__global__ __launch_bounds__(256) void spill_unpack_kernel(const unsigned long long* __restrict__ bits, const uint64_t* __restrict__ rank,
                                                           const uint16_t* __restrict__ packed, uint64_t n_packed, uint64_t slots, uint64_t W,
                                                           uint64_t n_words, uint32_t* __restrict__ counts)
{
    const uint64_t item = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_words) return;
    const uint64_t r = item / W, w = item - r * W;
    const uint32_t lane = lane_id();
    const uint64_t q = w * 64 + lane;
    const uint64_t m = bits[item];
    uint32_t c = 0;
    if ((m >> lane) & 1ull) {
        const uint64_t at = rank[item] + mbcnt(m);
        if (at < n_packed) c = packed[at];
    }
    if (q < slots) counts[r * slots + q] = c;
}

}  // namespace ipkgpu
