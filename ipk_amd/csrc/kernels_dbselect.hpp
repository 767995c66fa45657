// kernels_dbselect.hpp -- the selection of a database on the device: "the first M k-mers in filter order, entries above a log-score t"
// (ipkgpu_db_select in include/ipkgpu.h; the definition is this library's own -- i2l::load(file, mu, omega) is un-vendored).
//
//   db_select_mark_kernel      candidate flags scattered from order[0 .. M)
//   db_select_wanted_kernel    candidate flags of ipkgpu_db_select_keys: is the key's bit set in a k-mer set's bitmap (db_key_wanted)
//   db_select_flag_kernel      per ENTRY: keep = its key is a candidate and score > t          (entry ranges, as db_unpack_entries_kernel)
//   db_select_keys_kernel      per key: does an entry of it stay (two reads of the scanned keep flags)
//   db_select_records_kernel   per record i < M: does its key stay
//   db_select_copy_kernel      per ENTRY: entries and positions to their scanned places
//   db_select_compact_kernel   per key: key, filter values and entry offset to the key's scanned place
//   db_select_order_kernel     per record i < M: the new index of its key to the record's scanned place
// Every output position comes from an exclusive scan of flags (scan_u32), none from an atomic: the result is the same bits on every run
// and a key's entries keep their order.  Streaming kernels: consecutive lanes take consecutive elements, entries move as 8-byte words.
#pragma once
#include "kernels_dbload.hpp"

namespace ipkgpu {

__global__ __launch_bounds__(256) void db_select_mark_kernel(const uint32_t* __restrict__ order, uint64_t m, uint32_t* __restrict__ cand)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) cand[order[i]] = 1u;
}

// Is `key` in the k-mer set whose bitmap holds n_codes bits?  The bound is tested before the bitmap is read: a key can come from a file,
// which no host check covers, and a key at or beyond n_codes is in no set.
__device__ __forceinline__ bool db_key_wanted(const uint32_t* __restrict__ bitmap, uint64_t n_codes, uint32_t key)
{
    if ((uint64_t)key >= n_codes) return false;
    return ((bitmap[key >> 5] >> (key & 31u)) & 1u) != 0u;
}

__global__ __launch_bounds__(256) void db_select_wanted_kernel(const uint32_t* __restrict__ keys, uint64_t n_keys, const uint32_t* __restrict__ bitmap,
                                                               uint64_t n_codes, uint32_t* __restrict__ cand)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n_keys) cand[j] = db_key_wanted(bitmap, n_codes, keys[j]) ? 1u : 0u;
}

// Work by ENTRY ranges (DB_UNPACK_TILE entries per workgroup, whatever keys they belong to).  ALL: every key is a candidate, no key is
// looked up.  SCORE false (ipkgpu_db_select_keys): no score is compared, a candidate keeps every entry whatever its bits.  Otherwise the keys a tile touches are found once and each lane finds its entry's key among those (db_key_of_entry: the
// last key whose offset is not beyond the entry, so keys without entries are passed over).  The comparison is binary32 and strict; a
// NaN score fails it.
template <bool ALL, bool SCORE = true>
__global__ __launch_bounds__(256) void db_select_flag_kernel(const uint2* __restrict__ entries, const uint64_t* __restrict__ key_off,
                                                             const uint32_t* __restrict__ cand, uint64_t n_keys, uint64_t n_entries, float t,
                                                             uint32_t* __restrict__ keep)
{
    const uint64_t e0 = (uint64_t)blockIdx.x * DB_UNPACK_TILE;
    if (e0 >= n_entries) return;
    const uint64_t e_last = min(e0 + DB_UNPACK_TILE, n_entries) - 1;
    uint64_t j_lo = 0, j_hi = 0;
    if (!ALL) {
        j_lo = db_key_of_entry(key_off, 0, n_keys - 1, e0);
        j_hi = db_key_of_entry(key_off, j_lo, n_keys - 1, e_last);
    }
#pragma unroll
    for (uint32_t r = 0; r < DB_UNPACK_PER_THREAD; ++r) {
        const uint64_t e = e0 + r * 256 + threadIdx.x;
        if (e > e_last) break;
        const uint2 ent = entries[e];
        bool k = !SCORE || __uint_as_float(ent.y) > t;
        if (!ALL) k = k && cand[db_key_of_entry(key_off, j_lo, j_hi, e)] != 0u;
        keep[e] = k ? 1u : 0u;
    }
}

// e_scan: the exclusive scan of keep, n_entries + 1 values.  A key stays iff one of its entries does.
__global__ __launch_bounds__(256) void db_select_keys_kernel(const uint64_t* __restrict__ key_off, const uint64_t* __restrict__ e_scan, uint64_t n_keys,
                                                             uint32_t* __restrict__ key_keep)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_keys) return;
    key_keep[j] = e_scan[key_off[j + 1]] > e_scan[key_off[j]] ? 1u : 0u;
}

__global__ __launch_bounds__(256) void db_select_records_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ key_keep, uint64_t m,
                                                                uint32_t* __restrict__ rec_keep)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) rec_keep[i] = key_keep[order[i]];
}

template <bool POS>
__global__ __launch_bounds__(256) void db_select_copy_kernel(const uint2* __restrict__ entries, const uint32_t* __restrict__ positions,
                                                             const uint32_t* __restrict__ keep, const uint64_t* __restrict__ e_scan, uint64_t n_entries,
                                                             uint2* __restrict__ out_entries, uint32_t* __restrict__ out_positions)
{
    const uint64_t e0 = (uint64_t)blockIdx.x * DB_UNPACK_TILE;
#pragma unroll
    for (uint32_t r = 0; r < DB_UNPACK_PER_THREAD; ++r) {
        const uint64_t e = e0 + r * 256 + threadIdx.x;
        if (e >= n_entries) break;
        if (keep[e]) {
            const uint64_t to = e_scan[e];
            out_entries[to] = entries[e];
            if (POS) out_positions[to] = positions[e];
        }
    }
}

// k_scan: the exclusive scan of key_keep.  The key at its new index, its filter values bit for bit, its entries' new start; the thread
// of key 0 closes the offsets with the totals the host has read back.
__global__ __launch_bounds__(256) void db_select_compact_kernel(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ key_off,
                                                                const float* __restrict__ fv32, const double* __restrict__ fv64,
                                                                const uint32_t* __restrict__ key_keep, const uint64_t* __restrict__ k_scan,
                                                                const uint64_t* __restrict__ e_scan, uint64_t n_keys, uint64_t n_out, uint64_t ne_out,
                                                                uint32_t* __restrict__ out_keys, uint64_t* __restrict__ out_key_off,
                                                                float* __restrict__ out_fv32, double* __restrict__ out_fv64)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_keys) return;
    if (j == 0) out_key_off[n_out] = ne_out;
    if (!key_keep[j]) return;
    const uint64_t q = k_scan[j];
    out_keys[q] = keys[j];
    out_key_off[q] = e_scan[key_off[j]];
    out_fv32[q] = fv32[j];
    out_fv64[q] = fv64[j];
}

// r_scan: the exclusive scan of rec_keep.  out_order[r] = the new index of the r-th surviving record's key.
__global__ __launch_bounds__(256) void db_select_order_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ rec_keep,
                                                              const uint64_t* __restrict__ r_scan, const uint64_t* __restrict__ k_scan, uint64_t m,
                                                              uint32_t* __restrict__ out_order)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m || !rec_keep[i]) return;
    out_order[r_scan[i]] = (uint32_t)k_scan[order[i]];
}

}  // namespace ipkgpu
