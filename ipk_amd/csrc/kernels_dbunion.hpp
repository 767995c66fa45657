// kernels_dbunion.hpp -- the union of N databases with disjoint key sets on the device (ipkgpu_db_union in include/ipkgpu.h; host side:
// db_union.hpp).
//
//   db_union_sortkey_kernel    per key of the concatenation of the sources' key lists: key << 32 | concatenated index
//   db_union_keys_kernel       behind the sort, per sorted position j: source, key, filter value bits, entry count and the start of
//                              the entries in the source; the smallest j whose key equals its left neighbour's
//   db_union_entries_kernel    per ENTRY of the union: 8 bytes (and the position) from the key's source   (entry ranges, as
//                              db_unpack_entries_kernel and db_select_copy_kernel)
//   db_union_entries16_kernel  the same copy, two entries and one 16-byte store per lane: the form the union uses (8 % faster where
//                              measured, profiles/db_union_probe.txt); "union_copy_bytes" = 8 selects the other
// The order is the filter stage's own (filter_sortkey_kernel, the radix sort, filter_order_kernel), called from the host code.
// Every output position comes from the sort or from an exclusive scan of the counts (scan_u32), none from an atomic: the result is
// the same bits on every run.  (The one atomic, a minimum over the duplicate positions, orders nothing and is read by the host alone.)
//
// The sources are described by one small table in device memory.  A pointer read from it is generic to the compiler: every access
// through one goes through an address_space(1) type (as global_u32_ptr in kernels_keymajor.hpp), or FLAT loads appear.
#pragma once
#include "kernels_dbload.hpp"
#include "kernels_keymajor.hpp"

namespace ipkgpu {

// One row per source and one more behind the last: `first` = the keys of the sources before this one (the row behind the last: all).
struct DbUnionSrc {
    const uint32_t* keys;
    const uint64_t* key_off;
    const uint2* entries;            // read as 64-bit words
    const uint32_t* positions;       // null in a union of plain databases
    const float* fv32;               // read as their bits
    const double* fv64;
    uint64_t first;
};

typedef const unsigned long long __attribute__((address_space(1)))* global_u64_ptr_t;

// the source of concatenated index c: the last s of [0, n_srcs) with first[s] <= c (sources without keys are passed over)
__device__ __forceinline__ uint32_t db_union_source_of(const DbUnionSrc* __restrict__ table, uint32_t n_srcs, uint64_t c)
{
    uint32_t lo = 0, hi = n_srcs - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (table[mid].first <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void db_union_sortkey_kernel(const DbUnionSrc* __restrict__ table, uint32_t n_srcs, uint64_t n,
                                                               unsigned long long* __restrict__ sortkey)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const uint32_t s = db_union_source_of(table, n_srcs, c);
    const uint32_t key = ((global_u32_ptr)table[s].keys)[c - table[s].first];
    sortkey[c] = ((unsigned long long)key << 32) | (unsigned long long)c;
}

// One thread per sorted position j.  fv32 / fv64 leave as the source's bits.  *dup_at (0xFFFFFFFF before the launch; n < 2^32) ends as
// the smallest j > 0 whose key is its left neighbour's.
__global__ __launch_bounds__(256) void db_union_keys_kernel(const DbUnionSrc* __restrict__ table, uint32_t n_srcs,
                                                            const unsigned long long* __restrict__ sorted, uint64_t n,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ fv32_bits,
                                                            unsigned long long* __restrict__ fv64_bits, uint32_t* __restrict__ counts,
                                                            uint32_t* __restrict__ src_of, uint64_t* __restrict__ start_of,
                                                            uint32_t* __restrict__ dup_at)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long sk = sorted[j];
    const uint32_t key = (uint32_t)(sk >> 32);
    const uint64_t c = (uint32_t)sk;
    const uint32_t s = db_union_source_of(table, n_srcs, c);
    const uint64_t i = c - table[s].first;
    const global_u64_ptr_t off = (global_u64_ptr_t)table[s].key_off;
    const uint64_t a = off[i], b = off[i + 1];
    if (j > 0 && (uint32_t)(sorted[j - 1] >> 32) == key) atomicMin(dup_at, (uint32_t)j);
    keys[j] = key;
    fv32_bits[j] = ((global_u32_ptr)table[s].fv32)[i];
    fv64_bits[j] = ((global_u64_ptr_t)table[s].fv64)[i];
    counts[j] = (uint32_t)(b - a);
    src_of[j] = s;
    start_of[j] = a;
}

// Work by ENTRY ranges: a workgroup moves the union's entries [tile * DB_UNPACK_TILE, ...) whatever keys they belong to, so a key of
// one entry and one of thousands cost alike.  The keys a tile touches are found once (two searches over key_off, the same in every
// lane); each lane then finds its entry's key among those (db_key_of_entry: keys without entries are passed over) and reads 8 bytes
// of the key's source at start + (e - key_off[j]), and 4 bytes of position.  The four loads of a lane are issued before its stores;
// consecutive lanes store consecutive entries.
template <bool POS>
__global__ __launch_bounds__(256) void db_union_entries_kernel(const DbUnionSrc* __restrict__ table, const uint64_t* __restrict__ key_off,
                                                               const uint32_t* __restrict__ src_of, const uint64_t* __restrict__ start_of,
                                                               uint64_t n_keys, uint64_t n_entries,
                                                               unsigned long long* __restrict__ entries, uint32_t* __restrict__ positions)
{
    const uint64_t e0 = (uint64_t)blockIdx.x * DB_UNPACK_TILE;
    if (e0 >= n_entries) return;
    const uint64_t e_last = min(e0 + DB_UNPACK_TILE, n_entries) - 1;
    const uint64_t j_lo = db_key_of_entry(key_off, 0, n_keys - 1, e0);
    const uint64_t j_hi = db_key_of_entry(key_off, j_lo, n_keys - 1, e_last);
    unsigned long long v[DB_UNPACK_PER_THREAD];
    uint32_t p[DB_UNPACK_PER_THREAD];
#pragma unroll
    for (uint32_t r = 0; r < DB_UNPACK_PER_THREAD; ++r) {
        const uint64_t e = e0 + r * 256 + threadIdx.x;
        v[r] = 0; p[r] = 0;
        if (e <= e_last) {
            const uint64_t j = db_key_of_entry(key_off, j_lo, j_hi, e);
            const uint64_t in_key = e - key_off[j];
            const uint64_t at = start_of[j] + in_key;
            const DbUnionSrc& src = table[src_of[j]];
            v[r] = ((global_u64_ptr_t)src.entries)[at];
            if (POS) p[r] = ((global_u32_ptr)src.positions)[at];
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < DB_UNPACK_PER_THREAD; ++r) {
        const uint64_t e = e0 + r * 256 + threadIdx.x;
        if (e <= e_last) {
            entries[e] = v[r];
            if (POS) positions[e] = p[r];
        }
    }
}

// The 16-byte form of the copy, the default (tools/db_union_probe.py measures it beside the 8-byte form, "union_copy_bytes" = 8): a lane takes
// the PAIR of entries (e, e + 1), e even -- the pair's second entry is looked up anew only where it leaves the first one's key -- and
// stores 16 bytes (and 8 of positions) at once; the reads stay 8 bytes, for a key's entries in its source are 8-byte aligned and no more.
// The same entry ranges, the same output bits.
template <bool POS>
__global__ __launch_bounds__(256) void db_union_entries16_kernel(const DbUnionSrc* __restrict__ table, const uint64_t* __restrict__ key_off,
                                                                 const uint32_t* __restrict__ src_of, const uint64_t* __restrict__ start_of,
                                                                 uint64_t n_keys, uint64_t n_entries,
                                                                 unsigned long long* __restrict__ entries, uint32_t* __restrict__ positions)
{
    const uint64_t e0 = (uint64_t)blockIdx.x * DB_UNPACK_TILE;
    if (e0 >= n_entries) return;
    const uint64_t e_last = min(e0 + DB_UNPACK_TILE, n_entries) - 1;
    const uint64_t j_lo = db_key_of_entry(key_off, 0, n_keys - 1, e0);
    const uint64_t j_hi = db_key_of_entry(key_off, j_lo, n_keys - 1, e_last);
    constexpr uint32_t PAIRS = DB_UNPACK_PER_THREAD / 2;
    ulonglong2 v[PAIRS];
    uint2 p[PAIRS];
#pragma unroll
    for (uint32_t r = 0; r < PAIRS; ++r) {
        const uint64_t e = e0 + 2 * (uint64_t)(r * 256 + threadIdx.x);
        v[r] = make_ulonglong2(0, 0); p[r] = make_uint2(0, 0);
        if (e <= e_last) {
            const uint64_t j = db_key_of_entry(key_off, j_lo, j_hi, e);
            const uint64_t at = start_of[j] + (e - key_off[j]);
            const DbUnionSrc& src = table[src_of[j]];
            v[r].x = ((global_u64_ptr_t)src.entries)[at];
            if (POS) p[r].x = ((global_u32_ptr)src.positions)[at];
            if (e + 1 <= e_last) {
                // (e + 1 <= e_last lies in a key of [j, j_hi]; beyond key j's end that key is at least j + 1, and key_off[j + 1] <= e + 1)
                const uint64_t j2 = e + 1 < key_off[j + 1] ? j : db_key_of_entry(key_off, j + 1, j_hi, e + 1);
                const uint64_t at2 = start_of[j2] + (e + 1 - key_off[j2]);
                const DbUnionSrc& src2 = table[src_of[j2]];
                v[r].y = ((global_u64_ptr_t)src2.entries)[at2];
                if (POS) p[r].y = ((global_u32_ptr)src2.positions)[at2];
            }
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < PAIRS; ++r) {
        const uint64_t e = e0 + 2 * (uint64_t)(r * 256 + threadIdx.x);
        if (e + 1 <= e_last) {                                    // (e is even and the arrays are 256-byte aligned: 16- and 8-byte aligned stores)
            *reinterpret_cast<ulonglong2*>(entries + e) = v[r];
            if (POS) *reinterpret_cast<uint2*>(positions + e) = p[r];
        } else if (e <= e_last) {
            entries[e] = v[r].x;
            if (POS) positions[e] = p[r].x;
        }
    }
}

}  // namespace ipkgpu
