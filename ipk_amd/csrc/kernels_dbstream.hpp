// kernels_dbstream.hpp -- the kernels of the streamed, restricted load (ipkgpu_db_load_wanted; db_stream.hpp).
//
// The file's body passes through a device window of bounded size, whole records at a time; of each window only the records whose key
// is in a k-mer set stay.  Per window, behind db_unpack_heads_kernel (kernels_dbload.hpp, as it is):
//   db_stream_flag_kernel     per record: wanted = the key's bit in the set (db_key_wanted: the bound first, the key is the file's), and
//                             its count if it is wanted, else 0
//   (two scans: of the flags -- the record's place among the window's kept records -- and of those counts -- its entries' place)
//   db_stream_append_kernel   per wanted record: (key, kept index), filter bits, count and the place of its entries to the end of the
//                             kept heads, in file order; and its (destination offset, body offset) segment for
//                             db_unpack_entries_kernel, which then appends the wanted entries by entry ranges, as it is
// After the last window the kept heads are sorted by (key, kept index) and db_load_order_kernel<false> makes the arrays in key order;
//   db_stream_gather_kernel   per ENTRY: kept entries from file order into key order, by db_unpack_entries_kernel's tile scheme
// ipkgpu_db_load_key_range takes db_stream_flag_range_kernel (key_lo <= key < key_hi) in place of the bitmap test.  The histogram pass
// of ipkgpu_db_diff_files keeps nothing: behind the heads only db_stream_hist_kernel, records and entries per key bin.
// No output place comes from an atomic: the kept records keep the file's order, the result is the same bits on every run (the
// histogram's integer sums do not depend on the order of their atomics either).
#pragma once
#include "kernels_dbselect.hpp"

namespace ipkgpu {

constexpr uint64_t DB_STREAM_WINDOW = (uint64_t)256 << 20;           // bytes of the device window when "db_load_window_bytes" is 0
constexpr uint32_t DB_HIST_BINS = 1u << 16;                          // key bins of ipkgpu_db_diff_files' histogram pass

__global__ __launch_bounds__(256) void db_stream_flag_kernel(const unsigned long long* __restrict__ sortkey, const uint32_t* __restrict__ counts, uint64_t n,
                                                             const uint32_t* __restrict__ bitmap, uint64_t n_codes, uint32_t* __restrict__ flag,
                                                             uint32_t* __restrict__ cnt_wanted)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool w = db_key_wanted(bitmap, n_codes, (uint32_t)(sortkey[i] >> 32));
    flag[i] = w ? 1u : 0u;
    cnt_wanted[i] = w ? counts[i] : 0u;
}

// The second predicate of the streamed load (ipkgpu_db_load_key_range): wanted = key_lo <= key < key_hi, in 64 bits (key_hi may be
// 2^32).  A kernel of its own, so that the bitmap path above compiles to what it was.
__global__ __launch_bounds__(256) void db_stream_flag_range_kernel(const unsigned long long* __restrict__ sortkey, const uint32_t* __restrict__ counts, uint64_t n,
                                                                   uint64_t key_lo, uint64_t key_hi, uint32_t* __restrict__ flag,
                                                                   uint32_t* __restrict__ cnt_wanted)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = (uint64_t)(sortkey[i] >> 32);
    const bool w = key >= key_lo && key < key_hi;
    flag[i] = w ? 1u : 0u;
    cnt_wanted[i] = w ? counts[i] : 0u;
}

// The histogram pass of ipkgpu_db_diff_files: one thread per record of the window; bin = min(key >> shift, DB_HIST_BINS - 1).
// rec_hist[bin] += 1, ent_hist[bin] += the record's entry count: integer vector atomics in global memory (sums of integers: the same
// totals on every run whatever the order).  Both histograms have DB_HIST_BINS elements; the bin is clamped before it indexes.
__global__ __launch_bounds__(256) void db_stream_hist_kernel(const unsigned long long* __restrict__ sortkey, const uint32_t* __restrict__ counts, uint64_t n,
                                                             uint32_t shift, uint32_t* __restrict__ rec_hist, unsigned long long* __restrict__ ent_hist)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = (uint32_t)(sortkey[i] >> 32);
    const uint32_t bin = min(key >> shift, DB_HIST_BINS - 1);
    atomicAdd(&rec_hist[bin], 1u);
    const uint32_t c = counts[i];
    if (c) atomicAdd(&ent_hist[bin], (unsigned long long)c);
}

// f_scan, c_scan: the exclusive scans of flag and cnt_wanted, n + 1 values each.  kept_base, entry_base: the kept records and entries
// of the windows before.  seg_dst / seg_src: [kept in this window (+ 1)] what db_unpack_entries_kernel takes as key_off / body_off.
__global__ __launch_bounds__(256) void db_stream_append_kernel(const unsigned long long* __restrict__ sortkey, const uint32_t* __restrict__ fv_bits,
                                                               const uint32_t* __restrict__ counts, const uint64_t* __restrict__ starts,
                                                               const uint32_t* __restrict__ flag, const uint64_t* __restrict__ f_scan,
                                                               const uint64_t* __restrict__ c_scan, uint64_t n, uint64_t kept_base, uint64_t entry_base,
                                                               unsigned long long* __restrict__ k_sortkey, uint32_t* __restrict__ k_fv_bits,
                                                               uint32_t* __restrict__ k_counts, uint64_t* __restrict__ k_entry_off,
                                                               uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) seg_dst[f_scan[n]] = c_scan[n];
    if (!flag[i]) return;
    const uint64_t f = f_scan[i], g = kept_base + f;
    k_sortkey[g] = (sortkey[i] & 0xFFFFFFFF00000000ull) | (unsigned long long)g;
    k_fv_bits[g] = fv_bits[i];
    k_counts[g] = counts[i];
    k_entry_off[g] = entry_base + c_scan[i];
    seg_dst[f] = c_scan[i];
    seg_src[f] = starts[i] + ipkfmt::RECORD_HEAD_BYTES;
}

// Work by ENTRY ranges, as db_unpack_entries_kernel: the keys a tile touches are found once, each lane finds its entry's key among those.
// src_off[j]: where key j's entries start in the file-order arrays.
template <bool POS>
__global__ __launch_bounds__(256) void db_stream_gather_kernel(const uint64_t* __restrict__ key_off, const uint64_t* __restrict__ src_off, uint64_t n_keys,
                                                               uint64_t n_entries, const uint2* __restrict__ k_entries,
                                                               const uint32_t* __restrict__ k_positions, uint2* __restrict__ entries,
                                                               uint32_t* __restrict__ positions)
{
    const uint64_t e0 = (uint64_t)blockIdx.x * DB_UNPACK_TILE;
    if (e0 >= n_entries) return;
    const uint64_t e_last = min(e0 + DB_UNPACK_TILE, n_entries) - 1;
    const uint64_t j_lo = db_key_of_entry(key_off, 0, n_keys - 1, e0);
    const uint64_t j_hi = db_key_of_entry(key_off, j_lo, n_keys - 1, e_last);
#pragma unroll
    for (uint32_t r = 0; r < DB_UNPACK_PER_THREAD; ++r) {
        const uint64_t e = e0 + r * 256 + threadIdx.x;
        if (e > e_last) break;
        const uint64_t j = db_key_of_entry(key_off, j_lo, j_hi, e);
        const uint64_t from = src_off[j] + (e - key_off[j]);
        entries[e] = k_entries[from];
        if (POS) positions[e] = k_positions[from];
    }
}

}  // namespace ipkgpu
