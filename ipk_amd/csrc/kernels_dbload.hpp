// kernels_dbload.hpp -- unpacks the k-mer records of a database file on the device (layout: ipk_format.hpp): the reverse of
// kernels_dbfile.hpp.
//
// The reference loads a database with i2l::load (un-vendored), record by record into a hash map; its tools work on that object
// (tools/src/diff.cpp:118-135).  Here the file's body lies in device memory as one image, the host has walked the count fields
// (ipkfmt::RecordWalker: every record start is known and every record ends inside the image) and the kernels only move bytes:
//   db_unpack_heads_kernel    per record: key, filter value bits, count -- in FILE order
//   db_load_order_kernel      behind the sort of (key, record): the arrays in KEY order, the file's record order, duplicates
//   db_unpack_entries_kernel  per ENTRY: image -> entries[key_off[j] ..] (and the u16 positions -> u32)
// The image starts at a 256-byte aligned address, so a plain record (16 + 8 n bytes) is 8-byte aligned and a positioned one
// (16 + 10 n) 2-byte aligned.  No kernel takes an index from the image: offsets come from the host's walk, counts are the ones it checked.
#pragma once
#include "dcla_device.hpp"
#include "ipk_format.hpp"

namespace ipkgpu {

// One thread per record.  sortkey = key << 32 | record index: sorted, it gives ascending keys and, for each, its record.
template <bool POS>
__global__ __launch_bounds__(256) void db_unpack_heads_kernel(const unsigned char* __restrict__ image, const uint64_t* __restrict__ starts,
                                                              uint64_t n, unsigned long long* __restrict__ sortkey,
                                                              uint32_t* __restrict__ fv_bits, uint32_t* __restrict__ counts)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned char* p = image + starts[i];
    uint32_t key, fv, cnt;
    if (POS) {                                                // 2-byte aligned: 16-bit loads (the high count word is zero: checked by the host)
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
        key = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
        fv = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
        cnt = (uint32_t)h[4] | ((uint32_t)h[5] << 16);
    } else {
        const uint2 a = reinterpret_cast<const uint2*>(p)[0];
        key = a.x; fv = a.y;
        cnt = reinterpret_cast<const uint2*>(p)[1].x;
    }
    sortkey[i] = ((unsigned long long)key << 32) | (unsigned long long)i;
    fv_bits[i] = fv;
    counts[i] = cnt;
}

// One thread per key position j of the sorted (key, record) list.  order[record] = j: keys[order[i]] is the file's i-th record.
// BODY: starts are record starts in the image and body_off the places of the records' entries there; false (the streamed load,
// kernels_dbstream.hpp): starts are already the places of the records' entries, in its file-order entry array, and go through as they are.
template <bool BODY = true>
__global__ __launch_bounds__(256) void db_load_order_kernel(const unsigned long long* __restrict__ sorted, const uint64_t* __restrict__ starts,
                                                            const uint32_t* __restrict__ fv_bits, const uint32_t* __restrict__ counts, uint64_t n,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ counts_sorted,
                                                            uint64_t* __restrict__ body_off, float* __restrict__ fv32, double* __restrict__ fv64,
                                                            uint32_t* __restrict__ order, uint32_t* __restrict__ duplicate)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long s = sorted[j];
    const uint32_t key = (uint32_t)(s >> 32), rec = (uint32_t)s;
    if (j > 0 && (uint32_t)(sorted[j - 1] >> 32) == key) atomicOr(duplicate, 1u);
    keys[j] = key;
    counts_sorted[j] = counts[rec];
    body_off[j] = starts[rec] + (BODY ? ipkfmt::RECORD_HEAD_BYTES : 0);
    const float f = __uint_as_float(fv_bits[rec]);
    fv32[j] = f;
    fv64[j] = (double)f;
    order[rec] = (uint32_t)j;
}

constexpr uint32_t DB_UNPACK_PER_THREAD = 4;
constexpr uint32_t DB_UNPACK_TILE = 256 * DB_UNPACK_PER_THREAD;      // entries per workgroup

// the last j of [lo, hi] with key_off[j] <= e (key_off[lo] <= e given)
__device__ __forceinline__ uint64_t db_key_of_entry(const uint64_t* __restrict__ key_off, uint64_t lo, uint64_t hi, uint64_t e)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (key_off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Work by ENTRY ranges: a workgroup moves the entries [tile * DB_UNPACK_TILE, ...) whatever records they belong to, so a key of one
// entry and one of thousands cost alike.  The keys a tile touches are found once (two searches over all of key_off, the same in every
// lane); each lane then finds its entry's key among those alone -- no step for a tile inside one long record, ten for 1024 keys of
// one entry each -- and reads 8 bytes (plain) or three aligned dwords funnel-shifted by the record's 2-byte phase (positioned: the
// image is padded so that the third dword of the last entry exists).  Stores: 8 bytes per lane, consecutive lanes consecutive entries.
template <bool POS>
__global__ __launch_bounds__(256) void db_unpack_entries_kernel(const unsigned char* __restrict__ image, const uint64_t* __restrict__ key_off,
                                                                const uint64_t* __restrict__ body_off, uint64_t n_keys, uint64_t n_entries,
                                                                uint2* __restrict__ entries, uint32_t* __restrict__ positions)
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
        const uint64_t in_key = e - key_off[j];
        if (POS) {
            const uint64_t at = body_off[j] + ipkfmt::ENTRY_POS_BYTES * in_key;         // 2-byte aligned
            const uint32_t* w = reinterpret_cast<const uint32_t*>(image + (at & ~(uint64_t)3));
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            const uint32_t sh = (uint32_t)(at & 2) * 8;                                  // 0 or 16 bits
            entries[e] = make_uint2(__funnelshift_r(w0, w1, sh), __funnelshift_r(w1, w2, sh));
            positions[e] = (w2 >> sh) & 0xFFFFu;
        } else {
            entries[e] = *reinterpret_cast<const uint2*>(image + body_off[j] + ipkfmt::ENTRY_BYTES * in_key);
        }
    }
}

}  // namespace ipkgpu
