// kernels_dbfile.hpp -- packs the k-mer records of the database file on the device (layout: ipk_format.hpp).
//
// Device analogue of the serialisation loop at db_builder.cpp:323-327: `for (kmer, fv) in kmer_order: save_phylo_kmer(...)`.
// The file body is produced in filter order straight from the key-major database arrays; the host only writes bytes.
#pragma once
#include "dcla_device.hpp"
#include "ipk_format.hpp"

namespace ipkgpu {

// rec_bytes[i] = size of the record of the i-th k-mer in filter order (u32: a k-mer has at most one entry per branch group, and
// a batch holds < 2^22 groups -- ipkgpu_db_write refuses databases whose largest record would not fit)
__global__ __launch_bounds__(256) void db_record_sizes_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ key_off,
                                                              uint64_t n_keys, uint32_t* __restrict__ rec_bytes, uint32_t* __restrict__ too_big,
                                                              bool positions = false)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_keys) return;
    const uint32_t k = order[i];
    const uint64_t n = key_off[k + 1] - key_off[k];
    if (n >= (1ull << 28)) atomicOr(too_big, 1u);
    rec_bytes[i] = (uint32_t)(positions ? ipkfmt::record_bytes_positions(n) : ipkfmt::record_bytes(n));
}

// One wavefront per k-mer of [i_lo, i_hi) (positions in filter order): head words by lane 0, entries by all lanes.
// `out` receives the body bytes [rec_off[i_lo], rec_off[i_hi]).
__global__ __launch_bounds__(256) void db_pack_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ key_off, const uint2* __restrict__ entries,
                                                      const float* __restrict__ fv, const uint64_t* __restrict__ rec_off,
                                                      uint64_t i_lo, uint64_t i_hi, unsigned char* __restrict__ out)
{
    const uint64_t i = i_lo + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= i_hi) return;
    const uint32_t lane = lane_id();
    const uint32_t k = order[i];
    const uint64_t a = key_off[k], n = key_off[k + 1] - a;
    unsigned char* dst = out + (rec_off[i] - rec_off[i_lo]);
    if (lane == 0) {
        uint32_t w[4];
        ipkfmt::record_head(keys[k], __float_as_uint(fv[k]), n, w);
        // records are 16 + 8 n bytes: a head is 8-byte aligned, not 16 -- two 8-byte stores, not one uint4
        reinterpret_cast<uint2*>(dst)[0] = make_uint2(w[0], w[1]);
        reinterpret_cast<uint2*>(dst)[1] = make_uint2(w[2], w[3]);
    }
    uint2* e = reinterpret_cast<uint2*>(dst + ipkfmt::RECORD_HEAD_BYTES);
    for (uint64_t j = lane; j < n; j += 64) e[j] = entries[a + j];                // (branch, score bits) = the entry's bytes
}

// ---- the positioned database (ipk-aa-pos): entries of (branch, score, u16 position), ipk_format.hpp ENTRY_POS_BYTES
// raises *too_big if a window position does not fit the entry's field
__global__ __launch_bounds__(256) void db_positions_check_kernel(const uint32_t* __restrict__ positions, uint64_t n, uint32_t* __restrict__ too_big)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && positions[i] > ipkfmt::POSITION_MAX) atomicOr(too_big, 1u);
}

// db_pack_kernel for positioned records: 16 + 10 n bytes, so a record is aligned to two bytes only -- everything leaves as 16-bit stores
__global__ __launch_bounds__(256) void db_pack_positions_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ keys,
                                                                const uint64_t* __restrict__ key_off, const uint2* __restrict__ entries,
                                                                const uint32_t* __restrict__ positions, const float* __restrict__ fv,
                                                                const uint64_t* __restrict__ rec_off, uint64_t i_lo, uint64_t i_hi,
                                                                unsigned char* __restrict__ out)
{
    static_assert(ipkfmt::ENTRY_POS_BYTES == 10 && ipkfmt::RECORD_HEAD_BYTES == 16, "five and eight 16-bit words");
    const uint64_t i = i_lo + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= i_hi) return;
    const uint32_t lane = lane_id();
    const uint32_t k = order[i];
    const uint64_t a = key_off[k], n = key_off[k + 1] - a;
    uint16_t* dst = reinterpret_cast<uint16_t*>(out + (rec_off[i] - rec_off[i_lo]));
    if (lane < 4) {
        uint32_t w[4];
        ipkfmt::record_head(keys[k], __float_as_uint(fv[k]), n, w);
        const uint32_t v = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
        dst[2 * lane] = (uint16_t)v; dst[2 * lane + 1] = (uint16_t)(v >> 16);
    }
    uint16_t* e = dst + ipkfmt::RECORD_HEAD_BYTES / 2;
    for (uint64_t j = lane; j < n; j += 64) {
        const uint2 en = entries[a + j];
        uint16_t* d = e + 5 * j;
        d[0] = (uint16_t)en.x; d[1] = (uint16_t)(en.x >> 16); d[2] = (uint16_t)en.y; d[3] = (uint16_t)(en.y >> 16);
        d[4] = (uint16_t)positions[a + j];
    }
}

}  // namespace ipkgpu
