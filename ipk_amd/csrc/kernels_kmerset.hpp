// kernels_kmerset.hpp -- the k-mer set of a batch of queries: every code a placement of them would look up (ipkgpu_kmer_set_of_queries).
//
// Placement never reads a key that none of the batch's windows encodes, so a database restricted to these codes places the batch bit
// for bit as the whole database does (ipkgpu_db_select_keys, ipkgpu_db_load_wanted).  The set is a bitmap over the code space, bit
// `code` of word code >> 5: 2^(bits per symbol * k) bits.
//
//   kmer_set_kernel        one wavefront per query, 64 windows a step, as place_ext_kernel: the same symbol and mask tables, the same
//                          ballot planes (place_plane_at, place_window_code of kernels_place.hpp), the reverse strand read through the
//                          complemented tables.  Where the placement looks a code up, the lane sets its bit: one vector atomicOr for an
//                          exact window, one per resolution for an ambiguous one.  No order matters: OR is idempotent and commutative.
//   kmer_set_count_kernel  the number of set bits: popcounts, a wavefront reduction, one 64-bit atomicAdd per wavefront
#pragma once
#include "kernels_place.hpp"

namespace ipkgpu {

struct KmerSetArgs {
    const unsigned char* seqs; const uint64_t* seq_off; uint64_t seq_base; uint32_t n_queries;
    uint32_t sigma, k, ambiguity, strands;
    uint32_t* bitmap;
};

template <int BITS>
__global__ __launch_bounds__(64) void kmer_set_kernel(KmerSetArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char set_lds[PLACE_EXT_TAB_BYTES];
    unsigned char* symtab = set_lds;
    uint32_t* masktab = reinterpret_cast<uint32_t*>(set_lds + 512);
    const uint32_t lane = lane_id();
    for (uint32_t t = lane; t < 256; t += 64) {
        const uint32_t s = place_symbol(a.sigma, t);
        const uint32_t other = (a.ambiguity && place_ambiguity_mask(a.sigma, t)) ? PLACE_SYM_AMBIGUOUS : 0xFFu;
        symtab[t] = (unsigned char)(s != 0xFFu ? s : other);
        symtab[256 + t] = (unsigned char)(s != 0xFFu ? 3u - s : other);          // (read on the reverse strand: DNA only)
    }
    if (lane < 32) {
        const uint32_t m = a.ambiguity ? place_ambiguity_mask(a.sigma, 64u + lane) : 0u;
        masktab[lane] = m;
        masktab[32 + lane] = ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3);
    }
    wave_lds_sync();
    const uint32_t k = a.k, mask_k = (1u << k) - 1u;

    for (uint32_t q = blockIdx.x; q < a.n_queries; q += gridDim.x) {
        const uint64_t q0 = a.seq_off[q] - a.seq_base;
        const uint32_t n = (uint32_t)(a.seq_off[q + 1] - a.seq_base - q0);
        const unsigned char* seq = a.seqs + q0;
        for (uint32_t pass = 0; pass <= a.strands; ++pass) {
            const unsigned char* tab = symtab + pass * 256u;
            const uint32_t* masks = masktab + pass * 32u;
            auto at = [&](uint64_t p) -> uint32_t { return pass ? seq[n - 1 - p] : seq[p]; };
            for (uint64_t base = 0; base + k <= n; base += 64) {
                const uint64_t p0 = base + lane, p1 = base + 64 + lane;
                const uint32_t s_lo = p0 < n ? tab[at(p0)] : 0xFFu;
                const uint32_t s_hi = (lane + 1 < k && p1 < n) ? tab[at(p1)] : 0xFFu;
                const uint32_t valid_bits = place_plane_at(ballot64(s_lo != 0xFFu), ballot64(s_hi != 0xFFu), lane);
                bool win = (valid_bits & mask_k) == mask_k;                  // (a window that runs past the end meets an invalid symbol there)
                const uint32_t amb_bits = place_plane_at(ballot64(s_lo == PLACE_SYM_AMBIGUOUS), ballot64(s_hi == PLACE_SYM_AMBIGUOUS), lane) & mask_k;
                const bool amb = win && __popc(amb_bits) == 1;
                win = win && amb_bits == 0;
                uint32_t code = place_window_code<BITS>(s_lo, s_hi, lane, k);
                if (win) atomicOr(&a.bitmap[code >> 5], 1u << (code & 31u));
                if (amb) {                                                   // every resolution of the one ambiguous position
                    const uint32_t pos = (uint32_t)__builtin_ctz(amb_bits);
                    const uint32_t a_shift = (uint32_t)BITS * (k - 1u - pos);
                    code &= ~(((1u << BITS) - 1u) << a_shift);
                    uint32_t m = masks[at(base + lane + pos) & 31u];
                    while (m) {
                        const uint32_t sym = (uint32_t)__builtin_ctz(m);
                        m &= m - 1u;
                        const uint32_t c = code | (sym << a_shift);
                        atomicOr(&a.bitmap[c >> 5], 1u << (c & 31u));
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void kmer_set_count_kernel(const uint32_t* __restrict__ bitmap, uint64_t n_words, unsigned long long* __restrict__ count)
{
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256) c += (uint32_t)__popc(bitmap[i]);
    for (int s = 32; s > 0; s >>= 1) c += (uint32_t)__shfl_xor((int)c, s, 64);
    if (lane_id() == 0 && c) atomicAdd(count, (unsigned long long)c);
}

}  // namespace ipkgpu
