// kernels_place.hpp -- places query sequences on a database that lives on the device (ipkgpu_db_place; DESIGN.md section 3, "Placement").
//
// The definition (include/ipkgpu.h): every valid window of a query is a k-mer code; the codes that are keys of the database add
// their entries' scores to S[branch] IN WINDOW ORDER, in binary32, and 1 to C[branch]; score[b] = S[b] + (float)(W - C[b]) * log_eps
// over the W valid windows; the best `keep` branches by (score descending, branch ascending) and their likelihood weight ratios.
//
//   place_index_kernel     once per database: lower bounds into keys[] of the 2^P prefixes of the code (P = min(16, code bits)), so a
//                          lookup is a binary search inside one prefix's short range
//   place_max_branch_kernel, place_dupcheck_kernel   once per database: B = 1 + the largest branch id, and the precondition that
//                          a key names a branch once (a bitmap per wavefront in LDS, PLACE_DUP_BITS branches per pass)
//   place_kernel           one wavefront per query.  64 windows at a time: the lanes' symbols become bit planes (one ballot per bit of
//                          the symbol code and one for "valid symbol"), a lane's window code and validity are shifts of those planes --
//                          no lane reads a symbol twice; every lane looks its window up.  Then the 64 windows are walked in order, the
//                          lanes taking a window's entries 64 at a time (branches are distinct inside a key: no conflicts, no atomics),
//                          the next tile's entries loaded under the current tile's adds: one branch's scores are added in window
//                          order by construction.  S, C and the list of touched branches live in LDS up to PLACE_LDS_BRANCHES
//                          branches (template parameter GLOBAL = false), beyond that in the workgroup's slice of a global scratch
//                          block (GLOBAL = true); the address space is fixed per instantiation, never a generic pointer.
//                          Epilogue: over the touched branches only -- scores, a sorted top list of one 64-bit (score, branch) word
//                          per lane, the f64 denominator; the same walk clears S and C for the workgroup's next query.
//                          Each phase is one inlined function (place_tables .. place_store) that place_ext_kernel calls as well.
#pragma once
#include "../../include/ipkgpu.h"
#include "dcla_device.hpp"

namespace ipkgpu {

constexpr uint32_t PLACE_INDEX_BITS = 16;        // the prefix table has at most 2^16 + 1 lower bounds
// S (f32), C (u32) and the touched list (u32) of a query stay in LDS up to this many branches: 12 bytes each, 48 KiB of the CU's
// 160 KiB at the bound (three queries per CU there); the launch sizes the block's LDS by the database's own branch count, so a tree of a
// few hundred branches leaves the CU to the wavefront limit.  Trees beyond the bound use the global tables.
constexpr uint32_t PLACE_LDS_BRANCHES = 4096;
constexpr uint32_t PLACE_DUP_BITS = 32768;       // branches per pass of the per-wavefront bitmap of place_dupcheck_kernel (4 KiB)
constexpr uint32_t PLACE_NONE = 0xFFFFFFFFu;     // "no placement" in the branch array
constexpr uint32_t PLACE_SYMTAB_BYTES = 256;

// code of a sequence byte in the database's symbol order (DNA ACGT, U = T; AA RHKDESTNQCGPAILMFWYV), case-insensitive; 0xFF: invalid
__device__ __forceinline__ uint32_t place_symbol(uint32_t sigma, uint32_t byte)
{
    const uint32_t c = (byte >= 'a' && byte <= 'z') ? byte - 32u : byte;
    if (sigma == 4) {
        switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': case 'U': return 3; default: return 0xFF; }
    }
    switch (c) {
    case 'R': return 0; case 'H': return 1; case 'K': return 2; case 'D': return 3; case 'E': return 4; case 'S': return 5; case 'T': return 6;
    case 'N': return 7; case 'Q': return 8; case 'C': return 9; case 'G': return 10; case 'P': return 11; case 'A': return 12; case 'I': return 13;
    case 'L': return 14; case 'M': return 15; case 'F': return 16; case 'W': return 17; case 'Y': return 18; case 'V': return 19;
    default: return 0xFF;
    }
}

// table[j] = the number of keys below j << shift, j = 0 .. n_slots (table[n_slots] = n_keys)
__global__ __launch_bounds__(256) void place_index_kernel(const uint32_t* __restrict__ keys, uint32_t n_keys, uint32_t shift, uint32_t n_slots,
                                                          uint32_t* __restrict__ table)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > n_slots) return;
    uint32_t lo = 0, hi = n_keys;
    if (j == n_slots) lo = n_keys;
    else {
        const uint32_t key = j << shift;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
    }
    table[j] = lo;
}

__global__ __launch_bounds__(256) void place_max_branch_kernel(const uint2* __restrict__ entries, uint64_t n_entries, uint32_t* __restrict__ max_branch)
{
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_entries; i += (uint64_t)gridDim.x * 256) m = max(m, entries[i].x);
    for (int s = 32; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    if (lane_id() == 0) atomicMax(max_branch, m);
}

// One wavefront per key (keys [first, ...)): *bad_key = the lowest index of a key whose entries name a branch twice.
__global__ __launch_bounds__(256) void place_dupcheck_kernel(const uint64_t* __restrict__ key_off, const uint2* __restrict__ entries, uint64_t n_keys,
                                                             uint32_t n_branches, uint64_t first, unsigned long long* __restrict__ bad_key)
{
    __shared__ uint32_t bits[4][PLACE_DUP_BITS / 32];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = lane_id();
    uint32_t* bm = bits[wave];
    for (uint32_t t = lane; t < PLACE_DUP_BITS / 32; t += 64) bm[t] = 0;
    wave_lds_sync();
    const uint64_t i = first + (uint64_t)blockIdx.x * 4 + wave;
    if (i >= n_keys) return;
    const uint64_t a0 = key_off[i], n = key_off[i + 1] - a0;
    if (n < 2) return;
    bool dup = false;
    for (uint32_t r0 = 0; r0 < n_branches; r0 += PLACE_DUP_BITS) {
        for (uint64_t t0 = 0; t0 < n; t0 += 64) {
            const uint32_t rel = (t0 + lane < n ? entries[a0 + t0 + lane].x : PLACE_NONE) - r0;
            if (t0 + lane < n && rel < PLACE_DUP_BITS) {
                const uint32_t old = atomicOr(&bm[rel >> 5], 1u << (rel & 31));
                dup |= (old >> (rel & 31)) & 1u;
            }
        }
        wave_lds_sync();
        for (uint64_t t0 = 0; t0 < n; t0 += 64) {                        // the words this key touched, back to zero
            const uint32_t rel = (t0 + lane < n ? entries[a0 + t0 + lane].x : PLACE_NONE) - r0;
            if (t0 + lane < n && rel < PLACE_DUP_BITS) bm[rel >> 5] = 0;
        }
        wave_lds_sync();
    }
    if (ballot64(dup) != 0 && lane == 0) atomicMin(bad_key, (unsigned long long)i);
}

struct PlaceArgs {
    // the database and its prefix table
    const uint32_t* keys; const uint64_t* key_off; const uint2* entries; const uint32_t* index;
    uint32_t shift, k, sigma, n_branches, b_pad;
    float log_eps;
    // the batch: query q is bytes [seq_off[q] - seq_base, seq_off[q + 1] - seq_base) of seqs
    const unsigned char* seqs; const uint64_t* seq_off; uint64_t seq_base; uint32_t n_queries, keep;
    // GLOBAL: [gridDim.x][b_pad] each, S and C zero on entry (and left zero)
    float* g_s; uint32_t* g_c; uint32_t* g_touched;
    // results of the batch: [n_queries][keep] and [n_queries]
    uint32_t* out_branch; float* out_score; uint32_t* out_count; double* out_lwr; uint32_t* out_n_kmers; uint32_t* out_n_found; uint32_t* out_n_branches;
};

__device__ __forceinline__ uint64_t place_readlane64(uint64_t v, uint32_t l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}
// bits [lane, lane + 32) of the 128-bit plane (hi : lo)
__device__ __forceinline__ uint32_t place_plane_at(uint64_t lo, uint64_t hi, uint32_t lane)
{
    return (uint32_t)(lane ? (lo >> lane) | (hi << (64 - lane)) : lo);
}
// (score, branch) as one word: a larger word is a better placement (higher score; on equal scores the lower branch id); never 0
__device__ __forceinline__ uint64_t place_rank_word(float score, uint32_t branch)
{
    return ((uint64_t)enc_score_bits(__float_as_uint(score)) << 32) | (uint64_t)(0xFFFFFFFFu - branch);
}

// ---- the phases of a placement: one text each, inlined into place_kernel and place_ext_kernel ------------------------------------------
// S, C and touched are plain pointers whose address space the caller's GLOBAL fixes: the functions are inlined, so every instantiation
// keeps its LDS or global instructions (no generic pointer, no FLAT instruction).

// One pass over a query (one strand): the figures counted on the way, then what the epilogue leaves -- lane r's placement of rank r
// (branch PLACE_NONE: none), the best score and the denominator of the likelihood weight ratios.
struct PlacePass {
    uint32_t W = 0, n_found = 0, n_touched = 0, n_amb = 0;
    uint32_t branch = PLACE_NONE, count = 0;
    float score = 0.0f, best = 0.0f;
    double den = 0.0;
};

// S, C and the touched list of the workgroup: its slice of the global block, or the LDS behind the kernel's `tab_bytes` of symbol
// tables, which are zeroed here (the global ones are zero on entry).  The caller syncs once its own tables are written as well.
template <bool GLOBAL>
__device__ __forceinline__ void place_tables(const PlaceArgs& a, unsigned char* lds, uint32_t tab_bytes, uint32_t lane, float*& S, uint32_t*& C,
                                             uint32_t*& touched)
{
    if constexpr (GLOBAL) {
        S = a.g_s + (size_t)blockIdx.x * a.b_pad; C = a.g_c + (size_t)blockIdx.x * a.b_pad; touched = a.g_touched + (size_t)blockIdx.x * a.b_pad;
    } else {
        S = reinterpret_cast<float*>(lds + tab_bytes);
        C = reinterpret_cast<uint32_t*>(S + a.b_pad);
        touched = C + a.b_pad;
        for (uint32_t t = lane; t < a.b_pad; t += 64) { S[t] = 0.0f; C[t] = 0; }
    }
}

// the code of the lane's window (k symbols of BITS bits from the lane's position on) out of the ballot planes of the symbols
// s_lo (positions base + lane) and s_hi (base + 64 + lane)
template <int BITS>
__device__ __forceinline__ uint32_t place_window_code(uint32_t s_lo, uint32_t s_hi, uint32_t lane, uint32_t k)
{
    uint32_t plane[BITS];
#pragma unroll
    for (int p = 0; p < BITS; ++p) plane[p] = place_plane_at(ballot64((s_lo >> p) & 1u), ballot64((s_hi >> p) & 1u), lane);
    uint32_t code = 0;
    for (uint32_t i = 0; i < k; ++i) {
        uint32_t sym = 0;
#pragma unroll
        for (int p = 0; p < BITS; ++p) sym |= ((plane[p] >> i) & 1u) << p;
        code = (code << BITS) | sym;
    }
    return code;
}

// the entry range of `code` if it is a key: a binary search inside its prefix's range of keys[]
__device__ __forceinline__ bool place_lookup(const PlaceArgs& a, uint32_t code, uint64_t& off, uint32_t& cnt)
{
    const uint32_t j = code >> a.shift;
    uint32_t lo = a.index[j];
    const uint32_t end = a.index[j + 1];
    uint32_t hi = end;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.keys[mid] < code) lo = mid + 1; else hi = mid;
    }
    if (lo < end && a.keys[lo] == code) {
        off = a.key_off[lo];
        cnt = (uint32_t)(a.key_off[lo + 1] - off);
        return true;
    }
    return false;
}

// The lanes with v set add y to their branch b (distinct among them): S[b] += y, C[b] += 1, and a branch that had no contribution yet
// joins the touched list.  Ends with the sync that lets the next call name these branches from other lanes.  (The ambiguous window's
// P / c tables keep their own text of this: through here their f64 adds compiled to more SGPR spills, profiles/place_shared.txt.)
__device__ __forceinline__ void place_add(float* S, uint32_t* C, uint32_t* touched, uint32_t& n_touched, bool v, uint32_t b, float y)
{
    bool fresh = false;
    if (v) {
        S[b] = S[b] + y;
        const uint32_t c = C[b];
        C[b] = c + 1;
        fresh = c == 0;
    }
    const uint64_t fm = ballot64(fresh);
    if (fresh) touched[n_touched + mbcnt(fm)] = b;
    n_touched += (uint32_t)__popcll(fm);
    wave_lds_sync();
}

// The windows of `todo` (bit w: lane w's window, entries [off, off + cnt) of that lane) in order, a window's entries 64 at a time,
// the next tile loaded under this tile's adds: one branch's scores are added in window order.
__device__ __forceinline__ void place_walk(const PlaceArgs& a, float* S, uint32_t* C, uint32_t* touched, uint32_t& n_touched, uint64_t todo,
                                           uint64_t off, uint32_t cnt, uint32_t lane)
{
    uint64_t t_off = 0;
    uint32_t t_cnt = 0, t_at = 0;
    auto fetch = [&](uint2& e, bool& v) -> bool {
        if (t_at >= t_cnt) {
            if (todo == 0) return false;
            const uint32_t w = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            t_off = place_readlane64(off, w);
            t_cnt = (uint32_t)__builtin_amdgcn_readlane((int)cnt, (int)w);
            t_at = 0;
        }
        v = t_at + lane < t_cnt;
        e = v ? a.entries[t_off + t_at + lane] : make_uint2(0, 0);
        t_at += 64;
        return true;
    };
    uint2 cur; bool cur_v;
    bool more = fetch(cur, cur_v);
    while (more) {
        uint2 nxt = make_uint2(0, 0); bool nxt_v = false;
        more = fetch(nxt, nxt_v);
        place_add(S, C, touched, n_touched, cur_v, cur.x, __uint_as_float(cur.y));
        cur = nxt; cur_v = nxt_v;
    }
}

// the best `keep` of the touched branches sorted across the lanes: lane r's word is rank r's (0: no such rank)
__device__ __forceinline__ uint64_t place_top(const float* S, const uint32_t* C, const uint32_t* touched, uint32_t n_touched, uint32_t W,
                                              float log_eps, uint32_t keep, uint32_t lane)
{
    uint64_t top = 0;
    uint64_t kth = 0;                                                     // the word at rank keep - 1: what a candidate has to beat
    for (uint32_t i0 = 0; i0 < n_touched; i0 += 64) {
        uint64_t word = 0;
        if (i0 + lane < n_touched) {
            const uint32_t b = touched[i0 + lane];
            const float pen = (float)(W - C[b]) * log_eps;
            word = place_rank_word(S[b] + pen, b);
        }
        uint64_t pend = ballot64(word > kth);
        while (pend) {
            const uint32_t src = (uint32_t)__builtin_ctzll(pend);
            pend &= pend - 1;
            const uint64_t w = place_readlane64(word, src);
            if (w <= kth) continue;
            const uint64_t prev = __shfl_up((unsigned long long)top, 1, 64);
            if (w > top) top = (lane > 0 && w > prev) ? prev : w;
            kth = place_readlane64(top, keep - 1);
        }
    }
    return top;
}

// the denominator over ALL touched branches (f64, any order); S and C back to zero for the workgroup's next pass
__device__ __forceinline__ double place_denominator(float* S, uint32_t* C, const uint32_t* touched, uint32_t n_touched, uint32_t W, float log_eps,
                                                    float best, uint32_t lane)
{
    double den = 0.0;
    for (uint32_t i0 = 0; i0 < n_touched; i0 += 64) {
        if (i0 + lane < n_touched) {
            const uint32_t b = touched[i0 + lane];
            const float pen = (float)(W - C[b]) * log_eps;
            const float score = S[b] + pen;
            den += exp10((double)score - (double)best);
            S[b] = 0.0f; C[b] = 0;
        }
    }
    for (int s = 32; s > 0; s >>= 1) den += __shfl_xor(den, s, 64);
    wave_lds_sync();
    return den;
}

// the epilogue of a pass, over the touched branches only: the lanes' placements out of the top list, then the denominator
__device__ __forceinline__ void place_epilogue(const PlaceArgs& a, float* S, uint32_t* C, const uint32_t* touched, uint32_t lane, PlacePass& r)
{
    const uint64_t top = place_top(S, C, touched, r.n_touched, r.W, a.log_eps, a.keep, lane);
    r.branch = top ? 0xFFFFFFFFu - (uint32_t)top : PLACE_NONE;
    r.score = top ? __uint_as_float(dec_score_bits((uint32_t)(top >> 32))) : 0.0f;
    r.count = top ? C[r.branch] : 0;
    r.best = __uint_as_float(dec_score_bits((uint32_t)(place_readlane64(top, 0) >> 32)));
    wave_lds_sync();
    r.den = place_denominator(S, C, touched, r.n_touched, r.W, a.log_eps, r.best, lane);
}

// query q's results: lane r writes rank r, lane 0 the query's figures
__device__ __forceinline__ void place_store(const PlaceArgs& a, uint32_t q, uint32_t lane, const PlacePass& r)
{
    if (lane < a.keep) {
        const size_t o = (size_t)q * a.keep + lane;
        a.out_branch[o] = r.branch;
        a.out_score[o] = r.score;
        a.out_count[o] = r.count;
        a.out_lwr[o] = r.branch != PLACE_NONE ? exp10((double)r.score - (double)r.best) / r.den : 0.0;
    }
    if (lane == 0) { a.out_n_kmers[q] = r.W; a.out_n_found[q] = r.n_found; a.out_n_branches[q] = r.n_touched; }
}

template <int BITS, bool GLOBAL>
__global__ __launch_bounds__(64) void place_kernel(PlaceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char place_lds[];
    unsigned char* symtab = place_lds;
    const uint32_t lane = lane_id();
    for (uint32_t t = lane; t < 256; t += 64) symtab[t] = (unsigned char)place_symbol(a.sigma, t);
    float* S; uint32_t* C; uint32_t* touched;
    place_tables<GLOBAL>(a, place_lds, PLACE_SYMTAB_BYTES, lane, S, C, touched);
    wave_lds_sync();
    const uint32_t k = a.k, mask_k = (1u << k) - 1u;

    for (uint32_t q = blockIdx.x; q < a.n_queries; q += gridDim.x) {
        const uint64_t q0 = a.seq_off[q] - a.seq_base;
        const uint32_t n = (uint32_t)(a.seq_off[q + 1] - a.seq_base - q0);
        const unsigned char* seq = a.seqs + q0;
        PlacePass r;

        for (uint64_t base = 0; base + k <= n; base += 64) {
            // ---- phase one: the codes of windows base .. base + 63 out of bit planes, and their lookup
            const uint64_t p0 = base + lane, p1 = base + 64 + lane;
            const uint32_t s_lo = p0 < n ? symtab[seq[p0]] : 0xFFu;
            const uint32_t s_hi = (lane + 1 < k && p1 < n) ? symtab[seq[p1]] : 0xFFu;
            const uint32_t valid_bits = place_plane_at(ballot64(s_lo != 0xFFu), ballot64(s_hi != 0xFFu), lane);
            const bool win = (valid_bits & mask_k) == mask_k;            // (a window that runs past the end meets an invalid symbol there)
            const uint32_t code = place_window_code<BITS>(s_lo, s_hi, lane, k);
            uint64_t off = 0;
            uint32_t cnt = 0;
            bool found = false;
            if (win) found = place_lookup(a, code, off, cnt);
            r.W += (uint32_t)__popcll(ballot64(win));
            r.n_found += (uint32_t)__popcll(ballot64(found));
            // ---- phase two: the found windows in order
            place_walk(a, S, C, touched, r.n_touched, ballot64(cnt != 0), off, cnt, lane);
        }
        place_epilogue(a, S, C, touched, lane, r);
        place_store(a, q, lane, r);
    }
}

// ---- the extended modes (ipkgpu_db_place_opts): ambiguous symbols expanded, both strands --------------------------------------------
// place_ext_kernel is place_kernel's sibling.  Every phase the two have in common is one of the functions above, called by both: the
// table prologue, the window codes, the lookup, the ordered tile walk and the add it is made of, the top list, the denominator and
// the result stores.  The kernels themselves stay two, each with its own loops and nothing in a shared loop that asks which kernel
// runs it: place_kernel as an instantiation of this body with the additions compiled out took its SGPR spills from 3 to 196
// (place_kernel<2, true>; profiles/place_ext.txt, "tried and dropped"), while with the shared functions no instantiation of either
// kernel spills more or holds fewer wavefronts than it did with its own text (profiles/place_shared.txt).
//
//   tables     symtab[2][256]: the symbol code of a byte on the given strand and, complemented (3 - code), on the reverse strand;
//              0xFE: an ambiguous symbol (with ambiguity on), 0xFF: invalid.  masktab[2][32]: the resolution mask (bit c = symbol code c)
//              of an ambiguous LETTER, indexed by byte & 31 -- only a byte whose symtab entry is 0xFE is looked up, so the 32 entries
//              say what a 256-entry table would, and the block's LDS stays within 512 bytes of place_kernel's.  The reverse strand's
//              masks are the given strand's with bit c moved to bit 3 - c.
//   reverse    position p of rc(q) is byte n - 1 - p of the uploaded query through the complemented tables: no second copy, no host work
//   phase one  one more ballot plane, "ambiguous symbol": a lane's window is ambiguous iff its k valid-or-ambiguous bits are set and
//              exactly one of its k ambiguous bits is; ctz is the position, whose bits of the code are cleared
//   phase two  the found exact windows below the next ambiguous window are walked as place_kernel walks a tile; then the ambiguous
//              window: lane r looks resolution r up (R <= 20), the resolutions' entries are added one key after the other, 64 entries
//              at a time, into the per-window tables P (f64), c (u32) and their touched list; the touched branches get
//              y = (float)log10((P + (R - c) E) / R) into S and C and are cleared for the next window
//   tables P, c, touched-by-the-window: 16 bytes per branch in the workgroup's slice of a global block for BOTH variants (ambiguous
//              windows are the rare ones: a read with one N has k of them), so LDS holds what it held
//   strands    the wavefront runs the query twice, the epilogue of each pass leaves S and C zero; the given strand's results are
//              written after its pass and only "placed at all" and its best score wait in registers: the reverse strand's pass
//              writes over them iff it wins (it is placed and the given strand is not or scores less)
constexpr uint32_t PLACE_SYM_AMBIGUOUS = 0xFEu;
constexpr uint32_t PLACE_EXT_TAB_BYTES = 2 * 256 + 2 * 32 * 4;

// resolution mask of an ambiguous symbol (bit c = symbol code c), 0 for every other byte; either letter case
__device__ __forceinline__ uint32_t place_ambiguity_mask(uint32_t sigma, uint32_t byte)
{
    const uint32_t c = (byte >= 'a' && byte <= 'z') ? byte - 32u : byte;
    if (sigma == 4) {
        switch (c) {                                                     // A = 1, C = 2, G = 4, T = 8
        case 'R': return 5; case 'Y': return 10; case 'S': return 6; case 'W': return 9; case 'K': return 12; case 'M': return 3;
        case 'B': return 14; case 'D': return 13; case 'H': return 11; case 'V': return 7; case 'N': return 15;
        default: return 0;
        }
    }
    switch (c) {
    case 'B': return (1u << 3) | (1u << 7);                              // D, N
    case 'Z': return (1u << 4) | (1u << 8);                              // E, Q
    case 'J': return (1u << 13) | (1u << 14);                            // I, L
    case 'X': return (1u << 20) - 1u;
    default: return 0;
    }
}

struct PlaceExtArgs {
    uint32_t ambiguity, strands;
    double E;                                                            // 10^log_eps
    // [gridDim.x][b_pad] each, P and c zero on entry (and left zero)
    double* g_p; uint32_t* g_wc; uint32_t* g_wtouched;
    uint32_t* out_strand; uint32_t* out_n_ambiguous;                     // [n_queries]
};

template <int BITS, bool GLOBAL>
__global__ __launch_bounds__(64) void place_ext_kernel(PlaceArgs a, PlaceExtArgs x)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char place_lds[];
    unsigned char* symtab = place_lds;
    const uint32_t lane = lane_id();
    uint32_t* masktab = reinterpret_cast<uint32_t*>(place_lds + 512);
    for (uint32_t t = lane; t < 256; t += 64) {
        const uint32_t s = place_symbol(a.sigma, t);
        const uint32_t other = (x.ambiguity && place_ambiguity_mask(a.sigma, t)) ? PLACE_SYM_AMBIGUOUS : 0xFFu;
        symtab[t] = (unsigned char)(s != 0xFFu ? s : other);
        symtab[256 + t] = (unsigned char)(s != 0xFFu ? 3u - s : other);          // (read on the reverse strand: DNA only)
    }
    if (lane < 32) {
        const uint32_t m = x.ambiguity ? place_ambiguity_mask(a.sigma, 64u + lane) : 0u;
        masktab[lane] = m;
        masktab[32 + lane] = ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3);
    }
    float* S; uint32_t* C; uint32_t* touched;
    place_tables<GLOBAL>(a, place_lds, PLACE_EXT_TAB_BYTES, lane, S, C, touched);
    wave_lds_sync();
    const uint32_t k = a.k, mask_k = (1u << k) - 1u;

    for (uint32_t q = blockIdx.x; q < a.n_queries; q += gridDim.x) {
        const uint64_t q0 = a.seq_off[q] - a.seq_base;
        const uint32_t n = (uint32_t)(a.seq_off[q + 1] - a.seq_base - q0);
        const unsigned char* seq = a.seqs + q0;
        bool given_any = false;                                          // the given strand's pass: has it a placement, and its best score
        float given_best = 0.0f;

        for (uint32_t pass = 0; pass <= x.strands; ++pass) {
            const unsigned char* tab = symtab + pass * 256u;
            // byte p of the strand this pass places
            auto at = [&](uint64_t p) -> uint32_t { return pass ? seq[n - 1 - p] : seq[p]; };
            PlacePass r;

            for (uint64_t base = 0; base + k <= n; base += 64) {
                // ---- phase one: the codes of windows base .. base + 63 out of bit planes, and their lookup
                const uint64_t p0 = base + lane, p1 = base + 64 + lane;
                const uint32_t s_lo = p0 < n ? tab[at(p0)] : 0xFFu;
                const uint32_t s_hi = (lane + 1 < k && p1 < n) ? tab[at(p1)] : 0xFFu;
                const uint32_t valid_bits = place_plane_at(ballot64(s_lo != 0xFFu), ballot64(s_hi != 0xFFu), lane);
                bool win = (valid_bits & mask_k) == mask_k;                  // (a window that runs past the end meets an invalid symbol there)
                const uint32_t amb_bits = place_plane_at(ballot64(s_lo == PLACE_SYM_AMBIGUOUS), ballot64(s_hi == PLACE_SYM_AMBIGUOUS), lane) & mask_k;
                const bool amb = win && __popc(amb_bits) == 1;
                win = win && amb_bits == 0;
                uint32_t code = place_window_code<BITS>(s_lo, s_hi, lane, k);
                uint64_t off = 0;
                uint32_t cnt = 0;
                bool found = false;
                if (win) found = place_lookup(a, code, off, cnt);
                r.W += (uint32_t)__popcll(ballot64(win));
                r.n_found += (uint32_t)__popcll(ballot64(found));

                // ---- phase two: the windows in order, the exact ones as place_kernel walks them, an ambiguous one through P
                double* P = x.g_p + (size_t)blockIdx.x * a.b_pad;
                uint32_t* WC = x.g_wc + (size_t)blockIdx.x * a.b_pad;
                uint32_t* wtouched = x.g_wtouched + (size_t)blockIdx.x * a.b_pad;
                const uint32_t* masks = masktab + pass * 32u;
                // an ambiguous lane: the position's bits out of the code, and the symbol's resolutions
                uint32_t a_shift = 0, a_mask = 0;
                if (amb) {
                    const uint32_t pos = (uint32_t)__builtin_ctz(amb_bits);
                    a_shift = (uint32_t)BITS * (k - 1u - pos);
                    code &= ~(((1u << BITS) - 1u) << a_shift);
                    a_mask = masks[at(base + lane + pos) & 31u];
                }
                uint64_t todo = ballot64(cnt != 0), ambiguous = ballot64(amb);
                r.W += (uint32_t)__popcll(ambiguous);
                r.n_amb += (uint32_t)__popcll(ambiguous);
                while (ambiguous) {
                    const uint32_t w = (uint32_t)__builtin_ctzll(ambiguous);
                    ambiguous &= ambiguous - 1;
                    const uint64_t below = (1ull << w) - 1ull;
                    place_walk(a, S, C, touched, r.n_touched, todo & below, off, cnt, lane);   // the exact windows before it, in order
                    todo &= ~below;
                    // window w: resolution r (ascending symbol code) is lane r's
                    const uint32_t w_code = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)w);
                    const uint32_t w_shift = (uint32_t)__builtin_amdgcn_readlane((int)a_shift, (int)w);
                    const uint32_t w_mask = (uint32_t)__builtin_amdgcn_readlane((int)a_mask, (int)w);
                    const uint32_t R = (uint32_t)__popc(w_mask);
                    uint32_t sym = 0, at_r = 0;
                    for (uint32_t s = 0; s < (1u << BITS); ++s)
                        if ((w_mask >> s) & 1u) { if (at_r == lane) sym = s; ++at_r; }
                    uint64_t r_off = 0;
                    uint32_t r_cnt = 0;
                    bool r_found = false;
                    if (lane < R) r_found = place_lookup(a, w_code | (sym << w_shift), r_off, r_cnt);
                    r.n_found += ballot64(r_found) != 0 ? 1u : 0u;
                    uint64_t keys_todo = ballot64(r_cnt != 0);
                    uint32_t n_wt = 0;
                    while (keys_todo) {                                   // one resolution after the other: P's order is the definition's
                        const uint32_t res = (uint32_t)__builtin_ctzll(keys_todo);
                        keys_todo &= keys_todo - 1;
                        const uint64_t t_off = place_readlane64(r_off, res);
                        const uint32_t t_cnt = (uint32_t)__builtin_amdgcn_readlane((int)r_cnt, (int)res);
                        for (uint32_t t0 = 0; t0 < t_cnt; t0 += 64) {
                            bool fresh = false;
                            uint32_t b = 0;
                            if (t0 + lane < t_cnt) {
                                const uint2 e = a.entries[t_off + t0 + lane];
                                b = e.x;
                                P[b] = P[b] + exp10((double)__uint_as_float(e.y));
                                const uint32_t c = WC[b];
                                WC[b] = c + 1;
                                fresh = c == 0;
                            }
                            const uint64_t fm = ballot64(fresh);
                            if (fresh) wtouched[n_wt + mbcnt(fm)] = b;
                            n_wt += (uint32_t)__popcll(fm);
                            wave_lds_sync();
                        }
                    }
                    for (uint32_t i0 = 0; i0 < n_wt; i0 += 64) {          // the window's branches get y; its tables go back to zero
                        const bool v = i0 + lane < n_wt;
                        uint32_t b = 0;
                        float y = 0.0f;
                        if (v) {
                            b = wtouched[i0 + lane];
                            const double p = P[b] + (double)(R - WC[b]) * x.E;
                            y = (float)log10(p / (double)R);
                            P[b] = 0.0; WC[b] = 0;
                        }
                        place_add(S, C, touched, r.n_touched, v, b, y);
                    }
                }
                place_walk(a, S, C, touched, r.n_touched, todo, off, cnt, lane);
            }

            place_epilogue(a, S, C, touched, lane, r);
            // the reverse strand's results replace the given strand's iff it has a placement and the given strand has none or a
            // smaller best score (as floats)
            const bool any = (uint32_t)__builtin_amdgcn_readlane((int)r.branch, 0) != PLACE_NONE;
            if (pass == 0 || (any && (!given_any || r.best > given_best))) {
                place_store(a, q, lane, r);
                if (lane == 0) { x.out_strand[q] = pass; x.out_n_ambiguous[q] = r.n_amb; }
            }
            given_any = any; given_best = r.best;
        }
    }
}

}  // namespace ipkgpu
