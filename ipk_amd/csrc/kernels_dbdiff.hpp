// kernels_dbdiff.hpp -- compares two databases on the device: the rules of the reference's ipkdiff, check_phylo_kmers
// (tools/src/diff.cpp:210-295), over the key-major arrays instead of two hash maps.
//
//   for every k-mer of A: in B too?  then every entry of A against B's entry of the same branch (scores match iff
//   fabs(a - b) < eps, the difference in float, the comparison in double; :233), A's branches B does not score (:245-249), then
//   B's branches A does not score (:253-262); not in B: all of A's entries (:266-274); then the k-mers only B has (:279-293).
//
// Both key lists ascend, so the join is a binary search each way (db_diff_join_kernel).  One wavefront per k-mer then walks the two
// entry lists.  An entry is matched with the FIRST entry of the same branch in the other list (the reference builds a map per list,
// so there the last one wins; lists that name a branch once -- all this library writes -- give the same either way).  The order of
// a key's entries carries no meaning:
//   fast path     the two branch sequences are equal (the common case): a lockstep compare, linear.  Entries are compared position
//                 by position here; only lists that repeat a branch could tell that from "the first entry of the same branch".
//   general path  any order, any lengths: the other list's branches are staged in LDS, DB_DIFF_CHUNK at a time, and every lane
//                 looks for its entry's branch chunk after chunk -- quadratic in the list length, for lists that differ in order.
// Records are deterministic -- ascending key; inside a key A's entries in A's order, then B's unmatched ones in B's order -- so
// there are two passes: COUNT (differences per key, exact totals), a scan, and WRITE (the first max_records of them; only the
// keys that have any are walked again).
#pragma once
#include "../../include/ipkgpu.h"
#include "dcla_device.hpp"

namespace ipkgpu {

constexpr uint32_t DB_DIFF_CHUNK = 1024;                 // branches of the other list a wavefront keeps in LDS at a time
constexpr uint32_t DB_DIFF_NAN = 0x7FC00000u;            // "not scored" in a record

struct DbDiffView {
    const uint32_t* keys; const uint64_t* key_off; const uint2* entries; const uint32_t* positions; uint64_t n_keys;
};
struct DbDiffTotals {                                    // device side of ipkgpu_db_diff_counts
    unsigned long long keys_only_a, keys_only_b, entries_only_a, entries_only_b, scores_differ, positions_differ;
    uint32_t max_diff_bits, pad;                         // bits of the largest float |a - b| (non-negative floats order as their bits)
};

// lb[i] = the number of keys of Y below X's i-th key (its place in Y: the key is in Y iff Y.keys[lb[i]] equals it)
__global__ __launch_bounds__(256) void db_diff_join_kernel(const uint32_t* __restrict__ x_keys, uint64_t n_x, const uint32_t* __restrict__ y_keys,
                                                           uint64_t n_y, uint32_t* __restrict__ lb)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_x) return;
    const uint32_t key = x_keys[i];
    uint64_t lo = 0, hi = n_y;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (y_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    lb[i] = (uint32_t)lo;
}

__device__ __forceinline__ bool db_diff_scores_match(uint32_t a_bits, uint32_t b_bits, double eps, float& d)
{
    d = fabsf(__uint_as_float(a_bits) - __uint_as_float(b_bits));
    return eps == 0.0 ? a_bits == b_bits : (double)d < eps;
}

// Per lane: the first place in Y's list [y0, y0 + ny) whose branch is `br` (lanes with `valid`), ~0 if none.  Y's branches pass
// through the wavefront's LDS chunk; a list that fits one chunk stays there for the caller's next tile (`resident`).
__device__ __forceinline__ uint64_t db_diff_find_first(uint32_t br, bool valid, const uint2* __restrict__ y_entries, uint64_t y0, uint64_t ny,
                                                       uint32_t* chunk, bool& resident)
{
    const uint32_t lane = lane_id();
    uint64_t found = ~0ull;
    bool pending = valid;
    for (uint64_t cb = 0; cb < ny; cb += DB_DIFF_CHUNK) {
        const uint32_t cn = (uint32_t)min((uint64_t)DB_DIFF_CHUNK, ny - cb);
        if (!(resident && ny <= DB_DIFF_CHUNK)) {
            wave_lds_sync();                                              // (the reads of what the chunk held)
            for (uint32_t t = lane; t < cn; t += 64) chunk[t] = y_entries[y0 + cb + t].x;
            wave_lds_sync();
            resident = true;
        }
        if (ballot64(pending) == 0) break;
        for (uint32_t c = 0; c < cn; c += 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(chunk + c);   // the same address in every lane: a broadcast
            if (pending && v.x == br) { found = cb + c; pending = false; }
            if (pending && c + 1 < cn && v.y == br) { found = cb + c + 1; pending = false; }
            if (pending && c + 2 < cn && v.z == br) { found = cb + c + 2; pending = false; }
            if (pending && c + 3 < cn && v.w == br) { found = cb + c + 3; pending = false; }
            if (ballot64(pending) == 0) break;
        }
    }
    return found;
}

// a difference of this tile's lanes: counted, and in the WRITE pass stored at its place among the key's records
template <bool WRITE>
__device__ __forceinline__ void db_diff_emit(bool is_diff, uint32_t key, uint32_t branch, uint32_t a_bits, uint32_t b_bits, uint64_t out,
                                             uint32_t& n_rec, uint4* __restrict__ rec, uint64_t max_records)
{
    const uint64_t mask = ballot64(is_diff);
    if (WRITE) {
        const uint64_t at = out + n_rec + mbcnt(mask);
        if (is_diff && at < max_records) rec[at] = make_uint4(key, branch, a_bits, b_bits);
    }
    n_rec += (uint32_t)__popcll(mask);
}

// One wavefront per k-mer of A (keys [first, ...)): everything the reference's first loop finds (:218-275).
template <bool WRITE>
__global__ __launch_bounds__(256) void db_diff_keys_kernel(DbDiffView A, DbDiffView B, const uint32_t* __restrict__ lb_a, double eps,
                                                           uint32_t* __restrict__ cnt_a, DbDiffTotals* __restrict__ tot,
                                                           const uint64_t* __restrict__ scan_a, const uint64_t* __restrict__ scan_b,
                                                           uint4* __restrict__ rec, uint64_t max_records, uint64_t first)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[4][DB_DIFF_CHUNK];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t i = first + (uint64_t)blockIdx.x * 4 + wave;
    if (i >= A.n_keys) return;
    const uint32_t lane = lane_id();
    uint32_t* chunk = lds[wave];
    const uint32_t key = A.keys[i];
    const uint64_t lb = lb_a[i];
    const bool in_b = lb < B.n_keys && B.keys[lb] == key;
    const uint64_t a0 = A.key_off[i], na = A.key_off[i + 1] - a0;
    uint64_t out = 0;
    if (WRITE) {
        if (scan_a[i + 1] == scan_a[i]) return;                          // no difference in this key
        out = scan_a[i] + scan_b[lb];                                     // (the records of B's own keys below this one come first)
        if (out >= max_records) return;
    }
    uint32_t n_rec = 0, n_only_a = 0, n_only_b = 0, n_sdiff = 0, n_pdiff = 0;
    float dmax = 0.0f;
    if (!in_b) {
        for (uint64_t t0 = 0; t0 < na; t0 += 64) {
            const bool valid = t0 + lane < na;
            const uint2 ea = valid ? A.entries[a0 + t0 + lane] : make_uint2(0, 0);
            db_diff_emit<WRITE>(valid, key, ea.x, ea.y, DB_DIFF_NAN, out, n_rec, rec, max_records);
        }
        n_only_a = n_rec;
    } else {
        const uint64_t b0 = B.key_off[lb], nb = B.key_off[lb + 1] - b0;
        const bool both_pos = A.positions && B.positions;
        bool fast = !WRITE && na == nb;                                   // (the WRITE pass walks only keys with differences: one path there)
        if (fast) {
            uint32_t f_sdiff = 0, f_pdiff = 0;
            float f_dmax = 0.0f;
            for (uint64_t t0 = 0; t0 < na; t0 += 64) {
                const bool valid = t0 + lane < na;
                const uint2 ea = valid ? A.entries[a0 + t0 + lane] : make_uint2(0, 0);
                const uint2 eb = valid ? B.entries[b0 + t0 + lane] : make_uint2(0, 0);
                if (ballot64(ea.x != eb.x) != 0) { fast = false; break; }
                float d = 0.0f;
                const bool same = !valid || db_diff_scores_match(ea.y, eb.y, eps, d);
                f_dmax = fmaxf(f_dmax, d);
                f_sdiff += (uint32_t)__popcll(ballot64(!same));
                if (both_pos) {
                    const bool pd = valid && same && A.positions[a0 + t0 + lane] != B.positions[b0 + t0 + lane];
                    f_pdiff += (uint32_t)__popcll(ballot64(pd));
                }
            }
            if (fast) { n_sdiff = f_sdiff; n_pdiff = f_pdiff; dmax = f_dmax; n_rec = f_sdiff; }
        }
        if (!fast) {
            bool resident = false;
            for (uint64_t t0 = 0; t0 < na; t0 += 64) {                    // A's entries in A's order
                const bool valid = t0 + lane < na;
                const uint2 ea = valid ? A.entries[a0 + t0 + lane] : make_uint2(0, 0);
                const uint64_t at = db_diff_find_first(ea.x, valid, B.entries, b0, nb, chunk, resident);
                const bool scored = valid && at != ~0ull;
                const uint2 eb = scored ? B.entries[b0 + at] : make_uint2(0, DB_DIFF_NAN);
                float d = 0.0f;
                const bool same = scored && db_diff_scores_match(ea.y, eb.y, eps, d);
                dmax = fmaxf(dmax, d);
                n_only_a += (uint32_t)__popcll(ballot64(valid && !scored));
                n_sdiff += (uint32_t)__popcll(ballot64(scored && !same));
                if (both_pos) {
                    const bool pd = same && A.positions[a0 + t0 + lane] != B.positions[b0 + at];
                    n_pdiff += (uint32_t)__popcll(ballot64(pd));
                }
                db_diff_emit<WRITE>(valid && !same, key, ea.x, ea.y, eb.y, out, n_rec, rec, max_records);
            }
            resident = false;
            for (uint64_t t0 = 0; t0 < nb; t0 += 64) {                    // then B's entries A does not score, in B's order
                const bool valid = t0 + lane < nb;
                const uint2 eb = valid ? B.entries[b0 + t0 + lane] : make_uint2(0, 0);
                const uint64_t at = db_diff_find_first(eb.x, valid, A.entries, a0, na, chunk, resident);
                const bool only_b = valid && at == ~0ull;
                n_only_b += (uint32_t)__popcll(ballot64(only_b));
                db_diff_emit<WRITE>(only_b, key, eb.x, DB_DIFF_NAN, eb.y, out, n_rec, rec, max_records);
            }
        }
    }
    if (WRITE) return;
    for (int s = 32; s > 0; s >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, s, 64));
    if (lane == 0) {
        cnt_a[i] = n_rec;
        if (!in_b) atomicAdd(&tot->keys_only_a, 1ull);
        if (n_only_a) atomicAdd(&tot->entries_only_a, (unsigned long long)n_only_a);
        if (n_only_b) atomicAdd(&tot->entries_only_b, (unsigned long long)n_only_b);
        if (n_sdiff) atomicAdd(&tot->scores_differ, (unsigned long long)n_sdiff);
        if (n_pdiff) atomicAdd(&tot->positions_differ, (unsigned long long)n_pdiff);
        if (dmax > 0.0f) atomicMax(&tot->max_diff_bits, __float_as_uint(dmax));
    }
}

// One wavefront per k-mer of B: the k-mers A does not have, all their entries (the reference's second loop, :279-293).
template <bool WRITE>
__global__ __launch_bounds__(256) void db_diff_only_b_kernel(DbDiffView B, const uint32_t* __restrict__ a_keys, uint64_t n_a,
                                                             const uint32_t* __restrict__ lb_b, uint32_t* __restrict__ cnt_b,
                                                             DbDiffTotals* __restrict__ tot, const uint64_t* __restrict__ scan_a,
                                                             const uint64_t* __restrict__ scan_b, uint4* __restrict__ rec, uint64_t max_records,
                                                             uint64_t first)
{
    const uint64_t j = first + (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (j >= B.n_keys) return;
    const uint32_t lane = lane_id();
    const uint32_t key = B.keys[j];
    const uint64_t lb = lb_b[j];
    const bool in_a = lb < n_a && a_keys[lb] == key;
    const uint64_t b0 = B.key_off[j], nb = in_a ? 0 : B.key_off[j + 1] - b0;
    if (!WRITE) {
        if (lane == 0) {
            cnt_b[j] = (uint32_t)nb;
            if (!in_a) { atomicAdd(&tot->keys_only_b, 1ull); if (nb) atomicAdd(&tot->entries_only_b, (unsigned long long)nb); }
        }
        return;
    }
    const uint64_t out = scan_b[j] + scan_a[lb];                          // (A's keys below this one, with all their records, come first)
    if (nb == 0 || out >= max_records) return;
    uint32_t n_rec = 0;
    for (uint64_t t0 = 0; t0 < nb; t0 += 64) {
        const bool valid = t0 + lane < nb;
        const uint2 eb = valid ? B.entries[b0 + t0 + lane] : make_uint2(0, 0);
        db_diff_emit<true>(valid, key, eb.x, DB_DIFF_NAN, eb.y, out, n_rec, rec, max_records);
    }
}

}  // namespace ipkgpu
