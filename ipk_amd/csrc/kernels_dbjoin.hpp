// kernels_dbjoin.hpp -- the join of N databases whose key sets may overlap (ipkgpu_db_join in include/ipkgpu.h; host side: db_join.hpp).
//
// A RUN is one source's record of one key.  Behind the union's sort of (key << 32 | concatenated key index) the runs of a key stand
// side by side in source order, so the CONCATENATED LAYOUT -- every run's entries in sorted run order -- holds each key's joined list
// in the order the definition asks for.
//   db_join_runs_kernel         per sorted position j: head flag (first run of its key), entry count, source, start in the source
//   db_join_keys_kernel         per head: the key and the list's start in the concatenated layout; counts the keys with several runs
//   db_union_entries16_kernel   (kernels_dbunion.hpp) copies the concatenated layout by entry ranges of 1024 per workgroup; its "keys"
//                               are the runs -- a lane's search is over (sorted position, source run), the offsets those of the runs
//   db_join_branch_owner_kernel, db_join_branch_shared_kernel    can any branch lie in two sources?  (a hashed branch table)
//   db_join_dups_wave_kernel    lists of up to 64 entries: a wavefront per key, lane against lane
//   db_join_dups_lds_kernel     lists of 65 .. 4096 entries: (branch, index) sorted in LDS, one walker per run of equal branches
//   db_join_sortpair_kernel, db_join_dups_sorted_kernel          longer lists: a sorted (key, branch) -> index pass in global memory
//   db_join_compact_kernel, db_join_offsets_kernel               the kept entries, positions and key offsets of the result
// Every output position comes from the sort or from an exclusive scan, none from an atomic.  The atomics here fill a work list whose
// order changes no result (each listed key is resolved on its own), count, and take minima and maxima.
#pragma once
#include "kernels_dbunion.hpp"

namespace ipkgpu {

constexpr uint32_t DB_JOIN_BRANCH_SLOTS = 1u << 18;   // slots of the branch table: branch & (slots - 1)
constexpr uint32_t DB_JOIN_WAVE_LIST = 64;            // the longest list a wavefront resolves in registers
constexpr uint32_t DB_JOIN_LDS_LIST = 4096;           // the longest list a workgroup sorts in LDS (32 KiB of 64-bit words)
// words of the call's counter block
constexpr uint32_t DB_JOIN_C_SHARED = 0, DB_JOIN_C_MAYBE = 1, DB_JOIN_C_LONG = 2, DB_JOIN_C_MAXLEN = 3, DB_JOIN_C_FIRST_DROP = 4 /* 64-bit, words 4..5 */,
                   DB_JOIN_C_LOCATE = 8 /* key, branch, first source, second source */, DB_JOIN_C_WORDS = 16;

__global__ __launch_bounds__(256) void db_join_runs_kernel(const DbUnionSrc* __restrict__ table, uint32_t n_srcs,
                                                           const unsigned long long* __restrict__ sorted, uint64_t n,
                                                           uint32_t* __restrict__ head, uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ src_of, uint64_t* __restrict__ start_of)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const unsigned long long sk = sorted[j];
    const uint64_t c = (uint32_t)sk;
    const uint32_t s = db_union_source_of(table, n_srcs, c);
    const uint64_t i = c - table[s].first;
    const global_u64_ptr_t off = (global_u64_ptr_t)table[s].key_off;
    const uint64_t a = off[i], b = off[i + 1];
    head[j] = (j == 0 || (uint32_t)(sorted[j - 1] >> 32) != (uint32_t)(sk >> 32)) ? 1u : 0u;
    counts[j] = (uint32_t)(b - a);
    src_of[j] = s;
    start_of[j] = a;
}

// hpos = the exclusive scan of head (hpos[j] = the J-key index of a head j), run_off = the exclusive scan of counts.
// cat_off has n_jkeys + 1 elements; the thread of the last run writes the last one.
__global__ __launch_bounds__(256) void db_join_keys_kernel(const unsigned long long* __restrict__ sorted, uint64_t n, const uint32_t* __restrict__ head,
                                                           const uint64_t* __restrict__ hpos, const uint64_t* __restrict__ run_off,
                                                           uint32_t* __restrict__ keys, uint64_t* __restrict__ cat_off, uint32_t* __restrict__ counters)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool shared = false;
    if (j < n) {
        if (head[j]) {
            const uint64_t jk = hpos[j];
            keys[jk] = (uint32_t)(sorted[j] >> 32);
            cat_off[jk] = run_off[j];
            shared = j + 1 < n && !head[j + 1];
        }
        if (j == n - 1) cat_off[hpos[n]] = run_off[n];
    }
    const unsigned long long m = __ballot(shared);
    if (shared && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(&counters[DB_JOIN_C_SHARED], (uint32_t)__popcll(m));
}

// the source of concatenated ENTRY g: the last s with efirst[s] <= g
__device__ __forceinline__ uint32_t db_join_source_of_entry(const uint64_t* __restrict__ efirst, uint32_t n_srcs, uint64_t g)
{
    uint32_t lo = 0, hi = n_srcs - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (efirst[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// lo_src / hi_src[slot]: the smallest and the largest source that holds a branch of the slot (0xFFFFFFFF / 0 before the launch)
__global__ __launch_bounds__(256) void db_join_branch_owner_kernel(const DbUnionSrc* __restrict__ table, const uint64_t* __restrict__ efirst, uint32_t n_srcs,
                                                                   uint64_t n_entries, uint32_t* __restrict__ lo_src, uint32_t* __restrict__ hi_src)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_entries) return;
    const uint32_t s = db_join_source_of_entry(efirst, n_srcs, g);
    const uint32_t branch = (uint32_t)((global_u64_ptr_t)table[s].entries)[g - efirst[s]];
    const uint32_t slot = branch & (DB_JOIN_BRANCH_SLOTS - 1);
    // (a tree has few branches and a source many entries of each: nearly every lane finds its source noted already, and an atomic
    //  per entry on so few addresses took 40 - 170 ms where the whole join takes 3 -- profiles/db_join_probe.txt; a stale value
    //  read here only costs an atomic that changes nothing)
    if (lo_src[slot] > s) atomicMin(&lo_src[slot], s);
    if (hi_src[slot] < s) atomicMax(&hi_src[slot], s);
}

__global__ __launch_bounds__(256) void db_join_branch_shared_kernel(const uint32_t* __restrict__ lo_src, const uint32_t* __restrict__ hi_src,
                                                                    uint32_t* __restrict__ counters)
{
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= DB_JOIN_BRANCH_SLOTS) return;
    const uint32_t lo = lo_src[slot];
    if (lo != 0xFFFFFFFFu && lo != hi_src[slot]) counters[DB_JOIN_C_MAYBE] = 1u;      // (every writer stores the same word)
}

// `put`: a later occurrence replaces the kept score only if it is strictly greater as a float
__device__ __forceinline__ bool db_join_replaces(uint32_t later_bits, uint32_t kept_bits) { return __uint_as_float(later_bits) > __uint_as_float(kept_bits); }

// A wavefront per J-key (first + 4 * block + wave).  A list of up to 64 entries: lane p holds entry p; for q = 0 .. len - 1 entry q is
// broadcast: an equal branch at q < p makes p a later occurrence (dropped), one at q > p may replace p's score -- in ascending q, which
// is the order of the walk.  keep[e] = 1 for first occurrences, whose slot then carries the winner's score and position.
// A longer list is appended to long_list (its order changes nothing: each listed key is resolved on its own).
template <bool POS>
__global__ __launch_bounds__(256) void db_join_dups_wave_kernel(const uint64_t* __restrict__ cat_off, uint64_t n_jkeys, uint64_t first,
                                                                uint2* __restrict__ cat, uint32_t* __restrict__ cat_pos, uint32_t* __restrict__ keep,
                                                                uint32_t* __restrict__ long_list, uint32_t* __restrict__ counters)
{
    const uint64_t jk = first + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jk >= n_jkeys) return;                                       // (the whole wavefront leaves)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t base = cat_off[jk], len64 = cat_off[jk + 1] - base;
    if (len64 > DB_JOIN_WAVE_LIST) {
        if (lane == 0) {
            long_list[atomicAdd(&counters[DB_JOIN_C_LONG], 1u)] = (uint32_t)jk;
            atomicMax(&counters[DB_JOIN_C_MAXLEN], (uint32_t)min(len64, (uint64_t)0xFFFFFFFFull));
        }
        return;
    }
    const uint32_t len = (uint32_t)len64;
    uint2 mine = make_uint2(0xFFFFFFFFu, 0u);
    uint32_t mypos = 0;
    if (lane < len) {
        mine = cat[base + lane];
        if (POS) mypos = cat_pos[base + lane];
    }
    const uint32_t score0 = mine.y;
    uint32_t score = mine.y, pos = mypos;
    bool later = false;
    for (uint32_t q = 0; q < len; ++q) {
        const uint32_t bq = __shfl(mine.x, q), sq = __shfl(score0, q);
        const uint32_t pq = POS ? __shfl(mypos, q) : 0u;
        if (lane < len && bq == mine.x) {
            if (q < lane) later = true;
            else if (q > lane && db_join_replaces(sq, score)) { score = sq; pos = pq; }
        }
    }
    if (lane < len) {
        keep[base + lane] = later ? 0u : 1u;
        if (!later && score != score0) {
            cat[base + lane].y = score;
            if (POS) cat_pos[base + lane] = pos;
        }
    }
}

// the walker of one run of equal branches whose members' list indices ascend: idx_at(u) for u = 0 .. while same_run(u)
// (shared by the LDS and the sorted pass; first = the run's first member's concatenated index)
template <bool POS>
__device__ __forceinline__ void db_join_settle(uint2* __restrict__ cat, uint32_t* __restrict__ cat_pos, uint64_t first_e, uint32_t score0, uint32_t score,
                                               uint32_t pos)
{
    if (score != score0) {
        cat[first_e].y = score;
        if (POS) cat_pos[first_e] = pos;
    }
}

// A workgroup per listed key with 65 .. 4096 entries: (branch << 32 | index in the list) sorted in LDS (bitonic, padded with all-ones to a
// power of two); a thread at the head of a run of equal branches -- the members' indices ascend -- keeps the first member and walks the
// rest.  A walker reads and writes the scores of its own run alone.
template <bool POS>
__global__ __launch_bounds__(256) void db_join_dups_lds_kernel(const uint64_t* __restrict__ cat_off, const uint32_t* __restrict__ long_list,
                                                               uint2* __restrict__ cat, uint32_t* __restrict__ cat_pos, uint32_t* __restrict__ keep)
{
    __shared__ unsigned long long a[DB_JOIN_LDS_LIST];
    const uint64_t jk = long_list[blockIdx.x];
    const uint64_t base = cat_off[jk], len64 = cat_off[jk + 1] - base;
    if (len64 > DB_JOIN_LDS_LIST) return;                            // (the sorted pass takes it; uniform in the workgroup)
    const uint32_t len = (uint32_t)len64;
    uint32_t padded = DB_JOIN_WAVE_LIST * 2;
    while (padded < len) padded <<= 1;
    for (uint32_t i = threadIdx.x; i < padded; i += 256)
        a[i] = i < len ? ((unsigned long long)cat[base + i].x << 32) | i : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= padded; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < padded; i += 256) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const unsigned long long u = a[i], v = a[x];
                    if ((u > v) == ((i & k) == 0)) { a[i] = v; a[x] = u; }
                }
            }
            __syncthreads();
        }
    for (uint32_t t = threadIdx.x; t < len; t += 256) {
        const unsigned long long w = a[t];
        const uint32_t branch = (uint32_t)(w >> 32);
        if (t > 0 && (uint32_t)(a[t - 1] >> 32) == branch) continue;
        const uint64_t first_e = base + (uint32_t)w;
        const uint32_t score0 = cat[first_e].y;
        uint32_t score = score0, pos = 0;
        keep[first_e] = 1u;
        for (uint32_t u = t + 1; u < len && (uint32_t)(a[u] >> 32) == branch; ++u) {
            const uint64_t e = base + (uint32_t)a[u];
            keep[e] = 0u;
            const uint32_t sq = cat[e].y;
            if (db_join_replaces(sq, score)) { score = sq; if (POS) pos = cat_pos[e]; }
        }
        db_join_settle<POS>(cat, cat_pos, first_e, score0, score, pos);
    }
}

// The sorted pass, for lists beyond LDS.  Per concatenated entry e (entry ranges, as the copy): its J-key j; the sort key
// (j << 32 | branch) where j's list is longer than DB_JOIN_LDS_LIST, else all-ones (sorted behind every real key and passed over);
// the value is e itself.  The radix sort is stable, so within equal (key, branch) the values ascend.
__global__ __launch_bounds__(256) void db_join_sortpair_kernel(const uint64_t* __restrict__ cat_off, uint64_t n_jkeys, uint64_t n_entries,
                                                               const uint2* __restrict__ cat, unsigned long long* __restrict__ pair_key,
                                                               unsigned long long* __restrict__ pair_val)
{
    const uint64_t e0 = (uint64_t)blockIdx.x * DB_UNPACK_TILE;
    if (e0 >= n_entries) return;
    const uint64_t e_last = min(e0 + DB_UNPACK_TILE, n_entries) - 1;
    const uint64_t j_lo = db_key_of_entry(cat_off, 0, n_jkeys - 1, e0);
    const uint64_t j_hi = db_key_of_entry(cat_off, j_lo, n_jkeys - 1, e_last);
#pragma unroll
    for (uint32_t r = 0; r < DB_UNPACK_PER_THREAD; ++r) {
        const uint64_t e = e0 + r * 256 + threadIdx.x;
        if (e <= e_last) {
            const uint64_t j = db_key_of_entry(cat_off, j_lo, j_hi, e);
            const bool far = cat_off[j + 1] - cat_off[j] > DB_JOIN_LDS_LIST;
            pair_key[e] = far ? ((unsigned long long)j << 32) | cat[e].x : ~0ull;
            pair_val[e] = e;
        }
    }
}

// per sorted position t at the head of a run of equal real keys: the first member is kept, the rest walked
template <bool POS>
__global__ __launch_bounds__(256) void db_join_dups_sorted_kernel(const unsigned long long* __restrict__ pair_key, const unsigned long long* __restrict__ pair_val,
                                                                  uint64_t n_entries, uint2* __restrict__ cat, uint32_t* __restrict__ cat_pos,
                                                                  uint32_t* __restrict__ keep)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_entries) return;
    const unsigned long long w = pair_key[t];
    if (w == ~0ull || (t > 0 && pair_key[t - 1] == w)) return;
    const uint64_t first_e = pair_val[t];
    const uint32_t score0 = cat[first_e].y;
    uint32_t score = score0, pos = 0;
    keep[first_e] = 1u;
    for (uint64_t u = t + 1; u < n_entries && pair_key[u] == w; ++u) {
        const uint64_t e = pair_val[u];
        keep[e] = 0u;
        const uint32_t sq = cat[e].y;
        if (db_join_replaces(sq, score)) { score = sq; if (POS) pos = cat_pos[e]; }
    }
    db_join_settle<POS>(cat, cat_pos, first_e, score0, score, pos);
}

// kept_at = the exclusive scan of keep (n_entries + 1 values).  A kept entry moves to kept_at[e]; the smallest dropped e is recorded
// for the caller who asked to be refused ("join_route" = 2).
template <bool POS>
__global__ __launch_bounds__(256) void db_join_compact_kernel(const uint2* __restrict__ cat, const uint32_t* __restrict__ cat_pos, const uint32_t* __restrict__ keep,
                                                              const uint64_t* __restrict__ kept_at, uint64_t n_entries, uint2* __restrict__ entries,
                                                              uint32_t* __restrict__ positions, uint32_t* __restrict__ counters)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    if (keep[e]) {
        const uint64_t at = kept_at[e];
        entries[at] = cat[e];
        if (POS) positions[at] = cat_pos[e];
    } else {
        atomicMin(reinterpret_cast<unsigned long long*>(counters + DB_JOIN_C_FIRST_DROP), (unsigned long long)e);
    }
}

__global__ __launch_bounds__(256) void db_join_offsets_kernel(const uint64_t* __restrict__ cat_off, const uint64_t* __restrict__ kept_at, uint64_t n_jkeys,
                                                              uint64_t* __restrict__ key_off)
{
    const uint64_t jk = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (jk <= n_jkeys) key_off[jk] = kept_at[cat_off[jk]];
}

// One thread: the dropped entry e of the concatenated layout -> its key, its branch, the source of the branch's first occurrence in the
// key's list and e's own source (the message of "join_route" = 2).  run_off: the runs' offsets (n_runs + 1).
__global__ void db_join_locate_kernel(const unsigned long long* __restrict__ sorted, const uint64_t* __restrict__ run_off, const uint32_t* __restrict__ src_of,
                                      const uint32_t* __restrict__ head, uint64_t n_runs, const uint2* __restrict__ cat, uint64_t e,
                                      uint32_t* __restrict__ counters)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t run = db_key_of_entry(run_off, 0, n_runs - 1, e);
    uint64_t h = run;
    while (!head[h]) --h;                                            // (head[0] = 1)
    const uint32_t branch = cat[e].x;
    uint64_t p = run_off[h];
    while (p < e && cat[p].x != branch) ++p;
    counters[DB_JOIN_C_LOCATE + 0] = (uint32_t)(sorted[run] >> 32);
    counters[DB_JOIN_C_LOCATE + 1] = branch;
    counters[DB_JOIN_C_LOCATE + 2] = src_of[db_key_of_entry(run_off, h, run, p)];
    counters[DB_JOIN_C_LOCATE + 3] = src_of[run];
}

}  // namespace ipkgpu
