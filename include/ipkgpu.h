/*
 * ipkgpu.h -- C ABI of the MI355X phylo-k-mer scoring engine (libipkgpu.so).
 *
 * Drop-in boundary for ONE path of phylo42/IPK: what db_builder::explore_kmers /
 * explore_group consume from the scoring layer (citations relative to the IPK tree):
 *
 *   ipk/src/db_builder.cpp:576-627   explore_kmers   (the group loop)
 *   ipk/src/db_builder.cpp:629-698   explore_group   (windows -> DCLA -> put -> DB insert)
 *   ipk/src/pk_compute.cpp:28-119    DCLA::run / DC  (divide-and-conquer with look-ahead)
 *   ipk/src/window.cpp:16-27,69-72   matrix::preprocess / range_max_sum
 *   ipk/src/branch_group.cpp:88-107  put / kmer_batch
 *
 * IPK itself has no FFI; INTEGRATION.md shows the ~30-line patch to db_builder.cpp that
 * binds these entry points.  Plain pointers and sizes only; no exceptions cross the ABI:
 * every call returns an int status (0 = ok) and ipkgpu_last_error() gives the message.
 *
 * Threading: one host thread per context; calls on a context are serialised by the caller.
 * One context drives one GPU (one process per GPU; multi-GPU sharding is by branch group).
 *
 * Streams: a context works on its OWN non-blocking HIP stream.  Device buffers handed in by raw
 * pointer (logp_dev, counts_dev, entries_dev ...) must be complete before the call: synchronise the
 * stream that produced them (hipStreamSynchronize / hipEventSynchronize) first.  Every call returns
 * after its device work has finished, so results may be read from any stream afterwards.
 *
 * Not supported (IPKGPU_ERR_INVALID, never a silent fallback): in one call over the whole key space DNA k > 14, amino
 * acids k > 6 (the reference's command line advertises k <= 31, ipk.py:116; its key type here is u32: DNA k <= 16).
 * DNA k = 15, 16 are built in key-range passes instead (ipkgpu_score_groups_keyrange_device: the k-mers of one class of
 * leading symbols per call, one owner; each pass' shard written as a file of its own, the files merged by
 * ipkgpu_db_merge_files) -- not on several ranks (owners inside a key range would need a slot mapping of their own), not
 * through the per-branch result or the positions path, not for amino acids k = 7 (35-bit keys).
 * DNA k >= 13: the kernels that score a window with long half lists (its 6- to 8-symbol prefixes or suffixes above their
 * threshold) keep a list of at most 6144 entries in LDS.  By default a call in which one window's half list is longer fails
 * (every scoring entry point, ipkgpu_score_groups_positions included); near-flat columns get there, and among the hundreds
 * of thousands of windows of an alignment of ordinary length at k = 15, 16 a few do.  With the option "slice_long_lists" = 1
 * such a window is scored one class of the list's leading symbols at a time (a 7-symbol half in 4 slices, an 8-symbol half
 * in 16, each at most 4^6 entries), the same k-mers and score bits as the reference's, and no call fails for its lists.
 * The reference's on-disk mode (db_builder.cpp:673-681, branch_group.cpp:109-185: per-group files
 * merged later) is ipkgpu_parts_spill / ipkgpu_spill_merge below: one GPU, no positions, no key-range passes.
 */
#ifndef IPKGPU_H
#define IPKGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ipkgpu_ctx ipkgpu_ctx;
typedef struct ipkgpu_result ipkgpu_result;
typedef struct ipkgpu_parts ipkgpu_parts;
typedef struct ipkgpu_db ipkgpu_db;

enum {
    IPKGPU_OK = 0,
    IPKGPU_ERR_INVALID = 1,     /* bad argument (sigma/k unsupported, sites < k, null pointer ...) */
    IPKGPU_ERR_HIP = 2,         /* a HIP runtime call failed */
    IPKGPU_ERR_NOMEM = 3,       /* device or host allocation failed */
    IPKGPU_ERR_NODEVICE = 4     /* no usable GPU: the engine has NO CPU fallback */
};

/* ipkgpu_result_time_ms selectors */
enum {
    IPKGPU_T_TOTAL = 0,         /* whole call on the device stream (first event -> last event) */
    IPKGPU_T_PREFIX = 1,        /* prefix-of-column-maxima kernel  (matrix::preprocess) */
    IPKGPU_T_SCORE = 2,         /* scoring + max-reduce kernels (DCLA + put), summed over batches */
    IPKGPU_T_COMPACT = 3,       /* table -> sorted (key, score) compaction kernels */
    IPKGPU_T_SCORE_LAUNCHES = 4,/* number of scoring passes (batches of groups) the sums cover */
    IPKGPU_T_SCORE_MAIN = 5,    /* the dominant kernel alone: list building + pair emission (score_stream_kernel /
                                   score_tiles_kernel), summed over batches */
    IPKGPU_T_SCORE_REDUCE = 6,  /* per-bucket LDS max-reduce (reduce_buckets_kernel / reduce_ranges_kernel) */
    IPKGPU_T_XP_COUNT = 7,      /* exact-partition variant: the count pass alone (parts only) */
    IPKGPU_T_XP_WRITE = 8,      /* exact-partition variant: the write pass alone (parts only) */
    IPKGPU_T_KM_WRITE = 9       /* key-major writer kernel alone (km_write_kernel / km_write_c_kernel; parts only) */
};

/* ---- context ------------------------------------------------------------------------- */

/* Creates an engine on HIP device `device_id`.  Fails with IPKGPU_ERR_NODEVICE when no GPU
 * is present.  (Replaces nothing in IPK; owns the stream and workspaces.) */
int ipkgpu_create(int device_id, ipkgpu_ctx** ctx);
void ipkgpu_destroy(ipkgpu_ctx* ctx);

/* Message of the last failing call on this context ("" if none); owned by the context.
 * ipkgpu_last_error(NULL) returns the message of the last failed ipkgpu_create. */
const char* ipkgpu_last_error(const ipkgpu_ctx* ctx);
/* Name of the dominant kernel of the context's last scoring call ("score_quad_kernel", "score_stream_kernel",
 * "score_xp_kernel", "score_tiles_kernel"): what IPKGPU_T_SCORE_MAIN timed. */
const char* ipkgpu_last_main_kernel(const ipkgpu_ctx* ctx);
/* 1 if the last scoring batch left its per-group tables in the compressed form (occupancy bits + rank + score codes: AA k=6,
 * DNA k=11, 12), 0 for dense tables: tells the benchmark which reduce / key-major writer kernels ran. */
int ipkgpu_last_tables_compressed(const ipkgpu_ctx* ctx);

/* Diagnostics: -1 in the shipped build; in an IPK_EXEC_ASSERT build (ipk_amd/build.py, variant "execassert") the number of
 * times one of the kernels' exec-writing inline-asm helpers was entered with a partial exec mask (must be 0). */
int64_t ipkgpu_debug_exec_violations(ipkgpu_ctx* ctx);

/* Options: "workspace_bytes" (max bytes of per-group score tables resident at once; groups are
 * processed in batches that fit); "variant" (0 = auto: LDS max-reduce fed by the chunked pair pool, or by
 * the exact-partition passes for AA k=6; 1 = global-atomic max-reduce; 2 = force the chunked pool;
 * 3 = force the exact partition with dense tables; 4 = exact partition ending in compressed tables (occupancy
 * bits + rank + scores instead of dense per-group tables; what auto picks for AA k=6); 5 = ask for the quad kernel, 6 / 7 = force
 * the compressed / the dense table form behind the chunked pool); "debug_flags" (bits 0-4: timing experiments inside the scoring
 * kernels, results wrong; 5: no first chunks by position; 6: every host wait of a call kept -- no device-side counts, no
 * allocations from estimates, no key list inside the scoring call; 7 / 8: the quad kernel's workgroups never / always draw
 * their tiles; 9 / 10: the dense key-major writer with tile-by-tile / with line-cut stores whatever the group count; 11: 128-KB
 * table slices reduced by the workgroup-per-slice kernel instead of the persistent one; 12 / 13: the compressed key-major writer
 * per key block / per run of key blocks whatever the group count; 14: the line-cut writer's stores all plain, none non-temporal;
 * 15: the dense table slices of the 6-byte-pair reduce (DNA k = 8..10) leave by plain stores, not non-temporal ones),
 * "debug_pool_chunks", "debug_pool_limit_bytes",
 * "debug_wg_chunks2", "debug_rounds", "debug_kmc_pass" (groups per pass of the compressed key-major writer),
 * "debug_prefix_mats" (matrices per workgroup of the prefix-sum kernel: 1, 2, 4, 8; 0 = by the matrix count) (diagnostics and tests only);
 * "slice_long_lists" (0 / 1, default 0; DNA k >= 13 only: 1 = a window whose half list exceeds the 6144 entries the big-list
 * kernels keep in LDS is scored in slices instead of failing the call -- see "Not supported" above; applies to every scoring entry
 * point: per-branch result, key-major with and without owners or positions, key-range passes, ipkgpu_score_groups_positions, the
 * pieces of the on-disk build; results of calls without such a window do not change);
 * "device_budget_bytes" (ipkgpu_mem_stats below; 0 = none); "db_load_chunk_bytes" (bytes of each of the two pinned buffers a file passes
 * through in ipkgpu_db_load; 0 = the default, 64 MiB, also the most); "db_load_window_bytes" (bytes of the device window of
 * ipkgpu_db_load_wanted and ipkgpu_db_load_key_range; 0 = the default, 256 MiB -- in ipkgpu_db_diff_files and ipkgpu_db_join_files a sixteenth of what the budget leaves); "place_batch_queries" (queries per batch of ipkgpu_db_place; 0 = automatic);
 * "place_lds_branches" (0..4096: the branch count up to which ipkgpu_db_place keeps a query's sums in LDS; 0 = 4096; tests lower it to reach
 * the global tables with small inputs); "release_workspaces" (any value: the context's workspaces and cached result
 * blocks go back to the device now -- between the stages of the on-disk build; later calls allocate theirs again).
 * Every variant yields identical results.  Returns IPKGPU_ERR_INVALID for unknown names.
 *
 * Calls on one context are synchronous, but from its second scoring call on a context waits on its stream ONCE per key-major
 * call: sizes it used to read back mid-call (chunks drawn, big-list windows, entry total) are taken from the previous call
 * as estimates and checked at that one wait; a wrong estimate costs a repeated pass, never a wrong result. */
int ipkgpu_set_option(ipkgpu_ctx* ctx, const char* name, int64_t value);

/* ---- host helpers (no GPU needed) ------------------------------------------------------ */

/* log10 of IPK's score threshold: db_builder.cpp:640 `std::log10(score_threshold(omega, k))`.
 * score_threshold is un-vendored i2l code; documented as (omega/sigma)^k
 * (docs/source/usage.rst:224-229) and evaluated here in float: log10f(powf(omega/sigma, k)). */
float ipkgpu_log_threshold(float omega, uint32_t sigma, uint32_t k);

/* Bits per symbol of the packed k-mer code: i2l::bit_length<seq_type>() as used at
 * pk_compute.cpp:99 (sigma 4 -> 2, sigma 20 -> 5).  0 for unsupported sigma. */
uint32_t ipkgpu_bits_per_symbol(uint32_t sigma);

/* ipk::kmer_batch -- branch_group.cpp:104-107. */
size_t ipkgpu_kmer_batch(uint32_t key, size_t n_ranges);

/* Largest k that one call covering the whole key space accepts (DNA: 14, AA: 6); 0 for unsupported sigma. */
uint32_t ipkgpu_max_k(uint32_t sigma);
/* Largest k buildable in key-range passes (ipkgpu_score_groups_keyrange_device): 16 for DNA (u32 keys), = ipkgpu_max_k for
 * amino acids (no key-range passes: AA k = 7 needs 35-bit keys). */
uint32_t ipkgpu_max_k_keyrange(uint32_t sigma);

/* ---- the hot path ---------------------------------------------------------------------- */

/*
 * Replaces the body of the group loop, db_builder.cpp:606-625 + explore_group :629-698
 * (RAM mode), for a batch of ghost-node matrices.
 *
 *   logp       n_mats site-major matrices [mat][site][state] of float32 log10 posteriors --
 *              exactly the values raxmlng_reader::read_node produces (ar.cpp:257-260; AA columns
 *              already in IPK order, ar.cpp:232-234).  Host pointer.
 *   mat_group  [n_mats] branch id of each matrix = original post-order id
 *              (explore_kmers: _extended_mapping.at(node_group[0]), db_builder.cpp:613).
 *              Matrices with equal ids form one group (X0, X1 of a branch) in first-seen order.
 *   k, log_eps k-mer length and log10 score threshold (db_builder.cpp:640).
 *
 * Result (ipkgpu_result_* accessors): for every distinct branch id, the max-reduced set
 * {(key, score)} identical to group_map after explore_group (db_builder.cpp:685), keys packed
 * bits-per-symbol as at pk_compute.cpp:96-104, sorted ascending within the group (the
 * reference's order is hash order), plus the number of scored phylo-k-mers (the reference's
 * `count`, db_builder.cpp:664).
 *
 * Errors: IPKGPU_ERR_INVALID if sigma not in {4, 20}, k < 2, k > ipkgpu_max_k(sigma) or
 * sites < k (the reference reads out of range there, window.cpp:164-182; we reject).
 */
int ipkgpu_score_groups(ipkgpu_ctx* ctx, const float* logp, uint32_t n_mats, uint32_t sites,
                        uint32_t sigma, const uint32_t* mat_group, uint32_t k, float log_eps,
                        ipkgpu_result** out);

/* Same, with `logp` already resident in device memory (the measured configuration: no PCIe in
 * the timed region).  mat_group stays a host pointer.  The call returns after the device work
 * has completed; results stay in device memory until an accessor asks for a host copy. */
int ipkgpu_score_groups_device(ipkgpu_ctx* ctx, const float* logp_dev, uint32_t n_mats,
                               uint32_t sites, uint32_t sigma, const uint32_t* mat_group,
                               uint32_t k, float log_eps, ipkgpu_result** out);

/* KEEP_POSITIONS flavour (`ipk-aa-pos`: db_builder.cpp:655-662,687-689; branch_group.cpp:73-86): every kept score
 * carries the position (window start, window::get_position) of the window that produced it; on equal scores the
 * window processed first (group's matrices in input order, then ascending start) keeps its place, as `put`
 * replaces only on a strictly larger score.  Group-major output only; uses the global-atomic max-reduce with
 * 64-bit table entries.  ipkgpu_result_positions() gives the positions aligned with keys/scores. */
int ipkgpu_score_groups_positions(ipkgpu_ctx* ctx, const float* logp, uint32_t n_mats, uint32_t sites,
                                  uint32_t sigma, const uint32_t* mat_group, uint32_t k, float log_eps,
                                  ipkgpu_result** out);
const uint32_t* ipkgpu_result_positions(ipkgpu_result* r);   /* NULL unless produced by the call above */

/* ---- result accessors -------------------------------------------------------------------- */

uint32_t ipkgpu_result_num_groups(const ipkgpu_result* r);
/* [num_groups] branch ids in first-seen order (the order explore_kmers appends groups). */
const uint32_t* ipkgpu_result_group_ids(const ipkgpu_result* r);
/* [num_groups + 1] CSR offsets into keys/scores. */
const uint64_t* ipkgpu_result_offsets(const ipkgpu_result* r);
/* Total scored phylo-k-mers (sum over windows of |DCLA result|; db_builder.cpp:664,697). */
uint64_t ipkgpu_result_emitted(const ipkgpu_result* r);
/* Host copies (made on first use; NULL on failure) and the device-resident arrays. */
const uint32_t* ipkgpu_result_keys(ipkgpu_result* r);
const float* ipkgpu_result_scores(ipkgpu_result* r);
const uint32_t* ipkgpu_result_keys_device(const ipkgpu_result* r);
const float* ipkgpu_result_scores_device(const ipkgpu_result* r);
/* HIP-event timings of the call that produced r (milliseconds; see IPKGPU_T_*). */
double ipkgpu_result_time_ms(const ipkgpu_result* r, int which);
void ipkgpu_result_free(ipkgpu_result* r);

/* ---- key-major database parts and the k-mer-keyed merge (multi-GPU exchange step) ---------------- */

/*
 * Same scoring pass as ipkgpu_score_groups_device, but the result is delivered KEY-major and split
 * by owner -- the device analogue of the insertion loop at db_builder.cpp:685-694
 * (`_phylo_kmer_db.unsafe_insert(kmer, {branch, score})`, group after group) and of the on-disk
 * path's k-mer-keyed partition (kmer_batch, branch_group.cpp:104-107; merge_batch :45-70).
 *
 * Owner of a k-mer = dense_code % n_owners, where dense_code is the base-sigma value of the k-mer
 * (for DNA this IS the packed key, so owner = kmer_batch(key, n_owners)).  For owner o, key slot q
 * stands for dense code q * n_owners + o; slots = ceil(sigma^k / n_owners) per owner (zero padded).
 *
 *   counts   u32 [n_owners][slots]   number of (branch, score) entries of the key
 *   entries  {u32 branch, f32 score} owner-major, then ascending key, then group (first-seen) order
 *   owner_offsets  u64 [n_owners + 1] (host) entry offset of every owner's block
 *
 * With n_owners = world size, block o is what this rank sends to rank o (all-to-all over RCCL);
 * ipkgpu_merge_parts on the receiver concatenates, per key, the blocks of ranks 0..P-1.
 */
int ipkgpu_score_groups_keymajor_device(ipkgpu_ctx* ctx, const float* logp_dev, uint32_t n_mats, uint32_t sites,
                                        uint32_t sigma, const uint32_t* mat_group, uint32_t k, float log_eps,
                                        uint32_t n_owners, ipkgpu_parts** out);
/*
 * Key-range pass (DNA k = 14..16 built in pieces): as ipkgpu_score_groups_keymajor_device with one owner, for only the k-mers
 * whose first `lead_symbols` symbols spell `lead_class` (base sigma, first symbol most significant).  Those are the keys
 * [lead_class * sigma^(k - lead_symbols), (lead_class + 1) * sigma^(k - lead_symbols)): the key space of the call is
 * sigma^(k - lead_symbols) slots, slot q standing for key ipkgpu_parts_key_base(parts) + q.  The restriction is applied where
 * the leading symbols enter a window's left half list, so a pass scores only its own k-mers; sets and scores equal those of a
 * whole-key-space call restricted to the range.  ipkgpu_db_from_parts materialises the keys; one database per pass.
 * Supported: DNA, lead_symbols >= 1, 13 <= k - lead_symbols <= 14, i.e. (k, lead_symbols) in (14,1) (15,1) (15,2) (16,2) (16,3);
 * anything else is IPKGPU_ERR_INVALID.  A window whose half list exceeds the big-list cap fails the call, as at k = 13, 14.
 */
int ipkgpu_score_groups_keyrange_device(ipkgpu_ctx* ctx, const float* logp_dev, uint32_t n_mats, uint32_t sites,
                                        uint32_t sigma, const uint32_t* mat_group, uint32_t k, float log_eps,
                                        uint32_t lead_symbols, uint32_t lead_class, ipkgpu_parts** out);
/*
 * Positioned database (the reference's ipk-aa-pos flavour, db_builder.cpp:655-662,687-689; branch_group.cpp:73-86): as
 * ipkgpu_score_groups_keymajor_device, every entry also carrying the start of the window that produced its score -- among windows of
 * equal score bits the one explore_group processes first (the group's matrices in input order, then ascending start).  Keys, key
 * order, entry order and score bits equal those of ipkgpu_score_groups_keymajor_device on the same input; the position rides
 * along through ONE scoring pass (the exact partition with compressed tables: sequence numbers beside the pairs, an LDS reduce on
 * (score, first window), the key-major writer run over the position values as well).
 * n_owners must be 1 and n_mats > 0 here (several owners: ipkgpu_score_groups_keymajor_positions_owners_device below); supported where the exact partition exists: amino acids k = 2..6,
 * DNA k = 4..14; a group's matrices x windows must stay below 2^32.  Anything else: IPKGPU_ERR_INVALID with a message.
 * ipkgpu_db_from_parts moves the positions into the database with the entries; ipkgpu_db_write then writes the positioned file.
 */
int ipkgpu_score_groups_keymajor_positions_device(ipkgpu_ctx* ctx, const float* logp_dev, uint32_t n_mats, uint32_t sites,
                                                  uint32_t sigma, const uint32_t* mat_group, uint32_t k, float log_eps,
                                                  uint32_t n_owners, ipkgpu_parts** out);
/*
 * The positioned call split by owner, for several ranks: the same arguments, the same path and the same refusals as
 * ipkgpu_score_groups_keymajor_positions_device, with any n_owners >= 1.  counts [n_owners][slots] and entries are those of
 * ipkgpu_score_groups_keymajor_device(..., n_owners); ipkgpu_parts_positions_device gives the window starts aligned entry for entry
 * with the entries, block o being [owner_offsets[o], owner_offsets[o + 1]) of both.  A group's matrices are all in one call, so the
 * tie rule needs nothing from other ranks: the positions only travel (ipkgpu_exchange_begin) and are merged
 * (ipkgpu_merge_parts_positions_ptrs) beside their entries.  n_mats == 0 gives empty positioned parts (zero counts, no entries,
 * ipkgpu_parts_positions_device non-NULL): a rank or a piece without groups takes part in a positioned exchange with them.
 */
int ipkgpu_score_groups_keymajor_positions_owners_device(ipkgpu_ctx* ctx, const float* logp_dev, uint32_t n_mats, uint32_t sites,
                                                         uint32_t sigma, const uint32_t* mat_group, uint32_t k, float log_eps,
                                                         uint32_t n_owners, ipkgpu_parts** out);
/* u32 [entries] window starts aligned entry for entry with ipkgpu_parts_entries_device; NULL for parts of the other calls */
const uint32_t* ipkgpu_parts_positions_device(const ipkgpu_parts* p);
/* lead_class * sigma^(k - lead_symbols) for key-range parts; 0 for other parts */
uint64_t ipkgpu_parts_key_base(const ipkgpu_parts* p);
uint32_t ipkgpu_parts_num_owners(const ipkgpu_parts* p);
uint64_t ipkgpu_parts_slots(const ipkgpu_parts* p);
const uint32_t* ipkgpu_parts_counts_device(const ipkgpu_parts* p);
const void* ipkgpu_parts_entries_device(const ipkgpu_parts* p);
const uint64_t* ipkgpu_parts_owner_offsets(const ipkgpu_parts* p);
uint64_t ipkgpu_parts_emitted(const ipkgpu_parts* p);
double ipkgpu_parts_time_ms(const ipkgpu_parts* p, int which);
void ipkgpu_parts_free(ipkgpu_parts* p);

/*
 * Merges, for one owner, the blocks received from n_sources ranks (or produced by n_sources batches):
 *   counts_dev      u32 [n_sources][slots] (device), source-major
 *   entries_dev     the sources' entry blocks (device); source s starts at entry source_offsets[s]
 *   source_offsets  u64 [n_sources] (host)
 * Result: this owner's shard of the phylo-k-mer database -- keys (IPK bit-packed codes, ascending),
 * key_offsets [num_keys + 1], entries {branch, score} with each key's entries in source order then
 * group order, i.e. the order the reference appends them (db_builder.cpp:606-618,685-694).
 */
int ipkgpu_merge_parts(ipkgpu_ctx* ctx, uint32_t sigma, uint32_t k, uint32_t owner, uint32_t n_owners,
                       uint32_t n_sources, const uint32_t* counts_dev, const void* entries_dev,
                       const uint64_t* source_offsets, ipkgpu_db** out);
/* Like ipkgpu_merge_parts, with one pointer pair per source instead of one base and offsets: counts_dev[s] = the source's
 * counts row [slots] (device), entries_dev[s] = its entry block (device).  Both pointer arrays live in HOST memory. */
int ipkgpu_merge_parts_ptrs(ipkgpu_ctx* ctx, uint32_t sigma, uint32_t k, uint32_t owner, uint32_t n_owners, uint32_t n_sources,
                            const uint32_t* const* counts_dev, const void* const* entries_dev, ipkgpu_db** out);
/* ipkgpu_merge_parts_ptrs over positioned sources: positions_dev[s] = source s's window starts (u32, device), aligned entry for
 * entry with entries_dev[s].  Every position is copied beside its entry in the same pass (merge_copy_pos_kernel), and the database
 * has them (ipkgpu_db_positions), so ipkgpu_db_filter_mif0 and ipkgpu_db_write treat it as ipkgpu_db_from_parts' positioned one. */
int ipkgpu_merge_parts_positions_ptrs(ipkgpu_ctx* ctx, uint32_t sigma, uint32_t k, uint32_t owner, uint32_t n_owners, uint32_t n_sources,
                                      const uint32_t* const* counts_dev, const void* const* entries_dev,
                                      const uint32_t* const* positions_dev, ipkgpu_db** out);

/* ---- the exchange step itself: RCCL over xGMI, inside the library ------------------------------------------------
 * One process per GPU.  Rank 0 draws an id (ipkgpu_comm_unique_id) and hands its 128 bytes to the other ranks by any means
 * (MPI, a file, torch.distributed); every rank then calls ipkgpu_comm_init.  Per range ("piece") of its branch groups a rank
 * calls ipkgpu_score_groups_keymajor_device(..., n_owners = world) and ipkgpu_exchange_begin, which enqueues block o -> rank o
 * (grouped ncclSend/ncclRecv on the communicator's own stream) and returns, so the transfer runs under the next piece's
 * scoring; ipkgpu_exchange_merge waits for the pieces and merges (rank, piece)-ordered sources into this rank's shard.
 * Positioned pieces (ipkgpu_score_groups_keymajor_positions_owners_device) send their window starts beside the entries, one more
 * send/receive pair per peer in the same group; the size word that travels first carries "positioned" in bit 63, and a rank whose
 * peers' flags differ from its own fails ipkgpu_exchange_begin with IPKGPU_ERR_INVALID before the payload group.
 * ipkgpu_exchange_merge gives a database with positions when all pieces are positioned and refuses a mixture (IPKGPU_ERR_INVALID).
 * All ranks must use the same number of pieces.  RCCL is loaded at run time: IPKGPU_ERR_NODEVICE if it is not there.
 * Failure must be symmetric, or the healthy ranks wait for ever inside a collective: everything that can fail on one rank
 * alone (loading RCCL, the exchange stream and buffers) is done by ipkgpu_comm_prepare, BEFORE the collective
 * ncclCommInitRank inside ipkgpu_comm_init -- the ranks agree on the prepare results first (an all-reduce by whatever carried
 * the id) and enter ipkgpu_comm_init only if all succeeded.  A rank whose ipkgpu_exchange_begin fails aborts the communicator
 * (ncclCommAbort), which makes its peers' pending transfers fail instead of hang; it should then exit non-zero.
 * CPU analogue: branch_group.cpp:45-70,104-107 (merge_batch, kmer_batch), db_builder.cpp:392-458 (merge_stage2). */
typedef struct ipkgpu_xfer ipkgpu_xfer;
int ipkgpu_comm_available(void);                          /* IPKGPU_OK if RCCL can be loaded in this process (no GPU call) */
int ipkgpu_comm_unique_id(uint8_t* id128);
int ipkgpu_comm_prepare(ipkgpu_ctx* ctx, int world);       /* the local, non-collective half of the set-up (idempotent) */
int ipkgpu_comm_init(ipkgpu_ctx* ctx, const uint8_t* id128, int rank, int world);
int ipkgpu_comm_rank(const ipkgpu_ctx* ctx);
int ipkgpu_comm_world(const ipkgpu_ctx* ctx);
int ipkgpu_exchange_begin(ipkgpu_ctx* ctx, ipkgpu_parts* parts, ipkgpu_xfer** out);     /* parts stay alive until the merge */
int ipkgpu_exchange_merge(ipkgpu_ctx* ctx, ipkgpu_xfer* const* xfers, uint32_t n_pieces, uint32_t sigma, uint32_t k, ipkgpu_db** out,
                          double* exposed_ms /* optional: time spent waiting for transfers */);
double ipkgpu_xfer_exposed_ms(const ipkgpu_xfer* x);
void ipkgpu_xfer_free(ipkgpu_xfer* x);

/* ---- the on-disk build: a database larger than device memory (db_builder.cpp:137,340-458,673-681; branch_group.cpp:104-185) ----
 * Stage 1: the groups are scored in pieces (contiguous ranges of the first-seen group order), each with
 * ipkgpu_score_groups_keymajor_device(..., n_owners = B); ipkgpu_parts_spill takes the piece's B owner blocks off the device, one file
 * `dir`/p<piece>_b<owner>.blk each (layout: ipk_amd/csrc/spill_format.hpp -- occupancy bits of the counts row, the non-empty slots'
 * counts as u16, the entries unchanged; an empty block is written too: head and zero bits).  Stage 2, per batch b: ipkgpu_spill_merge reads the
 * pieces' blocks of owner b IN THE ORDER GIVEN (piece order = group order = the reference's append order), unpacks them and merges them as
 * ipkgpu_merge_parts does; the database is filtered and written like any other, its file merged with the other batches' by
 * ipkgpu_db_merge_files.  The device never holds more than one piece's result or one batch of the database.
 * ipkgpu_parts_spill refuses (IPKGPU_ERR_INVALID) positioned parts (the reference keeps no positions on disk either, db_builder.cpp:469),
 * key-range parts, and a piece in which a key has more than 65535 entries (more groups than that in one piece); a failed write leaves no
 * file under a block's final name.  ipkgpu_spill_merge checks every block on the host before anything is launched -- the head (magic, version,
 * sigma, k, n_owners, owner, slots, the file size against its totals), then the body against the head as it is read -- and names the file it
 * refuses; the head checks need no context (ctx == NULL: the message is ipkgpu_last_error(NULL)'s, the status IPKGPU_ERR_INVALID in any case). */
int ipkgpu_parts_spill(ipkgpu_ctx* ctx, ipkgpu_parts* parts, const char* dir, uint32_t piece, uint64_t* bytes_written);
int ipkgpu_spill_merge(ipkgpu_ctx* ctx, uint32_t sigma, uint32_t k, uint32_t owner, uint32_t n_owners, const char* const* block_paths,
                       uint32_t n_blocks, ipkgpu_db** out);
/* Device memory the context holds from hipMalloc -- its workspaces and its result blocks, live or cached -- and the high-water mark of
 * that figure (reset_peak != 0: the mark restarts from the current figure after it has been reported).  Option "device_budget_bytes"
 * (0 = none, the default) makes the context behave like a device of that size: an allocation that would take the figure beyond the budget
 * first drops the cached blocks and, if it still would, fails with IPKGPU_ERR_NOMEM; work sized by free device memory sees at most what
 * the budget leaves.  The context stays usable after such a failure.  Device memory of the caller (the matrices) is not counted. */
int ipkgpu_mem_stats(ipkgpu_ctx* ctx, uint64_t* held, uint64_t* held_peak, int reset_peak);
/* Reads back "workspace_bytes", "device_budget_bytes", "db_load_chunk_bytes", "db_load_window_bytes" or "slice_long_lists" (a caller that sets them for a while restores them),
 * "debug_sliced_windows" (the windows this context has scored in slices so far), "debug_pool_bytes" (the bytes its pair pool holds), or "last_refused_bytes":
 * the bytes held plus the size of the last allocation the device or the budget refused -- what the failed step needed at least.
 * IPKGPU_ERR_INVALID for other names. */
int ipkgpu_get_option(const ipkgpu_ctx* ctx, const char* name, int64_t* value);

/* Single-GPU shortcut (n_owners == 1): the parts already ARE the database; produces the key list and
 * MOVES the entry array out of `parts` (which stays valid for its counts/timings, entries become NULL).
 * Key-range parts give the keys of their range (key_base + slot); k is the k-mer length of the pass. */
int ipkgpu_db_from_parts(ipkgpu_ctx* ctx, ipkgpu_parts* parts, uint32_t sigma, uint32_t k, ipkgpu_db** out);
uint64_t ipkgpu_db_num_keys(const ipkgpu_db* d);
uint64_t ipkgpu_db_num_entries(const ipkgpu_db* d);
/* host copies (made on first use): keys u32[num_keys], key_offsets u64[num_keys+1], entries u32[num_entries][2] */
const uint32_t* ipkgpu_db_keys(ipkgpu_db* d);
const uint64_t* ipkgpu_db_key_offsets(ipkgpu_db* d);
const uint32_t* ipkgpu_db_entries(ipkgpu_db* d);
const uint32_t* ipkgpu_db_keys_device(const ipkgpu_db* d);
const uint64_t* ipkgpu_db_key_offsets_device(const ipkgpu_db* d);
const void* ipkgpu_db_entries_device(const ipkgpu_db* d);
/* window starts u32[num_entries] of a database built from positioned parts, aligned with the entries (host copy on first use);
 * NULL for databases without positions */
const uint32_t* ipkgpu_db_positions(ipkgpu_db* d);
const uint32_t* ipkgpu_db_positions_device(const ipkgpu_db* d);
double ipkgpu_db_time_ms(const ipkgpu_db* d);
void ipkgpu_db_free(ipkgpu_db* d);

/* ---- "next" row n1: filter values (MIF0, random) and k-mer order (filter.cpp:55-145, db_builder.cpp:254-284) -- */

/* IPK's score threshold itself (un-vendored i2l::score_threshold; assumed powf(omega/sigma, k)). */
float ipkgpu_score_threshold(float omega, uint32_t sigma, uint32_t k);

/*
 * mif0_filter::calc_filter_values over a database shard, then the order of db_builder.cpp:284
 * (ascending filter value; ties -- unspecified in the reference -- by ascending key).
 *   total_num_groups  N = node count of the original tree (db_builder.cpp:261)
 *   threshold         score_threshold(omega, k), NOT its log (db_builder.cpp:260)
 * Filter values are per k-mer, so a shard is filtered independently of the other owners.
 * Double arithmetic on the device, the entries' terms ADDED IN ENTRY ORDER (the association of the reference's two
 * sequential loops, filter.cpp:60-119): the float filter values and the k-mer order equal a sequential host evaluation;
 * only the last bit of the device's pow / log2 could differ from the host's libm.
 */
int ipkgpu_db_filter_mif0(ipkgpu_ctx* ctx, ipkgpu_db* db, uint64_t total_num_groups, float threshold);
/*
 * The random filter (ipk.py build --filter random) over a database shard: filter value = a fixed draw in [0, 1) per k-mer CODE --
 * the splitmix64 finaliser of the code, its top 24 bits times 2^-24 (exact in float) -- then the same order as above.
 * This is THIS project's draw, not the reference's: random_filter (filter.cpp:122-145) draws uniform(0, 1) from
 * std::default_random_engine(42) in the hash map's iteration order, which no other build reproduces.  One fixed draw per code
 * means the file does not depend on sharding, key-range passes or on-disk batches.  Replaces the filter arrays the database
 * has (as ipkgpu_db_filter_mif0 does); the accessors below and ipkgpu_db_write serve either filter.
 */
int ipkgpu_db_filter_random(ipkgpu_ctx* ctx, ipkgpu_db* db);
/* host copies: filter value per k-mer (as the float i2l::kmer_fv stores, and in double), and the
 * positions of the k-mers in filter order: keys[order[0]] is written first */
const float* ipkgpu_db_filter_values(ipkgpu_db* d);
const double* ipkgpu_db_filter_values_f64(ipkgpu_db* d);
const uint32_t* ipkgpu_db_filter_order(ipkgpu_db* d);
const float* ipkgpu_db_filter_values_device(const ipkgpu_db* d);
const uint32_t* ipkgpu_db_filter_order_device(const ipkgpu_db* d);
double ipkgpu_db_filter_time_ms(const ipkgpu_db* d);

/* ---- "next" row n3: RAxML-ng ancestral-probabilities loader (host, multi-threaded) -------------------- */

typedef struct ipkgpu_ar ipkgpu_ar;

/* raxmlng_reader (ar.cpp:144-188): memory-maps `<prefix>.raxml.ancestralProbs` (TSV, one header line, rows
 * `Node \t Site \t State \t p_1 .. p_sigma`, contiguous per node) and indexes the node blocks. */
int ipkgpu_ar_open(const char* path, uint32_t sigma, ipkgpu_ar** out);
void ipkgpu_ar_close(ipkgpu_ar* ar);
const char* ipkgpu_ar_last_error(void);           /* message of the last failing ipkgpu_ar_* call of this thread */
uint32_t ipkgpu_ar_num_nodes(const ipkgpu_ar* ar);
uint32_t ipkgpu_ar_sites(const ipkgpu_ar* ar);    /* rows of the first node's block */
const char* ipkgpu_ar_node_label(const ipkgpu_ar* ar, uint32_t i);   /* labels in order of first appearance */
int64_t ipkgpu_ar_find(const ipkgpu_ar* ar, const char* label);      /* -1 if absent */
/* raxmlng_reader::read_node (ar.cpp:200-270) for n nodes at once: out[i] = [sites][sigma] float32 log10
 * posteriors of node node_idx[i] (AA columns permuted to IPK order), ready for ipkgpu_score_groups.
 * n_threads = 0 uses all host cores. */
int ipkgpu_ar_read_nodes(ipkgpu_ar* ar, const uint32_t* node_idx, uint32_t n, float* out, uint32_t n_threads);

/* ---- "next" row n3 (second half): reference tree, ghost nodes, node mapping (host) -------------------------- */

typedef struct ipkgpu_tree ipkgpu_tree;
typedef struct ipkgpu_ghost_plan ipkgpu_ghost_plan;

/* Own newick reader (i2l::io::load_newick is un-vendored): children in file order, post-order ids from 0, quoted labels
 * and [comments] accepted.  ipkgpu_tree_last_error(): message of the last failing ipkgpu_tree_* / ipkgpu_ghost_plan_*
 * call of this thread. */
int ipkgpu_tree_parse(const char* newick, ipkgpu_tree** out);
int ipkgpu_tree_load(const char* path, ipkgpu_tree** out);
void ipkgpu_tree_free(ipkgpu_tree* t);
const char* ipkgpu_tree_last_error(void);
uint32_t ipkgpu_tree_num_nodes(const ipkgpu_tree* t);
uint32_t ipkgpu_tree_num_leaves(const ipkgpu_tree* t);
int ipkgpu_tree_is_rooted(const ipkgpu_tree* t);                      /* root has exactly two children */
const char* ipkgpu_tree_label(const ipkgpu_tree* t, uint32_t postorder_id);
int64_t ipkgpu_tree_parent(const ipkgpu_tree* t, uint32_t postorder_id);   /* post-order id of the parent, -1 for the root */
double ipkgpu_tree_branch_length(const ipkgpu_tree* t, uint32_t postorder_id);
const char* ipkgpu_tree_newick(ipkgpu_tree* t);                       /* owned by the tree, valid until the next call */
/* The database header's tree index (db_builder.cpp:192-197): per node in post-order, the size of its subtree and the
 * total branch length below it.  Arrays of ipkgpu_tree_num_nodes() elements. */
int ipkgpu_tree_index(const ipkgpu_tree* t, uint32_t* num_nodes, double* subtree_length);
/* tree_extender::extend (extended_tree.cpp:76-150): ghost nodes <counter>_X0 / _X1 (+ dummy leaves _X2 / _X3) on every
 * non-root branch, counter from node_count + 1; the result remembers ghost label -> original post-order id. */
int ipkgpu_tree_extend(const ipkgpu_tree* original, ipkgpu_tree** extended);
/* reroot_tree (extended_tree.cpp:186-205), applied to the AR tree when the reference tree is rooted (main.cpp:172-178). */
int ipkgpu_tree_reroot(ipkgpu_tree* t);
/* get_ghost_ids + group_ghost_ids (db_builder.cpp:495-553) + map_nodes (ar.cpp:790-834): the ghost nodes in the order
 * explore_kmers scores them, each with its label in the AR output and its branch id = mat_group of ipkgpu_score_groups.
 * strategy: 0 both, 1 inner only (_X0), 2 outer only (_X1).  ar_tree may be NULL (AR labels = extended labels). */
int ipkgpu_ghost_plan_make(const ipkgpu_tree* original, const ipkgpu_tree* extended, const ipkgpu_tree* ar_tree, int strategy,
                           ipkgpu_ghost_plan** out);
void ipkgpu_ghost_plan_free(ipkgpu_ghost_plan* p);
uint32_t ipkgpu_ghost_plan_size(const ipkgpu_ghost_plan* p);
const char* ipkgpu_ghost_plan_ext_label(const ipkgpu_ghost_plan* p, uint32_t i);
const char* ipkgpu_ghost_plan_ar_label(const ipkgpu_ghost_plan* p, uint32_t i);
const uint32_t* ipkgpu_ghost_plan_branches(const ipkgpu_ghost_plan* p);

/* ---- "next" row n2: the database file (db_builder.cpp:145-146,176-177,297-306,323-327) ------------------------ */

/* Header fields in the order of i2l::ipk_header as db_builder.cpp:297-305 fills it. */
typedef struct ipkgpu_db_header {
    const char* sequence_type;            /* seq_type::name: "DNA" | "AA" */
    uint64_t tree_index_size;             /* nodes of the original tree */
    const uint32_t* tree_num_nodes;       /* [tree_index_size] (ipkgpu_tree_index) */
    const double* tree_subtree_length;    /* [tree_index_size] */
    const char* newick;                   /* the original tree */
    uint64_t kmer_size;
    float omega;
} ipkgpu_db_header;

/* save_header + save_phylo_kmer for every k-mer in filter order (db_builder.cpp:297-306,323-327), streamed from device
 * memory: the records are packed on the GPU in pieces, copied through pinned buffers and written while the next piece is
 * being packed.  Needs ipkgpu_db_filter_mif0 or ipkgpu_db_filter_random first.  Byte layout: ipk_amd/csrc/ipk_format.hpp -- i2l and Boost are
 * un-vendored, so the layout is a reconstruction (Boost binary_oarchive primitives) and NOT pinned against a real .ipk.
 * A database that has positions (ipkgpu_db_positions_device != NULL) is written as the positioned file, byte for byte what
 * ipkgpu_db_write_host_positions writes from its host arrays; refused with that function's messages, before the file is created,
 * when a window position exceeds 65535 or when IPKGPU_IPK_PROTOCOL_VERSION=0. */
int ipkgpu_db_write(ipkgpu_ctx* ctx, ipkgpu_db* db, const ipkgpu_db_header* header, const char* path, uint64_t* bytes_written);
/* The same serialiser over host arrays (merged shards of several GPUs, or a filter computed on the host):
 * entries u32 [n][2] = (branch, score bits); order = positions of the k-mers in output order (NULL: as stored). */
int ipkgpu_db_write_host(const ipkgpu_db_header* header, uint64_t n_keys, const uint32_t* keys, const uint64_t* key_offsets,
                         const uint32_t* entries, const float* filter_values, const uint32_t* order, const char* path,
                         uint64_t* bytes_written);
/* The positioned database of ipk-aa-pos (KEEP_POSITIONS: db_builder.cpp:655-662,687-689; branch_group.cpp:73-86): as
 * ipkgpu_db_write_host, with positions[n] = the window position that goes with every entry's score (ipkgpu_score_groups_positions),
 * the header's positions flag set and entries of (branch, score, position).  The position's width in the file (u16) is a guess like
 * the rest of the layout; positions beyond 65535 are refused. */
int ipkgpu_db_write_host_positions(const ipkgpu_db_header* header, uint64_t n_keys, const uint32_t* keys, const uint64_t* key_offsets,
                                   const uint32_t* entries, const uint32_t* positions, const float* filter_values, const uint32_t* order,
                                   const char* path, uint64_t* bytes_written);
const char* ipkgpu_db_write_last_error(void);
/* The database file of a multi-GPU build -- the role of merge_stage2 (db_builder.cpp:392-458: batch files opened together,
 * a priority queue on the filter value hands out the k-mer to append next).  Every rank writes ITS shard (the k-mers it owns,
 * filter values computed, in its filter order) as a database file of its own with ipkgpu_db_write / ipkgpu_db_write_host
 * (any header: only the totals are read back); one rank then merges the P shard files by (filter value, key) into `path`
 * under header `h`, streaming through bounded buffers: resident memory does not depend on the number of entries, and the
 * result equals, byte for byte, the file one GPU writes for the same input.  Host code, no GPU needed.
 * Positioned shards (the positions flag in their headers; records of 16 + 10 n bytes) merge into a positioned file, the flag
 * set in its header.  A mixture of positioned and plain shards is IPKGPU_ERR_INVALID, and so are positioned shards under
 * IPKGPU_IPK_PROTOCOL_VERSION=0, whose layout has no flag to read. */
int ipkgpu_db_merge_files(const ipkgpu_db_header* h, const char* const* shard_paths, uint32_t n_shards, const char* path,
                          uint64_t* total_kmers, uint64_t* total_entries, uint64_t* bytes_written);
const char* ipkgpu_db_merge_last_error(void);
/* seconds of the last ipkgpu_db_write of this context: 0 = total, 1 = device packing + copies (waited for), 2 = file writes */
double ipkgpu_db_write_time_s(const ipkgpu_ctx* ctx, int which);
/* The protocol version the writers put behind the archive preamble, followed (after the sequence type) by the positions flag --
 * what phylo_kmer_db::version() / positions_loaded() answer for a loaded database (tools/src/diff.cpp:41-46,137-145).  Position,
 * width and value are guesses (ipk_format.hpp); IPKGPU_IPK_PROTOCOL_VERSION in the environment sets the value, 0 = neither field
 * is written.  Readers of this library's files (ipkgpu_db_merge_files, the tests' parser) ask here what to expect. */
uint32_t ipkgpu_db_protocol_version(void);

/* ---- reading a database file back: description and validation on the host, the load on the device ----------------------
 * The reference loads a database with i2l::load and ships two tools over the loaded object, ipkdiff and ipkdump
 * (tools/src/diff.cpp, tools/src/dump.cpp); `ipk.py diff` / `ipk.py dump` are this library's.  The layout read is the one the
 * writers above write (ipk_format.hpp: a reconstruction, NOT pinned against a real .ipk -- reading a real .ipk is not claimed),
 * under the protocol version of the running process (ipkgpu_db_protocol_version); a file of another one is refused. */
typedef struct ipkgpu_db_file ipkgpu_db_file;

/* Parses and validates everything in front of the first k-mer record (host only, no GPU).  IPKGPU_ERR_INVALID with
 * ipkgpu_db_file_last_error() (this thread's last failing ipkgpu_db_file_* call) if the file is not of the layout. */
int ipkgpu_db_file_open(const char* path, ipkgpu_db_file** out);
void ipkgpu_db_file_close(ipkgpu_db_file* f);
const char* ipkgpu_db_file_last_error(void);
/* The head's fields; strings and arrays are owned by the handle. */
const char* ipkgpu_db_file_sequence_type(const ipkgpu_db_file* f);
int ipkgpu_db_file_positions_loaded(const ipkgpu_db_file* f);           /* the positions flag (0 where the layout has none) */
uint32_t ipkgpu_db_file_protocol_version(const ipkgpu_db_file* f);       /* the protocol word (0 where the layout has none) */
uint32_t ipkgpu_db_file_library_version(const ipkgpu_db_file* f);        /* the archive preamble's library version */
uint64_t ipkgpu_db_file_tree_index_size(const ipkgpu_db_file* f);
const uint32_t* ipkgpu_db_file_tree_num_nodes(const ipkgpu_db_file* f);  /* [tree_index_size] */
const double* ipkgpu_db_file_tree_subtree_length(const ipkgpu_db_file* f);
const char* ipkgpu_db_file_newick(const ipkgpu_db_file* f);
uint64_t ipkgpu_db_file_kmer_size(const ipkgpu_db_file* f);
float ipkgpu_db_file_omega(const ipkgpu_db_file* f);
uint64_t ipkgpu_db_file_total_kmers(const ipkgpu_db_file* f);            /* the header's totals, as written */
uint64_t ipkgpu_db_file_total_entries(const ipkgpu_db_file* f);
uint64_t ipkgpu_db_file_bytes(const ipkgpu_db_file* f);                  /* size of the file */
uint64_t ipkgpu_db_file_body_offset(const ipkgpu_db_file* f);            /* where the first k-mer record starts */
/* The head as the writers take it (pointers into the handle): ipkgpu_db_write(ctx, loaded, &h, ...) reproduces the file. */
int ipkgpu_db_file_header(const ipkgpu_db_file* f, ipkgpu_db_header* h);
/* Walks the records by their count fields (16 + 8 n bytes each, 16 + 10 n with positions): the one serial part of reading a
 * file, streamed once.  IPKGPU_ERR_INVALID, the message naming the record's index and its byte offset in the file, when a count
 * would carry a record past the end of the file, when the walk does not end exactly at the end of the file, or when the numbers
 * of records or entries differ from the header's totals. */
int ipkgpu_db_file_check(ipkgpu_db_file* f, uint64_t* n_records, uint64_t* n_entries);

/* Loads a database file onto the device: the same object the builds produce (every accessor, ipkgpu_db_write included, takes it).
 * keys ascending, key_offsets, entries in the file's order inside a key, positions for a positioned file; the filter arrays hold
 * the file's filter values (ipkgpu_db_filter_values: their bits; _f64: their widening) and the file's record order
 * (ipkgpu_db_filter_order: keys[order[i]] is the i-th record), so ipkgpu_db_write with ipkgpu_db_file_header(ipkgpu_db_header_of(d))
 * gives the file back byte for byte.
 * The file goes chunk by chunk through the context's two pinned buffers (option "db_load_chunk_bytes"; 0 = 64 MiB, the spill
 * blocks') into a device image of its body, the next read under the previous copy, while the host walks the count fields
 * (ipkgpu_db_file_check's walk); then db_unpack_heads_kernel, a sort of (key, record), a scan of the counts and
 * db_unpack_entries_kernel (kernels_dbload.hpp).  No kernel indexes by a number of the file the host has not checked: a bad file
 * is IPKGPU_ERR_INVALID before the first of them is launched.  Also IPKGPU_ERR_INVALID: a key in two records, more than
 * 2^32 - 1 records, a record of 2^32 entries or more.  Device memory: the image (the body's bytes, freed before the call returns)
 * plus the database plus 44 bytes per k-mer of workspace and the sort's own, all counted by ipkgpu_mem_stats and held to "device_budget_bytes";
 * what does not fit is IPKGPU_ERR_NOMEM and leaves the context usable.  A file larger than device memory is not loaded whole
 * (ipkgpu_db_load_select below loads a prefix of it, ipkgpu_db_load_wanted the records a batch of queries can look up,
 * ipkgpu_db_load_key_range the records of a key range, and ipkgpu_db_diff_files compares two such files range by range). */
int ipkgpu_db_load(ipkgpu_ctx* ctx, const char* path, ipkgpu_db** out);
/* The head of the file a database was loaded from (owned by the database); NULL for databases that were not loaded. */
const ipkgpu_db_file* ipkgpu_db_header_of(const ipkgpu_db* d);
/* The last ipkgpu_db_load or ipkgpu_db_load_select of this context: 0 = seconds in all, 1 = file reads, 2 = the host's walk,
 * 3 = waiting for the device; 4 = db_unpack_heads_kernel ms, 5 = db_unpack_entries_kernel ms, 6 = all device work behind the last
 * copy, ms; 7 = the bytes of the file's body the call touched: the whole body for a full load; for a prefix load the prefix rounded
 * up to a load chunk (the extent of the walk -- the copy then reads exactly the prefix, inside that extent). */
double ipkgpu_db_load_time(const ipkgpu_ctx* ctx, int which);

/* ---- selection: the consumer of the filter order -- the most informative fraction mu of a database, at a raised threshold ------------
 * The filter stages put the k-mers of a database (and the records of its file) into filter order so that a consumer can take only
 * the first of them, and can raise the score threshold without a rebuild.  THE DEFINITION BELOW IS THIS LIBRARY'S OWN AND UNPINNED:
 * the reference's reader, i2l::load(file, mu, omega), is un-vendored and could not be read, so what it does with mu and omega beyond
 * what their names say was not checked (as for the ambiguity expansion of ipkgpu_db_place_opts).
 *
 * Source database D: keys ascending, key_offsets, entries, positions if it has them, filter values (float and double) and order,
 * keys[order[i]] being the i-th record.  For keep_kmers = M and min_log_score = t the selection V is:
 *   1. candidates  the records i < min(M, num_keys) of D's order, i.e. the keys order[i].  M larger than num_keys behaves as num_keys.
 *   2. entries     of a candidate key, in D's order, those with score > t: a binary32 comparison, strict -- the build's own rule
 *                  (an entry is stored iff its score exceeds the threshold).  A NaN score fails it; t = -inf keeps every entry (of a
 *                  score that is neither NaN nor -inf: no build stores those); positions travel with their entries.
 *   3. keys        a candidate left without an entry is dropped, like every non-candidate.  M counts records BEFORE step 2, as a
 *                  reader that stops after M records counts them.
 *   4. arrays      V's keys ascend; its filter values are D's bit for bit, float and double (nothing is recomputed); V's order is
 *                  the surviving records in D's order, renumbered to V's key indices.
 *   5. head        ipkgpu_db_header_of(V): for a loaded D a copy of D's head with the two totals replaced by V's -- omega stays
 *                  as it is, for the call takes t and no omega; NULL when D was not loaded.
 * IPKGPU_ERR_INVALID: a NaN t, a D without filter arrays (built and never filtered), NULL arguments, a D of another context.
 * An empty V (M = 0, t = +inf, ...) is IPKGPU_OK with num_keys 0: every accessor, ipkgpu_db_write and placement take it (every query
 * then has no placement).  V is an ordinary database, independent of D; D is only read and stays valid.
 * All device work (kernels_dbselect.hpp): candidate flags scattered from the order, a keep flag per entry -- by entry ranges, so one
 * key of 5000 entries costs what 5000 keys of one entry cost --, exclusive scans of the flags, then compacting copies.  Output places
 * come from the scans alone (no atomics): the same bits on every run.  Device memory: V, plus 12 bytes per entry and 12 per key of D
 * and 12 per record i < M of workspace and the scans' own, counted by ipkgpu_mem_stats and held to "device_budget_bytes"; what does
 * not fit is IPKGPU_ERR_NOMEM and leaves the context usable.  ipkgpu_db_select_time_ms: device time of the context's last selection. */
int ipkgpu_db_select(ipkgpu_ctx* ctx, const ipkgpu_db* src, uint64_t keep_kmers, float min_log_score, ipkgpu_db** out);
double ipkgpu_db_select_time_ms(const ipkgpu_ctx* ctx);
/* mu -> M: min(n_kmers, (uint64_t)ceil((double)mu * (double)n_kmers)), in binary64.  Callers refuse mu outside [0, 1] and NaN
 * (here: mu <= 0 and NaN give 0, mu >= 1 gives n_kmers).  Host only. */
uint64_t ipkgpu_db_mu_kmers(double mu, uint64_t n_kmers);
/* ipkgpu_db_select(ipkgpu_db_load(path), keep_kmers, min_log_score) bit for bit in every array, the order included -- reading and
 * walking only the prefix of the file's body that holds its first min(keep_kmers, header total) records (the file IS in filter
 * order).  File bytes read, and the device image, are at most that prefix rounded up to one load chunk ("db_load_chunk_bytes");
 * ipkgpu_db_load_time(ctx, 7) tells that rounded-up figure.  The head is validated as by ipkgpu_db_load; the walk stops at keep_kmers records
 * and every one of them must end inside the file (else IPKGPU_ERR_INVALID naming the record).  That the walk ends at the end of the
 * file, and that its totals are the header's, cannot be checked on a prefix: both checks are made only when keep_kmers >= the
 * header's total -- the call is then a full ipkgpu_db_load followed by the selection -- and DAMAGE BEHIND THE PREFIX IS NOT SEEN.
 * The prefix walk reads the count fields through a read-only mapping of the file (its length is known only at the walk's end, and the
 * image is allocated at exactly that length before the prefix is read through the pinned buffers).  The file's size is checked against
 * the one the head was parsed at before it is mapped; a file that ANOTHER PROCESS TRUNCATES DURING THE CALL, or an I/O error under the
 * mapping, is a SIGBUS to this process -- not the IPKGPU_ERR_INVALID the full load's reads make of the same events.  Do not load a
 * prefix of a file that is being rewritten.
 * A file larger than device memory loads this way for every keep_kmers whose prefix (plus its database and the selection) fits. */
int ipkgpu_db_load_select(ipkgpu_ctx* ctx, const char* path, uint64_t keep_kmers, float min_log_score, ipkgpu_db** out);

/* ipkdiff's comparison of two databases of one context (tools/src/diff.cpp:210-295), on the device (kernels_dbdiff.hpp). */
typedef struct ipkgpu_db_diff_counts {
    uint64_t keys_a, keys_b, keys_only_a, keys_only_b;
    uint64_t entries_a, entries_b;
    uint64_t entries_only_a, entries_only_b;      /* (k-mer, branch) scored in one database only; includes those of keys_only_* */
    uint64_t scores_differ;                        /* (k-mer, branch) in both, scores do not match */
    uint64_t positions_differ;                     /* both positioned, scores match, positions differ; else 0 */
    double   max_abs_diff;                         /* over (k-mer, branch) pairs present in both */
} ipkgpu_db_diff_counts;
typedef struct ipkgpu_db_diff_record { uint32_t key, branch; float a_score, b_score; } ipkgpu_db_diff_record;  /* NaN = not scored */
/* Scores of a (k-mer, branch) in both match iff fabs(a - b) < eps -- the difference in float, the comparison in double (:233);
 * eps == 0: iff the score bits are equal.  An entry is matched with the FIRST entry of the same branch in the other database's
 * list of that k-mer (the files of this library name a branch once per k-mer; where the two lists of a k-mer name the same branches
 * in the same order they are compared place by place); the order of a k-mer's entries carries no meaning.  max_abs_diff is taken
 * over A's entries that B scores too.  records (may be NULL with max_records == 0) receives the first max_records differences --
 * entries scored in one database only, and scores that do not match -- in this order: ascending k-mer; inside a k-mer A's entries
 * in A's order, then B's entries A does not score in B's order.  *n_records = how many were written; the counts are exact
 * whatever max_records is.  ipkgpu_db_diff_time_ms: device time of the context's last call. */
int ipkgpu_db_diff(ipkgpu_ctx* ctx, const ipkgpu_db* a, const ipkgpu_db* b, double eps,
                   ipkgpu_db_diff_counts* counts, ipkgpu_db_diff_record* records, uint64_t max_records, uint64_t* n_records);
double ipkgpu_db_diff_time_ms(const ipkgpu_ctx* ctx);
/* DB_DIFF_CHUNK: the entries of a list the general path of ipkgpu_db_diff keeps in LDS at a time (tests build a longer list). */
uint32_t ipkgpu_db_diff_chunk(void);

/* ---- placement: the k-mers of query sequences looked up in a database on the device ---------------------------------------
 * What every consumer of a phylo-k-mer database does with it.  For a database of alphabet sigma and k-mer size k, the threshold
 * log_eps (ipkgpu_log_threshold of the database's omega) and a query q of n bytes:
 *   symbols    the database's code order (DNA ACGT, 2 bits; AA RHKDESTNQCGPAILMFWYV, 5 bits), either letter case, DNA U = T; every
 *              other byte (N, X, *, -, . included) is invalid
 *   windows    start s (0 <= s <= n - k) is valid iff its k bytes are; its code packs them, first symbol in the highest bits; W = the
 *              number of valid windows, every occurrence of a k-mer counting
 *   sums       S[b] = +0.0f, C[b] = 0; the valid windows in ASCENDING s: where the code is a key, for each of its entries (b, x)
 *              S[b] = S[b] + x in binary32 and C[b] += 1 -- a branch's scores are added in window order, as a sequential loop adds them
 *   score      for C[b] > 0: score[b] = S[b] + ((float)(W - C[b]) * log_eps), product and sum each rounded to binary32
 *   placements the branches with C[b] > 0 by score descending, then branch id ascending; the first keep_at_most of them
 *   lwr        (binary64) m = the best score, den = the sum of 10^((double)score[b] - (double)m) over ALL branches with C[b] > 0 (in any
 *              order), lwr[b] = 10^(score[b] - m) / den
 * Precondition: a key's entries name a branch at most once (every build of this library; checked on a database's first placement
 * call, IPKGPU_ERR_INVALID naming the key).  That first call also builds the database's prefix table (at most 2^16 + 1 lower bounds
 * into the key list) and finds the branch count; both stay with the database until ipkgpu_db_free.
 *   seqs, seq_off   host arrays: query i is bytes [seq_off[i], seq_off[i + 1]) of seqs
 * The queries go to the device in batches (option "place_batch_queries"; 0 = sized from what the device or "device_budget_bytes"
 * leaves), one wavefront per query (kernels_place.hpp); S and C live in LDS while the database has at most "place_lds_branches"
 * branches (0 = the default and the most, 4096), else in global tables -- the same bits either way.
 * IPKGPU_ERR_INVALID: sigma / k that are not the database's (codes of more than 32 bits, a key beyond sigma's k symbols, the head of
 * the file a database was loaded from), keep_at_most outside 1..64, a decreasing seq_off, a query of 2^32 bytes or more.
 * IPKGPU_ERR_NOMEM leaves the context usable.  ipkgpu_db_place places the strand given and treats ambiguous symbols as invalid bytes;
 * ipkgpu_db_place_opts (below) expands them and places both strands.  Not done here: jplace output. */
typedef struct ipkgpu_placements ipkgpu_placements;
int ipkgpu_db_place(ipkgpu_ctx* ctx, ipkgpu_db* db, uint32_t sigma, uint32_t k, float log_eps, const char* seqs, const uint64_t* seq_off,
                    uint64_t n_queries, uint32_t keep_at_most, ipkgpu_placements** out);
uint64_t ipkgpu_placements_num_queries(const ipkgpu_placements* p);
uint32_t ipkgpu_placements_keep(const ipkgpu_placements* p);
/* [num_queries][keep], best first; past a query's last placement: branch 0xFFFFFFFF, score 0, count 0, lwr 0 */
const uint32_t* ipkgpu_placements_branches(const ipkgpu_placements* p);
const float* ipkgpu_placements_scores(const ipkgpu_placements* p);
const uint32_t* ipkgpu_placements_counts(const ipkgpu_placements* p);    /* C[b]: the query's windows that scored the branch */
const double* ipkgpu_placements_lwr(const ipkgpu_placements* p);
/* [num_queries]: valid windows (W), those whose code is a key, branches with C > 0 */
const uint32_t* ipkgpu_placements_n_kmers(const ipkgpu_placements* p);
const uint32_t* ipkgpu_placements_n_found(const ipkgpu_placements* p);
const uint32_t* ipkgpu_placements_n_branches(const ipkgpu_placements* p);
/* milliseconds: 0 = the whole call on the host's clock, 1 = the index build (0 when the database had it), 2 = the placement kernels */
double ipkgpu_placements_time_ms(const ipkgpu_placements* p, int which);
void ipkgpu_placements_free(ipkgpu_placements* p);

/* ---- placement with options: ambiguous symbols expanded, both strands placed ----------------------------------------------
 * opts == NULL or {0, 0}: ipkgpu_db_place's result bit for bit (the same kernels), strand and n_ambiguous all zero.  Any other value
 * of either field, and strands = 1 with sigma = 20: IPKGPU_ERR_INVALID.  Every refusal of ipkgpu_db_place and its IPKGPU_ERR_NOMEM
 * contract carry over.
 *
 * ambiguity = 1.  Ambiguous symbols, either letter case, and their resolutions:
 *   DNA          R = AG   Y = CT   S = CG   W = AT   K = GT   M = AC   B = CGT   D = AGT   H = ACT   V = ACG   N = ACGT
 *   amino acids  B = DN   Z = EQ   J = IL   X = all 20
 * every other byte stays invalid.  A window is EXACT if its k bytes are plain symbols, AMBIGUOUS if k - 1 are plain and exactly one
 * is an ambiguous symbol, invalid otherwise.  W counts exact and ambiguous windows, n_ambiguous the ambiguous ones.  An ambiguous
 * window has R resolutions: its code with the ambiguous position replaced by each resolution, in ascending symbol code.  If any
 * resolution is a key, n_found grows by 1.  For every branch b named by at least one resolution's key, c = the number of resolutions
 * that name it:
 *     P = 0.0;  for the resolutions in ascending order that name b with score x:  P = P + 10^(double)x          (binary64)
 *     P = P + (double)(R - c) * E        E = 10^(double)log_eps, product and sum each rounded to binary64
 *     y = (float)log10(P / (double)R)    one rounding to binary32
 *     S[b] = S[b] + y;  C[b] += 1        at the window's own place in the ascending order of starts
 * -- the mean of the resolutions' probabilities, the threshold standing in for the resolutions that do not score the branch.  A
 * branch that no resolution names gets nothing from the window (the (W - C[b]) log_eps term covers it as it covers any window).
 * This definition is this library's own: it follows what the placement tools that read such databases do with a window of one
 * ambiguous symbol, and was not checked against their code.
 * 10^x and log10 are not the same functions bit for bit in every implementation: two implementations of this definition can differ
 * in the last bit of y where the binary64 value of log10(P / R) lies within their error of a binary32 rounding midpoint.
 *
 * strands = 1 (DNA only).  rc(q) is q reversed with A <-> T (U -> A), C <-> G, R <-> Y, K <-> M, B <-> V, D <-> H; S, W and N map to
 * themselves, every other byte stays as it is (an invalid byte stays invalid).  q and rc(q) are each placed by the whole
 * definition, independently.  The reverse strand is the query's result iff it has a placement and either the given strand has none
 * or its best score is greater (as floats); equal scores go to the given strand.  Every output of the query comes from the chosen
 * strand; strand[i] says which.
 * The device reads rc(q) out of the uploaded bytes of q; the per-window tables of ambiguous windows (16 bytes per branch and
 * workgroup) live in device memory and count against "device_budget_bytes" like the batch's other workspaces. */
typedef struct ipkgpu_place_options {
    uint32_t ambiguity;   /* 0: an ambiguous symbol is an invalid byte (ipkgpu_db_place). 1: expanded, above */
    uint32_t strands;     /* 0: the strand given. 1: both strands, DNA only */
} ipkgpu_place_options;
int ipkgpu_db_place_opts(ipkgpu_ctx* ctx, ipkgpu_db* db, uint32_t sigma, uint32_t k, float log_eps, const char* seqs,
                         const uint64_t* seq_off, uint64_t n_queries, uint32_t keep_at_most, const ipkgpu_place_options* opts,
                         ipkgpu_placements** out);
const uint8_t* ipkgpu_placements_strand(const ipkgpu_placements* p);        /* [num_queries] 0 = given, 1 = reverse complement */
const uint32_t* ipkgpu_placements_n_ambiguous(const ipkgpu_placements* p);  /* [num_queries] expanded (ambiguous) windows */

/* ---- placing on a database file that does not fit device memory: the queries' k-mer set, the restriction, the streamed load --------
 * Placement never reads a key that none of the queries' windows encodes.  So the database restricted to the codes the queries can
 * look up gives THE SAME PLACEMENTS BIT FOR BIT -- not a prefix of the file and not a re-ordered sum: every S[b] receives the same
 * scores in the same window order -- and a batch of 10^5 reads of 150 symbols names at most 1.5 * 10^7 codes whatever the file's size.
 *
 * The k-mer set K of (sigma, k, opts, queries): every code ipkgpu_db_place_opts with the same sigma, k and opts would pass to its lookup
 * for any of the queries -- the codes of the exact windows; with ambiguity = 1 every resolution of every ambiguous window; with
 * strands = 1 the same for rc(q).  Bytes, windows, letter case, U = T and the ambiguous symbols are those of the placement definition
 * above.  K is a bitmap on the device of 2^(bits per symbol * k) bits, bit `code` of 32-bit word code >> 5 (at least two words): 512 MiB
 * at DNA k = 16, 128 MiB at amino acids k = 6.  It counts against "device_budget_bytes" and shows in ipkgpu_mem_stats until it is freed.
 * One wavefront per query sets the bits with vector atomicOr (kernels_kmerset.hpp); the queries go up in the placement's batches
 * ("place_batch_queries").  Refusals are ipkgpu_db_place_opts': sigma / k, options, strands = 1 with sigma = 20, a decreasing
 * seq_off, a query of 2^32 bytes or more; IPKGPU_ERR_NOMEM leaves the context usable. */
typedef struct ipkgpu_kmer_set ipkgpu_kmer_set;
int ipkgpu_kmer_set_of_queries(ipkgpu_ctx* ctx, uint32_t sigma, uint32_t k, const char* seqs, const uint64_t* seq_off, uint64_t n_queries,
                               const ipkgpu_place_options* opts, ipkgpu_kmer_set** out);
uint64_t ipkgpu_kmer_set_count(const ipkgpu_kmer_set* set);          /* distinct codes */
uint64_t ipkgpu_kmer_set_num_words(const ipkgpu_kmer_set* set);      /* 32-bit words of the bitmap: max(2, 2^bits / 32) */
const uint32_t* ipkgpu_kmer_set_words(ipkgpu_kmer_set* set);         /* host copy of the bitmap, made on first use */
uint32_t ipkgpu_kmer_set_sigma(const ipkgpu_kmer_set* set);
uint32_t ipkgpu_kmer_set_k(const ipkgpu_kmer_set* set);
void ipkgpu_kmer_set_free(ipkgpu_kmer_set* set);

/* The restriction R(D, K) of a database to a k-mer set: the keys of D that are in K, each with ALL its entries in D's order (no score is
 * compared; a key in K stays even if D gives it no entry), positions if D has them.  Arrays by rule 4 of ipkgpu_db_select, the head by
 * rule 5.  A key at or beyond 2^bits is in no set: the bound is tested before the bitmap is read.  IPKGPU_ERR_INVALID: a D without
 * filter arrays (as ipkgpu_db_select), a set or D of another context, a set whose sigma / k are not those of the head of D's file.
 * Device work and memory: ipkgpu_db_select's, the candidate flags coming from the bitmap instead of the order. */
int ipkgpu_db_select_keys(ipkgpu_ctx* ctx, const ipkgpu_db* src, const ipkgpu_kmer_set* set, ipkgpu_db** out);

/* ipkgpu_db_select_keys(ipkgpu_db_load_select(path, keep_kmers, min_log_score), set) in every array (keys, offsets, entries,
 * positions, both filter value arrays, order) and in the head -- WITHOUT an image of the body, and without the database of the file:
 * the body goes through the two pinned buffers ("db_load_chunk_bytes"), the host walking every chunk, into a device window of
 * "db_load_window_bytes" (0 = 256 MiB, or the body if that is smaller), and only the wanted records stay (db_stream.hpp,
 * kernels_dbstream.hpp).  A window holds whole records: it is cut at a record start of the walk; one record longer than the window
 * grows the window to hold it, or the call returns IPKGPU_ERR_NOMEM.  Per window: db_unpack_heads_kernel, the wanted flags (the
 * bounded bitmap test: the key is the file's), two scans, the wanted heads and -- through db_unpack_entries_kernel -- the wanted
 * entries appended in file order.  Behind the last window: the sort of (key, kept record) with the duplicate-key check, the arrays in
 * key order, the entries moved from file order into key order by entry ranges; then ipkgpu_db_select at min_log_score over the kept
 * records.  keep_kmers stops the walk after that many records, as ipkgpu_db_load_select does, and reads no chunk behind them; with
 * keep_kmers at or beyond the header's total the walk must end at the end of the file with the header's totals, as in ipkgpu_db_load.
 * A file the walk refuses -- in whichever window -- is IPKGPU_ERR_INVALID; what was kept is freed and the context stays usable.
 * (Unlike the loads above, windows before the damage have been through the kernels by then: every one of their records was walked.)
 * Device memory at its peak, with W = the window's bytes, n_w = the most records of one window, and kept k-mers n_R and entries e_R
 * BEFORE min_log_score is applied (e = 8 bytes an entry, 12 with positions):
 *     bitmap (the caller's)  +  W + 32  +  60 n_w + 24 (the window's workspaces)  +  2 * (24 n_R + e e_R) (the kept arrays, in file
 *     order; they double when full, so up to twice their content)  +  the scans' own
 * and behind the last window, the window and its workspaces still held:
 *     kept arrays  +  R itself (28 n_R + 8 + e e_R, each array rounded up to 256 bytes)  +  20 n_R and the sort's own;
 * then R and the selection V with ipkgpu_db_select's workspaces.  Every temporary is given back before the call returns.
 * ipkgpu_db_load_time: as for the other loads, 6 = the host's time in the windows' device work and behind the last window (ms; each
 * window is waited for), 7 = body bytes read, and 8 = the number of windows, 9 = the records kept before min_log_score.
 * The duplicate-key check sees only the kept records, and so does the first placement's duplicate-branch check: damage of those
 * kinds in records the set does not name is NOT seen.  IPKGPU_ERR_INVALID as well: a set of another context, or whose sigma / k are
 * not the file's. */
int ipkgpu_db_load_wanted(ipkgpu_ctx* ctx, const char* path, const ipkgpu_kmer_set* set, uint64_t keep_kmers, float min_log_score,
                          ipkgpu_db** out);

/* ---- comparing database files that do not fit device memory, by key ranges ------------------------------------------------------------
 * The records of a file whose key lies in [key_lo, key_hi), key_lo <= key_hi <= 2^32 (else IPKGPU_ERR_INVALID): every kept key with
 * all its entries, a record without entries included -- the call makes no selection and drops no key.  Arrays and head by the rules of
 * ipkgpu_db_select_keys (keys ascending, filter values bit for bit, the order renumbered, the head's totals replaced).  It is the
 * streamed load of ipkgpu_db_load_wanted with a second predicate (db_stream_flag_range_kernel in place of the bitmap test): the same
 * windows, the same walk of the WHOLE file with its end-of-file and totals checks on every call, the same duplicate-key check over the
 * kept records, the same memory (no bitmap).  key_lo == key_hi: an empty database and IPKGPU_OK, the file walked and checked all
 * the same. */
int ipkgpu_db_load_key_range(ipkgpu_ctx* ctx, const char* path, uint64_t key_lo, uint64_t key_hi, ipkgpu_db** out);

/* ipkgpu_db_diff(ipkgpu_db_load(path_a), ipkgpu_db_load(path_b), eps, ...) field for field and bit for bit -- positions_differ, the
 * bits of max_abs_diff and the order of the records included -- with neither file ever resident whole (db_diff_files.hpp).
 * A comparison composes exactly over disjoint ascending key ranges: every count adds, max_abs_diff is the maximum, the record list is
 * the concatenation.  Per range: A's range and B's range through the key-range load, ipkgpu_db_diff, the counts added, the records
 * appended until max_records is reached OVER ALL ranges (the counts stay exact behind that), both range databases freed.
 *
 * The plan.  avail = what "device_budget_bytes" leaves beside what the context holds, without a budget the device's free memory; the
 * context's cached result blocks and the workspaces ipkgpu_db_diff and the scans cache are given back first, after every range and
 * when the call returns.  If range_bytes (below) at the two heads' totals is at most avail there is ONE range [0, 2^32) and each file
 * is read once.  Otherwise one HISTOGRAM PASS over each file: streamed as a load that keeps nothing, per window
 * db_unpack_heads_kernel and db_stream_hist_kernel (kernels_dbstream.hpp), which adds 1 to rec_hist[bin] (u32) and the record's
 * entry count to ent_hist[bin] (u64) with integer vector atomics; 65 536 bins of each, bin = min(key >> shift, 65535),
 * shift = max(0, bits - 16), bits = min(32, bits per symbol * k) of the file's head -- the larger of the two files', 32 for a sequence
 * type that is neither DNA nor AA.  The pass also yields n_w, the most records of one window, and L, the longest record's bytes.
 * The ranges are then cut greedily from bin 0 upward: a range is closed before the first bin whose addition would take range_bytes
 * beyond avail; one bin may be a range of its own; one bin that alone exceeds avail is IPKGPU_ERR_NOMEM before any range is loaded,
 * the message naming the bin's key interval and the bytes it needs.  The first range starts at key 0 and the LAST ENDS AT 2^32
 * whatever the head says, so a record whose key lies beyond the code space is compared like any other.
 *
 * The window.  "db_load_window_bytes" if set; else avail / 16, at least 4 KiB and at most 256 MiB -- with 60 bytes of workspace per
 * record of at least 16 bytes the fixed part below then stays under a third of avail whatever the files hold.  Per file the window is
 * at most its body.  Every pass over a file uses the same window, so the cuts, n_w and L are the same on every pass.
 *
 * Device memory, a true upper bound of what ipkgpu_mem_stats counts.  m(x) = max(x, 256): a block of the streamed load;
 * r(x) = max(x rounded up to 256, 256): an array of a database; sort(n) = 9 n + 32768 and scan(n) = n / 8 + 4096 bound rocprim's own
 * space (the n keys again, digit counters and one look-back state per digit and block; 16 bytes per block of a scan);
 * scanx(n) = scan(n) * 17 / 16 + 16, for the scans' workspace may be regrown with ensure's margin; pos = 1 for a positioned file.
 *   ipkgpu_db_stream_window_bytes(W, n_w, L), the fixed part of one file's passes:
 *       W + 32  +  (L > W ? L + 32 : 0)   the window; a longer record grows it, the old block alive during the copy
 *       + 3 m(8 n_w) + 4 m(4 n_w) + 3 m(8 (n_w + 1))  +  scanx(n_w + 1)          the per-record workspaces and the windows' scans
 *     Before a histogram pass n_w and L are bounded from the head: n_w <= min(total k-mers, max(W / 16, 1)),
 *     L <= min(body, 16 + (8 or 10) * total entries).  fixed = the larger of the two files' figures (one file is streamed at a time).
 *   db(n, e)    = 3 r(4 n) + r(8 (n + 1)) + r(8 n) + r(8 e) + pos r(4 e)           a resident database
 *   load(n, e)  = 2 m(8 n) + 2 m(4 n) + m(8 e) + pos m(4 e)                        the kept arrays at their exact size
 *                 + db(n, e)  +  2 m(8 n) + m(4 n) + m(sort(n))                    behind the last window: the result and the sort
 *   ipkgpu_db_diff_files_range_bytes(fixed, n_A, e_A, pos_A, n_B, e_B, pos_B, max_records) =
 *       max( fixed + load(n_A, e_A),   fixed + db(n_A, e_A) + load(n_B, e_B),
 *            db(n_A, e_A) + db(n_B, e_B) + 8 max(n_A, 1) + 8 (n_A + 1) + 8 max(n_B, 1) + 8 (n_B + 1) + 64 (each workspace 16 at least)
 *                         + r(16 min(max_records, e_A + e_B)) )                    ipkgpu_db_diff's workspaces and its records
 *       + scanx(max(n_A, n_B) + 1)
 * The whole call stays below max over the ranges of range_bytes, and during a histogram pass below
 *       786 432 (the two histograms)  +  W + 32 + (L > W ? L + 32 : 0) + 2 m(8 n_w) + 2 m(4 n_w).
 * The histograms are counted by ipkgpu_mem_stats but taken BESIDE "device_budget_bytes": their size does not depend on the files, and a
 * budget smaller than they are can still be planned.  With expected counts from the histograms every block of a range's loads is
 * allocated once at its exact size (the kept arrays of ipkgpu_db_load_wanted double when full, up to three times their content while a
 * copy is in flight); a file that then holds more records or entries in a range than were counted "changed between passes":
 * IPKGPU_ERR_INVALID, and nothing is written past an allocation.
 *
 * Cost: 1 pass over each file when one range fits, else 1 + (number of ranges) passes; a pass is one streamed read of the whole body
 * with the host's walk, which bounds it.  IPKGPU_ERR_INVALID as in the streamed load: a file the walk refuses (naming the record), a
 * key in two records of one range, a changed file; on every error everything is given back and the context stays usable.
 * The last call of a context: ipkgpu_db_diff_files_num_ranges and _range (each range's [lo, hi)); ipkgpu_db_diff_files_stat:
 * 0 = seconds in all, 1 = in the histogram passes, 2 = in the range loads, 3 = device ms in the diffs (ipkgpu_db_diff_time_ms gives
 * the same sum), 4 = body bytes read, 5 / 6 = passes over A's / B's body, 7 = seconds in the host's walk, 8 = the window's bytes,
 * 9 = avail, 10 = n_w, 11 = L.  ipkgpu_db_stream_window_bytes and ipkgpu_db_diff_files_range_bytes are host arithmetic (no GPU). */
uint64_t ipkgpu_db_stream_window_bytes(uint64_t window, uint64_t n_w, uint64_t longest);
uint64_t ipkgpu_db_diff_files_range_bytes(uint64_t fixed, uint64_t n_a, uint64_t e_a, int positioned_a, uint64_t n_b, uint64_t e_b,
                                          int positioned_b, uint64_t max_records);
int ipkgpu_db_diff_files(ipkgpu_ctx* ctx, const char* path_a, const char* path_b, double eps, ipkgpu_db_diff_counts* counts,
                         ipkgpu_db_diff_record* records, uint64_t max_records, uint64_t* n_records);
uint64_t ipkgpu_db_diff_files_num_ranges(const ipkgpu_ctx* ctx);
int ipkgpu_db_diff_files_range(const ipkgpu_ctx* ctx, uint64_t i, uint64_t* key_lo, uint64_t* key_hi);
double ipkgpu_db_diff_files_stat(const ipkgpu_ctx* ctx, int which);

/* ---- the union of databases with disjoint key sets, on the device ------------------------------------------------------------------------
 * Shards of several ranks (key % P), the files of key-range passes and the batches of an on-disk build are databases with disjoint
 * key sets.  ipkgpu_db_union makes one ordinary database of n_srcs of them (db_union.hpp, kernels_dbunion.hpp): every accessor,
 * ipkgpu_db_write, ipkgpu_db_select, ipkgpu_db_diff and ipkgpu_db_place take it.  The sources belong to ctx, each carries filter
 * values and an order (loaded from a file, or filtered by ipkgpu_db_filter_mif0 / _random), all have positions or none has; they are
 * only read and stay valid.  The result U:
 *   keys        ascending;  key_offsets;  a key's entries and positions bit for bit and in their source's order;
 *   fv32, fv64  bit for bit the source's (nothing is recomputed);
 *   order       the keys sorted by the filter stage's own sort key: the order-preserving code of the float32 value, then the key
 *               (filter_sortkey_kernel; dbfile.filter_sort_code);
 *   head        ipkgpu_db_header_of(U) is NULL.
 * THE CONDITION under which ipkgpu_db_write(U) equals ipkgpu_db_merge_files of the sources' files byte for byte: every source is itself
 * in that order -- order[i] of each source ascends by (code of fv32, key), as the filter calls leave it and as a file written from such a
 * database holds it.  The host's P-way merge hands the records of such sources out by exactly that key.  A source in another order
 * (a hand-made file) is still united, its own record order is not kept, and the two files then differ.
 * IPKGPU_ERR_INVALID with a message, before anything is allocated that outlives the call: n_srcs = 0, a null source, a source of
 * another context, a source without filter values, a mixture of positioned and plain sources (in ipkgpu_db_merge_files' wording),
 * more than 2^32 - 1 keys in all, and a key present in two sources -- the message names the key and both source indices; it is found
 * behind the key sort and before any entry moves (ipkgpu_db_join below takes such sources).  n_srcs = 1 gives a copy.
 * Device work: (key << 32 | concatenated index) sorted with the loader's radix sort; per sorted position the source (a search over the
 * n_srcs + 1 prefix values of a table in device memory, n_srcs unbounded), key, filter values, entry count and entry start; a scan of
 * the counts; the entries copied by ENTRY ranges of 1024 per workgroup (as ipkgpu_db_load's and the selection's copies: a key of one
 * entry and one of thousands cost alike); the order by the filter stage's sort.  No output position comes from an atomic: the same bits
 * on every run.
 * Device memory: everything goes through the context's accounting (ipkgpu_mem_stats, "device_budget_bytes"); the workspace is taken for
 * the call and given back before it returns.  ipkgpu_db_union_bytes(n, e, S, pos) -- n keys and e entries in all, S sources -- is a true
 * upper bound of what the call holds on top of its sources, host arithmetic (no GPU); with r, sort and scan as defined for
 * ipkgpu_db_diff_files_range_bytes above and m(x) = max(x, 256):
 *       3 r(4 n) + r(8 (n + 1)) + r(8 n) + r(8 e) + pos r(4 e)        the result
 *     + m(56 (S + 1))                                                 the source table
 *     + 3 m(8 n) + 2 m(4 n)                                           sort keys unsorted and sorted, entry starts; source indices, counts
 *     + m(sort(n)) + m(scan(n + 1)) + 256                             rocprim's own, the duplicate index
 * What does not fit is IPKGPU_ERR_NOMEM and leaves the context usable and the sources intact.
 * ipkgpu_db_union_time_ms, the context's last union, device ms: 0 = all, 1 = key sort (sort keys to key_offsets), 2 = entry copy,
 * 3 = order sort.  Option "union_copy_bytes" (ipkgpu_set_option): 0 = the default, 16 -- a lane copies two entries and stores them as
 * one 16-byte word; 8: one entry per store.  Both forms give the same bits (the 16-byte form was the faster one where measured). */
int ipkgpu_db_union(ipkgpu_ctx* ctx, const ipkgpu_db* const* srcs, uint32_t n_srcs, ipkgpu_db** out);
uint64_t ipkgpu_db_union_bytes(uint64_t n_keys, uint64_t n_entries, uint32_t n_srcs, int positioned);
double ipkgpu_db_union_time_ms(const ipkgpu_ctx* ctx, int which);
/* ipkgpu_db_merge_files on the device: every path loaded with ipkgpu_db_load (its refusals pass through), the sources united and freed,
 * the union written under header `h` with the streamed device writer (ipkgpu_db_write) and freed; the out-parameters are
 * ipkgpu_db_merge_files'.  IPKGPU_ERR_INVALID naming the file: a source whose sequence type, k-mer size or omega bits are not h's, or
 * whose positions flag is not the first source's.  All sources and the union are resident together: what does not fit is
 * IPKGPU_ERR_NOMEM -- the call does not fall back to the host merge by itself, its callers decide. */
int ipkgpu_db_union_files(ipkgpu_ctx* ctx, const ipkgpu_db_header* h, const char* const* paths, uint32_t n_paths, const char* path,
                          uint64_t* total_kmers, uint64_t* total_entries, uint64_t* bytes_written);

/* ---- the join of databases that share k-mers, on the device --------------------------------------------------------------------------------
 * Databases built over DIFFERENT BRANCH GROUPS of one tree (branch shards: `ipk.py build --group-range`, one job of an array each) hold
 * the same k-mers with different branches.  ipkgpu_db_union refuses them; ipkgpu_db_join makes one ordinary database of n_srcs of them
 * (db_join.hpp, kernels_dbjoin.hpp) by the rule with which the reference merges pieces of groups, `put` (branch_group.cpp:88-101,
 * db_builder.cpp:392-458).  The sources belong to ctx and all have positions or none has; they need NO filter values and no order (a
 * fresh ipkgpu_db_from_parts / ipkgpu_merge_parts result serves as a loaded file does); within one source a key's entries have distinct
 * branches, as in every database the engine makes or loads for placement.  They are only read and stay valid.  The result J:
 *   keys        the set union of the sources' keys, ascending;  key_offsets goes with it;
 *   entries     of key K: (1) the entries of K in source 0, 1, ..., S - 1, each in its source's order, concatenated; (2) of a branch
 *               that occurs more than once ONE entry stays, at the place of its first occurrence; (3) its score: walking the
 *               occurrences in order, a later one replaces the kept score only if it is strictly greater (`>` on the floats: equal
 *               scores, -0.0 against +0.0 and a NaN keep the earlier one); (4) its window position is the kept score's;
 *               a key without entries in every source that holds it stays a record without entries;
 *   fv32, fv64, order, head     none (ipkgpu_db_header_of(J) is NULL): the caller runs ipkgpu_db_filter_mif0 or _random on J as on any
 *               merged database; then ipkgpu_db_write, _select, _diff, _place and _union take it.
 * Disjoint key sets are a special case: keys, offsets, entries and positions are ipkgpu_db_union's.
 * WHY THE JOIN OF GROUP RANGES IS THE WHOLE BUILD: a build leaves a key's entries in group order; ipkgpu_db_filter_mif0 adds the
 * entries' terms in entry order; the random filter draws per k-mer code.  Shards of CONTIGUOUS ranges of the group order, joined in range
 * order and filtered with the whole tree's N, therefore give the one-call build's file byte for byte (another order of the sources gives
 * the same keys and counts and another entry order).
 * IPKGPU_ERR_INVALID with a message, before anything is allocated that outlives the call: n_srcs = 0, a null source, a source of
 * another context, a mixture of positioned and plain sources (ipkgpu_db_union's wording), more than 2^32 - 1 keys in all sources (the
 * sort's low word is the concatenated key index; the result holds no more), more entries than one launch covers (2^39 - 256).
 * Device work.  A RUN is one source's record of one key.  (key << 32 | concatenated key index) sorted with the loader's radix sort:
 * the runs of a key then stand side by side in source order.  Segment heads give J's keys; a scan of the head flags numbers them, a
 * scan of the runs' counts gives every run's -- and at the heads every key's -- offset in the CONCATENATED layout.  The entries are
 * copied by ENTRY ranges of 1024 per workgroup with the union's copy kernel, its "keys" being the runs: a lane searches (sorted
 * position, source run).  Whether duplicates can exist is decided from the sources: some key must have two runs, and a table of
 * 2^18 slots (branch mod 2^18), filled with the smallest and the largest source that holds a branch of the slot, must show a slot
 * with two sources (never wrong towards "none"; branch ids below 2^18 make it exact).  If they cannot, the copy goes straight into J
 * (route 0).  Else (route 1) it goes into a workspace and every joined list is resolved where it lies: up to 64 entries by one wavefront,
 * lane against lane; up to 4096 by a workgroup that sorts (branch, index) in LDS and walks each run of equal branches; longer ones by a
 * radix sort of ((key index << 32 | branch), entry index) pairs over the layout and the same walk.  The kept flags are scanned and the
 * kept entries, positions and key offsets compacted into J.  No output position comes from an atomic: the same bits on every run.
 * Option "join_route" (ipkgpu_set_option): 0 = decide as above; 1 = always resolve; 2 = decide, and IPKGPU_ERR_INVALID if a duplicate
 * exists -- the message names a key, a branch and the two sources that hold it -- for callers who expect branch-disjoint shards.
 * Routes 0 and 1 give the same bits.
 * Device memory: everything goes through the context's accounting (ipkgpu_mem_stats, "device_budget_bytes"); the workspace is taken for
 * the call and given back before it returns.  ipkgpu_db_join_bytes(n, e, S, pos) -- n keys and e entries IN ALL SOURCES, S sources -- is
 * a true upper bound of what the call holds on top of its sources, host arithmetic (no GPU); r, sort, scan and m as for
 * ipkgpu_db_union_bytes:
 *       r(4 max(n, 1)) + r(8 (n + 1)) + r(8 max(e, 1)) + pos r(4 max(e, 1))     the result (it has no filter arrays)
 *     + m(56 (S + 1)) + m(8 (S + 1))                                            the source table, the sources' entry prefix
 *     + 3 m(8 n) + 3 m(4 n) + 2 m(8 (n + 1))          sort keys unsorted and sorted, entry starts; sources, counts, head flags; the two scans
 *     + m(sort(n)) + m(scan(max(n, e) + 1)) + 256 + 2 m(4 * 2^18)               rocprim's own, the counters, the branch table
 *     + m(8 (n + 1)) + m(8 e) + pos m(4 e) + m(4 e) + m(8 (e + 1)) + m(4 (e / 65 + 1))
 *                                       route 1: concatenated offsets, entries, positions; kept flags and their scan; the long lists
 *     + (e > 4096 ?  4 m(8 e) + m(17 e + 32768)  :  0)                          the sorted pass, taken only for a list beyond 4096
 * What does not fit is IPKGPU_ERR_NOMEM and leaves the context usable and the sources intact.
 * ipkgpu_db_join_stat, the context's last join: 0 = device ms in all, 1 = key stage (sort keys to the offsets), 2 = entry copy,
 * 3 = duplicate stage (resolution, scan and compaction), 4 = J-keys found in more than one source, 5 = entries dropped as duplicates,
 * 6 = route taken (0 concatenation only, 1 duplicates resolved). */
int ipkgpu_db_join(ipkgpu_ctx* ctx, const ipkgpu_db* const* srcs, uint32_t n_srcs, ipkgpu_db** out);
uint64_t ipkgpu_db_join_bytes(uint64_t keys_in_all, uint64_t entries_in_all, uint32_t n_srcs, int positioned);
double ipkgpu_db_join_stat(const ipkgpu_ctx* ctx, int which);

/* ---- joining branch shards that do not fit device memory, by key ranges ---------------------------------------------------------------------
 * ipkgpu_db_join_files writes to out_path, byte for byte, the file that loading every path (ipkgpu_db_load), ipkgpu_db_join in the order
 * of `paths`, ipkgpu_db_filter_mif0(J, total_num_groups, threshold) (filter = 0) or ipkgpu_db_filter_random(J) (filter = 1) and
 * ipkgpu_db_write(J) under `h` write -- with no shard and no whole join ever resident (db_join_files.hpp).
 * WHY IT COMPOSES: a key's joined list depends on that key's runs alone; MIF0 works per k-mer with the caller's N and the random filter
 * draws per k-mer code, so filtering the join of a key range gives the values the whole join would; the files of disjoint key ranges,
 * each in filter order, are merged by ipkgpu_db_merge_files into the bytes of the whole (the argument of the key-range build).
 *
 * Head checks, before any pass: IPKGPU_ERR_INVALID naming the file whose sequence type, k-mer size or omega bits are not h's, or whose
 * positions flag is not the first file's (ipkgpu_db_union_files' wording).
 *
 * The plan is ipkgpu_db_diff_files', rule for rule, for S files in place of two.  avail = what "device_budget_bytes" leaves beside what
 * the context holds, else the device's free memory; the context's cached result blocks and workspaces are given back first, after every
 * range and on every return.  The window: "db_load_window_bytes", else avail / 16 clamped to 4 KiB .. 256 MiB, per file at most its
 * body.  If range_bytes (below) at the heads' totals is at most avail -- or no shard holds a record -- there is ONE range [0, 2^32): no
 * histogram pass, and the range is written straight to out_path (no range file, no directory, no host merge).  Otherwise one histogram
 * pass per shard (db_stream_hist_kernel, 65 536 bins, shift = max(0, bits - 16)); one pair of device histograms is alive at a time,
 * taken beside the budget, and copied to the host with the pass's n_w and L.  The ranges are cut greedily from bin 0 upward: a range is
 * closed before the first bin whose addition would take range_bytes beyond avail; a bin that alone exceeds avail is IPKGPU_ERR_NOMEM
 * before any range is loaded, the message naming the bin's key interval, the records and entries of every shard in it and the bytes
 * needed.  The first range starts at 0, the last ends at 2^32.  (Every range of such a cut holds the bin that opened it, so it has a
 * record; a range without one would be skipped: no load passes, no file.)
 *
 * Per range, ascending: for s = 0 .. S - 1 the key-range load of shard s with the counts expected from the histograms (more or fewer
 * found: "the file changed between passes", IPKGPU_ERR_INVALID); ipkgpu_db_join over the S range databases in the order of `paths`,
 * "join_route" honoured (a refusal of route 2 passes through with its message); the sources freed; the filter; the device writer into
 * tmp_dir/range_%05u.ipk under `h`; J freed, everything cached given back.  Then ipkgpu_db_merge_files(h, range files) into out_path;
 * the range files are removed, and tmp_dir too if the call created it (tmp_dir NULL: "<out_path>.ranges").  On every error the range
 * files, a directory the call created and an output it began are removed, everything on the device is given back and the context
 * stays usable.
 *
 * The writer's staging.  ipkgpu_db_write stages through two device buffers of min(256 MiB, body); here the piece is
 * write_piece = avail / 16 clamped to 64 KiB .. 256 MiB, raised to longest_joined, a bound of the longest joined record:
 * 16 + sum over s of (L_s - 16), L_s the longest record of shard s as its histogram pass saw it (0 for a shard without records); on
 * the one-range shortcut L_s <= min(body, 16 + (8 or 10) * total entries) from the head.  The bytes written do not depend on the piece.
 *
 * Device memory, a true upper bound of what ipkgpu_mem_stats counts, from the terms defined for ipkgpu_db_diff_files_range_bytes
 * (m, r, sort, scanx, db, load), ipkgpu_db_stream_window_bytes and ipkgpu_db_join_bytes.  fixed = the largest of the S files'
 * ipkgpu_db_stream_window_bytes; N = sum n_s, E = sum e_s (J holds no more: duplicates only shrink it); body = 16 N + (8 or 10) E:
 *   ipkgpu_db_join_files_range_bytes(fixed, S, n[], e[], pos, write_piece, longest_joined) =
 *       max( max over s of  fixed + sum over t < s of db(n_t, e_t) + load(n_s, e_s),                          the loads
 *            sum over s of db(n_s, e_s) + ipkgpu_db_join_bytes(N, E, S, pos),                                 the join
 *            db(N, E) + 2 max(8 N, 16) + max(sort(N), 16),                                      the filter: two key arrays, the sort
 *            db(N, E) + m(4 N) + m(8 (N + 1)) + 2 r(min(max(write_piece, longest_joined), body)) )    the write: sizes, offsets, staging
 *       + scanx(N + 1)
 * The whole call stays below the maximum of range_bytes over the ranges, and during a histogram pass below the figure given for
 * ipkgpu_db_diff_files.
 *
 * Cost: S passes when one range fits, else S * (1 + R) for R ranges; a pass is one streamed read of a whole body with the host's walk,
 * which bounds it; plus, with R ranges, one more write and read of the output (the range files and the host merge, which holds one open
 * file and one 4-MiB buffer per range).
 * The last call of a context, a refused one included: ipkgpu_db_join_files_num_ranges and _range; ipkgpu_db_join_files_stat: 0 = seconds in all, 1 = in the
 * histogram passes, 2 = in the range loads, 3 = device ms in the joins (sum), 4 = body bytes read, 5 = passes over a body (all shards),
 * 6 = seconds in the host's walk, 7 = seconds in filter and range writes, 8 = seconds in the final host merge, 9 = window bytes,
 * 10 = avail, 11 = J-keys found in more than one source (sum; exact, the ranges are key-disjoint), 12 = entries dropped (sum),
 * 13 = ranges that took route 1, 14 = the most device bytes the ranges held above what the context held when the call began (what
 * range_bytes bounds; ipkgpu_mem_stats' peak also sees the histograms).  ipkgpu_db_join_files_range_bytes is host arithmetic (no GPU). */
int ipkgpu_db_join_files(ipkgpu_ctx* ctx, const ipkgpu_db_header* h, const char* const* paths, uint32_t n_paths, int filter,
                         uint64_t total_num_groups, float threshold, const char* out_path, const char* tmp_dir, uint64_t* total_kmers,
                         uint64_t* total_entries, uint64_t* entries_dropped, uint64_t* bytes_written);
uint64_t ipkgpu_db_join_files_range_bytes(uint64_t fixed, uint32_t n_srcs, const uint64_t* n, const uint64_t* e, int positioned,
                                          uint64_t write_piece, uint64_t longest_joined);
uint64_t ipkgpu_db_join_files_num_ranges(const ipkgpu_ctx* ctx);
int ipkgpu_db_join_files_range(const ipkgpu_ctx* ctx, uint64_t i, uint64_t* key_lo, uint64_t* key_hi);
double ipkgpu_db_join_files_stat(const ipkgpu_ctx* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif /* IPKGPU_H */
