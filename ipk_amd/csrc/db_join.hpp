// db_join.hpp -- ipkgpu_db_join: N databases whose key sets may overlap made one on the device, the entries of a shared key joined by the
// reference's `put` (included by ipkgpu.hip behind db_union.hpp, whose workspace blocks and source table it shares; kernels_dbjoin.hpp).
//
// The host's part: the refusals, the source table, the workspace, and the sequence
//   db_union_sortkey_kernel -> radix sort of (key, concatenated index)             the union's
//   db_join_runs_kernel -> scans of the head flags and of the counts               the runs, their J-keys, the concatenated offsets
//   db_join_branch_owner_kernel -> db_join_branch_shared_kernel                    can the sources hold a duplicate?  ("join_route" = 0, 2)
//   the counts read back; then EITHER (route 0, concatenation only)
//   db_join_keys_kernel, db_union_entries16_kernel straight into the result
//   OR (route 1, duplicates resolved)
//   db_join_keys_kernel, db_union_entries16_kernel into a concatenated workspace
//   db_join_dups_wave_kernel [-> db_join_dups_lds_kernel] [-> db_join_sortpair_kernel, radix sort of pairs, db_join_dups_sorted_kernel]
//   scan of the keep flags -> the kept count read back -> db_join_compact_kernel, db_join_offsets_kernel into the result
// Every byte of workspace is taken with dev_malloc for this call and given back before it returns.
#pragma once

namespace {

int join_alloc_arrays(ipkgpu_ctx* ctx, ipkgpu_db* db, uint64_t n, uint64_t ne, bool positioned)
{
    db->n_keys = n; db->n_entries = ne;
    hipError_t e = ctx_alloc(ctx, (void**)&db->d_keys, std::max<uint64_t>(n, 1) * 4);
    if (e == hipSuccess) e = ctx_alloc(ctx, (void**)&db->d_key_off, (n + 1) * 8);
    if (e == hipSuccess) e = ctx_alloc(ctx, (void**)&db->d_entries, std::max<uint64_t>(ne, 1) * 8);
    if (e == hipSuccess && positioned) e = ctx_alloc(ctx, (void**)&db->d_positions, std::max<uint64_t>(ne, 1) * 4);
    if (e == hipSuccess) return IPKGPU_OK;
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "no room for the join's arrays (%llu k-mers, %llu entries): %s",
                (unsigned long long)n, (unsigned long long)ne, hipGetErrorString(e));
}

// rocprim's own space for a sort of n (64-bit key, 64-bit value) pairs: both arrays again and the counters
inline uint64_t dj_sort_pairs(uint64_t n) { return 17 * n + 32768; }
// the result without filter values and order
inline uint64_t dj_db(uint64_t n, uint64_t e, bool pos) { return df_r(4 * std::max<uint64_t>(n, 1)) + df_r(8 * (n + 1)) + df_r(8 * std::max<uint64_t>(e, 1)) + (pos ? df_r(4 * std::max<uint64_t>(e, 1)) : 0); }

}  // namespace

extern "C" {

uint64_t ipkgpu_db_join_bytes(uint64_t keys_in_all, uint64_t entries_in_all, uint32_t n_srcs, int positioned)
{
    const uint64_t n = keys_in_all, e = entries_in_all;
    const bool pos = positioned != 0;
    const uint64_t keys_ws = du_m(sizeof(DbUnionSrc) * ((uint64_t)n_srcs + 1)) + du_m(8 * ((uint64_t)n_srcs + 1)) + 3 * du_m(8 * n) + 3 * du_m(4 * n) +
                             2 * du_m(8 * (n + 1)) + du_m(df_sort(n)) + du_m(df_scan(std::max(n, e) + 1)) + 256 + 2 * du_m(4 * (uint64_t)DB_JOIN_BRANCH_SLOTS);
    const uint64_t dup_ws = du_m(8 * (n + 1)) + du_m(8 * e) + (pos ? du_m(4 * e) : 0) + du_m(4 * e) + du_m(8 * (e + 1)) + du_m(4 * (e / (DB_JOIN_WAVE_LIST + 1) + 1)) +
                            (e > DB_JOIN_LDS_LIST ? 4 * du_m(8 * e) + du_m(dj_sort_pairs(e)) : 0);
    return keys_ws + dup_ws + dj_db(n, e, pos);
}

double ipkgpu_db_join_stat(const ipkgpu_ctx* ctx, int which) { return ctx && which >= 0 && which < 7 ? ctx->join_stat[which] : 0; }

int ipkgpu_db_join(ipkgpu_ctx* ctx, const ipkgpu_db* const* srcs, uint32_t n_srcs, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!out) return fail(ctx, IPKGPU_ERR_INVALID, "null out pointer");
    if (n_srcs == 0 || !srcs) return fail(ctx, IPKGPU_ERR_INVALID, "a join needs at least one source database");
    uint64_t n = 0, ne = 0;
    for (uint32_t s = 0; s < n_srcs; ++s) {
        const ipkgpu_db* d = srcs[s];
        if (!d) return fail(ctx, IPKGPU_ERR_INVALID, "source %u of the join is null", s);
        if (d->ctx != ctx) return fail(ctx, IPKGPU_ERR_INVALID, "source %u of the join belongs to another context", s);
        if ((d->d_positions != nullptr) != (srcs[0]->d_positions != nullptr))
            return fail(ctx, IPKGPU_ERR_INVALID, "positioned and plain shards cannot be merged into one database: source %u %s source 0 %s", s,
                        d->d_positions ? "has positions," : "has none,", srcs[0]->d_positions ? "has" : "has none");
        n += d->n_keys; ne += d->n_entries;
    }
    // (the sort's low word is the concatenated key index, so the bound is on the sources' keys in all; the result holds no more)
    if (n > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%llu k-mers in all: a database holds at most 2^32 - 1 (its order is 32-bit)", (unsigned long long)n);
    if ((ne + 255) / 256 > 0x7FFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "too many entries for one launch");
    const bool positioned = srcs[0]->d_positions != nullptr;
    const int64_t route_opt = ctx->opt_join_route;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (double& t : ctx->join_stat) t = 0;

    std::vector<DbUnionSrc> h_table(n_srcs + (size_t)1);
    std::vector<uint64_t> h_efirst(n_srcs + (size_t)1);
    uint64_t first = 0, efirst = 0;
    for (uint32_t s = 0; s < n_srcs; ++s) {
        const ipkgpu_db* d = srcs[s];
        h_table[s] = DbUnionSrc{d->d_keys, d->d_key_off, d->d_entries, d->d_positions, nullptr, nullptr, first};
        h_efirst[s] = efirst;
        first += d->n_keys; efirst += d->n_entries;
    }
    h_table[n_srcs] = DbUnionSrc{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, first};
    h_efirst[n_srcs] = efirst;

    UnionBlocks ws{ctx, {}};                                  // (declared before the result's guard: it waits, then the result goes)
    ipkgpu_db* db = new (std::nothrow) ipkgpu_db();
    if (!db) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    db->ctx = ctx;
    struct Guard { ipkgpu_ctx* c; ipkgpu_db* r; ~Guard() { if (r) { (void)hipStreamSynchronize(c->stream); ipkgpu_db_free(r); } } } guard{ctx, db};
    Stopwatch sw(ctx->stream, &ctx->events);
    const int e0 = sw.mark();
    int e1 = e0, e2 = e0, e3 = e0, e4 = e0;
    uint64_t n_shared = 0, n_dropped = 0;
    int route = 0;
    if (n == 0) {
        RC_TRY(join_alloc_arrays(ctx, db, 0, 0, positioned));
        HIP_TRY(ctx, hipMemsetAsync(db->d_key_off, 0, 8, ctx->stream));
    } else {
        DbUnionSrc* d_table = nullptr;
        uint64_t *d_efirst = nullptr, *d_start = nullptr, *d_hpos = nullptr, *d_run_off = nullptr;
        unsigned long long *d_sk = nullptr, *d_sorted = nullptr;
        uint32_t *d_src = nullptr, *d_cnt = nullptr, *d_head = nullptr, *d_counters = nullptr, *d_lo = nullptr, *d_hi = nullptr;
        void *d_sort_tmp = nullptr, *d_scan_tmp = nullptr;
        size_t sort_bytes = 0, scan_bytes = 0;
        const uint64_t scan_items = std::max(n, ne) + 1;
        HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, sort_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        {
            const auto query_in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), ScanU32In{nullptr, scan_items - 1});
            HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, query_in, d_hpos, (uint64_t)0, (size_t)scan_items, rocprim::plus<uint64_t>(), ctx->stream));
        }
        // out[0 .. m] = the exclusive scan of in[0 .. m), out[m] the total (m + 1 <= scan_items; rocprim's space grows with the item count)
        auto scan = [&](const uint32_t* in, uint64_t m, uint64_t* to) -> hipError_t {
            const auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), ScanU32In{in, m});
            size_t need = 0;
            hipError_t e = rocprim::exclusive_scan(nullptr, need, it, to, (uint64_t)0, (size_t)(m + 1), rocprim::plus<uint64_t>(), ctx->stream);
            if (e != hipSuccess) return e;
            if (need > scan_bytes) return hipErrorInvalidValue;
            return rocprim::exclusive_scan(d_scan_tmp, need, it, to, (uint64_t)0, (size_t)(m + 1), rocprim::plus<uint64_t>(), ctx->stream);
        };
        const bool ask_branches = n_srcs > 1 && route_opt != 1 && ne > 0;
        RC_TRY(ws.take(&d_table, sizeof(DbUnionSrc) * h_table.size(), "source table"));
        RC_TRY(ws.take(&d_efirst, 8 * h_efirst.size(), "entry prefix"));
        RC_TRY(ws.take(&d_sk, 8 * n, "sort keys"));
        RC_TRY(ws.take(&d_sorted, 8 * n, "sorted keys"));
        RC_TRY(ws.take(&d_start, 8 * n, "entry starts"));
        RC_TRY(ws.take(&d_src, 4 * n, "source indices"));
        RC_TRY(ws.take(&d_cnt, 4 * n, "entry counts"));
        RC_TRY(ws.take(&d_head, 4 * n, "head flags"));
        RC_TRY(ws.take(&d_hpos, 8 * (n + 1), "key indices"));
        RC_TRY(ws.take(&d_run_off, 8 * (n + 1), "run offsets"));
        RC_TRY(ws.take(&d_sort_tmp, sort_bytes, "sort"));
        RC_TRY(ws.take(&d_scan_tmp, scan_bytes, "scan"));
        RC_TRY(ws.take(&d_counters, 4 * DB_JOIN_C_WORDS, "counters"));
        if (ask_branches) {
            RC_TRY(ws.take(&d_lo, 4 * (uint64_t)DB_JOIN_BRANCH_SLOTS, "branch table"));
            RC_TRY(ws.take(&d_hi, 4 * (uint64_t)DB_JOIN_BRANCH_SLOTS, "branch table"));
        }
        const uint32_t nb = (uint32_t)((n + 255) / 256);
        HIP_TRY(ctx, hipMemcpyAsync(d_table, h_table.data(), sizeof(DbUnionSrc) * h_table.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_efirst, h_efirst.data(), 8 * h_efirst.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_counters, 0, 4 * DB_JOIN_C_WORDS, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_counters + DB_JOIN_C_FIRST_DROP, 0xFF, 8, ctx->stream));
        hipLaunchKernelGGL(db_union_sortkey_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_table, n_srcs, n, d_sk);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, rocprim::radix_sort_keys(d_sort_tmp, sort_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        hipLaunchKernelGGL(db_join_runs_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_table, n_srcs, d_sorted, n, d_head, d_cnt, d_src, d_start);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, scan(d_head, n, d_hpos));
        HIP_TRY(ctx, scan(d_cnt, n, d_run_off));
        if (ask_branches) {
            HIP_TRY(ctx, hipMemsetAsync(d_lo, 0xFF, 4 * (size_t)DB_JOIN_BRANCH_SLOTS, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(d_hi, 0, 4 * (size_t)DB_JOIN_BRANCH_SLOTS, ctx->stream));
            hipLaunchKernelGGL(db_join_branch_owner_kernel, dim3((uint32_t)((ne + 255) / 256)), dim3(256), 0, ctx->stream, d_table, d_efirst, n_srcs, ne, d_lo, d_hi);
            HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(db_join_branch_shared_kernel, dim3(DB_JOIN_BRANCH_SLOTS / 256), dim3(256), 0, ctx->stream, d_lo, d_hi, d_counters);
            HIP_TRY(ctx, hipGetLastError());
        }
        uint64_t n_j = 0, h_total = 0;
        uint32_t h_counters[DB_JOIN_C_WORDS];
        HIP_TRY(ctx, hipMemcpyAsync(&n_j, d_hpos + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&h_total, d_run_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_counters, d_counters, sizeof h_counters, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (h_total != ne) return fail(ctx, IPKGPU_ERR_HIP, "the device counted %llu entries, the sources hold %llu", (unsigned long long)h_total, (unsigned long long)ne);
        if (n_j == 0 || n_j > n) return fail(ctx, IPKGPU_ERR_HIP, "the device counted %llu keys among %llu records", (unsigned long long)n_j, (unsigned long long)n);
        // a duplicate needs a key with two runs AND a branch in two sources
        const bool resolve = ne > 0 && (route_opt == 1 || (ask_branches && n_j < n && h_counters[DB_JOIN_C_MAYBE] != 0));
        route = resolve ? 1 : 0;
        const uint32_t tiles = (uint32_t)((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE);
        // the runs are the copy's "keys": run offsets, sources and starts per sorted position
        auto copy_runs = [&](uint2* to, uint32_t* to_pos) -> hipError_t {
            if (!ne) return hipSuccess;
            unsigned long long* w = reinterpret_cast<unsigned long long*>(to);
            if (positioned) hipLaunchKernelGGL(db_union_entries16_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, d_table, d_run_off, d_src, d_start, n, ne, w, to_pos);
            else hipLaunchKernelGGL(db_union_entries16_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, d_table, d_run_off, d_src, d_start, n, ne, w, (uint32_t*)nullptr);
            return hipGetLastError();
        };
        if (!resolve) {
            RC_TRY(join_alloc_arrays(ctx, db, n_j, ne, positioned));
            hipLaunchKernelGGL(db_join_keys_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_sorted, n, d_head, d_hpos, d_run_off, db->d_keys, db->d_key_off, d_counters);
            HIP_TRY(ctx, hipGetLastError());
            e1 = e2 = sw.mark();
            HIP_TRY(ctx, copy_runs(db->d_entries, db->d_positions));
            e3 = e4 = sw.mark();
        } else {
            uint64_t *d_cat_off = nullptr, *d_kept_at = nullptr;
            uint2* d_cat = nullptr;
            uint32_t *d_cat_pos = nullptr, *d_keep = nullptr, *d_long = nullptr;
            RC_TRY(ws.take(&d_cat_off, 8 * (n_j + 1), "concatenated offsets"));
            RC_TRY(ws.take(&d_cat, 8 * ne, "concatenated entries"));
            if (positioned) RC_TRY(ws.take(&d_cat_pos, 4 * ne, "concatenated positions"));
            RC_TRY(ws.take(&d_keep, 4 * ne, "keep flags"));
            RC_TRY(ws.take(&d_kept_at, 8 * (ne + 1), "kept offsets"));
            RC_TRY(ws.take(&d_long, 4 * std::min<uint64_t>(n_j, ne / (DB_JOIN_WAVE_LIST + 1) + 1), "long lists"));
            // the keys go to the result, whose key arrays do not depend on what the duplicate stage finds
            db->n_keys = n_j;
            {
                hipError_t e = ctx_alloc(ctx, (void**)&db->d_keys, n_j * 4);
                if (e == hipSuccess) e = ctx_alloc(ctx, (void**)&db->d_key_off, (n_j + 1) * 8);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "no room for the join's arrays (%llu k-mers): %s", (unsigned long long)n_j,
                                hipGetErrorString(e));
                }
            }
            hipLaunchKernelGGL(db_join_keys_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_sorted, n, d_head, d_hpos, d_run_off, db->d_keys, d_cat_off, d_counters);
            HIP_TRY(ctx, hipGetLastError());
            e1 = e2 = sw.mark();
            HIP_TRY(ctx, copy_runs(d_cat, d_cat_pos));
            e3 = sw.mark();
            for (uint64_t at = 0; at < n_j; at += WAVE_PER_ITEM_SPAN) {
                const uint32_t blocks = (uint32_t)((std::min<uint64_t>(WAVE_PER_ITEM_SPAN, n_j - at) + 3) / 4);
                if (positioned) hipLaunchKernelGGL(db_join_dups_wave_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, d_cat_off, n_j, at, d_cat, d_cat_pos, d_keep, d_long, d_counters);
                else hipLaunchKernelGGL(db_join_dups_wave_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, d_cat_off, n_j, at, d_cat, d_cat_pos, d_keep, d_long, d_counters);
            }
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(h_counters, d_counters, sizeof h_counters, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            const uint32_t n_long = h_counters[DB_JOIN_C_LONG], max_len = h_counters[DB_JOIN_C_MAXLEN];
            if (n_long) {
                if (positioned) hipLaunchKernelGGL(db_join_dups_lds_kernel<true>, dim3(n_long), dim3(256), 0, ctx->stream, d_cat_off, d_long, d_cat, d_cat_pos, d_keep);
                else hipLaunchKernelGGL(db_join_dups_lds_kernel<false>, dim3(n_long), dim3(256), 0, ctx->stream, d_cat_off, d_long, d_cat, d_cat_pos, d_keep);
                HIP_TRY(ctx, hipGetLastError());
            }
            if (max_len > DB_JOIN_LDS_LIST) {
                unsigned long long *d_pk = nullptr, *d_pv = nullptr, *d_pk2 = nullptr, *d_pv2 = nullptr;
                void* d_pair_tmp = nullptr;
                size_t pair_bytes = 0;
                HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, pair_bytes, d_pk, d_pk2, d_pv, d_pv2, (size_t)ne, 0, 64, ctx->stream));
                RC_TRY(ws.take(&d_pk, 8 * ne, "pair keys"));
                RC_TRY(ws.take(&d_pk2, 8 * ne, "sorted pair keys"));
                RC_TRY(ws.take(&d_pv, 8 * ne, "pair values"));
                RC_TRY(ws.take(&d_pv2, 8 * ne, "sorted pair values"));
                RC_TRY(ws.take(&d_pair_tmp, pair_bytes, "pair sort"));
                hipLaunchKernelGGL(db_join_sortpair_kernel, dim3(tiles), dim3(256), 0, ctx->stream, d_cat_off, n_j, ne, d_cat, d_pk, d_pv);
                HIP_TRY(ctx, hipGetLastError());
                HIP_TRY(ctx, rocprim::radix_sort_pairs(d_pair_tmp, pair_bytes, d_pk, d_pk2, d_pv, d_pv2, (size_t)ne, 0, 64, ctx->stream));
                const uint32_t eb = (uint32_t)((ne + 255) / 256);
                if (positioned) hipLaunchKernelGGL(db_join_dups_sorted_kernel<true>, dim3(eb), dim3(256), 0, ctx->stream, d_pk2, d_pv2, ne, d_cat, d_cat_pos, d_keep);
                else hipLaunchKernelGGL(db_join_dups_sorted_kernel<false>, dim3(eb), dim3(256), 0, ctx->stream, d_pk2, d_pv2, ne, d_cat, d_cat_pos, d_keep);
                HIP_TRY(ctx, hipGetLastError());
            }
            HIP_TRY(ctx, scan(d_keep, ne, d_kept_at));
            uint64_t n_kept = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&n_kept, d_kept_at + ne, 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (n_kept > ne) return fail(ctx, IPKGPU_ERR_HIP, "the device kept %llu of %llu entries", (unsigned long long)n_kept, (unsigned long long)ne);
            n_dropped = ne - n_kept;
            db->n_entries = n_kept;
            {
                hipError_t e = ctx_alloc(ctx, (void**)&db->d_entries, std::max<uint64_t>(n_kept, 1) * 8);
                if (e == hipSuccess && positioned) e = ctx_alloc(ctx, (void**)&db->d_positions, std::max<uint64_t>(n_kept, 1) * 4);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "no room for the join's arrays (%llu k-mers, %llu entries): %s",
                                (unsigned long long)n_j, (unsigned long long)n_kept, hipGetErrorString(e));
                }
            }
            const uint32_t eb = (uint32_t)((ne + 255) / 256);
            if (positioned) hipLaunchKernelGGL(db_join_compact_kernel<true>, dim3(eb), dim3(256), 0, ctx->stream, d_cat, d_cat_pos, d_keep, d_kept_at, ne, db->d_entries, db->d_positions, d_counters);
            else hipLaunchKernelGGL(db_join_compact_kernel<false>, dim3(eb), dim3(256), 0, ctx->stream, d_cat, d_cat_pos, d_keep, d_kept_at, ne, db->d_entries, (uint32_t*)nullptr, d_counters);
            HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(db_join_offsets_kernel, dim3((uint32_t)((n_j + 1 + 255) / 256)), dim3(256), 0, ctx->stream, d_cat_off, d_kept_at, n_j, db->d_key_off);
            HIP_TRY(ctx, hipGetLastError());
            e4 = sw.mark();
            if (route_opt == 2 && n_dropped) {                    // the caller expected branch-disjoint shards: name one duplicate
                unsigned long long first_drop = 0;
                HIP_TRY(ctx, hipMemcpyAsync(&first_drop, d_counters + DB_JOIN_C_FIRST_DROP, 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                if (first_drop >= ne) return fail(ctx, IPKGPU_ERR_HIP, "the device dropped %llu entries and named none", (unsigned long long)n_dropped);
                hipLaunchKernelGGL(db_join_locate_kernel, dim3(1), dim3(64), 0, ctx->stream, d_sorted, d_run_off, d_src, d_head, n, d_cat, (uint64_t)first_drop, d_counters);
                HIP_TRY(ctx, hipGetLastError());
                HIP_TRY(ctx, hipMemcpyAsync(h_counters, d_counters, sizeof h_counters, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                const uint32_t* w = h_counters + DB_JOIN_C_LOCATE;
                return fail(ctx, IPKGPU_ERR_INVALID, "k-mer %u has branch %u in source %u and in source %u (%llu duplicate entries in all): \"join_route\" = 2 takes branch-disjoint shards",
                            w[0], w[1], w[2], w[3], (unsigned long long)n_dropped);
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(h_counters, d_counters, sizeof h_counters, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        n_shared = h_counters[DB_JOIN_C_SHARED];
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    db->t_merge = n ? sw.ms(e0, e4) : 0;
    ctx->join_stat[0] = db->t_merge; ctx->join_stat[1] = n ? sw.ms(e0, e1) : 0; ctx->join_stat[2] = n ? sw.ms(e2, e3) : 0; ctx->join_stat[3] = n ? sw.ms(e3, e4) : 0;
    ctx->join_stat[4] = (double)n_shared; ctx->join_stat[5] = (double)n_dropped; ctx->join_stat[6] = (double)route;
    guard.r = nullptr;
    *out = db;
    return IPKGPU_OK;
}

}  // extern "C"
