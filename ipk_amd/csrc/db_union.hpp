// db_union.hpp -- ipkgpu_db_union / ipkgpu_db_union_files: N databases with disjoint key sets made one on the device (included by
// ipkgpu.hip behind db_diff_files.hpp, whose bounds of rocprim's own space it shares; kernels_dbunion.hpp).
//
// The host's part: the refusals, one table of the sources' pointers, the workspace, and the sequence
//   db_union_sortkey_kernel -> radix sort of (key, concatenated index)             the loader's sort of (key, record)
//   db_union_keys_kernel -> the duplicate read back -> scan of the counts          keys, filter values, key_off
//   db_union_entries16_kernel (or db_union_entries_kernel, "union_copy_bytes" = 8)  entries and positions
//   filter_sortkey_kernel -> the filter stage's sort -> filter_order_kernel        order
// Every byte of workspace is taken with dev_malloc for this call and given back before it returns -- none of it lives in the context's
// grow-only buffers -- so the call's peak is the formula of ipkgpu_db_union_bytes whatever the context did before.
#pragma once

namespace {

// a block of the union's workspace
inline uint64_t du_m(uint64_t x) { return std::max<uint64_t>(x, 256); }

struct UnionBlocks {                      // freed, behind a wait, however the call returns
    ipkgpu_ctx* ctx;
    std::vector<std::pair<void*, size_t>> held;
    ~UnionBlocks()
    {
        if (held.empty()) return;
        (void)hipStreamSynchronize(ctx->stream);
        for (auto& b : held) (void)dev_free(ctx, b.first, b.second);
        (void)hipGetLastError();
    }
    template <class T> int take(T** out, uint64_t bytes, const char* what)
    {
        void* p = nullptr;
        const size_t sz = (size_t)du_m(bytes);
        const hipError_t e = dev_malloc(ctx, &p, sz);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "no room for the union's %s (%llu bytes): %s", what,
                        (unsigned long long)sz, hipGetErrorString(e));
        }
        held.push_back({p, sz});
        *out = static_cast<T*>(p);
        return IPKGPU_OK;
    }
};

// ctx_alloc's failures as the union reports them (HIP_TRY names a source line; a budget's refusal is no HIP failure)
int union_alloc_arrays(ipkgpu_ctx* ctx, ipkgpu_db* db, uint64_t n, uint64_t ne, bool positioned)
{
    const int rc = db_alloc_arrays(ctx, db, n, ne, positioned);
    if (rc == IPKGPU_ERR_NOMEM) { (void)hipGetLastError(); return fail(ctx, rc, "no room for the union's arrays (%llu k-mers, %llu entries)", (unsigned long long)n, (unsigned long long)ne); }
    return rc;
}

}  // namespace

extern "C" {

uint64_t ipkgpu_db_union_bytes(uint64_t n_keys, uint64_t n_entries, uint32_t n_srcs, int positioned)
{
    const uint64_t n = n_keys;
    const uint64_t ws = du_m(sizeof(DbUnionSrc) * ((uint64_t)n_srcs + 1)) + 3 * du_m(8 * n) + 2 * du_m(4 * n) + du_m(df_sort(n)) + du_m(df_scan(n + 1)) + 256;
    return df_db(n, n_entries, positioned != 0) + ws;
}

double ipkgpu_db_union_time_ms(const ipkgpu_ctx* ctx, int which) { return ctx && which >= 0 && which < 4 ? ctx->t_union[which] : 0; }

int ipkgpu_db_union(ipkgpu_ctx* ctx, const ipkgpu_db* const* srcs, uint32_t n_srcs, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!out) return fail(ctx, IPKGPU_ERR_INVALID, "null out pointer");
    if (n_srcs == 0 || !srcs) return fail(ctx, IPKGPU_ERR_INVALID, "a union needs at least one source database");
    uint64_t n = 0, ne = 0;
    for (uint32_t s = 0; s < n_srcs; ++s) {
        const ipkgpu_db* d = srcs[s];
        if (!d) return fail(ctx, IPKGPU_ERR_INVALID, "source %u of the union is null", s);
        if (d->ctx != ctx) return fail(ctx, IPKGPU_ERR_INVALID, "source %u of the union belongs to another context", s);
        if (!d->d_fv32 || !d->d_fv64 || !d->d_order)
            return fail(ctx, IPKGPU_ERR_INVALID, "source %u of the union has no filter values and order (filter it, or load it from a file)", s);
        if ((d->d_positions != nullptr) != (srcs[0]->d_positions != nullptr))
            return fail(ctx, IPKGPU_ERR_INVALID, "positioned and plain shards cannot be merged into one database: source %u %s source 0 %s", s,
                        d->d_positions ? "has positions," : "has none,", srcs[0]->d_positions ? "has" : "has none");
        n += d->n_keys; ne += d->n_entries;
    }
    if (n > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%llu k-mers in all: a database holds at most 2^32 - 1 (its order is 32-bit)", (unsigned long long)n);
    if ((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE > 0x7FFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "too many entries for one launch");
    const bool positioned = srcs[0]->d_positions != nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (double& t : ctx->t_union) t = 0;

    // the source table on the host: one row per source, one behind the last
    std::vector<DbUnionSrc> h_table(n_srcs + (size_t)1);
    uint64_t first = 0;
    for (uint32_t s = 0; s < n_srcs; ++s) {
        const ipkgpu_db* d = srcs[s];
        h_table[s] = DbUnionSrc{d->d_keys, d->d_key_off, d->d_entries, d->d_positions, d->d_fv32, d->d_fv64, first};
        first += d->n_keys;
    }
    h_table[n_srcs] = DbUnionSrc{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, first};

    UnionBlocks ws{ctx, {}};                                  // (declared before the result's guard: it waits, then the result goes)
    ipkgpu_db* db = new (std::nothrow) ipkgpu_db();
    if (!db) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    db->ctx = ctx;
    struct Guard { ipkgpu_ctx* c; ipkgpu_db* r; ~Guard() { if (r) { (void)hipStreamSynchronize(c->stream); ipkgpu_db_free(r); } } } guard{ctx, db};
    RC_TRY(union_alloc_arrays(ctx, db, n, ne, positioned));
    Stopwatch sw(ctx->stream, &ctx->events);
    const int e0 = sw.mark();
    int e1 = e0, e2 = e0, e3 = e0, e4 = e0;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(db->d_key_off, 0, 8, ctx->stream));
    } else {
        DbUnionSrc* d_table = nullptr;
        unsigned long long *d_sk = nullptr, *d_sorted = nullptr;
        uint64_t* d_start = nullptr;
        uint32_t *d_src = nullptr, *d_cnt = nullptr, *d_dup = nullptr;
        void *d_sort_tmp = nullptr, *d_scan_tmp = nullptr;
        size_t sort_bytes = 0, scan_bytes = 0;
        HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, sort_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        const auto query_in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), ScanU32In{nullptr, n});
        HIP_TRY(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, query_in, db->d_key_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), ctx->stream));
        RC_TRY(ws.take(&d_table, sizeof(DbUnionSrc) * h_table.size(), "source table"));
        RC_TRY(ws.take(&d_sk, 8 * n, "sort keys"));
        RC_TRY(ws.take(&d_sorted, 8 * n, "sorted keys"));
        RC_TRY(ws.take(&d_start, 8 * n, "entry starts"));
        RC_TRY(ws.take(&d_src, 4 * n, "source indices"));
        RC_TRY(ws.take(&d_cnt, 4 * n, "entry counts"));
        RC_TRY(ws.take(&d_sort_tmp, sort_bytes, "sort"));
        RC_TRY(ws.take(&d_scan_tmp, scan_bytes, "scan"));
        RC_TRY(ws.take(&d_dup, 4, "duplicate index"));
        const auto counts_in = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), ScanU32In{d_cnt, n});
        const uint32_t nb = (uint32_t)((n + 255) / 256);
        HIP_TRY(ctx, hipMemcpyAsync(d_table, h_table.data(), sizeof(DbUnionSrc) * h_table.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_dup, 0xFF, 4, ctx->stream));
        hipLaunchKernelGGL(db_union_sortkey_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_table, n_srcs, n, d_sk);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, rocprim::radix_sort_keys(d_sort_tmp, sort_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        hipLaunchKernelGGL(db_union_keys_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_table, n_srcs, d_sorted, n, db->d_keys,
                           reinterpret_cast<uint32_t*>(db->d_fv32), reinterpret_cast<unsigned long long*>(db->d_fv64), d_cnt, d_src, d_start, d_dup);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, rocprim::exclusive_scan(d_scan_tmp, scan_bytes, counts_in, db->d_key_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), ctx->stream));
        e1 = sw.mark();
        uint32_t h_dup = 0;
        uint64_t h_total = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&h_dup, d_dup, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&h_total, db->d_key_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (h_dup != 0xFFFFFFFFu) {                           // before any entry moves: the key and the two sources that hold it
            unsigned long long pair[2] = {0, 0};
            HIP_TRY(ctx, hipMemcpy(pair, d_sorted + (h_dup - 1), 16, hipMemcpyDeviceToHost));
            auto source_of = [&](uint64_t c) { uint32_t s = 0; while (s + 1 < n_srcs && h_table[s + 1].first <= c) ++s; return s; };
            return fail(ctx, IPKGPU_ERR_INVALID, "k-mer %u is in source %u and in source %u: a union takes disjoint key sets", (uint32_t)(pair[1] >> 32),
                        source_of((uint32_t)pair[0]), source_of((uint32_t)pair[1]));
        }
        if (h_total != ne) return fail(ctx, IPKGPU_ERR_HIP, "the device counted %llu entries, the sources hold %llu", (unsigned long long)h_total, (unsigned long long)ne);
        e2 = sw.mark();
        if (ne) {
            const uint32_t tiles = (uint32_t)((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE);
            unsigned long long* out_entries = reinterpret_cast<unsigned long long*>(db->d_entries);
            const bool wide = ctx->opt_union_copy != 8;           // ("union_copy_bytes": 0 = the default, the 16-byte form -- the faster one)
            if (positioned && wide) hipLaunchKernelGGL(db_union_entries16_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, d_table, db->d_key_off, d_src, d_start,
                                                       n, ne, out_entries, db->d_positions);
            else if (wide) hipLaunchKernelGGL(db_union_entries16_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, d_table, db->d_key_off, d_src, d_start, n, ne,
                                              out_entries, (uint32_t*)nullptr);
            else if (positioned) hipLaunchKernelGGL(db_union_entries_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, d_table, db->d_key_off, d_src, d_start, n, ne,
                                                    out_entries, db->d_positions);
            else hipLaunchKernelGGL(db_union_entries_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, d_table, db->d_key_off, d_src, d_start, n, ne,
                                    out_entries, (uint32_t*)nullptr);
            HIP_TRY(ctx, hipGetLastError());
        }
        e3 = sw.mark();
        // the order: the filter stage's sort key over the union's values (keys ascend, so the index breaks ties by key), its sort
        hipLaunchKernelGGL(filter_sortkey_kernel, dim3(nb), dim3(256), 0, ctx->stream, db->d_fv32, n, d_sk);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, rocprim::radix_sort_keys(d_sort_tmp, sort_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        hipLaunchKernelGGL(filter_order_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_sorted, n, db->d_order);
        HIP_TRY(ctx, hipGetLastError());
    }
    e4 = sw.mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    db->t_merge = sw.ms(e0, e4);
    ctx->t_union[0] = db->t_merge; ctx->t_union[1] = n ? sw.ms(e0, e1) : 0; ctx->t_union[2] = n ? sw.ms(e2, e3) : 0; ctx->t_union[3] = n ? sw.ms(e3, e4) : 0;
    guard.r = nullptr;
    *out = db;
    return IPKGPU_OK;
}

int ipkgpu_db_union_files(ipkgpu_ctx* ctx, const ipkgpu_db_header* h, const char* const* paths, uint32_t n_paths, const char* path,
                          uint64_t* total_kmers, uint64_t* total_entries, uint64_t* bytes_written)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (!h || !h->sequence_type || !path || !paths || n_paths == 0) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument: a header, an output path and at least one shard are needed");
    std::vector<ipkgpu_db*> dbs;
    struct Free { std::vector<ipkgpu_db*>& v; ~Free() { for (ipkgpu_db* d : v) ipkgpu_db_free(d); } } free_all{dbs};
    for (uint32_t s = 0; s < n_paths; ++s) {
        if (!paths[s]) return fail(ctx, IPKGPU_ERR_INVALID, "shard path %u is null", s);
        ipkgpu_db* d = nullptr;
        RC_TRY(ipkgpu_db_load(ctx, paths[s], &d));
        dbs.push_back(d);
        const ipkfmt::Head& hd = d->file->head;
        uint32_t want = 0, got = 0;
        memcpy(&want, &h->omega, 4); memcpy(&got, &hd.omega, 4);
        if (hd.sequence_type != h->sequence_type || hd.kmer_size != h->kmer_size || want != got)
            return fail(ctx, IPKGPU_ERR_INVALID, "%s: a shard of %s, k = %llu, omega = %.9g; the header given is of %s, k = %llu, omega = %.9g", paths[s],
                        hd.sequence_type.c_str(), (unsigned long long)hd.kmer_size, (double)hd.omega, h->sequence_type, (unsigned long long)h->kmer_size, (double)h->omega);
        if (hd.positions_loaded != dbs[0]->file->head.positions_loaded)
            return fail(ctx, IPKGPU_ERR_INVALID, "positioned and plain shards cannot be merged into one database: %s %s %s %s", paths[s],
                        hd.positions_loaded ? "has positions," : "has none,", paths[0], dbs[0]->file->head.positions_loaded ? "has" : "has none");
    }
    ipkgpu_db* u = nullptr;
    RC_TRY(ipkgpu_db_union(ctx, dbs.data(), n_paths, &u));
    for (ipkgpu_db* d : dbs) ipkgpu_db_free(d);
    dbs.clear();
    uint64_t bytes = 0;
    const uint64_t nk = u->n_keys, ne = u->n_entries;
    const int rc = ipkgpu_db_write(ctx, u, h, path, &bytes);
    ipkgpu_db_free(u);
    if (rc) return rc;
    if (total_kmers) *total_kmers = nk;
    if (total_entries) *total_entries = ne;
    if (bytes_written) *bytes_written = bytes;
    return IPKGPU_OK;
}

}  // extern "C"
