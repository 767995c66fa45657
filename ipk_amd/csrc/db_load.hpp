// db_load.hpp -- a database file back onto the device, and the comparison of two databases (included by ipkgpu.hip).
//
// ipkgpu_db_load: the file's body goes chunk by chunk through the context's pinned staging buffers into one device image, the
// next read under the previous copy; on its way the host walks the count fields (ipkfmt::RecordWalker, the walk of
// ipkgpu_db_file_check) -- the only serial part, and the only place a number of the file is believed.  A file the walk refuses
// launches nothing.  Then kernels_dbload.hpp: heads in file order, a sort of (key, record) with the filter stage's radix sort,
// a scan of the counts in key order, entries by entry ranges.  The image is freed before the call returns.
// db_load_records is that load for the first M records of the file as well (ipkgpu_db_load_select, db_select.hpp).
// ipkgpu_db_diff: kernels_dbdiff.hpp -- join, count pass, scan, write pass.
#pragma once

extern "C" {

const ipkgpu_db_file* ipkgpu_db_header_of(const ipkgpu_db* d) { return d ? d->file : nullptr; }
double ipkgpu_db_load_time(const ipkgpu_ctx* ctx, int which) { return ctx && which >= 0 && which < 10 ? ctx->t_load[which] : 0; }
double ipkgpu_db_diff_time_ms(const ipkgpu_ctx* ctx) { return ctx ? ctx->t_diff_ms : 0; }
uint32_t ipkgpu_db_diff_chunk(void) { return DB_DIFF_CHUNK; }

}  // extern "C"

namespace {

// The seven device arrays of a database of n keys and ne entries (each at least one element, as every producer allocates them).
int db_alloc_arrays(ipkgpu_ctx* ctx, ipkgpu_db* db, uint64_t n, uint64_t ne, bool positioned)
{
    db->n_keys = n; db->n_entries = ne;
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_keys, std::max<uint64_t>(n, 1) * 4));
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_key_off, (n + 1) * 8));
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_entries, std::max<uint64_t>(ne, 1) * 8));
    if (positioned) HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_positions, std::max<uint64_t>(ne, 1) * 4));
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_fv64, std::max<uint64_t>(n, 1) * 8));
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_fv32, std::max<uint64_t>(n, 1) * 4));
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_order, std::max<uint64_t>(n, 1) * 4));
    return IPKGPU_OK;
}

// The load behind ipkgpu_db_load (keep_records = all) and ipkgpu_db_load_select: the first min(keep_records, header total) records of
// the file as a database.  keep_records >= the header's total is the whole file, read and checked as ever.  Fewer: only the prefix of
// the body that holds them is touched.  How long that prefix is shows only when the walk has seen its last record, so the walk goes
// first, over a read-only mapping of the file and chunk by chunk; then an image of exactly the prefix' bytes is allocated and the
// prefix streamed into it through the same pinned buffers (from the page cache the walk has just filled).  The walk stops at
// keep_records records, each of which ends inside the file; that it ends at the end of the file with the header's totals cannot be
// asked of a prefix, and the head kept with the database carries the prefix' own totals.  (A mapping, not reads: a file truncated by
// another process behind the size check below, or an I/O error, is a SIGBUS here where the full load's fread gives IPKGPU_ERR_INVALID;
// include/ipkgpu.h says so.)  t_load[7] for a prefix is the walk's extent, the prefix rounded up to a chunk.
int db_load_records(ipkgpu_ctx* ctx, const char* path, uint64_t keep_records, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!path || !out) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument");
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    ipkgpu_db_file* file = nullptr;
    if (const int rc = ipkgpu_db_file_open(path, &file)) return fail(ctx, rc, "%s", ipkgpu_db_file_last_error());
    struct FileGuard { ipkgpu_db_file* f; ~FileGuard() { ipkgpu_db_file_close(f); } } fguard{file};
    ipkfmt::Head& hd = file->head;
    const bool whole = keep_records >= hd.total_kmers;
    uint64_t n = hd.total_kmers, ne = hd.total_entries;
    const uint64_t body = file->body_bytes();
    const bool positioned = hd.positions_loaded;
    if (n > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %llu k-mers: a database holds at most 2^32 - 1 (its order is 32-bit)", path, (unsigned long long)n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // the image of the body or of its prefix (+16: the positioned entries are read as aligned dwords, the last one two bytes past its end)
    unsigned char* image = nullptr;
    size_t image_bytes = 0;
    struct ImageGuard { ipkgpu_ctx* c; unsigned char*& p; size_t& bytes;
        ~ImageGuard() { if (p) { (void)hipStreamSynchronize(c->stream); (void)dev_free(c, p, bytes); p = nullptr; } (void)hipGetLastError(); } } iguard{ctx, image, image_bytes};
    auto alloc_image = [&](uint64_t bytes) -> int {
        image_bytes = (size_t)bytes + 16;
        const hipError_t e = dev_malloc(ctx, (void**)&image, image_bytes);
        if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "%s: no room for the image of the file's body (%llu bytes): %s",
                                         path, (unsigned long long)bytes, hipGetErrorString(e));
        HIP_TRY(ctx, hipMemsetAsync(image + bytes, 0, 16, ctx->stream));
        return IPKGPU_OK;
    };
    const uint64_t chunk = std::min<uint64_t>(ctx->opt_load_chunk > 0 ? (uint64_t)ctx->opt_load_chunk : SPILL_STAGE, SPILL_STAGE);
    ipkfmt::RecordWalker walk;
    walk.begin(hd.body_at, body, positioned, n, whole ? ~(uint64_t)0 : keep_records);
    double t_read = 0, t_walk = 0, t_wait = 0;
    uint64_t bytes_read = 0;
    {
        FILE* fh = fopen(path, "rb");
        if (!fh) return fail(ctx, IPKGPU_ERR_INVALID, "cannot open %s", path);
        struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fh};
        setvbuf(fh, nullptr, _IONBF, 0);
        uint64_t extent = body;                                              // the body bytes that go to the device
        if (!whole) {
            // the walk of the prefix, ahead of everything: over a read-only mapping of the file, chunk by chunk, until the last record
            // asked for is known -- only then is the prefix' length known, and the image allocated at exactly that
            struct stat st;
            if (fstat(fileno(fh), &st) != 0 || (uint64_t)st.st_size != file->file_bytes) return fail(ctx, IPKGPU_ERR_INVALID, "%s: the file changed since it was opened", path);
            const auto t0 = std::chrono::steady_clock::now();
            uint64_t lo = 0;
            if (body && keep_records) {
                void* map = mmap(nullptr, (size_t)file->file_bytes, PROT_READ, MAP_PRIVATE, fileno(fh), 0);
                if (map == MAP_FAILED) return fail(ctx, IPKGPU_ERR_INVALID, "%s: cannot map the file", path);
                struct Unmap { void* p; size_t n; ~Unmap() { munmap(p, n); } } unmap{map, (size_t)file->file_bytes};
                (void)madvise(map, (size_t)file->file_bytes, MADV_SEQUENTIAL);
                const uint8_t* base = static_cast<const uint8_t*>(map) + hd.body_at;
                for (; lo < body && !(walk.done() && lo >= walk.pos); lo += chunk)
                    if (!walk.feed(base + lo, lo, std::min(body, lo + chunk))) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %s", path, walk.error.c_str());
            }
            t_walk += since(t0);
            bytes_read = std::min(body, lo);                                 // (the chunks the walk touched; the copy below reads inside them)
            if (!walk.done() || walk.pos > bytes_read)
                return fail(ctx, IPKGPU_ERR_INVALID, "%s: the file ends before record %llu of the first %llu has ended", path,
                            (unsigned long long)walk.starts.size(), (unsigned long long)keep_records);
            extent = walk.pos;
            n = walk.starts.size(); ne = walk.n_entries;
            hd.total_kmers = n; hd.total_entries = ne;
            file->file_bytes = hd.body_at + extent;
        } else {
            bytes_read = body;
        }
        RC_TRY(alloc_image(extent));
        if (fseeko(fh, (off_t)hd.body_at, SEEK_SET) != 0) return fail(ctx, IPKGPU_ERR_INVALID, "%s: seek failed", path);
        // file -> pinned buffer -> image, the next read under the previous copy; the whole file's walk sees every chunk before it leaves
        RC_TRY(spill_stage(ctx, (size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(extent, 1))));
        uint64_t j = 0;
        for (uint64_t lo = 0; lo < extent; lo += chunk, ++j) {
            const uint64_t hi = std::min(extent, lo + chunk);
            const int b = (int)(j & 1);
            auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev_spill[b]));        // (the copy out of this buffer two chunks ago; at once on a fresh event)
            t_wait += since(t0); t0 = std::chrono::steady_clock::now();
            uint8_t* src = static_cast<uint8_t*>(ctx->h_spill[b]);
            if (fread(src, 1, (size_t)(hi - lo), fh) != hi - lo) return fail(ctx, IPKGPU_ERR_INVALID, "%s: read failed", path);
            t_read += since(t0); t0 = std::chrono::steady_clock::now();
            if (whole && !walk.feed(src, lo, hi)) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %s", path, walk.error.c_str());
            t_walk += since(t0);
            HIP_TRY(ctx, hipMemcpyAsync(image + lo, src, (size_t)(hi - lo), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipEventRecord(ctx->ev_spill[b], ctx->stream));
        }
    }
    if (whole && !walk.finish(n, ne)) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %s", path, walk.error.c_str());
    if (walk.max_count > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: a k-mer with 2^32 entries or more", path);
    if ((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE > 0x7FFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: too many entries for one launch", path);
    file->walked = true; file->n_records = n; file->n_entries = ne; file->max_count = walk.max_count;

    // from here on every offset and count is the host's own
    ipkgpu_db* db = new (std::nothrow) ipkgpu_db();
    if (!db) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    db->ctx = ctx;
    struct Guard { ipkgpu_db* r; ~Guard() { if (r) ipkgpu_db_free(r); } } guard{db};
    RC_TRY(db_alloc_arrays(ctx, db, n, ne, positioned));
    Stopwatch sw(ctx->stream, &ctx->events);
    const int e0 = sw.mark();
    int eh = e0, e1 = e0, e2 = e0, e3 = e0;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(db->d_key_off, 0, 8, ctx->stream));
    } else {
        // workspaces: record starts | (key, record) unsorted, sorted | per record in file order: filter bits, count | in key order: count, body offset
        RC_TRY(ensure(ctx, ctx->sp_rank, n * 8));
        RC_TRY(ensure(ctx, ctx->tmp_a, n * 8));
        RC_TRY(ensure(ctx, ctx->tmp_b, n * 8));
        RC_TRY(ensure(ctx, ctx->sp_c16, n * 4));
        RC_TRY(ensure(ctx, ctx->counts, n * 4));
        RC_TRY(ensure(ctx, ctx->sp_pops, n * 4));
        RC_TRY(ensure(ctx, ctx->goff, n * 8));
        uint64_t* d_starts = ctx->sp_rank.as<uint64_t>();
        unsigned long long* d_sk = ctx->tmp_a.as<unsigned long long>();
        unsigned long long* d_sorted = ctx->tmp_b.as<unsigned long long>();
        uint32_t* d_fvb = ctx->sp_c16.as<uint32_t>();
        uint32_t* d_cnt = ctx->counts.as<uint32_t>();
        uint32_t* d_cnt_sorted = ctx->sp_pops.as<uint32_t>();
        uint64_t* d_body_off = ctx->goff.as<uint64_t>();
        uint32_t* d_dup = small_at(ctx, SMALL_REC_BIG);
        const uint32_t nb = (uint32_t)((n + 255) / 256);
        HIP_TRY(ctx, hipMemcpyAsync(d_starts, walk.starts.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(d_dup, 0, 4, ctx->stream));
        eh = sw.mark();
        if (positioned) hipLaunchKernelGGL(db_unpack_heads_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, image, d_starts, n, d_sk, d_fvb, d_cnt);
        else hipLaunchKernelGGL(db_unpack_heads_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, image, d_starts, n, d_sk, d_fvb, d_cnt);
        HIP_TRY(ctx, hipGetLastError());
        e1 = sw.mark();
        size_t tmp_bytes = 0;
        HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, tmp_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        RC_TRY(ensure(ctx, ctx->tmp_c, tmp_bytes));
        HIP_TRY(ctx, rocprim::radix_sort_keys(ctx->tmp_c.p, tmp_bytes, d_sk, d_sorted, (size_t)n, 0, 64, ctx->stream));
        hipLaunchKernelGGL(db_load_order_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, d_sorted, d_starts, d_fvb, d_cnt, n, db->d_keys, d_cnt_sorted,
                           d_body_off, db->d_fv32, db->d_fv64, db->d_order, d_dup);
        HIP_TRY(ctx, hipGetLastError());
        RC_TRY(scan_u32(ctx, d_cnt_sorted, n, db->d_key_off));
        uint32_t h_dup = 0;
        uint64_t h_total = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&h_dup, d_dup, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&h_total, db->d_key_off + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        const auto tw = std::chrono::steady_clock::now();
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        t_wait += since(tw);
        if (h_dup) return fail(ctx, IPKGPU_ERR_INVALID, "%s: a k-mer has more than one record", path);
        if (h_total != ne) return fail(ctx, IPKGPU_ERR_HIP, "%s: the device counted %llu entries, the host %llu", path, (unsigned long long)h_total, (unsigned long long)ne);
        e2 = sw.mark();
        if (ne) {
            const uint32_t tiles = (uint32_t)((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE);
            if (positioned) hipLaunchKernelGGL(db_unpack_entries_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, image, db->d_key_off, d_body_off, n, ne,
                                               db->d_entries, db->d_positions);
            else hipLaunchKernelGGL(db_unpack_entries_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, image, db->d_key_off, d_body_off, n, ne,
                                    db->d_entries, (uint32_t*)nullptr);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    e3 = sw.mark();
    {
        const auto tw = std::chrono::steady_clock::now();
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        t_wait += since(tw);
    }
    db->t_merge = sw.ms(e0, e3);
    ctx->t_load[1] = t_read; ctx->t_load[2] = t_walk; ctx->t_load[3] = t_wait;
    ctx->t_load[4] = n ? sw.ms(eh, e1) : 0; ctx->t_load[5] = n ? sw.ms(e2, e3) : 0; ctx->t_load[6] = db->t_merge;
    ctx->t_load[7] = (double)bytes_read;
    ctx->t_load[8] = 0; ctx->t_load[9] = 0;                              // (windows and records kept: ipkgpu_db_load_wanted's)
    db->file = file; fguard.f = nullptr;
    guard.r = nullptr;
    *out = db;
    ctx->t_load[0] = since(t_begin);
    return IPKGPU_OK;
}

}  // namespace

extern "C" {

int ipkgpu_db_load(ipkgpu_ctx* ctx, const char* path, ipkgpu_db** out) { return db_load_records(ctx, path, ~(uint64_t)0, out); }

int ipkgpu_db_diff(ipkgpu_ctx* ctx, const ipkgpu_db* a, const ipkgpu_db* b, double eps, ipkgpu_db_diff_counts* counts,
                   ipkgpu_db_diff_record* records, uint64_t max_records, uint64_t* n_records)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (n_records) *n_records = 0;
    if (!a || !b || a->ctx != ctx || b->ctx != ctx) return fail(ctx, IPKGPU_ERR_INVALID, "both databases must belong to this context");
    if (!counts || (max_records && (!records || !n_records))) return fail(ctx, IPKGPU_ERR_INVALID, "null argument");
    if (!(eps >= 0.0)) return fail(ctx, IPKGPU_ERR_INVALID, "eps must not be negative (0 = equal score bits)");
    static_assert(sizeof(ipkgpu_db_diff_record) == sizeof(uint4), "a record is stored as one 16-byte word");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t na = a->n_keys, nb = b->n_keys;
    const DbDiffView A{a->d_keys, a->d_key_off, a->d_entries, a->d_positions, na}, B{b->d_keys, b->d_key_off, b->d_entries, b->d_positions, nb};
    RC_TRY(ensure(ctx, ctx->sp_pops, std::max<uint64_t>(na, 1) * 4));     // A's keys: their place in B, differences, records before them
    RC_TRY(ensure(ctx, ctx->counts, std::max<uint64_t>(na, 1) * 4));
    RC_TRY(ensure(ctx, ctx->sp_rank, (na + 1) * 8));
    RC_TRY(ensure(ctx, ctx->sp_c16, std::max<uint64_t>(nb, 1) * 4));      // the same for B's keys
    RC_TRY(ensure(ctx, ctx->sp_bits, std::max<uint64_t>(nb, 1) * 4));
    RC_TRY(ensure(ctx, ctx->goff, (nb + 1) * 8));
    RC_TRY(ensure(ctx, ctx->tmp_c, sizeof(DbDiffTotals)));
    uint32_t* lb_a = ctx->sp_pops.as<uint32_t>(); uint32_t* cnt_a = ctx->counts.as<uint32_t>(); uint64_t* scan_a = ctx->sp_rank.as<uint64_t>();
    uint32_t* lb_b = ctx->sp_c16.as<uint32_t>(); uint32_t* cnt_b = ctx->sp_bits.as<uint32_t>(); uint64_t* scan_b = ctx->goff.as<uint64_t>();
    DbDiffTotals* d_tot = ctx->tmp_c.as<DbDiffTotals>();
    Stopwatch sw(ctx->stream, &ctx->events);
    const int e0 = sw.mark();
    HIP_TRY(ctx, hipMemsetAsync(d_tot, 0, sizeof(DbDiffTotals), ctx->stream));
    if (na) hipLaunchKernelGGL(db_diff_join_kernel, dim3((uint32_t)((na + 255) / 256)), dim3(256), 0, ctx->stream, a->d_keys, na, b->d_keys, nb, lb_a);
    if (nb) hipLaunchKernelGGL(db_diff_join_kernel, dim3((uint32_t)((nb + 255) / 256)), dim3(256), 0, ctx->stream, b->d_keys, nb, a->d_keys, na, lb_b);
    HIP_TRY(ctx, hipGetLastError());
    auto pass = [&](bool write, uint4* rec, uint64_t cap) -> int {
        for (uint64_t first = 0; first < na; first += WAVE_PER_ITEM_SPAN) {
            const dim3 grid((uint32_t)((std::min<uint64_t>(WAVE_PER_ITEM_SPAN, na - first) + 3) / 4));
            if (write) hipLaunchKernelGGL(db_diff_keys_kernel<true>, grid, dim3(256), 0, ctx->stream, A, B, lb_a, eps, cnt_a, d_tot, scan_a, scan_b, rec, cap, first);
            else hipLaunchKernelGGL(db_diff_keys_kernel<false>, grid, dim3(256), 0, ctx->stream, A, B, lb_a, eps, cnt_a, d_tot, scan_a, scan_b, rec, cap, first);
        }
        for (uint64_t first = 0; first < nb; first += WAVE_PER_ITEM_SPAN) {
            const dim3 grid((uint32_t)((std::min<uint64_t>(WAVE_PER_ITEM_SPAN, nb - first) + 3) / 4));
            if (write) hipLaunchKernelGGL(db_diff_only_b_kernel<true>, grid, dim3(256), 0, ctx->stream, B, a->d_keys, na, lb_b, cnt_b, d_tot, scan_a, scan_b, rec, cap, first);
            else hipLaunchKernelGGL(db_diff_only_b_kernel<false>, grid, dim3(256), 0, ctx->stream, B, a->d_keys, na, lb_b, cnt_b, d_tot, scan_a, scan_b, rec, cap, first);
        }
        HIP_TRY(ctx, hipGetLastError());
        return IPKGPU_OK;
    };
    RC_TRY(pass(false, nullptr, 0));
    RC_TRY(scan_u32(ctx, cnt_a, na, scan_a));
    RC_TRY(scan_u32(ctx, cnt_b, nb, scan_b));
    DbDiffTotals tot;
    uint64_t rec_a = 0, rec_b = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&rec_a, scan_a + na, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&rec_b, scan_b + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t want = std::min<uint64_t>(max_records, rec_a + rec_b);
    if (want) {
        uint4* d_rec = nullptr;
        struct RGuard { ipkgpu_ctx* c; uint4*& p; ~RGuard() { (void)hipStreamSynchronize(c->stream); ctx_release(c, p); } } rguard{ctx, d_rec};
        HIP_TRY(ctx, ctx_alloc(ctx, (void**)&d_rec, want * sizeof(uint4)));
        RC_TRY(pass(true, d_rec, want));
        HIP_TRY(ctx, hipMemcpyAsync(records, d_rec, want * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    const int e1 = sw.mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->t_diff_ms = sw.ms(e0, e1);
    counts->keys_a = na; counts->keys_b = nb; counts->keys_only_a = tot.keys_only_a; counts->keys_only_b = tot.keys_only_b;
    counts->entries_a = a->n_entries; counts->entries_b = b->n_entries;
    counts->entries_only_a = tot.entries_only_a; counts->entries_only_b = tot.entries_only_b;
    counts->scores_differ = tot.scores_differ; counts->positions_differ = tot.positions_differ;
    float dmax; memcpy(&dmax, &tot.max_diff_bits, 4);
    counts->max_abs_diff = (double)dmax;
    if (n_records) *n_records = want;
    return IPKGPU_OK;
}

}  // extern "C"
