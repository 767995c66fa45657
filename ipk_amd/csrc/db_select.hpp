// db_select.hpp -- ipkgpu_db_select / ipkgpu_db_load_select: the consumer of the filter order (included by ipkgpu.hip behind db_load.hpp;
// kernels_dbselect.hpp).
//
// The selection -- the first M k-mers in filter order, of those the entries with score > t -- is defined in include/ipkgpu.h.  It is
// this library's own definition: the reference reads a database with i2l::load(file, mu, omega), which is un-vendored and could not be
// read, so nothing here is pinned against it.
// ipkgpu_db_select: flags, three scans (scan_u32), one wait for the three totals (entries, keys, surviving records), then the compacting copies; the source is only read.
// ipkgpu_db_load_select: db_load_records (db_load.hpp) brings the first min(M, header total) records onto the device as a database of
// their own -- the selection of those records at t equals the selection of the whole file's database at (M, t), array for array --
// then the same selection, and the prefix database is freed.
#pragma once

namespace {

// The head a selection carries: the source's with the totals replaced (omega stays: the call takes t, not omega).
ipkgpu_db_file* select_head(const ipkgpu_db_file* src, uint64_t n, uint64_t ne)
{
    if (!src) return nullptr;
    ipkgpu_db_file* f = new (std::nothrow) ipkgpu_db_file(*src);
    if (!f) return nullptr;
    f->head.total_kmers = n; f->head.total_entries = ne;
    f->file_bytes = f->head.body_at + ipkfmt::RECORD_HEAD_BYTES * n + (f->head.positions_loaded ? ipkfmt::ENTRY_POS_BYTES : ipkfmt::ENTRY_BYTES) * ne;
    f->walked = true; f->n_records = n; f->n_entries = ne; f->max_count = std::min(f->max_count, ne);
    return f;
}

// Is `set` a k-mer set of this context over the codes of the file head `file` (NULL: nothing to compare with)?
int set_fits(ipkgpu_ctx* ctx, const ipkgpu_kmer_set* set, const ipkgpu_db_file* file)
{
    if (!set || set->ctx != ctx) return fail(ctx, IPKGPU_ERR_INVALID, "a k-mer set of this context is needed");
    if (file && (file->head.sequence_type != (set->sigma == 4 ? "DNA" : "AA") || file->head.kmer_size != set->k))
        return fail(ctx, IPKGPU_ERR_INVALID, "the k-mer set is of sigma %u and k = %u, the database's file of %s and k = %llu", set->sigma, set->k,
                    file->head.sequence_type.c_str(), (unsigned long long)file->head.kmer_size);
    return IPKGPU_OK;
}

// set == NULL: the selection at (keep_kmers, t).  With a set (ipkgpu_db_select_keys; keep_kmers and t are not looked at): the
// candidates are the keys in the set, a candidate keeps every entry and stays even without one -- the same scans and copies.
int db_select(ipkgpu_ctx* ctx, const ipkgpu_db* src, uint64_t keep_kmers, float t, ipkgpu_db** out, const ipkgpu_kmer_set* set = nullptr)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!src || !out || src->ctx != ctx) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument: a database of this context and an out pointer are needed");
    if (t != t) return fail(ctx, IPKGPU_ERR_INVALID, "min_log_score is NaN");
    if (!src->d_fv32 || !src->d_fv64 || !src->d_order)
        return fail(ctx, IPKGPU_ERR_INVALID, "the database has no filter values and order (filter it, or load it from a file): nothing to select by");
    if (set) RC_TRY(set_fits(ctx, set, src->file));
    const uint64_t n = src->n_keys, ne = src->n_entries, m = set ? n : std::min(keep_kmers, n);
    const bool positioned = src->d_positions != nullptr;
    if ((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE > 0x7FFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "too many entries for one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    ipkgpu_db* db = new (std::nothrow) ipkgpu_db();
    if (!db) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    db->ctx = ctx;
    struct Guard { ipkgpu_db* r; ~Guard() { if (r) ipkgpu_db_free(r); } } guard{db};
    Stopwatch sw(ctx->stream, &ctx->events);
    const int e0 = sw.mark();
    uint64_t n_out = 0, ne_out = 0;
    const uint32_t kb = (uint32_t)((n + 255) / 256), mb = (uint32_t)((m + 255) / 256);
    const uint32_t tiles = (uint32_t)((ne + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE);
    uint32_t *d_cand = nullptr, *d_keep = nullptr, *d_key_keep = nullptr, *d_rec_keep = nullptr;
    uint64_t *d_e_scan = nullptr, *d_k_scan = nullptr, *d_r_scan = nullptr;
    if (set ? n != 0 : (m && ne)) {                           // (no candidate or no entry at all: the empty selection, nothing launched)
        // workspaces: per entry the keep flag and its scan; per key the candidate flag, the key's flag and its scan; per record i < M the same
        RC_TRY(ensure(ctx, ctx->tmp_a, ne * 4));
        RC_TRY(ensure(ctx, ctx->tmp_b, (ne + 1) * 8));
        RC_TRY(ensure(ctx, ctx->counts, n * 4));
        RC_TRY(ensure(ctx, ctx->sp_pops, n * 4));
        RC_TRY(ensure(ctx, ctx->goff, (n + 1) * 8));
        RC_TRY(ensure(ctx, ctx->sp_c16, m * 4));
        RC_TRY(ensure(ctx, ctx->sp_rank, (m + 1) * 8));
        d_keep = ctx->tmp_a.as<uint32_t>(); d_e_scan = ctx->tmp_b.as<uint64_t>();
        d_cand = ctx->counts.as<uint32_t>(); d_key_keep = ctx->sp_pops.as<uint32_t>(); d_k_scan = ctx->goff.as<uint64_t>();
        d_rec_keep = ctx->sp_c16.as<uint32_t>(); d_r_scan = ctx->sp_rank.as<uint64_t>();
        if (set) {
            hipLaunchKernelGGL(db_select_wanted_kernel, dim3(kb), dim3(256), 0, ctx->stream, src->d_keys, n, set->d_words, set->n_codes, d_cand);
            if (ne) hipLaunchKernelGGL((db_select_flag_kernel<false, false>), dim3(tiles), dim3(256), 0, ctx->stream, src->d_entries, src->d_key_off, d_cand, n, ne, t, d_keep);
            d_key_keep = d_cand;                              // (a wanted key stays, with or without entries)
        } else if (m < n) {
            HIP_TRY(ctx, hipMemsetAsync(d_cand, 0, n * 4, ctx->stream));
            hipLaunchKernelGGL(db_select_mark_kernel, dim3(mb), dim3(256), 0, ctx->stream, src->d_order, m, d_cand);
            hipLaunchKernelGGL(db_select_flag_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, src->d_entries, src->d_key_off, d_cand, n, ne, t, d_keep);
        } else {
            hipLaunchKernelGGL(db_select_flag_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, src->d_entries, src->d_key_off, (const uint32_t*)nullptr, n, ne, t, d_keep);
        }
        HIP_TRY(ctx, hipGetLastError());
        RC_TRY(scan_u32(ctx, d_keep, ne, d_e_scan));
        if (!set) hipLaunchKernelGGL(db_select_keys_kernel, dim3(kb), dim3(256), 0, ctx->stream, src->d_key_off, d_e_scan, n, d_key_keep);
        HIP_TRY(ctx, hipGetLastError());
        RC_TRY(scan_u32(ctx, d_key_keep, n, d_k_scan));
        hipLaunchKernelGGL(db_select_records_kernel, dim3(mb), dim3(256), 0, ctx->stream, src->d_order, d_key_keep, m, d_rec_keep);
        HIP_TRY(ctx, hipGetLastError());
        RC_TRY(scan_u32(ctx, d_rec_keep, m, d_r_scan));
        uint64_t r_out = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&ne_out, d_e_scan + ne, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&n_out, d_k_scan + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&r_out, d_r_scan + m, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (n_out > n || ne_out > ne || r_out != n_out)
            return fail(ctx, IPKGPU_ERR_HIP, "the selection's scans disagree: %llu keys, %llu records, %llu entries kept of %llu and %llu",
                        (unsigned long long)n_out, (unsigned long long)r_out, (unsigned long long)ne_out, (unsigned long long)n, (unsigned long long)ne);
    }
    RC_TRY(db_alloc_arrays(ctx, db, n_out, ne_out, positioned));
    if (n_out == 0) {                                         // (a kept key has a kept entry: no key, no entry)
        HIP_TRY(ctx, hipMemsetAsync(db->d_key_off, 0, 8, ctx->stream));
    } else {
        if (!ne) {}
        else if (positioned) hipLaunchKernelGGL(db_select_copy_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, src->d_entries, src->d_positions, d_keep, d_e_scan, ne,
                                           db->d_entries, db->d_positions);
        else hipLaunchKernelGGL(db_select_copy_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, src->d_entries, (const uint32_t*)nullptr, d_keep, d_e_scan, ne,
                                db->d_entries, (uint32_t*)nullptr);
        hipLaunchKernelGGL(db_select_compact_kernel, dim3(kb), dim3(256), 0, ctx->stream, src->d_keys, src->d_key_off, src->d_fv32, src->d_fv64, d_key_keep, d_k_scan,
                           d_e_scan, n, n_out, ne_out, db->d_keys, db->d_key_off, db->d_fv32, db->d_fv64);
        hipLaunchKernelGGL(db_select_order_kernel, dim3(mb), dim3(256), 0, ctx->stream, src->d_order, d_rec_keep, d_r_scan, d_k_scan, m, db->d_order);
        HIP_TRY(ctx, hipGetLastError());
    }
    const int e1 = sw.mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    db->t_merge = sw.ms(e0, e1);
    ctx->t_select_ms = db->t_merge;
    if (src->file) {
        db->file = select_head(src->file, n_out, ne_out);
        if (!db->file) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    }
    guard.r = nullptr;
    *out = db;
    return IPKGPU_OK;
}

}  // namespace

extern "C" {

uint64_t ipkgpu_db_mu_kmers(double mu, uint64_t n_kmers)
{
    if (!(mu > 0.0)) return 0;                                // (NaN as well: the callers refuse it)
    if (mu >= 1.0) return n_kmers;
    return std::min<uint64_t>(n_kmers, (uint64_t)std::ceil(mu * (double)n_kmers));
}

double ipkgpu_db_select_time_ms(const ipkgpu_ctx* ctx) { return ctx ? ctx->t_select_ms : 0; }

int ipkgpu_db_select(ipkgpu_ctx* ctx, const ipkgpu_db* src, uint64_t keep_kmers, float min_log_score, ipkgpu_db** out)
{
    return db_select(ctx, src, keep_kmers, min_log_score, out);
}

int ipkgpu_db_select_keys(ipkgpu_ctx* ctx, const ipkgpu_db* src, const ipkgpu_kmer_set* set, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!set) return fail(ctx, IPKGPU_ERR_INVALID, "a k-mer set of this context is needed");
    return db_select(ctx, src, ~(uint64_t)0, 0.0f, out, set);
}

int ipkgpu_db_load_select(ipkgpu_ctx* ctx, const char* path, uint64_t keep_kmers, float min_log_score, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!path || !out) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument");
    if (min_log_score != min_log_score) return fail(ctx, IPKGPU_ERR_INVALID, "min_log_score is NaN");
    ipkgpu_db* prefix = nullptr;
    RC_TRY(db_load_records(ctx, path, keep_kmers, &prefix));
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = db_select(ctx, prefix, keep_kmers, min_log_score, out);
    ipkgpu_db_free(prefix);
    ctx->t_load[0] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // extern "C"
