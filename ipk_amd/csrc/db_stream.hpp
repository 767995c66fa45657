// db_stream.hpp -- ipkgpu_db_load_wanted: a database file through the device in bounded windows, only the records a k-mer set names
// staying (included by ipkgpu.hip behind db_select.hpp and db_kmerset.hpp; kernels_dbstream.hpp).
//
// The body travels as in ipkgpu_db_load -- file -> one of the two pinned buffers -> device, the next read under the previous copy, the
// host walking every chunk (ipkfmt::RecordWalker) before it leaves -- but into a window of "db_load_window_bytes", never into an image
// of the body.  A window holds whole records: it is closed at the start of the first record that would end beyond it, processed
// (heads, wanted flags, two scans, the wanted heads and entries appended to the kept arrays in file order) and the next one starts at
// that record.  A head that straddles two chunks has then up to 15 bytes in the closed window; they are moved to the new window's front
// on the device.  A record longer than the window finds it empty, grows the block and is a window of its own.  Behind the last window: the sort of (key, kept index),
// the arrays in key order, the entries gathered from file order into key order; then the selection at min_log_score over the result.
// Every temporary is taken through dev_malloc and given back before the call returns; the kept arrays double when they are full.
// The same load with a second predicate, a key range in place of the set, is ipkgpu_db_load_key_range; with the kept counts known
// beforehand (StreamKeep::expected) every block is taken once at its exact size; and without an output it is the histogram pass of
// ipkgpu_db_diff_files (db_diff_files.hpp), which keeps nothing.
#pragma once

namespace {

// a device block of the streamed load: grows by doubling, the first `used` bytes kept
struct StreamBuf {
    void* p = nullptr;
    size_t cap = 0;
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// exact: the block gets what is asked for and no more, and a block with nothing to keep is given back before the new one is taken (the
// loads whose sizes are known beforehand: their peak is the sum of what they hold, ipkgpu_db_diff_files plans by it)
int stream_grow(ipkgpu_ctx* ctx, StreamBuf& b, size_t used, size_t need, const char* what, bool exact = false)
{
    if (need <= b.cap && b.p) return IPKGPU_OK;
    need = std::max<size_t>(need, 256);
    size_t want = exact ? need : std::max(need, b.cap * 2);
    if (exact && b.p && !used) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)dev_free(ctx, b.p, b.cap);
        b.p = nullptr; b.cap = 0;
    }
    void* q = nullptr;
    hipError_t e = dev_malloc(ctx, &q, want);
    if (e != hipSuccess && want > need) { (void)hipGetLastError(); want = need; e = dev_malloc(ctx, &q, want); }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "no room for %s of the streamed load (%llu bytes): %s", what,
                    (unsigned long long)want, hipGetErrorString(e));
    }
    if (b.p) {
        hipError_t c = used ? hipMemcpyAsync(q, b.p, used, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
        if (c == hipSuccess) c = hipStreamSynchronize(ctx->stream);
        (void)dev_free(ctx, b.p, b.cap);
        b.p = nullptr; b.cap = 0;
        if (c != hipSuccess) { (void)dev_free(ctx, q, want); HIP_TRY(ctx, c); }
    }
    b.p = q; b.cap = want;
    return IPKGPU_OK;
}

// What a streamed pass over a file keeps, and what is known about the file beforehand.
struct StreamKeep {
    const ipkgpu_kmer_set* set = nullptr;        // the records whose key the set names (ipkgpu_db_load_wanted); without a set:
    uint64_t key_lo = 0, key_hi = 0;             // those with key_lo <= key < key_hi (ipkgpu_db_load_key_range)
    // expected: the kept records and entries are known (a histogram pass counted them).  The kept arrays are then allocated once at
    // that size, every other block at exactly what it needs; a file that holds more "changed between passes".
    bool expected = false;
    uint64_t exp_records = 0, exp_entries = 0;
    uint64_t window = 0;                         // the window's bytes (0: "db_load_window_bytes", or DB_STREAM_WINDOW)
    // in: the most records of one window and the longest record's bytes where a pass before has seen them (0: not known);
    // out: what this pass saw
    uint64_t n_w = 0, longest = 0;
    // the histogram pass (out == nullptr): nothing is kept; per window db_stream_hist_kernel over the heads
    uint32_t* rec_hist = nullptr; unsigned long long* ent_hist = nullptr; uint32_t shift = 0;
};

// R(prefix, K): the first min(keep_records, header total) records of the file restricted to the keys of keep.set (or of the key range),
// every kept key with all its entries, as a database with the head of the file (totals replaced).  t_load[8] = windows, [9] = records
// kept.  out == nullptr: the histogram pass.
int db_stream_load(ipkgpu_ctx* ctx, const char* path, StreamKeep& keep, uint64_t keep_records, ipkgpu_db** out)
{
    const ipkgpu_kmer_set* set = keep.set;
    const bool hist = out == nullptr, exact = keep.expected || hist;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    ipkgpu_db_file* file = nullptr;
    if (const int rc = ipkgpu_db_file_open(path, &file)) return fail(ctx, rc, "%s", ipkgpu_db_file_last_error());
    struct FileGuard { ipkgpu_db_file* f; ~FileGuard() { ipkgpu_db_file_close(f); } } fguard{file};
    ipkfmt::Head& hd = file->head;
    if (set) RC_TRY(set_fits(ctx, set, file));
    const bool whole = keep_records >= hd.total_kmers;
    const uint64_t n_total = hd.total_kmers, ne_total = hd.total_entries;
    const uint64_t body = file->body_bytes();
    const bool positioned = hd.positions_loaded;
    const uint64_t entry_bytes = positioned ? ipkfmt::ENTRY_POS_BYTES : ipkfmt::ENTRY_BYTES;
    if (n_total > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %llu k-mers: a database holds at most 2^32 - 1 (its order is 32-bit)", path, (unsigned long long)n_total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // every device block of the call but the result's; given back when the call returns, however it returns
    StreamBuf win, w_starts, w_sk, w_fvb, w_cnt, w_flag, w_cntw, w_fscan, w_cscan, w_segd, w_segs;      // the window and its per-record workspaces
    StreamBuf k_sk, k_fvb, k_cnt, k_eoff, k_ent, k_pos;                                               // the kept heads and entries, file order
    StreamBuf s_sorted, s_cnt, s_src, s_tmp;                                                          // behind the last window
    struct Blocks { ipkgpu_ctx* c; std::vector<StreamBuf*> all;
        ~Blocks() { (void)hipStreamSynchronize(c->stream); for (StreamBuf* b : all) if (b->p) { (void)dev_free(c, b->p, b->cap); b->p = nullptr; } (void)hipGetLastError(); } }
        blocks{ctx, {&win, &w_starts, &w_sk, &w_fvb, &w_cnt, &w_flag, &w_cntw, &w_fscan, &w_cscan, &w_segd, &w_segs, &k_sk, &k_fvb, &k_cnt, &k_eoff, &k_ent, &k_pos,
                     &s_sorted, &s_cnt, &s_src, &s_tmp}};

    const uint64_t chunk = std::min<uint64_t>(ctx->opt_load_chunk > 0 ? (uint64_t)ctx->opt_load_chunk : SPILL_STAGE, SPILL_STAGE);
    // the window's capacity in record bytes; the block has 16 bytes more for the head a chunk may end in, and 16 for the aligned dwords
    // the positioned entries are read as (the last one two bytes past its end)
    const uint64_t cap = std::max<uint64_t>(std::min<uint64_t>(keep.window ? keep.window : ctx->opt_load_window > 0 ? (uint64_t)ctx->opt_load_window : DB_STREAM_WINDOW, body),
                                            ipkfmt::RECORD_HEAD_BYTES);
    constexpr uint64_t WIN_SLACK = 32;
    ipkfmt::RecordWalker walk;
    walk.begin(hd.body_at, body, positioned, n_total, whole ? ~(uint64_t)0 : keep_records);
    double t_read = 0, t_walk = 0, t_wait = 0, t_device = 0;
    uint64_t bytes_read = 0, w_lo = 0, r0 = 0, r_seen = 0, kept = 0, kept_e = 0, n_windows = 0, seen_n_w = 0, seen_longest = 0;
    std::vector<uint64_t> rel;
    const uint64_t n_w_first = std::min<uint64_t>(keep.n_w, n_total);      // (a window has at most the file's records, whatever the caller says)

    // the records [r0, r1) of the window that starts at body offset w_lo: their wanted ones to the end of the kept arrays
    auto process = [&](uint64_t r1) -> int {
        const uint64_t nw = r1 - r0;
        if (nw == 0) return IPKGPU_OK;
        const auto t0 = std::chrono::steady_clock::now();
        seen_n_w = std::max(seen_n_w, nw);
        const uint64_t na = std::max(nw, n_w_first);                         // (the workspaces at once at the known most, where it is known)
        RC_TRY(stream_grow(ctx, w_starts, 0, na * 8, "a window's record starts", exact));
        RC_TRY(stream_grow(ctx, w_sk, 0, na * 8, "a window's keys", exact));
        RC_TRY(stream_grow(ctx, w_fvb, 0, na * 4, "a window's filter values", exact));
        RC_TRY(stream_grow(ctx, w_cnt, 0, na * 4, "a window's counts", exact));
        if (!hist) {
            RC_TRY(stream_grow(ctx, w_flag, 0, na * 4, "a window's flags", exact));
            RC_TRY(stream_grow(ctx, w_cntw, 0, na * 4, "a window's wanted counts", exact));
            RC_TRY(stream_grow(ctx, w_fscan, 0, (na + 1) * 8, "a window's flag scan", exact));
            RC_TRY(stream_grow(ctx, w_cscan, 0, (na + 1) * 8, "a window's count scan", exact));
            RC_TRY(stream_grow(ctx, w_segd, 0, (na + 1) * 8, "a window's segments", exact));
            RC_TRY(stream_grow(ctx, w_segs, 0, na * 8, "a window's segments", exact));
        }
        try { rel.resize(nw); } catch (const std::bad_alloc&) { return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory"); }
        for (uint64_t i = 0; i < nw; ++i) rel[i] = walk.starts[r0 + i] - w_lo;
        HIP_TRY(ctx, hipMemcpyAsync(w_starts.p, rel.data(), nw * 8, hipMemcpyHostToDevice, ctx->stream));
        const uint32_t nb = (uint32_t)((nw + 255) / 256);
        const unsigned char* image = win.as<unsigned char>();
        if (positioned) hipLaunchKernelGGL(db_unpack_heads_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, image, w_starts.as<uint64_t>(), nw,
                                           w_sk.as<unsigned long long>(), w_fvb.as<uint32_t>(), w_cnt.as<uint32_t>());
        else hipLaunchKernelGGL(db_unpack_heads_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, image, w_starts.as<uint64_t>(), nw,
                                w_sk.as<unsigned long long>(), w_fvb.as<uint32_t>(), w_cnt.as<uint32_t>());
        if (hist) {
            hipLaunchKernelGGL(db_stream_hist_kernel, dim3(nb), dim3(256), 0, ctx->stream, w_sk.as<unsigned long long>(), w_cnt.as<uint32_t>(), nw, keep.shift,
                               keep.rec_hist, keep.ent_hist);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                 // (`rel` is written again for the next window)
            ++n_windows;
            t_device += since(t0);
            return IPKGPU_OK;
        }
        if (set) hipLaunchKernelGGL(db_stream_flag_kernel, dim3(nb), dim3(256), 0, ctx->stream, w_sk.as<unsigned long long>(), w_cnt.as<uint32_t>(), nw, set->d_words,
                                    set->n_codes, w_flag.as<uint32_t>(), w_cntw.as<uint32_t>());
        else hipLaunchKernelGGL(db_stream_flag_range_kernel, dim3(nb), dim3(256), 0, ctx->stream, w_sk.as<unsigned long long>(), w_cnt.as<uint32_t>(), nw, keep.key_lo,
                                keep.key_hi, w_flag.as<uint32_t>(), w_cntw.as<uint32_t>());
        HIP_TRY(ctx, hipGetLastError());
        RC_TRY(scan_u32(ctx, w_flag.as<uint32_t>(), nw, w_fscan.as<uint64_t>()));
        RC_TRY(scan_u32(ctx, w_cntw.as<uint32_t>(), nw, w_cscan.as<uint64_t>()));
        uint64_t kw = 0, ew = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&kw, w_fscan.as<uint64_t>() + nw, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&ew, w_cscan.as<uint64_t>() + nw, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // (every count is one the walk accepted: the window's wanted entries are at most its records' entries, which lie inside it)
        if (kw > nw || ew > win.cap / entry_bytes)
            return fail(ctx, IPKGPU_ERR_HIP, "%s: a window's scans disagree with the walk: %llu records and %llu entries wanted of %llu records", path,
                        (unsigned long long)kw, (unsigned long long)ew, (unsigned long long)nw);
        // (with expected counts the kept arrays have exactly that room: nothing is written beyond it)
        if (keep.expected && (kept + kw > keep.exp_records || kept_e + ew > keep.exp_entries))
            return fail(ctx, IPKGPU_ERR_INVALID, "%s: the file changed between passes: more than the %llu records and %llu entries counted before have keys in [%llu, %llu)",
                        path, (unsigned long long)keep.exp_records, (unsigned long long)keep.exp_entries, (unsigned long long)keep.key_lo, (unsigned long long)keep.key_hi);
        if (kw) {
            RC_TRY(stream_grow(ctx, k_sk, kept * 8, (kept + kw) * 8, "the kept keys"));
            RC_TRY(stream_grow(ctx, k_fvb, kept * 4, (kept + kw) * 4, "the kept filter values"));
            RC_TRY(stream_grow(ctx, k_cnt, kept * 4, (kept + kw) * 4, "the kept counts"));
            RC_TRY(stream_grow(ctx, k_eoff, kept * 8, (kept + kw) * 8, "the kept entry offsets"));
            if (ew) {
                RC_TRY(stream_grow(ctx, k_ent, kept_e * 8, (kept_e + ew) * 8, "the kept entries"));
                if (positioned) RC_TRY(stream_grow(ctx, k_pos, kept_e * 4, (kept_e + ew) * 4, "the kept positions"));
            }
            hipLaunchKernelGGL(db_stream_append_kernel, dim3(nb), dim3(256), 0, ctx->stream, w_sk.as<unsigned long long>(), w_fvb.as<uint32_t>(), w_cnt.as<uint32_t>(),
                               w_starts.as<uint64_t>(), w_flag.as<uint32_t>(), w_fscan.as<uint64_t>(), w_cscan.as<uint64_t>(), nw, kept, kept_e,
                               k_sk.as<unsigned long long>(), k_fvb.as<uint32_t>(), k_cnt.as<uint32_t>(), k_eoff.as<uint64_t>(), w_segd.as<uint64_t>(),
                               w_segs.as<uint64_t>());
            if (ew) {
                const uint32_t tiles = (uint32_t)((ew + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE);
                if (positioned) hipLaunchKernelGGL(db_unpack_entries_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, image, w_segd.as<uint64_t>(),
                                                   w_segs.as<uint64_t>(), kw, ew, k_ent.as<uint2>() + kept_e, k_pos.as<uint32_t>() + kept_e);
                else hipLaunchKernelGGL(db_unpack_entries_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, image, w_segd.as<uint64_t>(), w_segs.as<uint64_t>(),
                                        kw, ew, k_ent.as<uint2>() + kept_e, (uint32_t*)nullptr);
            }
            HIP_TRY(ctx, hipGetLastError());
        }
        kept += kw; kept_e += ew; ++n_windows;
        t_device += since(t0);
        return IPKGPU_OK;
    };

    {
        FILE* fh = fopen(path, "rb");
        if (!fh) return fail(ctx, IPKGPU_ERR_INVALID, "cannot open %s", path);
        struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fh};
        setvbuf(fh, nullptr, _IONBF, 0);
        if (fseeko(fh, (off_t)hd.body_at, SEEK_SET) != 0) return fail(ctx, IPKGPU_ERR_INVALID, "%s: seek failed", path);
        RC_TRY(spill_stage(ctx, (size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(body, 1))));
        if (body && keep_records) RC_TRY(stream_grow(ctx, win, 0, std::max(cap, std::min(keep.longest, body)) + WIN_SLACK, "the window", exact));
        if (keep.expected && keep.exp_records) {                             // the kept arrays, once
            RC_TRY(stream_grow(ctx, k_sk, 0, keep.exp_records * 8, "the kept keys", true));
            RC_TRY(stream_grow(ctx, k_fvb, 0, keep.exp_records * 4, "the kept filter values", true));
            RC_TRY(stream_grow(ctx, k_cnt, 0, keep.exp_records * 4, "the kept counts", true));
            RC_TRY(stream_grow(ctx, k_eoff, 0, keep.exp_records * 8, "the kept entry offsets", true));
            if (keep.exp_entries) {
                RC_TRY(stream_grow(ctx, k_ent, 0, keep.exp_entries * 8, "the kept entries", true));
                if (positioned) RC_TRY(stream_grow(ctx, k_pos, 0, keep.exp_entries * 4, "the kept positions", true));
            }
        }
        uint64_t j = 0;
        for (uint64_t lo = 0; lo < body && keep_records && !(walk.done() && lo >= walk.pos); lo += chunk, ++j) {
            const uint64_t hi = std::min(body, lo + chunk);
            const int b = (int)(j & 1);
            auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev_spill[b]));        // (the copies out of this buffer two chunks ago; at once on a fresh event)
            t_wait += since(t0); t0 = std::chrono::steady_clock::now();
            uint8_t* src = static_cast<uint8_t*>(ctx->h_spill[b]);
            if (fread(src, 1, (size_t)(hi - lo), fh) != hi - lo) return fail(ctx, IPKGPU_ERR_INVALID, "%s: read failed", path);
            bytes_read = hi;
            t_read += since(t0); t0 = std::chrono::steady_clock::now();
            if (!walk.feed(src, lo, hi)) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %s", path, walk.error.c_str());
            t_walk += since(t0);
            if (walk.max_count > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: a k-mer with 2^32 entries or more", path);
            uint64_t cur = lo;                                               // the chunk's bytes below `cur` are in the window
            auto to_window = [&](uint64_t upto) -> int {
                if (upto > cur) {
                    HIP_TRY(ctx, hipMemcpyAsync(win.as<unsigned char>() + (cur - w_lo), src + (cur - lo), (size_t)(upto - cur), hipMemcpyHostToDevice, ctx->stream));
                    cur = upto;
                }
                return IPKGPU_OK;
            };
            for (uint64_t r = r_seen; r < walk.starts.size(); ++r) {
                const uint64_t s = walk.starts[r], e = r + 1 < walk.starts.size() ? walk.starts[r + 1] : walk.pos;
                seen_longest = std::max(seen_longest, e - s);
                if (e - w_lo <= cap) continue;
                if (r > r0) {                                                // the window is closed at this record's start
                    RC_TRY(to_window(s));
                    RC_TRY(process(r));
                    // (a head that straddles two chunks: its first bytes came with the last chunk; 16 bytes or more lie before them)
                    if (cur > s) HIP_TRY(ctx, hipMemcpyAsync(win.p, win.as<unsigned char>() + (s - w_lo), (size_t)(cur - s), hipMemcpyDeviceToDevice, ctx->stream));
                    w_lo = s; r0 = r;
                }
                // one record longer than the window, which is empty: the block grows to hold it (and stays so); the record is a window of
                // its own, for the cuts go on by "db_load_window_bytes"
                RC_TRY(stream_grow(ctx, win, (size_t)(cur > w_lo ? cur - w_lo : 0), (size_t)(e - w_lo + WIN_SLACK), "the window (one record is longer than it)", exact));
            }
            r_seen = walk.starts.size();
            RC_TRY(to_window(walk.done() ? std::min(hi, walk.pos) : hi));
            HIP_TRY(ctx, hipEventRecord(ctx->ev_spill[b], ctx->stream));
        }
    }
    if (whole) {
        if (!walk.finish(n_total, ne_total)) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %s", path, walk.error.c_str());
    } else if (keep_records && (!walk.done() || walk.pos > bytes_read)) {
        return fail(ctx, IPKGPU_ERR_INVALID, "%s: the file ends before record %llu of the first %llu has ended", path, (unsigned long long)walk.starts.size(),
                    (unsigned long long)keep_records);
    }
    RC_TRY(process(walk.starts.size()));
    keep.n_w = seen_n_w; keep.longest = seen_longest;
    auto times = [&]() {
        ctx->t_load[1] = t_read; ctx->t_load[2] = t_walk; ctx->t_load[3] = t_wait;
        ctx->t_load[4] = 0; ctx->t_load[5] = 0; ctx->t_load[6] = t_device * 1e3;
        ctx->t_load[7] = (double)bytes_read; ctx->t_load[8] = (double)n_windows; ctx->t_load[9] = (double)kept;
        ctx->t_load[0] = since(t_begin);
    };
    if (hist) { times(); return IPKGPU_OK; }
    if ((kept_e + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE > 0x7FFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: too many entries for one launch", path);

    // the kept heads into key order, the kept entries behind them
    const auto t_final = std::chrono::steady_clock::now();
    ipkgpu_db* db = new (std::nothrow) ipkgpu_db();
    if (!db) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    db->ctx = ctx;
    struct Guard { ipkgpu_db* r; ~Guard() { if (r) ipkgpu_db_free(r); } } guard{db};
    RC_TRY(db_alloc_arrays(ctx, db, kept, kept_e, positioned));
    if (kept == 0) {
        HIP_TRY(ctx, hipMemsetAsync(db->d_key_off, 0, 8, ctx->stream));
    } else {
        RC_TRY(stream_grow(ctx, s_sorted, 0, kept * 8, "the sorted keys", exact));
        RC_TRY(stream_grow(ctx, s_cnt, 0, kept * 4, "the counts in key order", exact));
        RC_TRY(stream_grow(ctx, s_src, 0, kept * 8, "the entry offsets in key order", exact));
        uint32_t* d_dup = small_at(ctx, SMALL_REC_BIG);
        HIP_TRY(ctx, hipMemsetAsync(d_dup, 0, 4, ctx->stream));
        size_t tmp_bytes = 0;
        HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, tmp_bytes, k_sk.as<unsigned long long>(), s_sorted.as<unsigned long long>(), (size_t)kept, 0, 64, ctx->stream));
        RC_TRY(stream_grow(ctx, s_tmp, 0, tmp_bytes, "the sort's workspace", exact));
        HIP_TRY(ctx, rocprim::radix_sort_keys(s_tmp.p, tmp_bytes, k_sk.as<unsigned long long>(), s_sorted.as<unsigned long long>(), (size_t)kept, 0, 64, ctx->stream));
        const uint32_t nb = (uint32_t)((kept + 255) / 256);
        hipLaunchKernelGGL(db_load_order_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, s_sorted.as<unsigned long long>(), k_eoff.as<uint64_t>(), k_fvb.as<uint32_t>(),
                           k_cnt.as<uint32_t>(), kept, db->d_keys, s_cnt.as<uint32_t>(), s_src.as<uint64_t>(), db->d_fv32, db->d_fv64, db->d_order, d_dup);
        HIP_TRY(ctx, hipGetLastError());
        RC_TRY(scan_u32(ctx, s_cnt.as<uint32_t>(), kept, db->d_key_off));
        uint32_t h_dup = 0;
        uint64_t h_total = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&h_dup, d_dup, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&h_total, db->d_key_off + kept, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (h_dup) return fail(ctx, IPKGPU_ERR_INVALID, "%s: a k-mer has more than one record", path);
        if (h_total != kept_e) return fail(ctx, IPKGPU_ERR_HIP, "%s: the device counted %llu kept entries, the windows %llu", path, (unsigned long long)h_total, (unsigned long long)kept_e);
        if (kept_e) {
            const uint32_t tiles = (uint32_t)((kept_e + DB_UNPACK_TILE - 1) / DB_UNPACK_TILE);
            if (positioned) hipLaunchKernelGGL(db_stream_gather_kernel<true>, dim3(tiles), dim3(256), 0, ctx->stream, db->d_key_off, s_src.as<uint64_t>(), kept, kept_e,
                                               k_ent.as<uint2>(), k_pos.as<uint32_t>(), db->d_entries, db->d_positions);
            else hipLaunchKernelGGL(db_stream_gather_kernel<false>, dim3(tiles), dim3(256), 0, ctx->stream, db->d_key_off, s_src.as<uint64_t>(), kept, kept_e,
                                    k_ent.as<uint2>(), (const uint32_t*)nullptr, db->d_entries, (uint32_t*)nullptr);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    t_device += since(t_final);
    db->t_merge = t_device * 1e3;
    hd.total_kmers = kept; hd.total_entries = kept_e;
    file->file_bytes = hd.body_at + ipkfmt::RECORD_HEAD_BYTES * kept + entry_bytes * kept_e;
    file->walked = true; file->n_records = kept; file->n_entries = kept_e; file->max_count = walk.max_count;
    db->file = file; fguard.f = nullptr;
    times();
    guard.r = nullptr;
    *out = db;
    return IPKGPU_OK;
}

}  // namespace

extern "C" {

int ipkgpu_db_load_wanted(ipkgpu_ctx* ctx, const char* path, const ipkgpu_kmer_set* set, uint64_t keep_kmers, float min_log_score, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!path || !out) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument");
    if (!set || set->ctx != ctx) return fail(ctx, IPKGPU_ERR_INVALID, "a k-mer set of this context is needed");
    if (min_log_score != min_log_score) return fail(ctx, IPKGPU_ERR_INVALID, "min_log_score is NaN");
    ipkgpu_db* restricted = nullptr;
    StreamKeep keep;
    keep.set = set;
    RC_TRY(db_stream_load(ctx, path, keep, keep_kmers, &restricted));
    // the selection's steps 2 and 3 over the kept records (every one a candidate): entries at or below the score go, and keys left without one
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = db_select(ctx, restricted, ~(uint64_t)0, min_log_score, out);
    ipkgpu_db_free(restricted);
    ctx->t_load[0] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // extern "C"
