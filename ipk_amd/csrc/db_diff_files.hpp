// db_diff_files.hpp -- ipkgpu_db_diff_files: two database files compared by key ranges, neither ever resident whole (included by
// ipkgpu.hip behind db_stream.hpp).
//
// ipkgpu_db_diff composes exactly over disjoint ascending key ranges: every count adds, max_abs_diff is the maximum, the record list
// is the concatenation.  So: a plan of ranges that each fit the device (the memory formula of include/ipkgpu.h, restated here as
// diff_files_range_bytes), per range the key-range load of A, of B (db_stream_load with its second predicate), ipkgpu_db_diff, and
// both range databases freed.  The plan comes from one histogram pass over each file (db_stream_hist_kernel: records and entries per
// key bin, 65 536 bins) and a greedy cut from bin 0 upward; where the formula at the heads' totals fits there is one range and no
// histogram pass.  Every pass over a file walks it and checks its end and its totals.
#pragma once

namespace {

inline uint64_t df_m(uint64_t x) { return std::max<uint64_t>(x, 256); }                          // a block of the streamed load
inline uint64_t df_r(uint64_t x) { return std::max<uint64_t>((x + 255) & ~(uint64_t)255, 256); }   // an array of a database (ctx_alloc)
inline uint64_t df_e(uint64_t x) { return std::max<uint64_t>(x, 16); }                           // an `ensure` workspace taken anew
// rocprim's own space, bounded from its sources (device_radix_sort.hpp, device_scan.hpp): the one-sweep sort of n 64-bit keys takes
// the n keys again, at most 256 x 8 digit counters of 8 bytes twice over, and 256 four-byte look-back states per block of at least
// 1024 keys (<= n + 1024 bytes); the merge sort of short inputs takes the keys again and less beside them.  The look-back scan of n
// 64-bit sums takes 16 bytes per block of at least 256 items and 64 blocks more.
inline uint64_t df_sort(uint64_t n) { return 9 * n + 32768; }
inline uint64_t df_scan(uint64_t n) { return n / 8 + 4096; }
// scan_sums is an `ensure` workspace that may grow inside a range: a regrown one gets a sixteenth more
inline uint64_t df_scanx(uint64_t n) { const uint64_t s = df_scan(n); return s + s / 16 + 16; }

inline uint64_t df_db(uint64_t n, uint64_t e, bool pos)
{
    return 3 * df_r(4 * n) + df_r(8 * (n + 1)) + df_r(8 * n) + df_r(8 * e) + (pos ? df_r(4 * e) : 0);
}
inline uint64_t df_load(uint64_t n, uint64_t e, bool pos)
{
    const uint64_t kept = 2 * df_m(8 * n) + 2 * df_m(4 * n) + df_m(8 * e) + (pos ? df_m(4 * e) : 0);
    const uint64_t sorted = 2 * df_m(8 * n) + df_m(4 * n) + df_m(df_sort(n));
    return kept + df_db(n, e, pos) + sorted;
}

}  // namespace

extern "C" {

uint64_t ipkgpu_db_stream_window_bytes(uint64_t window, uint64_t n_w, uint64_t longest)
{
    return (window + 32) + (longest > window ? longest + 32 : 0) + 3 * df_m(8 * n_w) + 4 * df_m(4 * n_w) + 3 * df_m(8 * (n_w + 1)) + df_scanx(n_w + 1);
}

uint64_t ipkgpu_db_diff_files_range_bytes(uint64_t fixed, uint64_t n_a, uint64_t e_a, int positioned_a, uint64_t n_b, uint64_t e_b, int positioned_b,
                                          uint64_t max_records)
{
    const bool pa = positioned_a != 0, pb = positioned_b != 0;
    const uint64_t load_a = fixed + df_load(n_a, e_a, pa);
    const uint64_t load_b = fixed + df_db(n_a, e_a, pa) + df_load(n_b, e_b, pb);
    const uint64_t na1 = std::max<uint64_t>(n_a, 1), nb1 = std::max<uint64_t>(n_b, 1);
    const uint64_t ws = 2 * df_e(4 * na1) + df_e(8 * (n_a + 1)) + 2 * df_e(4 * nb1) + df_e(8 * (n_b + 1)) + 64;
    const uint64_t rec = df_r(16 * std::min<uint64_t>(max_records, e_a + e_b));
    const uint64_t diff = df_db(n_a, e_a, pa) + df_db(n_b, e_b, pb) + ws + rec;
    return std::max(load_a, std::max(load_b, diff)) + df_scanx(std::max(n_a, n_b) + 1);
}

uint64_t ipkgpu_db_diff_files_num_ranges(const ipkgpu_ctx* ctx) { return ctx ? ctx->dfiles_ranges.size() / 2 : 0; }
int ipkgpu_db_diff_files_range(const ipkgpu_ctx* ctx, uint64_t i, uint64_t* key_lo, uint64_t* key_hi)
{
    if (!ctx || !key_lo || !key_hi || i >= ctx->dfiles_ranges.size() / 2) return IPKGPU_ERR_INVALID;
    *key_lo = ctx->dfiles_ranges[2 * i]; *key_hi = ctx->dfiles_ranges[2 * i + 1];
    return IPKGPU_OK;
}
double ipkgpu_db_diff_files_stat(const ipkgpu_ctx* ctx, int which) { return ctx && which >= 0 && which < 12 ? ctx->dfiles_stat[which] : 0; }

int ipkgpu_db_load_key_range(ipkgpu_ctx* ctx, const char* path, uint64_t key_lo, uint64_t key_hi, ipkgpu_db** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!path || !out) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument");
    if (key_hi > ((uint64_t)1 << 32) || key_lo > key_hi)
        return fail(ctx, IPKGPU_ERR_INVALID, "a key range [lo, hi) needs lo <= hi <= 2^32, not [%llu, %llu)", (unsigned long long)key_lo, (unsigned long long)key_hi);
    StreamKeep keep;
    keep.key_lo = key_lo; keep.key_hi = key_hi;
    return db_stream_load(ctx, path, keep, ~(uint64_t)0, out);
}

int ipkgpu_db_diff_files(ipkgpu_ctx* ctx, const char* path_a, const char* path_b, double eps, ipkgpu_db_diff_counts* counts,
                         ipkgpu_db_diff_record* records, uint64_t max_records, uint64_t* n_records)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (n_records) *n_records = 0;
    if (!path_a || !path_b) return fail(ctx, IPKGPU_ERR_INVALID, "two paths are needed");
    if (!counts || (max_records && (!records || !n_records))) return fail(ctx, IPKGPU_ERR_INVALID, "null argument");
    if (!(eps >= 0.0)) return fail(ctx, IPKGPU_ERR_INVALID, "eps must not be negative (0 = equal score bits)");
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    ctx->dfiles_ranges.clear();
    for (double& s : ctx->dfiles_stat) s = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // the two heads: totals, entry widths, the key bits
    struct Side { const char* path; uint64_t n = 0, e = 0, body = 0, window = 0, n_w = 0, longest = 0; bool pos = false; uint32_t bits = 32; } side[2];
    side[0].path = path_a; side[1].path = path_b;
    for (Side& s : side) {
        ipkgpu_db_file* f = nullptr;
        if (const int rc = ipkgpu_db_file_open(s.path, &f)) return fail(ctx, rc, "%s", ipkgpu_db_file_last_error());
        s.n = f->head.total_kmers; s.e = f->head.total_entries; s.body = f->body_bytes(); s.pos = f->head.positions_loaded;
        const uint32_t bps = f->head.sequence_type == "DNA" ? 2 : f->head.sequence_type == "AA" ? 5 : 0;
        s.bits = bps && f->head.kmer_size * bps <= 32 ? (uint32_t)(f->head.kmer_size * bps) : 32;
        ipkgpu_db_file_close(f);
        if (s.n > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %llu k-mers: a database holds at most 2^32 - 1 (its order is 32-bit)", s.path, (unsigned long long)s.n);
    }
    const uint32_t bits = std::max(side[0].bits, side[1].bits), shift = bits > 16 ? bits - 16 : 0;

    // The workspaces ipkgpu_db_diff and the scans keep in the context go back first and after every range: each range then takes
    // them anew at its own size, and the formula needs to know nothing of the ranges before it.
    DevBuf* const cached[] = {&ctx->sp_pops, &ctx->counts, &ctx->sp_rank, &ctx->sp_c16, &ctx->sp_bits, &ctx->goff, &ctx->tmp_c, &ctx->scan_sums};
    auto give_back = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (DevBuf* b : cached) if (b->p) { (void)dev_free(ctx, b->p, b->cap); b->p = nullptr; b->cap = 0; }
    };
    give_back();
    drop_cache(ctx);
    // (and when the call returns, however it returns: declared before every block of the call, so it runs behind their guards)
    struct AtExit { decltype(give_back)& g; ipkgpu_ctx* c; ~AtExit() { g(); drop_cache(c); (void)hipGetLastError(); } } at_exit{give_back, ctx};
    const uint64_t avail = mem_free_bytes(ctx);

    // the window: the option, else a sixteenth of what is there (4 KiB at least, 256 MiB at most): with its workspaces (60 bytes a
    // record of at least 16) the fixed part stays below a third of `avail` whatever the file holds, and near a sixteenth for long lists
    const uint64_t window = ctx->opt_load_window > 0 ? (uint64_t)ctx->opt_load_window : std::min<uint64_t>(std::max<uint64_t>(avail / 16, 4096), DB_STREAM_WINDOW);
    uint64_t fixed = 0;
    for (Side& s : side) {
        s.window = std::max<uint64_t>(std::min(window, s.body), ipkfmt::RECORD_HEAD_BYTES);
        // what the heads alone tell: a window holds at most one record per 16 bytes, the longest record at most every entry
        const uint64_t n_w = std::min<uint64_t>(s.n, std::max<uint64_t>(s.window / ipkfmt::RECORD_HEAD_BYTES, 1));
        const uint64_t longest = std::min(s.body, ipkfmt::RECORD_HEAD_BYTES + (s.pos ? ipkfmt::ENTRY_POS_BYTES : ipkfmt::ENTRY_BYTES) * s.e);
        fixed = std::max(fixed, ipkgpu_db_stream_window_bytes(s.window, n_w, longest));
    }
    auto cost = [&](uint64_t na, uint64_t ea, uint64_t nb, uint64_t eb) {
        return ipkgpu_db_diff_files_range_bytes(fixed, na, ea, side[0].pos, nb, eb, side[1].pos, max_records);
    };

    struct Range { uint64_t lo, hi, n[2], e[2]; };
    std::vector<Range> ranges;
    double t_hist = 0, t_loads = 0, t_walk = 0, ms_diff = 0, bytes_read = 0;
    uint64_t passes[2] = {0, 0};
    if (cost(side[0].n, side[0].e, side[1].n, side[1].e) <= avail) {
        ranges.push_back(Range{0, (uint64_t)1 << 32, {side[0].n, side[1].n}, {side[0].e, side[1].e}});
    } else {
        // the histogram pass over each file.  The two histograms (786 432 bytes, whatever the files hold) are counted by
        // ipkgpu_mem_stats and taken beside the budget: a budget too small for them can still be planned, and they are gone before
        // the first range is loaded.
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> h_rec[2];
        std::vector<unsigned long long> h_ent[2];
        {
            void* d_hist = nullptr;
            const size_t hist_bytes = (size_t)DB_HIST_BINS * 12;
            // (while they live the budget is that much larger: what is held with them stays comparable to it)
            const int64_t budget = ctx->budget;
            if (budget > 0) ctx->budget = budget + (int64_t)hist_bytes;
            const hipError_t e = dev_malloc(ctx, &d_hist, hist_bytes);
            if (e != hipSuccess) {
                ctx->budget = budget;
                (void)hipGetLastError();
                return fail(ctx, IPKGPU_ERR_NOMEM, "no room for the key histograms (%llu bytes): %s", (unsigned long long)hist_bytes, hipGetErrorString(e));
            }
            struct HGuard { ipkgpu_ctx* c; void* p; size_t n; int64_t budget;
                ~HGuard() { (void)hipStreamSynchronize(c->stream); (void)dev_free(c, p, n); c->budget = budget; (void)hipGetLastError(); } } hguard{ctx, d_hist, hist_bytes, budget};
            unsigned long long* d_ent = static_cast<unsigned long long*>(d_hist);
            uint32_t* d_rec = reinterpret_cast<uint32_t*>(d_ent + DB_HIST_BINS);
            for (int f = 0; f < 2; ++f) {
                try { h_rec[f].resize(DB_HIST_BINS); h_ent[f].resize(DB_HIST_BINS); } catch (const std::bad_alloc&) { return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory"); }
                HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, hist_bytes, ctx->stream));
                StreamKeep keep;
                keep.window = side[f].window; keep.rec_hist = d_rec; keep.ent_hist = d_ent; keep.shift = shift;
                RC_TRY(db_stream_load(ctx, side[f].path, keep, ~(uint64_t)0, nullptr));
                side[f].n_w = keep.n_w; side[f].longest = keep.longest;
                ++passes[f]; t_walk += ctx->t_load[2]; bytes_read += ctx->t_load[7];
                HIP_TRY(ctx, hipMemcpyAsync(h_rec[f].data(), d_rec, (size_t)DB_HIST_BINS * 4, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(h_ent[f].data(), d_ent, (size_t)DB_HIST_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                uint64_t n = 0, e_sum = 0;
                for (uint32_t b = 0; b < DB_HIST_BINS; ++b) { n += h_rec[f][b]; e_sum += h_ent[f][b]; }
                if (n != side[f].n || e_sum != side[f].e)
                    return fail(ctx, IPKGPU_ERR_HIP, "%s: the histograms hold %llu records and %llu entries, the walk %llu and %llu", side[f].path, (unsigned long long)n,
                                (unsigned long long)e_sum, (unsigned long long)side[f].n, (unsigned long long)side[f].e);
            }
        }
        give_back();
        t_hist = since(t0);
        // the fixed part as the passes saw it, then the greedy cut
        fixed = 0;
        for (const Side& s : side) fixed = std::max(fixed, ipkgpu_db_stream_window_bytes(s.window, s.n_w, s.longest));
        auto bin_lo = [&](uint64_t b) { return b >= DB_HIST_BINS ? (uint64_t)1 << 32 : b << shift; };
        Range cur{0, 0, {0, 0}, {0, 0}};
        uint64_t first = 0;
        for (uint64_t b = 0; b < DB_HIST_BINS; ++b) {
            const uint64_t add_n[2] = {h_rec[0][b], h_rec[1][b]}, add_e[2] = {h_ent[0][b], h_ent[1][b]};
            if (cost(cur.n[0] + add_n[0], cur.e[0] + add_e[0], cur.n[1] + add_n[1], cur.e[1] + add_e[1]) > avail) {
                const uint64_t alone = cost(add_n[0], add_e[0], add_n[1], add_e[1]);
                if (alone > avail)
                    return fail(ctx, IPKGPU_ERR_NOMEM, "bin %llu, the keys [%llu, %llu): %llu records and %llu entries of A, %llu and %llu of B need %llu bytes of device memory, %llu are there",
                                (unsigned long long)b, (unsigned long long)bin_lo(b), (unsigned long long)bin_lo(b + 1), (unsigned long long)add_n[0],
                                (unsigned long long)add_e[0], (unsigned long long)add_n[1], (unsigned long long)add_e[1], (unsigned long long)alone, (unsigned long long)avail);
                cur.lo = bin_lo(first); cur.hi = bin_lo(b);
                ranges.push_back(cur);
                first = b;
                cur = Range{0, 0, {0, 0}, {0, 0}};
            }
            for (int f = 0; f < 2; ++f) { cur.n[f] += add_n[f]; cur.e[f] += add_e[f]; }
        }
        cur.lo = bin_lo(first); cur.hi = (uint64_t)1 << 32;
        ranges.push_back(cur);
    }
    for (const Range& r : ranges) { ctx->dfiles_ranges.push_back(r.lo); ctx->dfiles_ranges.push_back(r.hi); }

    // the ranges, ascending
    ipkgpu_db_diff_counts total;
    memset(&total, 0, sizeof total);
    uint64_t written = 0;
    for (const Range& r : ranges) {
        ipkgpu_db* part[2] = {nullptr, nullptr};
        struct PGuard { ipkgpu_db** p; ~PGuard() { ipkgpu_db_free(p[0]); ipkgpu_db_free(p[1]); } } pguard{part};
        const auto t0 = std::chrono::steady_clock::now();
        for (int f = 0; f < 2; ++f) {
            StreamKeep keep;
            keep.key_lo = r.lo; keep.key_hi = r.hi;
            keep.expected = true; keep.exp_records = r.n[f]; keep.exp_entries = r.e[f];
            keep.window = side[f].window; keep.n_w = side[f].n_w; keep.longest = side[f].longest;
            RC_TRY(db_stream_load(ctx, side[f].path, keep, ~(uint64_t)0, &part[f]));
            ++passes[f]; t_walk += ctx->t_load[2]; bytes_read += ctx->t_load[7];
            side[f].n_w = keep.n_w; side[f].longest = keep.longest;      // (the same cuts on every pass: the same figures)
            if (part[f]->n_keys != r.n[f] || part[f]->n_entries != r.e[f])
                return fail(ctx, IPKGPU_ERR_INVALID, "%s: the file changed between passes: %llu records and %llu entries have keys in [%llu, %llu), %llu and %llu were counted before",
                            side[f].path, (unsigned long long)part[f]->n_keys, (unsigned long long)part[f]->n_entries, (unsigned long long)r.lo, (unsigned long long)r.hi,
                            (unsigned long long)r.n[f], (unsigned long long)r.e[f]);
        }
        t_loads += since(t0);
        ipkgpu_db_diff_counts c;
        uint64_t got = 0;
        const uint64_t room = max_records - written;
        RC_TRY(ipkgpu_db_diff(ctx, part[0], part[1], eps, &c, room ? records + written : nullptr, room, &got));
        written += got;
        ms_diff += ctx->t_diff_ms;
        total.keys_a += c.keys_a; total.keys_b += c.keys_b; total.keys_only_a += c.keys_only_a; total.keys_only_b += c.keys_only_b;
        total.entries_a += c.entries_a; total.entries_b += c.entries_b;
        total.entries_only_a += c.entries_only_a; total.entries_only_b += c.entries_only_b;
        total.scores_differ += c.scores_differ; total.positions_differ += c.positions_differ;
        total.max_abs_diff = std::max(total.max_abs_diff, c.max_abs_diff);
        ipkgpu_db_free(part[0]); ipkgpu_db_free(part[1]);
        part[0] = part[1] = nullptr;
        give_back();
        drop_cache(ctx);
    }
    *counts = total;
    if (n_records) *n_records = written;
    ctx->t_diff_ms = ms_diff;
    double* st = ctx->dfiles_stat;
    st[0] = since(t_begin); st[1] = t_hist; st[2] = t_loads; st[3] = ms_diff; st[4] = bytes_read; st[5] = (double)passes[0]; st[6] = (double)passes[1];
    st[7] = t_walk; st[8] = (double)window; st[9] = (double)avail; st[10] = (double)std::max(side[0].n_w, side[1].n_w);
    st[11] = (double)std::max(side[0].longest, side[1].longest);
    return IPKGPU_OK;
}

}  // extern "C"
