// db_join_files.hpp -- ipkgpu_db_join_files: branch shards joined by key ranges, no shard and no whole join ever resident (included by
// ipkgpu.hip behind db_join.hpp and db_diff_files.hpp, whose plan, window and bounds it shares).
//
// The join composes exactly over disjoint key ranges: a key's joined list depends on that key's runs alone, mif0_kernel works per
// k-mer with the caller's N, the random filter draws per k-mer code.  So: the plan of ipkgpu_db_diff_files generalised from 2 files to
// S (one histogram pass per shard, a greedy cut from bin 0 upward against join_files_range_bytes); per range the key-range load of every
// shard, ipkgpu_db_join, the sources freed, the filter, the device writer into a range file; and ipkgpu_db_merge_files over the range
// files, which are key-disjoint and each in filter order -- the bytes of the whole (the argument of the key-range build).  Where one
// range holds everything it is written straight to the output.  No kernel of its own.
#pragma once

#include <cerrno>
#include <unistd.h>

extern "C" {

uint64_t ipkgpu_db_join_files_range_bytes(uint64_t fixed, uint32_t n_srcs, const uint64_t* n, const uint64_t* e, int positioned, uint64_t write_piece,
                                          uint64_t longest_joined)
{
    const bool pos = positioned != 0;
    uint64_t n_all = 0, e_all = 0, resident = 0, loads = 0;
    for (uint32_t s = 0; s < n_srcs; ++s) {
        loads = std::max(loads, fixed + resident + df_load(n[s], e[s], pos));
        resident += df_db(n[s], e[s], pos);
        n_all += n[s]; e_all += e[s];
    }
    const uint64_t joined = df_db(n_all, e_all, pos);             // J with its filter arrays: duplicates only shrink it
    const uint64_t join = resident + ipkgpu_db_join_bytes(n_all, e_all, n_srcs, positioned);
    const uint64_t filter = joined + 2 * df_e(8 * n_all) + df_e(df_sort(n_all));
    const uint64_t body = 16 * n_all + (pos ? 10 : 8) * e_all;
    const uint64_t write = joined + df_m(4 * n_all) + df_m(8 * (n_all + 1)) + 2 * df_r(std::min(std::max(write_piece, longest_joined), body));
    return std::max(std::max(loads, join), std::max(filter, write)) + df_scanx(n_all + 1);
}

uint64_t ipkgpu_db_join_files_num_ranges(const ipkgpu_ctx* ctx) { return ctx ? ctx->jfiles_ranges.size() / 2 : 0; }
int ipkgpu_db_join_files_range(const ipkgpu_ctx* ctx, uint64_t i, uint64_t* key_lo, uint64_t* key_hi)
{
    if (!ctx || !key_lo || !key_hi || i >= ctx->jfiles_ranges.size() / 2) return IPKGPU_ERR_INVALID;
    *key_lo = ctx->jfiles_ranges[2 * i]; *key_hi = ctx->jfiles_ranges[2 * i + 1];
    return IPKGPU_OK;
}
double ipkgpu_db_join_files_stat(const ipkgpu_ctx* ctx, int which) { return ctx && which >= 0 && which < 15 ? ctx->jfiles_stat[which] : 0; }

int ipkgpu_db_join_files(ipkgpu_ctx* ctx, const ipkgpu_db_header* h, const char* const* paths, uint32_t n_paths, int filter, uint64_t total_num_groups,
                         float threshold, const char* out_path, const char* tmp_dir, uint64_t* total_kmers, uint64_t* total_entries,
                         uint64_t* entries_dropped, uint64_t* bytes_written)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (!h || !h->sequence_type || !out_path || !paths || n_paths == 0) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument: a header, an output path and at least one shard are needed");
    if (filter != 0 && filter != 1) return fail(ctx, IPKGPU_ERR_INVALID, "filter must be 0 (mif0) or 1 (random)");
    if (filter == 0 && (total_num_groups == 0 || !(threshold > 0.0f))) return fail(ctx, IPKGPU_ERR_INVALID, "need total_num_groups > 0 and threshold > 0");
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    ctx->jfiles_ranges.clear();
    for (double& s : ctx->jfiles_stat) s = 0;
    const uint32_t S = n_paths;

    // the heads, before any pass: totals, the key bits, and the fields on which the shards must agree with `h` and with each other
    struct Shard { const char* path; uint64_t n = 0, e = 0, body = 0, window = 0, n_w = 0, longest = 0; uint32_t bits = 32; };
    std::vector<Shard> shard(S);
    bool pos = false;
    for (uint32_t s = 0; s < S; ++s) {
        Shard& sh = shard[s];
        sh.path = paths[s];
        if (!sh.path) return fail(ctx, IPKGPU_ERR_INVALID, "shard path %u is null", s);
        ipkgpu_db_file* f = nullptr;
        if (const int rc = ipkgpu_db_file_open(sh.path, &f)) return fail(ctx, rc, "%s", ipkgpu_db_file_last_error());
        struct Close { ipkgpu_db_file* f; ~Close() { ipkgpu_db_file_close(f); } } close{f};
        const ipkfmt::Head& hd = f->head;
        uint32_t want = 0, got = 0;
        memcpy(&want, &h->omega, 4); memcpy(&got, &hd.omega, 4);
        if (hd.sequence_type != h->sequence_type || hd.kmer_size != h->kmer_size || want != got)
            return fail(ctx, IPKGPU_ERR_INVALID, "%s: a shard of %s, k = %llu, omega = %.9g; the header given is of %s, k = %llu, omega = %.9g", sh.path,
                        hd.sequence_type.c_str(), (unsigned long long)hd.kmer_size, (double)hd.omega, h->sequence_type, (unsigned long long)h->kmer_size, (double)h->omega);
        if (s == 0) pos = hd.positions_loaded;
        if (hd.positions_loaded != pos)
            return fail(ctx, IPKGPU_ERR_INVALID, "positioned and plain shards cannot be merged into one database: %s %s %s %s", sh.path,
                        hd.positions_loaded ? "has positions," : "has none,", paths[0], pos ? "has" : "has none");
        sh.n = hd.total_kmers; sh.e = hd.total_entries; sh.body = f->body_bytes();
        const uint32_t bps = hd.sequence_type == "DNA" ? 2 : hd.sequence_type == "AA" ? 5 : 0;
        sh.bits = bps && hd.kmer_size * bps <= 32 ? (uint32_t)(hd.kmer_size * bps) : 32;
        if (sh.n > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%s: %llu k-mers: a database holds at most 2^32 - 1 (its order is 32-bit)", sh.path, (unsigned long long)sh.n);
    }
    uint32_t bits = 0;
    uint64_t n_total = 0;
    for (const Shard& sh : shard) { bits = std::max(bits, sh.bits); n_total += sh.n; }
    const uint32_t shift = bits > 16 ? bits - 16 : 0;
    const uint64_t entry_bytes = pos ? ipkfmt::ENTRY_POS_BYTES : ipkfmt::ENTRY_BYTES;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // what this call leaves on disk until it has succeeded: the range files, the directory if the call made it, the output once begun
    struct OnDisk { std::vector<std::string> files; std::string dir, out; bool dir_made = false, out_begun = false, keep_out = false;
        ~OnDisk() { for (const std::string& f : files) (void)remove(f.c_str()); if (dir_made) (void)rmdir(dir.c_str()); if (out_begun && !keep_out) (void)remove(out.c_str()); } } disk;
    disk.out = out_path;
    disk.dir = tmp_dir ? std::string(tmp_dir) : std::string(out_path) + ".ranges";

    // The workspaces the loads' scans, the filter and the writer keep in the context go back first, between a range's filter and its write,
    // after every range and when the call returns: each step then takes them anew at its own size.
    DevBuf* const cached[] = {&ctx->sp_pops, &ctx->counts, &ctx->sp_rank, &ctx->sp_c16, &ctx->sp_bits, &ctx->goff, &ctx->tmp_a, &ctx->tmp_b, &ctx->tmp_c, &ctx->scan_sums};
    auto give_back = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (DevBuf* b : cached) if (b->p) { (void)dev_free(ctx, b->p, b->cap); b->p = nullptr; b->cap = 0; }
    };
    give_back();
    drop_cache(ctx);
    struct AtExit { decltype(give_back)& g; ipkgpu_ctx* c; ~AtExit() { g(); drop_cache(c); (void)hipGetLastError(); } } at_exit{give_back, ctx};
    const uint64_t avail = mem_free_bytes(ctx);

    // the window of ipkgpu_db_diff_files; the writer's piece by the same sixteenth
    const uint64_t window = ctx->opt_load_window > 0 ? (uint64_t)ctx->opt_load_window : std::min<uint64_t>(std::max<uint64_t>(avail / 16, 4096), DB_STREAM_WINDOW);
    const uint64_t write_piece = std::min<uint64_t>(std::max<uint64_t>(avail / 16, (uint64_t)64 << 10), DB_WRITE_PIECE);
    uint64_t fixed = 0, longest_joined = ipkfmt::RECORD_HEAD_BYTES;
    for (Shard& sh : shard) {
        sh.window = std::max<uint64_t>(std::min(window, sh.body), ipkfmt::RECORD_HEAD_BYTES);
        const uint64_t n_w = std::min<uint64_t>(sh.n, std::max<uint64_t>(sh.window / ipkfmt::RECORD_HEAD_BYTES, 1));
        const uint64_t longest = std::min(sh.body, ipkfmt::RECORD_HEAD_BYTES + entry_bytes * sh.e);
        fixed = std::max(fixed, ipkgpu_db_stream_window_bytes(sh.window, n_w, longest));
        longest_joined += longest > ipkfmt::RECORD_HEAD_BYTES ? longest - ipkfmt::RECORD_HEAD_BYTES : 0;
    }
    std::vector<uint64_t> arg_n(S), arg_e(S);
    auto cost = [&](const std::vector<uint64_t>& n, const std::vector<uint64_t>& e) {
        return ipkgpu_db_join_files_range_bytes(fixed, S, n.data(), e.data(), pos, write_piece, longest_joined);
    };

    struct Range { uint64_t lo, hi; std::vector<uint64_t> n, e; };
    std::vector<Range> ranges;
    double t_hist = 0, t_loads = 0, t_walk = 0, t_out = 0, t_merge = 0, ms_join = 0, bytes_read = 0;
    uint64_t passes = 0, dropped = 0, shared = 0, route1 = 0, range_peak = 0;
    // (the figures of the call however it returns: a refusal's passes are read from them)
    auto put_stats = [&]() {
        double* st = ctx->jfiles_stat;
        st[0] = since(t_begin); st[1] = t_hist; st[2] = t_loads; st[3] = ms_join; st[4] = bytes_read; st[5] = (double)passes; st[6] = t_walk; st[7] = t_out; st[8] = t_merge;
        st[9] = (double)window; st[10] = (double)avail; st[11] = (double)shared; st[12] = (double)dropped; st[13] = (double)route1; st[14] = (double)range_peak;
    };
    struct Stats { decltype(put_stats)& put; ~Stats() { put(); } } stats{put_stats};
    for (uint32_t s = 0; s < S; ++s) { arg_n[s] = shard[s].n; arg_e[s] = shard[s].e; }
    const bool one_range = n_total == 0 || cost(arg_n, arg_e) <= avail;
    if (one_range) {
        ranges.push_back(Range{0, (uint64_t)1 << 32, arg_n, arg_e});
    } else {
        // the histogram pass over each shard: one pair of histograms on the device, counted by ipkgpu_mem_stats and taken beside the
        // budget as in ipkgpu_db_diff_files, copied to the host after each shard and gone before the first range is loaded
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::vector<uint32_t>> h_rec(S);
        std::vector<std::vector<unsigned long long>> h_ent(S);
        {
            void* d_hist = nullptr;
            const size_t hist_bytes = (size_t)DB_HIST_BINS * 12;
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
            for (uint32_t s = 0; s < S; ++s) {
                Shard& sh = shard[s];
                try { h_rec[s].resize(DB_HIST_BINS); h_ent[s].resize(DB_HIST_BINS); } catch (const std::bad_alloc&) { return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory"); }
                HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, hist_bytes, ctx->stream));
                StreamKeep keep;
                keep.window = sh.window; keep.rec_hist = d_rec; keep.ent_hist = d_ent; keep.shift = shift;
                RC_TRY(db_stream_load(ctx, sh.path, keep, ~(uint64_t)0, nullptr));
                sh.n_w = keep.n_w; sh.longest = keep.longest;
                ++passes; t_walk += ctx->t_load[2]; bytes_read += ctx->t_load[7];
                HIP_TRY(ctx, hipMemcpyAsync(h_rec[s].data(), d_rec, (size_t)DB_HIST_BINS * 4, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(h_ent[s].data(), d_ent, (size_t)DB_HIST_BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                uint64_t n = 0, e_sum = 0;
                for (uint32_t b = 0; b < DB_HIST_BINS; ++b) { n += h_rec[s][b]; e_sum += h_ent[s][b]; }
                if (n != sh.n || e_sum != sh.e)
                    return fail(ctx, IPKGPU_ERR_HIP, "%s: the histograms hold %llu records and %llu entries, the walk %llu and %llu", sh.path, (unsigned long long)n,
                                (unsigned long long)e_sum, (unsigned long long)sh.n, (unsigned long long)sh.e);
            }
        }
        give_back();
        t_hist = since(t0);
        // the fixed part and the longest joined record as the passes saw them, then the greedy cut
        fixed = 0; longest_joined = ipkfmt::RECORD_HEAD_BYTES;
        for (const Shard& sh : shard) {
            fixed = std::max(fixed, ipkgpu_db_stream_window_bytes(sh.window, sh.n_w, sh.longest));
            longest_joined += sh.longest > ipkfmt::RECORD_HEAD_BYTES ? sh.longest - ipkfmt::RECORD_HEAD_BYTES : 0;
        }
        auto bin_lo = [&](uint64_t b) { return b >= DB_HIST_BINS ? (uint64_t)1 << 32 : b << shift; };
        const std::vector<uint64_t> zero(S, 0);
        Range cur{0, 0, zero, zero};
        std::vector<uint64_t> add_n(S), add_e(S), try_n(S), try_e(S);
        uint64_t first = 0;
        for (uint64_t b = 0; b < DB_HIST_BINS; ++b) {
            bool any = false;
            for (uint32_t s = 0; s < S; ++s) { add_n[s] = h_rec[s][b]; add_e[s] = h_ent[s][b]; any = any || add_n[s]; }
            if (!any) continue;                                              // (a bin without a record adds nothing and closes no range)
            for (uint32_t s = 0; s < S; ++s) { try_n[s] = cur.n[s] + add_n[s]; try_e[s] = cur.e[s] + add_e[s]; }
            if (cost(try_n, try_e) > avail) {
                const uint64_t alone = cost(add_n, add_e);
                if (alone > avail) {
                    std::string held;
                    for (uint32_t s = 0; s < S && held.size() < 300; ++s)
                        if (add_n[s]) held += " " + std::to_string(add_n[s]) + " records and " + std::to_string(add_e[s]) + " entries of shard " + std::to_string(s) + ",";
                    return fail(ctx, IPKGPU_ERR_NOMEM, "bin %llu, the keys [%llu, %llu):%s in all they need %llu bytes of device memory, %llu are there", (unsigned long long)b,
                                (unsigned long long)bin_lo(b), (unsigned long long)bin_lo(b + 1), held.c_str(), (unsigned long long)alone, (unsigned long long)avail);
                }
                cur.lo = bin_lo(first); cur.hi = bin_lo(b);
                ranges.push_back(cur);
                first = b;
                cur = Range{0, 0, zero, zero};
            }
            for (uint32_t s = 0; s < S; ++s) { cur.n[s] += add_n[s]; cur.e[s] += add_e[s]; }
        }
        cur.lo = bin_lo(first); cur.hi = (uint64_t)1 << 32;
        ranges.push_back(cur);
        if (mkdir(disk.dir.c_str(), 0777) == 0) disk.dir_made = true;
        else if (errno != EEXIST) return fail(ctx, IPKGPU_ERR_INVALID, "cannot create the directory %s for the range files", disk.dir.c_str());
    }
    for (const Range& r : ranges) { ctx->jfiles_ranges.push_back(r.lo); ctx->jfiles_ranges.push_back(r.hi); }

    // the ranges, ascending: the S loads, the join, the sources freed, the filter, the write.  Their own high-water mark is kept apart
    // (stat 14): the histograms, taken beside the budget, would hide it in ipkgpu_mem_stats' peak.
    const size_t held_before = ctx->held, peak_before = ctx->held_peak;
    ctx->held_peak = ctx->held;
    struct PeakBack { ipkgpu_ctx* c; size_t before; ~PeakBack() { c->held_peak = std::max(c->held_peak, before); } } peak_back{ctx, peak_before};
    uint64_t nk = 0, ne = 0, written = 0;
    for (size_t i = 0; i < ranges.size(); ++i) {
        const Range& r = ranges[i];
        uint64_t n_in = 0;
        for (uint32_t s = 0; s < S; ++s) n_in += r.n[s];
        if (!one_range && n_in == 0) continue;                               // no shard has a record in it: no load passes and no file
        std::vector<ipkgpu_db*> part(S, nullptr);
        ipkgpu_db* joined = nullptr;
        struct PGuard { ipkgpu_ctx* c; std::vector<ipkgpu_db*>& p; ipkgpu_db*& j;
            ~PGuard() { (void)hipStreamSynchronize(c->stream); for (ipkgpu_db* d : p) ipkgpu_db_free(d); ipkgpu_db_free(j); } } pguard{ctx, part, joined};
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t s = 0; s < S; ++s) {
            Shard& sh = shard[s];
            StreamKeep keep;
            keep.key_lo = r.lo; keep.key_hi = r.hi;
            keep.expected = true; keep.exp_records = r.n[s]; keep.exp_entries = r.e[s];
            keep.window = sh.window; keep.n_w = sh.n_w; keep.longest = sh.longest;
            RC_TRY(db_stream_load(ctx, sh.path, keep, ~(uint64_t)0, &part[s]));
            ++passes; t_walk += ctx->t_load[2]; bytes_read += ctx->t_load[7];
            sh.n_w = keep.n_w; sh.longest = keep.longest;                    // (the same cuts on every pass: the same figures)
            if (part[s]->n_keys != r.n[s] || part[s]->n_entries != r.e[s])
                return fail(ctx, IPKGPU_ERR_INVALID, "%s: the file changed between passes: %llu records and %llu entries have keys in [%llu, %llu), %llu and %llu were counted before",
                            sh.path, (unsigned long long)part[s]->n_keys, (unsigned long long)part[s]->n_entries, (unsigned long long)r.lo, (unsigned long long)r.hi,
                            (unsigned long long)r.n[s], (unsigned long long)r.e[s]);
        }
        t_loads += since(t0);
        RC_TRY(ipkgpu_db_join(ctx, part.data(), S, &joined));
        ms_join += ctx->join_stat[0]; shared += (uint64_t)ctx->join_stat[4]; dropped += (uint64_t)ctx->join_stat[5]; route1 += ctx->join_stat[6] != 0;
        for (ipkgpu_db*& d : part) { ipkgpu_db_free(d); d = nullptr; }
        drop_cache(ctx);
        const auto t1 = std::chrono::steady_clock::now();
        RC_TRY(filter == 0 ? ipkgpu_db_filter_mif0(ctx, joined, total_num_groups, threshold) : ipkgpu_db_filter_random(ctx, joined));
        give_back();
        std::string to = out_path;
        if (one_range) disk.out_begun = true;
        else {
            char name[32];
            snprintf(name, sizeof name, "/range_%05u.ipk", (unsigned)i);
            to = disk.dir + name;
            disk.files.push_back(to);
        }
        uint64_t bytes = 0;
        RC_TRY(db_write_pieces(ctx, joined, h, to.c_str(), &bytes, std::max(write_piece, longest_joined)));
        t_out += since(t1);
        nk += joined->n_keys; ne += joined->n_entries; written = bytes;
        ipkgpu_db_free(joined); joined = nullptr;
        give_back();
        drop_cache(ctx);
    }
    range_peak = ctx->held_peak - held_before;
    if (!one_range) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<const char*> files;
        for (const std::string& f : disk.files) files.push_back(f.c_str());
        uint64_t m_k = 0, m_e = 0;
        disk.out_begun = true;
        if (const int rc = ipkgpu_db_merge_files(h, files.data(), (uint32_t)files.size(), out_path, &m_k, &m_e, &written)) return fail(ctx, rc, "%s", ipkgpu_db_merge_last_error());
        if (m_k != nk || m_e != ne)
            return fail(ctx, IPKGPU_ERR_INVALID, "the range files hold %llu k-mers and %llu entries, the ranges wrote %llu and %llu", (unsigned long long)m_k, (unsigned long long)m_e,
                        (unsigned long long)nk, (unsigned long long)ne);
        t_merge = since(t0);
    }
    disk.keep_out = true;
    if (total_kmers) *total_kmers = nk;
    if (total_entries) *total_entries = ne;
    if (entries_dropped) *entries_dropped = dropped;
    if (bytes_written) *bytes_written = written;
    return IPKGPU_OK;
}

}  // extern "C"
