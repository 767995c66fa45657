// db_place.hpp -- ipkgpu_db_place: query sequences placed on a database of this context (included by ipkgpu.hip; kernels_place.hpp).
//
// ipkgpu_db_place_opts is the same call with ambiguous symbols expanded and / or both strands placed (place_ext_kernel); without
// options it launches what ipkgpu_db_place always launched.
// First call on a database: the prefix table over the keys' high bits, B = 1 + the largest branch id, and the check that no key names
// a branch twice (the kernels add a key's entries without atomics) -- cached in the database, freed with it.  Every call: the queries
// go to the device in batches sized from what the budget leaves, one wavefront places one query, the small results come back.
#pragma once

struct ipkgpu_placements {
    uint64_t n = 0;
    uint32_t keep = 0;
    std::vector<uint32_t> branches, counts, n_kmers, n_found, n_branches, n_ambiguous;
    std::vector<uint8_t> strand;
    std::vector<float> scores;
    std::vector<double> lwr;
    double t_index = 0, t_place = 0, t_total = 0;
};

namespace {

constexpr uint64_t PLACE_BATCH_QUERIES = 1ull << 18;      // most queries of an automatic batch, PLACE_BATCH_BYTES: most sequence bytes
constexpr uint64_t PLACE_BATCH_BYTES = 256ull << 20;

// device bytes of a batch's results and offsets per query (ext: strand and n_ambiguous as well)
inline uint64_t place_query_bytes(uint32_t keep, bool ext) { return 8 + (uint64_t)keep * (8 + 4 + 4 + 4) + 3 * 4 + (ext ? 2 * 4 : 0); }

// The database's placement index for codes of `bits` bits (sigma, k of the call): built once, kept in the database.
int place_prepare(ipkgpu_ctx* ctx, ipkgpu_db* db, uint32_t bits)
{
    if (db->d_place_index && db->place_bits == bits) return IPKGPU_OK;
    const uint64_t n = db->n_keys, ne = db->n_entries;
    if (n > 0xFFFFFFFFull) return fail(ctx, IPKGPU_ERR_INVALID, "%llu k-mers: the placement index holds 32-bit positions", (unsigned long long)n);
    RC_TRY(ensure(ctx, ctx->place_small, 64));
    uint32_t* d_max = ctx->place_small.as<uint32_t>();
    unsigned long long* d_bad = ctx->place_small.as<unsigned long long>() + 1;
    Stopwatch sw(ctx->stream, &ctx->events);
    const int e0 = sw.mark();
    uint32_t last_key = 0, max_branch = 0;
    if (n) HIP_TRY(ctx, hipMemcpyAsync(&last_key, db->d_keys + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_max, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
    if (ne) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((ne + 255) / 256, (uint64_t)ctx->num_cu * 8);
        hipLaunchKernelGGL(place_max_branch_kernel, dim3(grid), dim3(256), 0, ctx->stream, db->d_entries, ne, d_max);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&max_branch, d_max, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bits < 32 && n && (last_key >> bits) != 0)
        return fail(ctx, IPKGPU_ERR_INVALID, "the database holds key 0x%x: not a database of %u-bit k-mer codes (sigma / k of the call)", last_key, bits);
    if (ne && max_branch == 0xFFFFFFFFu) return fail(ctx, IPKGPU_ERR_INVALID, "branch id 0xFFFFFFFF is the placements' \"none\"");
    const uint32_t n_branches = ne ? max_branch + 1 : 0;
    // the precondition of the accumulation: a key names a branch once
    for (uint64_t first = 0; first < n && ne; first += WAVE_PER_ITEM_SPAN) {
        const dim3 grid((uint32_t)((std::min<uint64_t>(WAVE_PER_ITEM_SPAN, n - first) + 3) / 4));
        hipLaunchKernelGGL(place_dupcheck_kernel, grid, dim3(256), 0, ctx->stream, db->d_key_off, db->d_entries, n, n_branches, first, d_bad);
    }
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long bad = ~0ull;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != ~0ull) {
        uint32_t key = 0;
        HIP_TRY(ctx, hipMemcpy(&key, db->d_keys + bad, 4, hipMemcpyDeviceToHost));
        return fail(ctx, IPKGPU_ERR_INVALID, "key %u (0x%x) names a branch more than once: such a database is not placed on", key, key);
    }
    const uint32_t p = std::min(bits, PLACE_INDEX_BITS), slots = 1u << p;
    if (db->d_place_index) { ctx_release(ctx, db->d_place_index); db->d_place_index = nullptr; }
    HIP_TRY(ctx, ctx_alloc(ctx, (void**)&db->d_place_index, ((size_t)slots + 1) * 4));
    hipLaunchKernelGGL(place_index_kernel, dim3((slots + 1 + 255) / 256), dim3(256), 0, ctx->stream, db->d_keys, (uint32_t)n, bits - p, slots,
                       db->d_place_index);
    HIP_TRY(ctx, hipGetLastError());
    const int e1 = sw.mark();
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    db->place_bits = bits; db->place_shift = bits - p; db->place_slots = slots; db->place_branches = n_branches;
    db->t_place_index = sw.ms(e0, e1);
    return IPKGPU_OK;
}

int place_launch(ipkgpu_ctx* ctx, const PlaceArgs& a, const PlaceExtArgs* x, uint32_t bits_per_symbol, bool global, uint32_t grid)
{
    // the block's LDS: the kernel's symbol tables, and S, C and the touched list behind them unless they are global
    const size_t tables = global ? 0 : (size_t)a.b_pad * 12;
    auto launch = [&](auto BITS_, auto GLOBAL_) {
        if (x) hipLaunchKernelGGL((place_ext_kernel<BITS_, GLOBAL_>), dim3(grid), dim3(64), PLACE_EXT_TAB_BYTES + tables, ctx->stream, a, *x);
        else hipLaunchKernelGGL((place_kernel<BITS_, GLOBAL_>), dim3(grid), dim3(64), PLACE_SYMTAB_BYTES + tables, ctx->stream, a);
    };
    if (bits_per_symbol == 2) global ? launch(int_c<2>{}, std::true_type{}) : launch(int_c<2>{}, std::false_type{});
    else global ? launch(int_c<5>{}, std::true_type{}) : launch(int_c<5>{}, std::false_type{});
    HIP_TRY(ctx, hipGetLastError());
    return IPKGPU_OK;
}

}  // namespace

extern "C" {

int ipkgpu_db_place(ipkgpu_ctx* ctx, ipkgpu_db* db, uint32_t sigma, uint32_t k, float log_eps, const char* seqs, const uint64_t* seq_off,
                    uint64_t n_queries, uint32_t keep_at_most, ipkgpu_placements** out)
{
    return ipkgpu_db_place_opts(ctx, db, sigma, k, log_eps, seqs, seq_off, n_queries, keep_at_most, nullptr, out);
}

int ipkgpu_db_place_opts(ipkgpu_ctx* ctx, ipkgpu_db* db, uint32_t sigma, uint32_t k, float log_eps, const char* seqs, const uint64_t* seq_off,
                         uint64_t n_queries, uint32_t keep_at_most, const ipkgpu_place_options* opts, ipkgpu_placements** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!db || db->ctx != ctx || !out) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument");
    const uint32_t ambiguity = opts ? opts->ambiguity : 0, strands = opts ? opts->strands : 0;
    if (ambiguity > 1 || strands > 1) return fail(ctx, IPKGPU_ERR_INVALID, "place options: ambiguity and strands are 0 or 1 each");
    if (strands && sigma != 4) return fail(ctx, IPKGPU_ERR_INVALID, "both strands are placed for DNA only (sigma = 4)");
    const bool ext = ambiguity || strands;
    if (n_queries && (!seq_off || (!seqs && seq_off[n_queries] != seq_off[0]))) return fail(ctx, IPKGPU_ERR_INVALID, "null sequence arrays");
    const uint32_t bps = ipkgpu_bits_per_symbol(sigma);
    if (bps == 0 || k < 1 || k > 16 || bps * k > 32)
        return fail(ctx, IPKGPU_ERR_INVALID, "unsupported sigma / k (%u / %u): k-mer codes are at most 32 bits (DNA k <= 16, amino acids k <= 6)", sigma, k);
    if (db->file) {
        const char* want = sigma == 4 ? "DNA" : "AA";
        if (db->file->head.sequence_type != want || db->file->head.kmer_size != k)
            return fail(ctx, IPKGPU_ERR_INVALID, "sigma / k of the call (%u / %u) are not those of the database's file (%s, k = %llu)", sigma, k,
                        db->file->head.sequence_type.c_str(), (unsigned long long)db->file->head.kmer_size);
    }
    if (keep_at_most < 1 || keep_at_most > 64) return fail(ctx, IPKGPU_ERR_INVALID, "keep_at_most must be in 1 .. 64");
    for (uint64_t q = 0; q < n_queries; ++q) {
        if (seq_off[q + 1] < seq_off[q]) return fail(ctx, IPKGPU_ERR_INVALID, "seq_off decreases at query %llu", (unsigned long long)q);
        if (seq_off[q + 1] - seq_off[q] >= (1ull << 32)) return fail(ctx, IPKGPU_ERR_INVALID, "query %llu has 2^32 bytes or more", (unsigned long long)q);
    }
    const auto t_begin = std::chrono::steady_clock::now();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool had_index = db->d_place_index && db->place_bits == bps * k;
    RC_TRY(place_prepare(ctx, db, bps * k));

    ipkgpu_placements* res = new (std::nothrow) ipkgpu_placements();
    if (!res) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    std::unique_ptr<ipkgpu_placements> guard(res);
    const uint32_t keep = keep_at_most;
    res->n = n_queries; res->keep = keep;
    res->t_index = had_index ? 0 : db->t_place_index;
    try {
        res->branches.resize(n_queries * keep); res->counts.resize(n_queries * keep); res->scores.resize(n_queries * keep);
        res->lwr.resize(n_queries * keep);
        res->n_kmers.resize(n_queries); res->n_found.resize(n_queries); res->n_branches.resize(n_queries);
        res->n_ambiguous.assign(n_queries, 0); res->strand.assign(n_queries, 0);
    } catch (const std::bad_alloc&) { return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory"); }

    const uint32_t B = db->place_branches, b_pad = std::max<uint32_t>((B + 63) & ~63u, 64);
    const uint32_t lds_bound = ctx->opt_place_lds > 0 ? (uint32_t)ctx->opt_place_lds : PLACE_LDS_BRANCHES;
    const bool global = B > lds_bound;
    const uint64_t per_query = place_query_bytes(keep, ext);
    const uint32_t max_grid = (uint32_t)ctx->num_cu * (global ? 4 : 32);
    const uint64_t amb_slice_bytes = (uint64_t)b_pad * 16;                 // P (f64), c and the window's touched list per workgroup
    PlaceExtArgs x;
    x.ambiguity = ambiguity; x.strands = strands; x.E = std::pow(10.0, (double)log_eps);
    x.g_p = nullptr; x.g_wc = nullptr; x.g_wtouched = nullptr;
    std::vector<uint32_t> h_strand;
    uint32_t amb_slices = 0;
    Stopwatch sw(ctx->stream, &ctx->events);
    std::vector<std::pair<int, int>> marks;
    uint32_t slices = 0;
    for (uint64_t q0 = 0; q0 < n_queries;) {
        // the batch: as many queries as the option or the budget allows (a first query always: what it needs is then asked for and may be refused)
        // A workspace is no room for another: each is counted by what it would have to grow by, as ensure grows it (the old block
        // freed first, a sixteenth on top of what is asked for), and the three together take at most half of what is free.
        const uint64_t room = mem_free_bytes(ctx) / 2;
        const uint64_t most = ctx->opt_place_batch > 0 ? (uint64_t)ctx->opt_place_batch : PLACE_BATCH_QUERIES;
        auto grows = [](const DevBuf& b, uint64_t need) -> uint64_t { return need <= b.cap ? 0 : need + need / 16 - b.cap; };
        uint64_t q1 = q0 + 1;
        while (q1 < n_queries && q1 - q0 < most) {
            const uint64_t bytes = seq_off[q1 + 1] - seq_off[q0], n = q1 + 1 - q0;
            // (ambiguity: the per-window tables of the workgroups that n queries start)
            const uint64_t amb_grows = ambiguity ? grows(ctx->place_amb, std::min<uint64_t>(n, max_grid) * amb_slice_bytes) : 0;
            if (bytes > PLACE_BATCH_BYTES ||
                grows(ctx->place_seq, bytes + 16) + grows(ctx->place_off, (n + 1) * 8) + grows(ctx->place_out, n * per_query + 64) + amb_grows > room) break;
            ++q1;
        }
        const uint64_t nq = q1 - q0, bytes = seq_off[q1] - seq_off[q0];
        RC_TRY(ensure(ctx, ctx->place_seq, bytes + 16));
        RC_TRY(ensure(ctx, ctx->place_off, (nq + 1) * 8));
        RC_TRY(ensure(ctx, ctx->place_out, nq * per_query + 64));
        const uint32_t grid = (uint32_t)std::min<uint64_t>(nq, max_grid);
        if (global && grid > slices) {
            // a slice of S, C and the touched list per workgroup; S and C zero before the first launch, and every launch leaves them so
            uint32_t want = grid;
            const uint64_t slice_bytes = (uint64_t)b_pad * 12;
            if ((uint64_t)want * slice_bytes > ctx->place_tables.cap)
                want = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (mem_free_bytes(ctx) / 2 + ctx->place_tables.cap) / slice_bytes));
            RC_TRY(ensure(ctx, ctx->place_tables, (uint64_t)want * slice_bytes));
            HIP_TRY(ctx, hipMemsetAsync(ctx->place_tables.p, 0, (uint64_t)want * b_pad * 8, ctx->stream));
            slices = want;
        }
        if (ambiguity && grid > amb_slices) {
            // the same for P, c and the window's touched list: P and c zero before the first launch, and every launch leaves them so
            uint32_t want = grid;
            if ((uint64_t)want * amb_slice_bytes > ctx->place_amb.cap)
                want = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (mem_free_bytes(ctx) / 2 + ctx->place_amb.cap) / amb_slice_bytes));
            RC_TRY(ensure(ctx, ctx->place_amb, (uint64_t)want * amb_slice_bytes));
            HIP_TRY(ctx, hipMemsetAsync(ctx->place_amb.p, 0, (uint64_t)want * b_pad * 12, ctx->stream));
            amb_slices = want;
        }
        if (bytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->place_seq.p, seqs + seq_off[q0], bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->place_off.p, seq_off + q0, (nq + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        PlaceArgs a;
        a.keys = db->d_keys; a.key_off = db->d_key_off; a.entries = db->d_entries; a.index = db->d_place_index;
        a.shift = db->place_shift; a.k = k; a.sigma = sigma; a.n_branches = B; a.b_pad = b_pad; a.log_eps = log_eps;
        a.seqs = ctx->place_seq.as<unsigned char>(); a.seq_off = ctx->place_off.as<uint64_t>(); a.seq_base = seq_off[q0];
        a.n_queries = (uint32_t)nq; a.keep = keep;
        a.g_s = ctx->place_tables.as<float>();
        a.g_c = ctx->place_tables.as<uint32_t>() + (size_t)slices * b_pad;
        a.g_touched = ctx->place_tables.as<uint32_t>() + (size_t)2 * slices * b_pad;
        char* o = ctx->place_out.as<char>();
        a.out_lwr = reinterpret_cast<double*>(o); o += nq * keep * 8;
        a.out_branch = reinterpret_cast<uint32_t*>(o); o += nq * keep * 4;
        a.out_score = reinterpret_cast<float*>(o); o += nq * keep * 4;
        a.out_count = reinterpret_cast<uint32_t*>(o); o += nq * keep * 4;
        a.out_n_kmers = reinterpret_cast<uint32_t*>(o); o += nq * 4;
        a.out_n_found = reinterpret_cast<uint32_t*>(o); o += nq * 4;
        a.out_n_branches = reinterpret_cast<uint32_t*>(o); o += nq * 4;
        uint32_t launch_grid = global ? std::min(grid, slices) : grid;
        if (ext) {
            x.out_strand = reinterpret_cast<uint32_t*>(o); o += nq * 4;
            x.out_n_ambiguous = reinterpret_cast<uint32_t*>(o);
            if (ambiguity) {
                x.g_p = ctx->place_amb.as<double>();
                x.g_wc = ctx->place_amb.as<uint32_t>() + (size_t)2 * amb_slices * b_pad;
                x.g_wtouched = ctx->place_amb.as<uint32_t>() + (size_t)3 * amb_slices * b_pad;
                launch_grid = std::min(launch_grid, amb_slices);
            }
        }
        const int m0 = sw.mark();
        RC_TRY(place_launch(ctx, a, ext ? &x : nullptr, bps, global, launch_grid));
        marks.push_back({m0, sw.mark()});
        HIP_TRY(ctx, hipMemcpyAsync(res->lwr.data() + q0 * keep, a.out_lwr, nq * keep * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(res->branches.data() + q0 * keep, a.out_branch, nq * keep * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(res->scores.data() + q0 * keep, a.out_score, nq * keep * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(res->counts.data() + q0 * keep, a.out_count, nq * keep * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(res->n_kmers.data() + q0, a.out_n_kmers, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(res->n_found.data() + q0, a.out_n_found, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(res->n_branches.data() + q0, a.out_n_branches, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (ext) {
            try { h_strand.resize(nq); } catch (const std::bad_alloc&) { return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory"); }
            HIP_TRY(ctx, hipMemcpyAsync(h_strand.data(), x.out_strand, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(res->n_ambiguous.data() + q0, x.out_n_ambiguous, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                 // (the buffers serve the next batch)
        if (ext) for (uint64_t i = 0; i < nq; ++i) res->strand[q0 + i] = (uint8_t)h_strand[i];
        q0 = q1;
    }
    for (const auto& m : marks) res->t_place += sw.ms(m.first, m.second);
    res->t_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    *out = guard.release();
    return IPKGPU_OK;
}

uint64_t ipkgpu_placements_num_queries(const ipkgpu_placements* p) { return p ? p->n : 0; }
uint32_t ipkgpu_placements_keep(const ipkgpu_placements* p) { return p ? p->keep : 0; }
const uint32_t* ipkgpu_placements_branches(const ipkgpu_placements* p) { return p ? p->branches.data() : nullptr; }
const float* ipkgpu_placements_scores(const ipkgpu_placements* p) { return p ? p->scores.data() : nullptr; }
const uint32_t* ipkgpu_placements_counts(const ipkgpu_placements* p) { return p ? p->counts.data() : nullptr; }
const double* ipkgpu_placements_lwr(const ipkgpu_placements* p) { return p ? p->lwr.data() : nullptr; }
const uint32_t* ipkgpu_placements_n_kmers(const ipkgpu_placements* p) { return p ? p->n_kmers.data() : nullptr; }
const uint32_t* ipkgpu_placements_n_found(const ipkgpu_placements* p) { return p ? p->n_found.data() : nullptr; }
const uint32_t* ipkgpu_placements_n_branches(const ipkgpu_placements* p) { return p ? p->n_branches.data() : nullptr; }
const uint8_t* ipkgpu_placements_strand(const ipkgpu_placements* p) { return p ? p->strand.data() : nullptr; }
const uint32_t* ipkgpu_placements_n_ambiguous(const ipkgpu_placements* p) { return p ? p->n_ambiguous.data() : nullptr; }
double ipkgpu_placements_time_ms(const ipkgpu_placements* p, int which)
{
    if (!p) return 0;
    return which == 1 ? p->t_index : which == 2 ? p->t_place : p->t_total;
}
void ipkgpu_placements_free(ipkgpu_placements* p) { delete p; }

}  // extern "C"
