// db_kmerset.hpp -- ipkgpu_kmer_set_of_queries: the codes a placement of the queries would look up, as a bitmap on the device
// (included by ipkgpu.hip behind db_place.hpp; kernels_kmerset.hpp).
//
// The refusals and the batches are those of ipkgpu_db_place_opts: the queries go up through the placement's own sequence and offset
// workspaces, as many at a time as "place_batch_queries" or the budget allows.  The bitmap is taken through dev_malloc, so it counts
// against "device_budget_bytes" and shows in ipkgpu_mem_stats until ipkgpu_kmer_set_free.
#pragma once

extern "C" {

void ipkgpu_kmer_set_free(ipkgpu_kmer_set* set)
{
    if (!set) return;
    if (set->d_words) {
        (void)hipSetDevice(set->ctx->device);
        (void)hipStreamSynchronize(set->ctx->stream);
        (void)dev_free(set->ctx, set->d_words, set->bytes);
    }
    delete set;
}

int ipkgpu_kmer_set_of_queries(ipkgpu_ctx* ctx, uint32_t sigma, uint32_t k, const char* seqs, const uint64_t* seq_off, uint64_t n_queries,
                               const ipkgpu_place_options* opts, ipkgpu_kmer_set** out)
{
    if (!ctx) return IPKGPU_ERR_INVALID;
    if (out) *out = nullptr;
    if (!out) return fail(ctx, IPKGPU_ERR_INVALID, "bad argument");
    const uint32_t ambiguity = opts ? opts->ambiguity : 0, strands = opts ? opts->strands : 0;
    if (ambiguity > 1 || strands > 1) return fail(ctx, IPKGPU_ERR_INVALID, "place options: ambiguity and strands are 0 or 1 each");
    if (strands && sigma != 4) return fail(ctx, IPKGPU_ERR_INVALID, "both strands are placed for DNA only (sigma = 4)");
    if (n_queries && (!seq_off || (!seqs && seq_off[n_queries] != seq_off[0]))) return fail(ctx, IPKGPU_ERR_INVALID, "null sequence arrays");
    const uint32_t bps = ipkgpu_bits_per_symbol(sigma);
    if (bps == 0 || k < 1 || k > 16 || bps * k > 32)
        return fail(ctx, IPKGPU_ERR_INVALID, "unsupported sigma / k (%u / %u): k-mer codes are at most 32 bits (DNA k <= 16, amino acids k <= 6)", sigma, k);
    for (uint64_t q = 0; q < n_queries; ++q) {
        if (seq_off[q + 1] < seq_off[q]) return fail(ctx, IPKGPU_ERR_INVALID, "seq_off decreases at query %llu", (unsigned long long)q);
        if (seq_off[q + 1] - seq_off[q] >= (1ull << 32)) return fail(ctx, IPKGPU_ERR_INVALID, "query %llu has 2^32 bytes or more", (unsigned long long)q);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    ipkgpu_kmer_set* set = new (std::nothrow) ipkgpu_kmer_set();
    if (!set) return fail(ctx, IPKGPU_ERR_NOMEM, "out of host memory");
    struct Guard { ipkgpu_kmer_set* s; ~Guard() { if (s) ipkgpu_kmer_set_free(s); } } guard{set};
    set->ctx = ctx; set->sigma = sigma; set->k = k; set->bits = bps * k;
    set->n_codes = 1ull << set->bits;
    set->n_words = std::max<uint64_t>(set->n_codes / 32, 2);            // (an even number of words: the count behind them is 8-byte aligned)
    const size_t bytes = (size_t)set->n_words * 4 + 8;                   // (behind the words: the count)
    {
        const hipError_t e = dev_malloc(ctx, (void**)&set->d_words, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set->d_words = nullptr;
            return fail(ctx, e == hipErrorOutOfMemory ? IPKGPU_ERR_NOMEM : IPKGPU_ERR_HIP, "no room for the k-mer set's bitmap (%llu bytes): %s",
                        (unsigned long long)bytes, hipGetErrorString(e));
        }
        set->bytes = bytes;
    }
    HIP_TRY(ctx, hipMemsetAsync(set->d_words, 0, bytes, ctx->stream));
    const uint32_t max_grid = (uint32_t)ctx->num_cu * 32;
    for (uint64_t q0 = 0; q0 < n_queries;) {
        // the batch, counted as ipkgpu_db_place_opts counts its own: what the two workspaces would have to grow by takes at most half of what is free
        const uint64_t room = mem_free_bytes(ctx) / 2;
        const uint64_t most = ctx->opt_place_batch > 0 ? (uint64_t)ctx->opt_place_batch : PLACE_BATCH_QUERIES;
        auto grows = [](const DevBuf& b, uint64_t need) -> uint64_t { return need <= b.cap ? 0 : need + need / 16 - b.cap; };
        uint64_t q1 = q0 + 1;
        while (q1 < n_queries && q1 - q0 < most) {
            const uint64_t b = seq_off[q1 + 1] - seq_off[q0], n = q1 + 1 - q0;
            if (b > PLACE_BATCH_BYTES || grows(ctx->place_seq, b + 16) + grows(ctx->place_off, (n + 1) * 8) > room) break;
            ++q1;
        }
        const uint64_t nq = q1 - q0, nbytes = seq_off[q1] - seq_off[q0];
        RC_TRY(ensure(ctx, ctx->place_seq, nbytes + 16));
        RC_TRY(ensure(ctx, ctx->place_off, (nq + 1) * 8));
        if (nbytes) HIP_TRY(ctx, hipMemcpyAsync(ctx->place_seq.p, seqs + seq_off[q0], nbytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->place_off.p, seq_off + q0, (nq + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        KmerSetArgs a;
        a.seqs = ctx->place_seq.as<unsigned char>(); a.seq_off = ctx->place_off.as<uint64_t>(); a.seq_base = seq_off[q0];
        a.n_queries = (uint32_t)nq; a.sigma = sigma; a.k = k; a.ambiguity = ambiguity; a.strands = strands; a.bitmap = set->d_words;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(nq, max_grid);
        if (bps == 2) hipLaunchKernelGGL(kmer_set_kernel<2>, dim3(grid), dim3(64), 0, ctx->stream, a);
        else hipLaunchKernelGGL(kmer_set_kernel<5>, dim3(grid), dim3(64), 0, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                 // (the buffers serve the next batch)
        q0 = q1;
    }
    unsigned long long* d_count = reinterpret_cast<unsigned long long*>(set->d_words + set->n_words);
    const uint32_t cgrid = (uint32_t)std::min<uint64_t>((set->n_words + 255) / 256, (uint64_t)ctx->num_cu * 8);
    hipLaunchKernelGGL(kmer_set_count_kernel, dim3(cgrid), dim3(256), 0, ctx->stream, set->d_words, set->n_words, d_count);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long count = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&count, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    set->count = count;
    guard.s = nullptr;
    *out = set;
    return IPKGPU_OK;
}

uint64_t ipkgpu_kmer_set_count(const ipkgpu_kmer_set* set) { return set ? set->count : 0; }
uint32_t ipkgpu_kmer_set_sigma(const ipkgpu_kmer_set* set) { return set ? set->sigma : 0; }
uint32_t ipkgpu_kmer_set_k(const ipkgpu_kmer_set* set) { return set ? set->k : 0; }
uint64_t ipkgpu_kmer_set_num_words(const ipkgpu_kmer_set* set) { return set ? set->n_words : 0; }

const uint32_t* ipkgpu_kmer_set_words(ipkgpu_kmer_set* set)
{
    if (!set) return nullptr;
    if (!set->h_ok) {
        try { set->h_words.resize(set->n_words); } catch (const std::bad_alloc&) { return nullptr; }
        (void)hipSetDevice(set->ctx->device);
        if (hipMemcpy(set->h_words.data(), set->d_words, set->n_words * 4, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
        set->h_ok = true;
    }
    return set->h_words.data();
}

}  // extern "C"
