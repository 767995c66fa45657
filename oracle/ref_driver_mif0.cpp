// ref_driver_mif0.cpp -- TEST INFRASTRUCTURE: a main() around the reference's own MIF0 filter.
//
// Linked by oracle/ref_build.py with the reference's ipk/src/filter.cpp, compiled unchanged against the stand-in headers
// of oracle/ref_shim/.  This file is the project's own text; it fills the stand-in database and calls
// make_filter(filter_type::mif0, ...)->calc_filter_values.
//
// stdin (binary, host byte order):
//   uint64 N (total number of groups), uint32 threshold_bits (a float), uint32 n_keys
//   n_keys x { uint32 n, n x float32 log10 score }                   key i is the i-th list; its entries keep their order
// stdout: n_keys x 8 bytes, the double filter value of key 0, 1, ...
// Exit status 2 on a short or malformed input.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <filter.h>

int main()
{
    uint64_t N;
    uint32_t head[2];
    if (std::fread(&N, 8, 1, stdin) != 1 || std::fread(head, 4, 2, stdin) != 2)
        return 2;
    float threshold;
    std::memcpy(&threshold, &head[0], 4);
    const uint32_t n_keys = head[1];

    i2l::phylo_kmer_db db;
    std::vector<float> scores;
    for (uint32_t key = 0; key < n_keys; ++key)
    {
        uint32_t n;
        if (std::fread(&n, 4, 1, stdin) != 1 || n == 0)
            return 2;
        scores.resize(n);
        if (std::fread(scores.data(), 4, n, stdin) != n)
            return 2;
        for (uint32_t e = 0; e < n; ++e)
            db.unsafe_insert(key, { e, scores[e] });
    }

    const auto filter = ipk::make_filter(ipk::filter_type::mif0, size_t(N), "", 1, threshold);
    const auto values = filter->calc_filter_values(db);
    if (values.size() != n_keys)
        return 2;
    std::vector<double> out(n_keys);
    for (const auto& fv : values)
        out[fv.key] = fv.filter_value;
    return std::fwrite(out.data(), 8, out.size(), stdout) == out.size() ? 0 : 2;
}
