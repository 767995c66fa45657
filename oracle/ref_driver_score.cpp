// ref_driver_score.cpp -- TEST INFRASTRUCTURE: a main() around the reference's own scoring code.
//
// Linked by oracle/ref_build.py with the reference's ipk/src/window.cpp and ipk/src/pk_compute.cpp, compiled unchanged
// against the stand-in headers of oracle/ref_shim/ (DNA, or amino acids with -DSEQ_TYPE_AA).  This file is the
// project's own text; it only calls matrix, matrix::preprocess, to_windows, window::get_position and DCLA.
//
// stdin (binary, host byte order):
//   uint32 n_mats, uint32 sites, uint32 k, uint32 eps_bits           eps as the bit pattern of a float
//   n_mats x [sites][sigma] float32                                  site-major log10 probabilities
// stdout, for every matrix in order and every window of to_windows(&matrix, k) in iteration order:
//   uint64 window.get_position(), uint64 count
//   count x (uint32 key, uint32 score_bits)                          DCLA(window, k).run(eps), in emission order
// Exit status 2 on a short or malformed input.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <pk_compute.h>
#include <window.h>

namespace
{
    bool read_all(void* dst, size_t bytes)
    {
        return bytes == 0 || std::fread(dst, 1, bytes, stdin) == bytes;
    }

    void put_u32(std::vector<unsigned char>& out, uint32_t v)
    {
        unsigned char b[4];
        std::memcpy(b, &v, 4);
        out.insert(out.end(), b, b + 4);
    }

    void put_u64(std::vector<unsigned char>& out, uint64_t v)
    {
        unsigned char b[8];
        std::memcpy(b, &v, 8);
        out.insert(out.end(), b, b + 8);
    }
}

int main()
{
    constexpr size_t sigma = i2l::seq_traits::alphabet_size;
    uint32_t head[4];
    if (!read_all(head, sizeof(head)))
        return 2;
    const uint32_t n_mats = head[0], sites = head[1], k = head[2];
    float eps;
    std::memcpy(&eps, &head[3], 4);
    if (k == 0 || sites < k)                         // to_windows does not guard sites < k
        return 2;

    std::vector<unsigned char> out;
    std::vector<float> raw(size_t(sites) * sigma);
    for (uint32_t q = 0; q < n_mats; ++q)
    {
        if (!read_all(raw.data(), raw.size() * sizeof(float)))
            return 2;
        std::vector<ipk::matrix::column> data(sites);
        for (size_t j = 0; j < sites; ++j)
            for (size_t i = 0; i < sigma; ++i)
                data[j][i] = raw[j * sigma + i];

        ipk::matrix m(std::move(data), "m");
        m.preprocess();
        for (auto& window : ipk::to_windows(&m, k))
        {
            ipk::DCLA dcla(window, k);
            dcla.run(eps);
            const auto& result = dcla.get_result();
            put_u64(out, window.get_position());
            put_u64(out, result.size());
            for (const auto& kmer : result)
            {
                uint32_t bits;
                const float score = kmer.score;
                std::memcpy(&bits, &score, 4);
                put_u32(out, kmer.key);
                put_u32(out, bits);
            }
        }
    }
    return std::fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 2;
}
