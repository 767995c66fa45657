// Stand-in for the un-vendored i2l header <i2l/phylo_kmer.h> (and, through i2l/seq.h, for <i2l/seq.h>).
// TEST INFRASTRUCTURE: it exists so that oracle/ref_build.py can compile the reference's scoring and
// filter translation units unchanged; nothing of the product includes it.
//
// Names supplied (exactly what window.cpp, pk_compute.cpp, filter.cpp and their headers require):
//   i2l::seq_type, i2l::seq_traits::alphabet_size, i2l::bit_length<seq_type>(),
//   i2l::phylo_kmer::{key_type, score_type, branch_type, pos_type} with members key, score,
//   i2l::unpositioned_phylo_kmer{key, score}, and <stdexcept> (std::runtime_error).
//
// Where the constants come from (the i2l sources are not available):
//   alphabet_size  4 for DNA, 20 for amino acids (-DSEQ_TYPE_AA)       -- App. B, i2l/seq.h row
//   bit_length     2 bits a DNA symbol, 5 bits an amino-acid symbol    -- App. B, i2l/seq.h row
//   key_type       32-bit unsigned, score_type float                   -- App. A.1, App. B i2l/phylo_kmer.h row
//   branch_type    32-bit unsigned, pos_type 16-bit unsigned           -- App. B; neither enters the compiled code paths
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

namespace i2l
{
    struct dna {};
    struct aa {};

#ifdef SEQ_TYPE_AA
    using seq_type = aa;
    struct seq_traits { static constexpr size_t alphabet_size = 20; };
    template<class T> constexpr size_t bit_length() { return 5; }
#else
    using seq_type = dna;
    struct seq_traits { static constexpr size_t alphabet_size = 4; };
    template<class T> constexpr size_t bit_length() { return 2; }
#endif

    struct phylo_kmer
    {
        using key_type = uint32_t;
        using score_type = float;
        using branch_type = uint32_t;
        using pos_type = uint16_t;

        key_type key;
        score_type score;
    };

    struct unpositioned_phylo_kmer
    {
        phylo_kmer::key_type key;
        phylo_kmer::score_type score;
    };
}
