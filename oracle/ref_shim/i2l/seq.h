// Stand-in for the un-vendored i2l header <i2l/seq.h>.  TEST INFRASTRUCTURE (see phylo_kmer.h next to it).
// Names supplied: i2l::seq_type, i2l::seq_traits::alphabet_size, i2l::bit_length<seq_type>() -- all defined in
// the stand-in phylo_kmer.h, which also says where each constant comes from.
#pragma once
#include <i2l/phylo_kmer.h>
