// Stand-in for the un-vendored i2l header <i2l/hash_map.h>.  TEST INFRASTRUCTURE (see phylo_kmer.h next to it).
// Names supplied: i2l::hash_map<K, V>, which branch_group.h needs to declare group_hash_map (SURVEY.md App. B,
// i2l/hash_map.h row: upstream selects an implementation at build time).  The alias is only declared against, no
// compiled code path touches a hash map.  No constant is defined here.
#pragma once
#include <unordered_map>

namespace i2l
{
    template<class K, class V>
    using hash_map = std::unordered_map<K, V>;
}
