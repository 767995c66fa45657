// Stand-in for the un-vendored i2l header <i2l/phylo_kmer_db.h>.  TEST INFRASTRUCTURE: lets oracle/ref_build.py
// compile the reference's filter.cpp unchanged.
//
// Names supplied (what filter.cpp, filter.h and branch_group.h require):
//   i2l::pkdb_value{branch, score}          one database entry; filter.cpp binds it as [branch, log_score]
//   i2l::phylo_kmer_db                      iteration as [key, entries] in ascending key order, entries.size(),
//                                           and unsafe_insert(key, {branch, score}) for the driver to fill it
//   i2l::kmer_fv{key, filter_value}         filter_value is a double here so that the driver sees the value
//                                           filter.cpp computes before any narrowing (the narrowing to float
//                                           happens inside i2l and stays an assumption, DESIGN.md "Oracle")
// No constant is defined here.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>
#include <i2l/phylo_kmer.h>

namespace i2l
{
    struct pkdb_value
    {
        phylo_kmer::branch_type branch;
        phylo_kmer::score_type score;
    };

    class phylo_kmer_db
    {
    public:
        using key_type = phylo_kmer::key_type;
        using value_type = std::vector<pkdb_value>;
        using storage = std::map<key_type, value_type>;
        using const_iterator = storage::const_iterator;

        void unsafe_insert(key_type key, const pkdb_value& value) { _map[key].push_back(value); }
        const_iterator begin() const { return _map.begin(); }
        const_iterator end() const { return _map.end(); }
        size_t size() const { return _map.size(); }

    private:
        storage _map;
    };

    struct kmer_fv
    {
        phylo_kmer::key_type key;
        double filter_value;
    };
}
