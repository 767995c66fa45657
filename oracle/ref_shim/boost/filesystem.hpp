// Stand-in for <boost/filesystem.hpp>, which is not needed to compute a filter value.  TEST INFRASTRUCTURE (see
// i2l/phylo_kmer.h next to it).  filter.cpp only declares `namespace fs = boost::filesystem;` -- the namespace is all
// that is supplied.  No constant is defined here.
#pragma once

namespace boost { namespace filesystem {} }
