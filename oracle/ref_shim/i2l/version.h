// Stand-in for the un-vendored i2l header <i2l/version.h>.  TEST INFRASTRUCTURE (see phylo_kmer.h next to it).
// filter.cpp includes it and uses nothing of it: no name and no constant is supplied.
#pragma once
