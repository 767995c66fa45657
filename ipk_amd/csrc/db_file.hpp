// db_file.hpp -- what ipkgpu_db_file_open keeps of a database file (host): the parsed head and, once the records have been
// walked (ipkgpu_db_file_check, or ipkgpu_db_load on its way through the file), their totals.  Bytes: ipk_format.hpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ipk_format.hpp"

struct ipkgpu_db_file {
    std::string path;
    uint64_t file_bytes = 0;
    ipkfmt::Head head;
    bool walked = false;                  // the records' walk has succeeded: n_records / n_entries are the file's
    uint64_t n_records = 0, n_entries = 0, max_count = 0;
    uint64_t body_bytes() const { return file_bytes - head.body_at; }
};
