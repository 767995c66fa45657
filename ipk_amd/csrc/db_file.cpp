// db_file.cpp -- reading a database file back on the host: the head's fields and the walk over the records' count fields.
//
// The reference loads a database with i2l::load (un-vendored) and its tools ipkdiff / ipkdump work on the loaded object
// (tools/src/diff.cpp:118-135, tools/src/dump.cpp).  Here the head is parsed by ipk_format.hpp's reading side and the body is
// walked once, count field by count field: nothing of a file is believed -- by the host or, later, by a kernel of
// ipkgpu_db_load -- before this walk has ended exactly at the end of the file with the header's totals.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../../include/ipkgpu.h"
#include "db_file.hpp"

namespace {

thread_local std::string g_file_err;

int file_fail(const std::string& msg) { g_file_err = msg; return IPKGPU_ERR_INVALID; }

}  // namespace

extern "C" {

const char* ipkgpu_db_file_last_error(void) { return g_file_err.c_str(); }

int ipkgpu_db_file_open(const char* path, ipkgpu_db_file** out)
{
    if (out) *out = nullptr;
    if (!path || !out) return file_fail("null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return file_fail(std::string("cannot open ") + path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    struct stat st;
    if (fstat(fileno(f), &st) != 0) return file_fail(std::string("cannot stat ") + path);
    ipkgpu_db_file* h = new (std::nothrow) ipkgpu_db_file();
    if (!h) { g_file_err = "out of host memory"; return IPKGPU_ERR_NOMEM; }
    h->path = path;
    h->file_bytes = (uint64_t)st.st_size;
    if (const char* what = ipkfmt::read_head_full(f, h->head, h->file_bytes)) {
        const std::string msg = std::string(path) + ": not a database file of this layout: " + what;
        delete h;
        return file_fail(msg);
    }
    if (h->head.body_at > h->file_bytes) { delete h; return file_fail(std::string(path) + ": the file ends inside its head"); }
    *out = h;
    return IPKGPU_OK;
}

void ipkgpu_db_file_close(ipkgpu_db_file* f) { delete f; }

const char* ipkgpu_db_file_sequence_type(const ipkgpu_db_file* f) { return f ? f->head.sequence_type.c_str() : ""; }
int ipkgpu_db_file_positions_loaded(const ipkgpu_db_file* f) { return f && f->head.positions_loaded ? 1 : 0; }
uint32_t ipkgpu_db_file_protocol_version(const ipkgpu_db_file* f) { return f ? f->head.protocol : 0; }
uint32_t ipkgpu_db_file_library_version(const ipkgpu_db_file* f) { return f ? f->head.library_version : 0; }
uint64_t ipkgpu_db_file_tree_index_size(const ipkgpu_db_file* f) { return f ? f->head.tree_num_nodes.size() : 0; }
const uint32_t* ipkgpu_db_file_tree_num_nodes(const ipkgpu_db_file* f) { return f ? f->head.tree_num_nodes.data() : nullptr; }
const double* ipkgpu_db_file_tree_subtree_length(const ipkgpu_db_file* f) { return f ? f->head.tree_subtree_length.data() : nullptr; }
const char* ipkgpu_db_file_newick(const ipkgpu_db_file* f) { return f ? f->head.newick.c_str() : ""; }
uint64_t ipkgpu_db_file_kmer_size(const ipkgpu_db_file* f) { return f ? f->head.kmer_size : 0; }
float ipkgpu_db_file_omega(const ipkgpu_db_file* f) { return f ? f->head.omega : 0.0f; }
uint64_t ipkgpu_db_file_total_kmers(const ipkgpu_db_file* f) { return f ? f->head.total_kmers : 0; }
uint64_t ipkgpu_db_file_total_entries(const ipkgpu_db_file* f) { return f ? f->head.total_entries : 0; }
uint64_t ipkgpu_db_file_bytes(const ipkgpu_db_file* f) { return f ? f->file_bytes : 0; }
uint64_t ipkgpu_db_file_body_offset(const ipkgpu_db_file* f) { return f ? f->head.body_at : 0; }

int ipkgpu_db_file_header(const ipkgpu_db_file* f, ipkgpu_db_header* h)
{
    if (!f || !h) return file_fail("null argument");
    h->sequence_type = f->head.sequence_type.c_str();
    h->tree_index_size = f->head.tree_num_nodes.size();
    h->tree_num_nodes = f->head.tree_num_nodes.data();
    h->tree_subtree_length = f->head.tree_subtree_length.data();
    h->newick = f->head.newick.c_str();
    h->kmer_size = f->head.kmer_size;
    h->omega = f->head.omega;
    return IPKGPU_OK;
}

int ipkgpu_db_file_check(ipkgpu_db_file* f, uint64_t* n_records, uint64_t* n_entries)
{
    if (!f) return file_fail("null argument");
    if (!f->walked) {
        FILE* fh = fopen(f->path.c_str(), "rb");
        if (!fh) return file_fail("cannot open " + f->path);
        struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fh};
        setvbuf(fh, nullptr, _IONBF, 0);
        struct stat st;
        if (fstat(fileno(fh), &st) != 0 || (uint64_t)st.st_size != f->file_bytes) return file_fail(f->path + ": the file changed since it was opened");
        if (fseeko(fh, (off_t)f->head.body_at, SEEK_SET) != 0) return file_fail(f->path + ": seek failed");
        ipkfmt::RecordWalker w;
        const uint64_t body = f->body_bytes();
        w.begin(f->head.body_at, body, f->head.positions_loaded, f->head.total_kmers);
        std::vector<uint8_t> buf((size_t)std::min<uint64_t>(std::max<uint64_t>(body, 1), (uint64_t)8 << 20));
        for (uint64_t lo = 0; lo < body; lo += buf.size()) {
            const uint64_t hi = std::min<uint64_t>(body, lo + buf.size());
            if (fread(buf.data(), 1, (size_t)(hi - lo), fh) != hi - lo) return file_fail(f->path + ": read failed");
            if (!w.feed(buf.data(), lo, hi)) return file_fail(f->path + ": " + w.error);
        }
        if (!w.finish(f->head.total_kmers, f->head.total_entries)) return file_fail(f->path + ": " + w.error);
        f->walked = true; f->n_records = w.starts.size(); f->n_entries = w.n_entries; f->max_count = w.max_count;
    }
    if (n_records) *n_records = f->n_records;
    if (n_entries) *n_entries = f->n_entries;
    return IPKGPU_OK;
}

}  // extern "C"
