// spill_format.hpp -- the bytes of a spill block (workdir/hashmaps/p<piece>_b<batch>.blk): the ONE place that knows them.
//
// A block is one owner's share of one piece of the on-disk build (the role of a batch of the reference's per-group hash-map
// files, branch_group.cpp:104-185): the owner's counts row of ipkgpu_score_groups_keymajor_device(..., n_owners = B) and its
// entry block, taken off the device between stage 1 and stage 2.  Little endian, every part a multiple of 8 bytes:
//
//   Head                 64 bytes (below)
//   bits                 u64 [ceil(slots / 64)]   bit (q & 63) of word q / 64 set <=> slot q has entries
//   counts               u16 [n_keys]             the non-empty slots' counts in slot order; zero bytes up to a multiple of 8
//   entries              {u32 branch, u32 score bits} [n_entries], the owner's entry block unchanged
//
// The dense row costs 4 bytes per slot whatever the piece holds; this form 1 bit per slot + 2 bytes per non-empty slot.  A key
// has at most one entry per group, so u16 holds the count of any piece of up to 65535 groups.
#pragma once
#include <cstdint>
#include <cstring>

namespace ipkspill {

constexpr char MAGIC[8] = {'I', 'P', 'K', 'S', 'P', 'I', 'L', 'L'};
constexpr uint32_t VERSION = 1;
constexpr uint32_t COUNT_MAX = 0xFFFFu;        // largest count the u16 field holds = most groups of a piece

struct Head {
    char magic[8];
    uint32_t version, sigma, k, n_owners, owner, piece;
    uint64_t slots, n_keys, n_entries, reserved;
};
static_assert(sizeof(Head) == 64, "the head is 64 bytes");

inline uint64_t bit_words(uint64_t slots) { return (slots + 63) / 64; }
inline uint64_t bits_bytes(uint64_t slots) { return bit_words(slots) * 8; }
inline uint64_t counts_bytes(uint64_t n_keys) { return (n_keys * 2 + 7) & ~7ull; }       // padded
inline uint64_t entries_bytes(uint64_t n_entries) { return n_entries * 8; }
inline uint64_t bits_at() { return sizeof(Head); }
inline uint64_t counts_at(uint64_t slots) { return bits_at() + bits_bytes(slots); }
inline uint64_t entries_at(uint64_t slots, uint64_t n_keys) { return counts_at(slots) + counts_bytes(n_keys); }
inline uint64_t file_bytes(uint64_t slots, uint64_t n_keys, uint64_t n_entries) { return entries_at(slots, n_keys) + entries_bytes(n_entries); }
// what the dense form of the same block would take: the counts row as it stands on the device, and the entries
inline uint64_t dense_bytes(uint64_t slots, uint64_t n_entries) { return slots * 4 + entries_bytes(n_entries); }

inline Head make_head(uint32_t sigma, uint32_t k, uint32_t n_owners, uint32_t owner, uint32_t piece, uint64_t slots, uint64_t n_keys,
                      uint64_t n_entries)
{
    Head h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, MAGIC, 8);
    h.version = VERSION; h.sigma = sigma; h.k = k; h.n_owners = n_owners; h.owner = owner; h.piece = piece;
    h.slots = slots; h.n_keys = n_keys; h.n_entries = n_entries;
    return h;
}

// nullptr if `h`, read from a file of `size` bytes, is the head of owner `owner`'s block of a (sigma, k, n_owners) build with
// `slots` slots per owner; otherwise what is wrong with it (a static string)
inline const char* check_head(const Head& h, uint64_t size, uint32_t sigma, uint32_t k, uint32_t n_owners, uint32_t owner, uint64_t slots)
{
    if (size < sizeof(Head)) return "shorter than a block's head";
    if (memcmp(h.magic, MAGIC, 8) != 0) return "not a spill block (magic)";
    if (h.version != VERSION) return "a spill block of another format version";
    if (h.sigma != sigma) return "written for another alphabet";
    if (h.k != k) return "written at another k";
    if (h.n_owners != n_owners) return "written for another number of batches";
    if (h.owner != owner) return "the block of another batch";
    if (h.slots != slots) return "another number of key slots";
    if (h.n_keys > h.slots || h.n_entries < h.n_keys || h.n_entries > h.n_keys * (uint64_t)COUNT_MAX) return "inconsistent totals";
    if (size != file_bytes(h.slots, h.n_keys, h.n_entries)) return "the file size does not match its head (truncated?)";
    return nullptr;
}

}  // namespace ipkspill
