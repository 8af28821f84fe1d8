// megaverse_amd/csrc/mv_env_store.h -- env stores (include/megaverse_hip.h: mv_save_envs, mv_load_envs): an env's episode state packed into a RECORD in
// caller-owned device memory, and a record loaded back into any env of a gym of the same configuration.  A record is fork::Table (mv_fork.h), packed; a load
// is a fork whose source is a record.  No reference counterpart.  DESIGN.md 3.11.
//
// Written once, here, for the kernels (mv_env_store.hip), the host validators (mv_save_envs_host, mv_load_envs_host) and the host-only test hooks
// (mv_debug_env_store_plan_host, mv_debug_env_record_pack_host, mv_debug_env_record_unpack_host):
//   * the LAYOUT of a record (layout_of): a 64-byte record header, the whole EnvHeader, every array of the table in table order -- each from a 16-byte
//     boundary, with its whole stride -- and the episode log's accumulators, double ret[A] and int32 len, which are always present;
//   * the record HEADER, dword by dword (header_dword), and the check a load makes on it (header_matches);
//   * the RULE of the two maps (save_resolve, load_resolve) and their tabulated host forms (save_plan, load_plan);
//   * what a load takes from a record's EnvHeader (loads_header_dword) and what goes into and comes out of the accumulators (saved_log_dword,
//     loaded_log_dword).
// The header is a guard against accidents -- a slot never written, a record of another configuration or format version -- not an authenticator: the bytes
// behind a header that matches are trusted, counts that kernels index by included.  A store comes from mv_save_envs or from a copy of what it wrote.
#pragma once
#include "mv_fork.h"

namespace mv {
namespace store {

enum : uint32_t { MAGIC = 0x5652454Du /* "MERV" */, FORMAT_VERSION = 1, HEADER_BYTES = 64, HEADER_DWORDS = 16, FLAG_LOG = 1 /* the log was on at save time */ };
enum : int { LEAVE = fork::LEAVE, INVALID = fork::INVALID };
// dwords of the record header: {magic, format version, layout word (2), record bytes (2), flags, 0 ...}
enum : int { HD_MAGIC = 0, HD_VERSION = 1, HD_LAYOUT = 2, HD_BYTES = 4, HD_FLAGS = 6, HD_CHECKED = 7 };

struct Layout {
    int32_t count, A;
    uint32_t env_hdr;                     // offset of the EnvHeader: HEADER_BYTES
    uint32_t off[fork::MAX_ARRAYS];       // offset of array k
    uint32_t ret, len;                    // offsets of the accumulators
    uint32_t bytes;                       // of the whole record: a multiple of 16
};

MV_FORK_HD uint32_t up16(uint32_t b) { return (b + 15u) & ~15u; }

MV_FORK_HD Layout layout_of(const uint32_t *array_bytes, int count, int A)
{
    Layout L{};
    L.count = count; L.A = A;
    L.env_hdr = HEADER_BYTES;
    uint32_t o = HEADER_BYTES + (uint32_t)sizeof(EnvHeader);
    for (int k = 0; k < count && k < fork::MAX_ARRAYS; ++k) { L.off[k] = o; o = up16(o + array_bytes[k]); }
    L.ret = o; o = up16(o + (uint32_t)A * 8u);
    L.len = o; o = up16(o + 4u);
    L.bytes = o;
    return L;
}
inline Layout layout_of(const fork::Table &t, int A)
{
    uint32_t b[fork::MAX_ARRAYS] = {};
    for (int k = 0; k < t.count; ++k) b[k] = t.a[k].bytes;
    return layout_of(b, t.count, A);
}

// dword i of the header of a record of `bytes` bytes and layout word `layout`, saved with `flags`
MV_FORK_HD uint32_t header_dword(int i, uint64_t layout, uint32_t bytes, uint32_t flags)
{
    return i == HD_MAGIC ? (uint32_t)MAGIC : i == HD_VERSION ? (uint32_t)FORMAT_VERSION : i == HD_LAYOUT ? (uint32_t)layout : i == HD_LAYOUT + 1 ? (uint32_t)(layout >> 32)
         : i == HD_BYTES ? bytes : i == HD_FLAGS ? flags : 0u;
}
// does dword i (< HD_CHECKED) of a record's header, `have`, let this gym load the record?  (the flags: any value made of known bits)
MV_FORK_HD bool header_dword_matches(int i, uint32_t have, uint64_t layout, uint32_t bytes)
{
    return i == HD_FLAGS ? (have & ~(uint32_t)FLAG_LOG) == 0 : have == header_dword(i, layout, bytes, 0);
}
MV_FORK_HD bool header_matches(const uint32_t *record, uint64_t layout, uint32_t bytes)
{
    bool ok = true;
    for (int i = 0; i < HD_CHECKED; ++i) ok = ok && header_dword_matches(i, record[i], layout, bytes);
    return ok;
}

// a load writes dword i of the record's EnvHeader into the env's, unless it is one of the identity's (mv_fork.h)
MV_FORK_HD bool loads_header_dword(int i) { return !((fork::IDENTITY_DWORDS >> i) & 1u); }

// The accumulators as dwords: 2 A of ret, then one of len (j = 2 A).  A save writes the gym's where its log is on, else zero; a load into a gym whose log
// is on takes the record's where its flag is set, else zero: the episode counts from the load, as when the log is switched on mid-episode.
MV_FORK_HD uint32_t saved_log_dword(bool log_on, uint32_t live) { return log_on ? live : 0u; }
MV_FORK_HD uint32_t loaded_log_dword(uint32_t flags, uint32_t recorded) { return flags & FLAG_LOG ? recorded : 0u; }
MV_FORK_HD uint32_t log_dword_offset(const Layout &L, int j) { return j < 2 * L.A ? L.ret + 4u * (uint32_t)j : L.len; }

// ---- the rule of the two maps.  slot_of[e] = -1: env e takes no part.  Save: an index out of range is invalid, and so is every entry whose slot another
// env names too (neither is written).  Load: an index out of range is invalid, that alone -- any number of envs may load one record.  (Whether the record
// itself can be loaded is the header's matter, which only the device sees.)
MV_FORK_HD bool slot_in_range(int32_t m, int32_t slots) { return m >= 0 && m < slots; }
// does one of the entries first, first + step, ... besides e's own name slot m?  (the kernel's threads share the loop out, as fork::named_as_source's do)
MV_FORK_HD bool slot_named_again(const int32_t *slot_of, int32_t N, int32_t e, int32_t m, int32_t first, int32_t step)
{
    for (int32_t i = first; i < N; i += step)
        if (i != e && slot_of[i] == m) return true;
    return false;
}
MV_FORK_HD int32_t load_resolve(const int32_t *slot_of, int32_t slots, int32_t e)
{
    const int32_t m = slot_of[e];
    return m == -1 ? (int32_t)LEAVE : slot_in_range(m, slots) ? m : (int32_t)INVALID;
}
MV_FORK_HD int32_t save_resolve(const int32_t *slot_of, int32_t N, int32_t slots, int32_t e)
{
    const int32_t m = load_resolve(slot_of, slots, e);
    return m >= 0 && slot_named_again(slot_of, N, e, m, 0, 1) ? (int32_t)INVALID : m;
}
// the same for every entry at once, for the host forms: `times` counts (to 2) how often each slot is named
inline void save_plan(const int32_t *slot_of, int32_t N, int32_t slots, int32_t *resolved, std::vector<uint8_t> &times)
{
    times.assign((size_t)(slots > 0 ? slots : 0), 0);
    for (int32_t i = 0; i < N; ++i)
        if (slot_in_range(slot_of[i], slots) && times[(size_t)slot_of[i]] < 2) ++times[(size_t)slot_of[i]];
    for (int32_t e = 0; e < N; ++e) {
        const int32_t m = load_resolve(slot_of, slots, e);
        resolved[e] = m >= 0 && times[(size_t)m] > 1 ? (int32_t)INVALID : m;
    }
}
inline void load_plan(const int32_t *slot_of, int32_t N, int32_t slots, int32_t *resolved)
{
    for (int32_t e = 0; e < N; ++e) resolved[e] = load_resolve(slot_of, slots, e);
}

// ---- the layout word: two gyms with the same word can exchange records.  FNV-1a over the format version, the scenario (id and name: the Obstacles variants
// share an id), the agents per env, the observation size, every float parameter (key and value, in key order) and every table array's bytes per env.
struct Hash {
    uint64_t h = 0xCBF29CE484222325ull;
    void bytes(const void *p, size_t n) { for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001B3ull; }
    void u32(uint32_t v) { bytes(&v, 4); }
    uint64_t word() const { return h ? h : 1; }   // (0 is mv_env_record_layout's "no gym")
};

// the launches (mv_env_store.hip).  log_ret / log_len: the gym's accumulators, null where its log is off.  Every valid entry is applied; ST_ENV_STORE is
// raised in status[N + 1] for an invalid one -- and, by the load, for a record whose header does not match.
void launch_save(const fork::Table &t, const Layout &L, uint64_t layout_word, const double *log_ret, const int32_t *log_len, const int32_t *device_slot_of,
                 int32_t N, uint8_t *store, int32_t slots, int32_t *status, hipStream_t stream);
void launch_load(const fork::Table &t, const Layout &L, uint64_t layout_word, double *log_ret, int32_t *log_len, const int32_t *device_slot_of, int32_t N,
                 const uint8_t *store, int32_t slots, int32_t *status, hipStream_t stream);

}  // namespace store
}  // namespace mv
