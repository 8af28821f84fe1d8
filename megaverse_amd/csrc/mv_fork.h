// megaverse_amd/csrc/mv_fork.h -- env forks (include/megaverse_hip.h: mv_fork_envs): env d leaves its running episode and continues env s's, from s's
// current state, inside one gym.  No reference counterpart (its envs are separate objects with no copy, env.hpp).  DESIGN.md 3.8.
//
// Two things are written once, here:
//   * the RULE of a fork map -- which source an entry resolves to, or that it is left alone, or invalid (fork_resolve) -- for the kernel (mv_fork.hip), the
//     host validator (mv_fork_envs_host) and the host-only test hook (mv_debug_fork_plan_host);
//   * the TABLE of an env's episode state (fork::Table): every per-env slice a tick or a frame setup reads or writes, as (base, bytes per env).  mv_create
//     fills it where it carves the arena (mv_api.hip); the launch takes it by value.  What is NOT in it is the env's identity: its entries of
//     episode_status, its ring of resident episodes, TowerGen, and the EnvHeader fields of IDENTITY_DWORDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mv_types.h"

namespace mv {
namespace fork {

#define MV_FORK_HD __host__ __device__ inline

enum : int { LEAVE = -1, INVALID = -2 };   // what an entry resolves to besides a source index

// src_of[d] = -1 or d: env d is left alone
MV_FORK_HD bool leaves_alone(int32_t s, int32_t d) { return s == -1 || s == d; }

// The part of the rule that looks at entry d and at its source's entry only: LEAVE, INVALID (an index out of range; a source that is itself a destination --
// an in-place gather cannot honour a chain), or the source s.
MV_FORK_HD int32_t entry_source(const int32_t *src_of, int32_t N, int32_t d)
{
    const int32_t s = src_of[d];
    if (leaves_alone(s, d)) return LEAVE;
    if (s < 0 || s >= N) return INVALID;
    if (!leaves_alone(src_of[s], s)) return INVALID;
    return s;
}

// ... and the part that looks at everybody else: does one of the entries first, first + step, ... name env d as its source?  (A destination may not serve
// as a source in the same call: the other half of "no chains".  An entry that is invalid itself still counts: what it names stays untouched.)  The kernel's
// threads share the loop out (first = thread, step = threads); the host walks it whole (0, 1).
MV_FORK_HD bool named_as_source(const int32_t *src_of, int32_t N, int32_t d, int32_t first, int32_t step)
{
    for (int32_t i = first; i < N; i += step)
        if (i != d && src_of[i] == d) return true;
    return false;
}

// the whole rule for entry d: the source env d continues from, LEAVE, or INVALID
MV_FORK_HD int32_t fork_resolve(const int32_t *src_of, int32_t N, int32_t d)
{
    const int32_t s = entry_source(src_of, N, d);
    if (s < 0) return s;
    return named_as_source(src_of, N, d, 0, 1) ? (int32_t)INVALID : s;
}

// The same rule for every entry at once in O(N), for the host form (a planner validates a map of a thousand envs per iteration; fork_resolve per entry is
// O(N) each): `named` tabulates named_as_source for every env.  resolved[d]: the source, LEAVE or INVALID.  mv_debug_fork_plan_host checks it against
// fork_resolve entry by entry.
inline void fork_plan(const int32_t *src_of, int32_t N, int32_t *resolved, std::vector<uint8_t> &named)
{
    named.assign((size_t)(N > 0 ? N : 0), 0);
    for (int32_t i = 0; i < N; ++i) {
        const int32_t s = src_of[i];
        if (!leaves_alone(s, i) && s >= 0 && s < N) named[(size_t)s] = 1;
    }
    for (int32_t d = 0; d < N; ++d) {
        const int32_t s = entry_source(src_of, N, d);
        resolved[d] = s >= 0 && named[(size_t)d] ? (int32_t)INVALID : s;
    }
}

// ---- the rule of a RESAMPLING map (include/megaverse_hip.h: mv_resample_envs): new state of env d = the state env src_of[d] had before the call, for ANY
// map -- chains, swaps, cycles, a source that is overwritten itself.  Entry d is left alone (-1 or d), invalid (an index out of range: that alone), or valid.
MV_FORK_HD int32_t resample_source(const int32_t *src_of, int32_t N, int32_t d)
{
    const int32_t s = src_of[d];
    if (leaves_alone(s, d)) return LEAVE;
    return s < 0 || s >= N ? (int32_t)INVALID : s;
}
// Env d is STAGED when its entry is valid and another valid entry names d as its source: its old state is still needed while its new one arrives.  ("Another
// valid entry names d" is named_as_source as it stands: an entry i != d that holds d holds an index in range and does not leave env i alone -- and an invalid
// entry holds no env's index, so it names nobody.)
// The copy has two phases, and these two functions are what decides them, for the kernels (mv_resample.hip) and the host hooks alike.  Phase 1, every valid d:
// env src_of[d]'s LIVE state goes to env d's live arrays (d is not staged: nobody reads them) or to slot d of the staging arena (d is staged).  Phase 2,
// every staged d: slot d goes to env d's live arrays.  No live env that phase 1 reads is written in phase 1 -- an env that is read is named, and a named
// env with a valid entry is staged by definition -- and phase 2 touches env d alone.
enum : int { TO_NOWHERE = 0, TO_LIVE = 1, TO_STAGING = 2 };
MV_FORK_HD int phase1_target(int32_t resolved, bool named) { return resolved < 0 ? (int)TO_NOWHERE : named ? (int)TO_STAGING : (int)TO_LIVE; }
MV_FORK_HD bool phase2_copies(int target) { return target == TO_STAGING; }   // (target: what phase 1 left in the env's byte of the plan)

// the whole rule for entry d, one entry at a time (the kernel's form; O(N) per entry on the host) -> phase1_target; resolved: the source, LEAVE or INVALID
MV_FORK_HD int resample_resolve(const int32_t *src_of, int32_t N, int32_t d, int32_t *resolved)
{
    const int32_t s = resample_source(src_of, N, d);
    *resolved = s;
    return phase1_target(s, s >= 0 && named_as_source(src_of, N, d, 0, 1));
}

// ... and for every entry at once in O(N), for the host form: target[d] = phase1_target.  mv_debug_resample_plan_host checks it against resample_resolve.
inline void resample_plan(const int32_t *src_of, int32_t N, int32_t *resolved, std::vector<uint8_t> &target)
{
    target.assign((size_t)(N > 0 ? N : 0), 0);   // (first pass: "named", as in fork_plan)
    for (int32_t i = 0; i < N; ++i) {
        const int32_t s = resample_source(src_of, N, i);
        if (s >= 0) target[(size_t)s] = 1;
    }
    for (int32_t d = 0; d < N; ++d) {
        resolved[d] = resample_source(src_of, N, d);
        target[(size_t)d] = (uint8_t)phase1_target(resolved[d], target[(size_t)d] != 0);
    }
}

// ---- the episode state of one env
enum : int { MAX_ARRAYS = 16 };
// A launch covers (destination env) x RANGES ranges of the env's state, THREADS threads each: three envs of a Hex gym (~73 KB each) still make 12
// workgroups of 18 KB, 1024 envs a streaming copy of 4096.  (Measured at 1024 destinations with 8 ranges and one array after the other: 22 us for
// TowerBuilding's 21.5 MB, and the same for half of them -- a launch of many rounds of short workgroups, each a chain of dependent memory round trips,
// not a stream; profiles/fork_measured.txt.)
enum : int { RANGES = 4, THREADS = 256, BATCH = 6 };   // BATCH: 16-byte loads a thread has in flight before its first store (HexMemory: 5 per thread)

struct Array {
    uint8_t *base;       // [N][bytes]
    uint32_t bytes;      // per env: the whole stride, not the live count (a fork's slices equal its source's byte for byte)
    uint32_t unit;       // 16 where base and bytes allow 16-byte loads and stores, else 4, else 1
};

struct Table {
    EnvHeader *hdr;      // copied dword by dword, the identity fields left out
    int32_t count;
    uint32_t total16;    // 16-byte rows of one env over all arrays of unit 16: the launch's ranges divide this one row space
    Array a[MAX_ARRAYS];
    uint32_t first16[MAX_ARRAYS + 1];   // array k holds rows first16[k] .. first16[k + 1] - 1 of that space (an array of another unit: none)
};

inline void table_add(Table &t, void *base, size_t bytes_per_env)
{
    if (!base || !bytes_per_env || t.count >= MAX_ARRAYS) return;
    const uintptr_t both = (uintptr_t)base | (uintptr_t)bytes_per_env;
    t.a[t.count++] = Array{(uint8_t *)base, (uint32_t)bytes_per_env, both % 16 == 0 ? 16u : both % 4 == 0 ? 4u : 1u};
    uint32_t rows = 0;
    for (int k = 0; k < MAX_ARRAYS; ++k) {
        t.first16[k] = rows;
        if (k < t.count && t.a[k].unit == 16) rows += t.a[k].bytes / 16;
    }
    t.first16[MAX_ARRAYS] = t.total16 = rows;
}
inline size_t table_bytes_per_env(const Table &t)
{
    size_t b = sizeof(EnvHeader);
    for (int i = 0; i < t.count; ++i) b += t.a[i].bytes;
    return b;
}

// EnvHeader dwords a fork leaves to env d: next_seed, seed_is_env_seed (its seed chain), episodes_consumed, starved (its place in the refill protocol)
constexpr uint32_t hdr_bit(size_t offset) { return 1u << (offset / 4); }
constexpr uint32_t IDENTITY_DWORDS = hdr_bit(offsetof(EnvHeader, next_seed)) | hdr_bit(offsetof(EnvHeader, seed_is_env_seed))
                                     | hdr_bit(offsetof(EnvHeader, episodes_consumed)) | hdr_bit(offsetof(EnvHeader, starved));
static_assert(sizeof(EnvHeader) == 32 * 4, "EnvHeader: 32 dwords, one bit each in IDENTITY_DWORDS");

// the slices are 16-byte rows: what the 16-byte path of the copy relies on (an array that breaks this still copies, on the dword or byte path)
static_assert(sizeof(LayoutBox) % 16 == 0 && sizeof(AgentState) % 16 == 0 && sizeof(TerrainBox) % 16 == 0 && sizeof(ArrangementItem) % 16 == 0
              && sizeof(HexRec) % 16 == 0 && sizeof(BoxAGoneState) % 16 == 0 && sizeof(FootballState) % 16 == 0, "per-env records are 16-byte rows");
static_assert(CHUNK_BYTES % 16 == 0 && HM_BYTES % 16 == 0 && (SOKO_DIM * SOKO_DIM) % 16 == 0 && (MAX_OBJECTS * sizeof(MovableObject)) % 16 == 0
              && (MAX_REWARDS * sizeof(MovableObject)) % 16 == 0 && (COLLECT_MAX_REWARDS * sizeof(MovableObject)) % 16 == 0, "per-env byte arrays are 16-byte rows");

// one launch: every valid entry of src_of applied, ST_FORK raised in status[N + 1] for an invalid one (mv_fork.hip)
void launch_fork(const Table &t, const int32_t *device_src_of, int32_t N, int32_t *status, hipStream_t stream);

// ---- the staging arena of mv_resample_envs: a second home for every staged env's incoming state, laid out like the live arrays -- the header slice [N],
// then one slice [N][bytes] per array of the table, each from a 16-byte boundary, so that a row of array k has the alignment it has in the live array --
// and the plan, one byte per env (phase1_target), which phase 1 writes and phase 2 reads.
struct Staging {
    EnvHeader *hdr;
    uint8_t *plan;                 // [N]
    uint8_t *a[MAX_ARRAYS];        // array k of the table: [N][t.a[k].bytes]
};
inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
// bytes of the arena for N envs of table t plus `extra` further bytes per env, each array rounded as above (the episode log's accumulators: the arena is
// sized once, for a log that may be switched on later)
inline size_t staging_bytes(const Table &t, int32_t N, size_t extra_a, size_t extra_b)
{
    size_t b = round16((size_t)N * sizeof(EnvHeader)) + round16((size_t)N);
    for (int k = 0; k < t.count; ++k) b += round16((size_t)N * t.a[k].bytes);
    return b + round16((size_t)N * extra_a) + round16((size_t)N * extra_b);
}
inline Staging staging_carve(const Table &t, int32_t N, uint8_t *arena)
{
    Staging st{};
    st.hdr = (EnvHeader *)arena;
    arena += round16((size_t)N * sizeof(EnvHeader));
    st.plan = arena;
    arena += round16((size_t)N);
    for (int k = 0; k < t.count; ++k) {
        st.a[k] = arena;
        arena += round16((size_t)N * t.a[k].bytes);
    }
    return st;
}

// two launches on one stream, the launch boundary between them the barrier: phase 1 (every valid entry: live -> live or staging; the plan bytes; ST_RESAMPLE
// in status[N + 1] for an invalid entry) and, unless the caller knows that nobody is staged, phase 2 (staging -> live)   (mv_resample.hip)
void launch_resample(const Table &t, const Staging &st, const int32_t *device_src_of, int32_t N, int32_t *status, bool phase2, hipStream_t stream);

}  // namespace fork
}  // namespace mv
