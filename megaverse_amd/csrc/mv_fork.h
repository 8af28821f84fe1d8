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

}  // namespace fork
}  // namespace mv
