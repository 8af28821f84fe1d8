// megaverse_amd/csrc/mv_draw_common.h -- what every device episode generator stands on (mv_collect_draw.h, mv_obstacles_draw.h, mv_hex_draw.h): where an
// env's generator stands (GenState), libstdc++'s random draws restated so that one GPU lane can run them, and the frame the draw kernels share -- the
// record's clear at the start, the episode's publication at the end.  The code is host code as well: the CPU tests run the generators without a GPU.
//
// The host generators (mv_gen_*.cpp) reach the reference's draws through libstdc++ (11.4 in this image): std::mt19937, uniform_int_distribution,
// generate_canonical and std::shuffle.  Those are third-party; their published algorithms are restated here:
//   * MT19937 (Matsumoto & Nishimura 1998), sequential form;
//   * uniform_int_distribution: Lemire's nearly-divisionless method on the 32-bit generator (bits/uniform_int_dist.h, _S_nd);
//   * std::shuffle: one draw for two swap positions while range^2 fits the generator's range (bits/stl_algo.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mv_gen.h"

namespace mv {
namespace draw {

#define MV_HD __host__ __device__ inline

// the capacity flags a generator raises, on the device as on the host (mv_gen.h)
enum : int { FLAG_SLABS = GEN_SLABS, FLAG_TERRAIN = GEN_TERRAIN, FLAG_OBJECTS = GEN_OBJECTS, FLAG_REWARDS = GEN_REWARDS, FLAG_COORDS = GEN_COORDS };

// where an env's generator stands (TowerGen's twin): the seed the NEXT episode's Env::reset re-seeds with, and the sequence number it will get
struct alignas(16) GenState {
    uint32_t seed;
    int32_t seed_is_env_seed;   // 1: `seed` is the Env::seed() value, the reset draws its seed from it first
    int32_t next_seq;
    int32_t flags;              // FLAG_* raised by this env's generator since the host last looked
};

// ---- MT19937, sequential -----------------------------------------------------------------------------------------------------------------
struct Mt {
    uint32_t *s;
    int idx;
};
MV_HD void mt_seed1(Mt &g, uint32_t seed)
{
    uint32_t x = seed;
    g.s[0] = x;
    for (int i = 1; i < 624; ++i) {
        x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
        g.s[i] = x;
    }
    g.idx = 624;
}
MV_HD uint32_t mt_next1(Mt &g)
{
    if (g.idx >= 624) {
        uint32_t *s = g.s;
        for (int k = 0; k < 624; ++k) {
            const uint32_t y = (s[k] & 0x80000000u) | (s[k == 623 ? 0 : k + 1] & 0x7fffffffu);
            s[k] = s[k < 227 ? k + 397 : k - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        g.idx = 0;
    }
    uint32_t y = g.s[g.idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
// unbiased integer in [0, range), range >= 1 (Lemire)
MV_HD uint32_t mt_below1(Mt &g, uint32_t range)
{
    uint64_t product = (uint64_t)mt_next1(g) * (uint64_t)range;
    uint32_t low = (uint32_t)product;
    if (low < range) {
        const uint32_t threshold = (0u - range) % range;
        while (low < threshold) {
            product = (uint64_t)mt_next1(g) * (uint64_t)range;
            low = (uint32_t)product;
        }
    }
    return (uint32_t)(product >> 32);
}
MV_HD int rand_range1(Mt &g, int lo, int hi) { return lo + (int)mt_below1(g, (uint32_t)(hi - lo)); }   // util.hpp:30-33
MV_HD float frand1(Mt &g)                                                                                 // util.hpp:46-49
{
    float ret = (float)mt_next1(g) / 4294967296.0f;
    if (ret >= 1.0f) ret = 0.99999994f;
    return ret;
}

// std::shuffle's walk, two swap positions per draw; `below(range)` draws, `swap(i, j)` exchanges
template <class Below, class Swap>
MV_HD void shuffle_walk(int n, Below below, Swap swap)
{
    if (n <= 0) return;
    int i = 1;
    if ((n % 2) == 0) {
        const int j = (int)below(2u);
        swap(i, j);
        ++i;
    }
    while (i < n) {
        const uint32_t r = (uint32_t)i + 1u;
        const uint32_t x = (uint32_t)below(r * (r + 1u));
        swap(i, (int)(x / (r + 1u)));
        ++i;
        swap(i, (int)(x % (r + 1u)));
        ++i;
    }
}

}  // namespace draw
}  // namespace mv

// ---- the draw kernels' shared frame (device code only) -------------------------------------------------------------------------------------
// One wavefront per episode: the wave finds its env's staging slot and GenState, clears the record (Collect's kernel writes every byte it publishes and does
// not), draws, and publishes: `seq` last, behind a release, so that whoever finds it set finds the whole episode.
#ifdef __HIPCC__
#include "mv_math.h"

namespace mv {
namespace draw {

// a ballot's run of ones from lane 0: how far a box grows when lane k tests the k-th cell / row / layer beyond it
__device__ __forceinline__ int trailing_ones(unsigned long long m) { return m == ~0ull ? 64 : __ffsll((long long)~m) - 1; }

// the record's `bytes` (a multiple of 16) zeroed by the wave's lanes: the zeros are in place before any lane writes a field over them
__device__ __forceinline__ void clear_record(void *out, size_t bytes, int lane)
{
    for (int i = lane; i < (int)(bytes / 16); i += 64) reinterpret_cast<uint4 *>(out)[i] = uint4{0u, 0u, 0u, 0u};
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    wave_sync();
}

// the episode is complete in its slot: its sequence number goes to *seq, the env's generator moves on to the next episode, the flags are reported
__device__ __forceinline__ void publish_episode(int32_t *seq, GenState *states, int env, GenState st, uint32_t nextSeed, int flags, int32_t *flag_word, int lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    wave_sync();
    if (lane == 0) {
        __hip_atomic_store(seq, st.next_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st.seed = nextSeed; st.seed_is_env_seed = 0; st.next_seq += 1; st.flags |= flags;
        states[env] = st;
        if (flags && flag_word) atomicOr(flag_word, flags);   // (a capacity of the episode record was hit: reported once by the next stepping call)
    }
}

}  // namespace draw
}  // namespace mv
#endif
