// megaverse_amd/csrc/mv_resample.hip -- env resampling (include/megaverse_hip.h: mv_resample_envs): the two kernels of the staged copy.  The rule of a
// resampling map, what decides where phase 1 writes and what phase 2 copies, the table of an env's episode state and the staging arena's layout are
// mv_fork.h's; the entry points stand beside the fork's in mv_fork.hip; DESIGN.md 3.8 has the hazard argument.
#include "mv_api_internal.h"

namespace mv {
namespace fork {

template <class T>
__device__ __forceinline__ void resample_copy_units(const T *__restrict__ src, T *__restrict__ dst, uint32_t n)
{
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) dst[i] = src[i];
}

typedef uint32_t Row __attribute__((ext_vector_type(4)));   // 16 bytes, read and written through global (not flat) addresses
typedef const Row __attribute__((address_space(1))) *GlobalSrc;
typedef Row __attribute__((address_space(1))) *GlobalDst;

// the array that holds row u of the row space: how many of the table's row offsets lie at or below it
__device__ __forceinline__ int array_of(const Table &t, uint32_t u)
{
    int k = 0;
    for (int j = 1; j < t.count; ++j) k += u >= t.first16[j] ? 1 : 0;
    return k;
}

// Both kernels move rows [lo, hi) of one env's row space from the addresses in `from` to those in `to` (LDS: where row 0 of the row SPACE would lie for
// array k), the first BATCH rows of every thread loaded before the first of them is stored (rows lo + q * THREADS + thread; a q whose rows all lie beyond hi
// is skipped by the whole workgroup).  One variable per row, not an array: hipcc merges an array of vectors into one wide value and then waits for each
// load where it is inserted.
#define MV_RESAMPLE_LOAD(q, from)                                                                     \
    Row v##q;                                                                                         \
    int a##q = 0;                                                                                     \
    if (lo + (uint32_t)(q) * THREADS < hi) {                                                          \
        const uint32_t u = lo + (uint32_t)(q) * THREADS + threadIdx.x;                                \
        a##q = array_of(t, u);                                                                        \
        if (u < hi) v##q = *(GlobalSrc)(from[a##q] + (uint64_t)u * 16u);                              \
    }
#define MV_RESAMPLE_STORE(q, to)                                                                      \
    {                                                                                                 \
        const uint32_t u = lo + (uint32_t)(q) * THREADS + threadIdx.x;                                \
        if (u < hi) *(GlobalDst)(to[a##q] + (uint64_t)u * 16u) = v##q;                                \
    }
#define MV_RESAMPLE_LOADS(from)                                                                                                                          \
    MV_RESAMPLE_LOAD(0, from) MV_RESAMPLE_LOAD(1, from) MV_RESAMPLE_LOAD(2, from) MV_RESAMPLE_LOAD(3, from) MV_RESAMPLE_LOAD(4, from) MV_RESAMPLE_LOAD(5, from)
#define MV_RESAMPLE_STORES(to)                                                                                                                           \
    MV_RESAMPLE_STORE(0, to) MV_RESAMPLE_STORE(1, to) MV_RESAMPLE_STORE(2, to) MV_RESAMPLE_STORE(3, to) MV_RESAMPLE_STORE(4, to) MV_RESAMPLE_STORE(5, to)
static_assert(BATCH == 6, "six rows per thread are written out above");

// Phase 1.  One workgroup per (env d, range r of RANGES), as in fork_kernel, and the same two dependent round trips: src_of[d]; then, together, the scan of
// the map for "is d somebody's source" and the first BATCH rows of env s (read before the entry is known to be valid: `from` is in range, and reading an env
// is harmless); then the stores -- to env d's live slices where nobody names d, to its slices of the staging arena where somebody does (phase1_target): the
// two address tables lie side by side in LDS and the workgroup picks one.  An entry that leaves its env alone exits after that one load; an entry out of
// range raises ST_RESAMPLE and stores no state.  Range 0 leaves the env's plan byte for phase 2, whatever the entry is.
__global__ __launch_bounds__(THREADS) void resample_gather_kernel(const Table t, const Staging st, const int32_t *__restrict__ src_of, int32_t N,
                                                                  int32_t *status)
{
    __shared__ uint64_t s_from[MAX_ARRAYS], s_to[2][MAX_ARRAYS];   // [0]: env d's live slices, [1]: its slices of the staging arena
    const int32_t d = (int32_t)(blockIdx.x / RANGES), r = (int32_t)(blockIdx.x % RANGES);
    const int32_t e = __builtin_amdgcn_readfirstlane(src_of[d]);
    if (leaves_alone(e, d)) {
        if (r == 0 && threadIdx.x == 0) st.plan[d] = (uint8_t)TO_NOWHERE;
        return;
    }
    const int32_t from = e >= 0 && e < N ? e : d;   // (an index out of range: nothing is read through it)
    if (threadIdx.x < MAX_ARRAYS) {
        const int k = (int)threadIdx.x;
        const uint64_t rows = (uint64_t)t.first16[k] * 16u, live0 = (uint64_t)(uintptr_t)t.a[k].base - rows;
        s_from[k] = live0 + (uint64_t)from * t.a[k].bytes;
        s_to[0][k] = live0 + (uint64_t)d * t.a[k].bytes;
        s_to[1][k] = (uint64_t)(uintptr_t)st.a[k] - rows + (uint64_t)d * t.a[k].bytes;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)((uint64_t)t.total16 * (uint32_t)r / RANGES), hi = (uint32_t)((uint64_t)t.total16 * (uint32_t)(r + 1) / RANGES);
    const bool hdrLane = r == 0 && threadIdx.x < 32 && !((IDENTITY_DWORDS >> threadIdx.x) & 1u);
    uint32_t hv = 0;
    if (hdrLane) hv = reinterpret_cast<const uint32_t *>(t.hdr + from)[threadIdx.x];
    MV_RESAMPLE_LOADS(s_from)
    const int32_t s = __builtin_amdgcn_readfirstlane(resample_source(src_of, N, d));   // (the same for every thread: it depends on d alone)
    const int named = __syncthreads_or(named_as_source(src_of, N, d, (int32_t)threadIdx.x, THREADS) ? 1 : 0);
    const int target = phase1_target(s, named != 0);
    if (r == 0 && threadIdx.x == 0) {
        st.plan[d] = (uint8_t)target;
        if (s == INVALID) atomicOr(status + N + 1, (int)ST_RESAMPLE);
    }
    if (target == TO_NOWHERE) return;
    const bool staged = target == TO_STAGING;
    const int w = staged ? 1 : 0;
    if (hdrLane) reinterpret_cast<uint32_t *>((staged ? st.hdr : t.hdr) + d)[threadIdx.x] = hv;
    MV_RESAMPLE_STORES(s_to[w])
    for (uint32_t u = lo + BATCH * THREADS + threadIdx.x; u < hi; u += THREADS) {   // (a larger state: the rest row by row)
        const int k = array_of(t, u);
        *(GlobalDst)(s_to[w][k] + (uint64_t)u * 16u) = *(GlobalSrc)(s_from[k] + (uint64_t)u * 16u);
    }
    if (r != 0) return;
    for (int k = 0; k < t.count; ++k) {   // arrays that are no 16-byte rows (the episode log's accumulators with an odd agent count): a few dwords or bytes
        const Array a = t.a[k];
        const uint8_t *src = a.base + (size_t)s * a.bytes;
        uint8_t *dst = (staged ? st.a[k] : a.base) + (size_t)d * a.bytes;
        if (a.unit == 4) resample_copy_units(reinterpret_cast<const uint32_t *>(src), reinterpret_cast<uint32_t *>(dst), a.bytes / 4);
        else if (a.unit == 1) resample_copy_units(src, dst, a.bytes);
    }
}

// Phase 2, behind the launch boundary: every env whose plan byte says so takes slot d of the staging arena into its live slices -- a plain per-env copy with
// the same shape; every other workgroup exits after one byte.  Slot d was written by env d's workgroups of phase 1 alone, and nothing else touches env d.
__global__ __launch_bounds__(THREADS) void resample_commit_kernel(const Table t, const Staging st)
{
    __shared__ uint64_t s_stage[MAX_ARRAYS], s_live[MAX_ARRAYS];
    const int32_t d = (int32_t)(blockIdx.x / RANGES), r = (int32_t)(blockIdx.x % RANGES);
    const int target = __builtin_amdgcn_readfirstlane((int)st.plan[d]);
    if (!phase2_copies(target)) return;
    if (threadIdx.x < MAX_ARRAYS) {
        const int k = (int)threadIdx.x;
        const uint64_t rows = (uint64_t)t.first16[k] * 16u;
        s_stage[k] = (uint64_t)(uintptr_t)st.a[k] - rows + (uint64_t)d * t.a[k].bytes;
        s_live[k] = (uint64_t)(uintptr_t)t.a[k].base - rows + (uint64_t)d * t.a[k].bytes;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)((uint64_t)t.total16 * (uint32_t)r / RANGES), hi = (uint32_t)((uint64_t)t.total16 * (uint32_t)(r + 1) / RANGES);
    const bool hdrLane = r == 0 && threadIdx.x < 32 && !((IDENTITY_DWORDS >> threadIdx.x) & 1u);
    uint32_t hv = 0;
    if (hdrLane) hv = reinterpret_cast<const uint32_t *>(st.hdr + d)[threadIdx.x];
    MV_RESAMPLE_LOADS(s_stage)
    if (hdrLane) reinterpret_cast<uint32_t *>(t.hdr + d)[threadIdx.x] = hv;
    MV_RESAMPLE_STORES(s_live)
    for (uint32_t u = lo + BATCH * THREADS + threadIdx.x; u < hi; u += THREADS) {
        const int k = array_of(t, u);
        *(GlobalDst)(s_live[k] + (uint64_t)u * 16u) = *(GlobalSrc)(s_stage[k] + (uint64_t)u * 16u);
    }
    if (r != 0) return;
    for (int k = 0; k < t.count; ++k) {
        const Array a = t.a[k];
        const uint8_t *src = st.a[k] + (size_t)d * a.bytes;
        uint8_t *dst = a.base + (size_t)d * a.bytes;
        if (a.unit == 4) resample_copy_units(reinterpret_cast<const uint32_t *>(src), reinterpret_cast<uint32_t *>(dst), a.bytes / 4);
        else if (a.unit == 1) resample_copy_units(src, dst, a.bytes);
    }
}
#undef MV_RESAMPLE_LOAD
#undef MV_RESAMPLE_STORE
#undef MV_RESAMPLE_LOADS
#undef MV_RESAMPLE_STORES

void launch_resample(const Table &t, const Staging &st, const int32_t *device_src_of, int32_t N, int32_t *status, bool phase2, hipStream_t stream)
{
    hipLaunchKernelGGL(resample_gather_kernel, dim3((unsigned)N * RANGES), dim3(THREADS), 0, stream, t, st, device_src_of, N, status);
    if (phase2) hipLaunchKernelGGL(resample_commit_kernel, dim3((unsigned)N * RANGES), dim3(THREADS), 0, stream, t, st);
}

}  // namespace fork
}  // namespace mv
