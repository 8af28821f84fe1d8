// megaverse_amd/csrc/mv_debug_physics.hip -- test hooks of the C ABI (include/megaverse_hip.h: mv_debug_sweep, mv_debug_recover,
// mv_debug_player_step): the controller's sweep, push-out and step of mv_physics.h on caller-given colliders and queries, without a gym.
// The kernels only load the records and call the templates the step kernels call, in the instantiations the step kernels use; no
// arithmetic of mv_physics.h is restated here.  One full 64-lane wave per record (the DPP reductions and ballots of a sweep need every
// lane): blocks of 4 waves, no lane returns early, a wave past the last record repeats it and stores nothing.  Used by tests/ only.
#include "mv_api_internal.h"
#include "mv_physics.h"

namespace {

#pragma pack(push, 4)
struct DbgCol { int32_t kind; float lo[3], hi[3]; };
struct DbgQuery { float from[3], to[3], up[3], min_slope_dot; };
struct DbgSweepOut { int32_t hit; float fraction, normal[3]; };
struct DbgRecoverOut { int32_t pushes; float pos[5][3]; };
struct DbgAgent { float pos[3], hvx, hvz, vvel, voffset, step_offset, jump_speed; int32_t was_jumping; float reach2; };
#pragma pack(pop)

constexpr int DBG_WAVES = 4;   // waves (records) per block

// lane l holds slots l + 64 k, as the tick headers load them; slots from n_cols on are empty
template <int NC>
__device__ __forceinline__ void debug_load_cols(const DbgCol *cols, int n_cols, Col (&col)[NC])
{
    const int lane = lane_id();
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int slot = lane + 64 * k;
        col[k].kind = 0; col[k].lo = v3(0, 0, 0); col[k].hi = v3(0, 0, 0);
        if (slot < n_cols) {
            const DbgCol c = cols[slot];
            col[k].kind = c.kind; col[k].lo = v3(c.lo[0], c.lo[1], c.lo[2]); col[k].hi = v3(c.hi[0], c.hi[1], c.hi[2]);
        }
    }
}

template <int NC, bool OBB, bool BALL>
__global__ __launch_bounds__(64 * DBG_WAVES) void debug_sweep_kernel(const DbgCol *cols, int n_cols, const DbgQuery *queries, int n, DbgSweepOut *out)
{
    const int idx = blockIdx.x * DBG_WAVES + (int)(threadIdx.x >> 6);
    Col col[NC];
    debug_load_cols<NC>(cols, n_cols, col);
    const DbgQuery q = queries[min(idx, n - 1)];
    float f = 1.0f;
    V3 nrm = v3(0, 0, 0);
    const bool hit = sweep<NC, OBB, BALL>(col, v3(q.from[0], q.from[1], q.from[2]), v3(q.to[0], q.to[1], q.to[2]), v3(q.up[0], q.up[1], q.up[2]),
                                          q.min_slope_dot, f, nrm);
    if (idx < n && lane_id() == 0) {
        DbgSweepOut o;
        o.hit = hit ? 1 : 0; o.fraction = f; o.normal[0] = nrm.x; o.normal[1] = nrm.y; o.normal[2] = nrm.z;
        out[idx] = o;
    }
}

template <int NC, bool OBB, bool BALL>
__global__ __launch_bounds__(64 * DBG_WAVES) void debug_recover_kernel(const DbgCol *cols, int n_cols, const float *positions, int n, DbgRecoverOut *out)
{
    const int idx = blockIdx.x * DBG_WAVES + (int)(threadIdx.x >> 6);
    Col col[NC];
    debug_load_cols<NC>(cols, n_cols, col);
    const float *p = positions + 3 * (size_t)min(idx, n - 1);
    V3 pos = v3(p[0], p[1], p[2]);
    // `seen` is told the position after every call, the one that found nothing to push included: a call pushed when it moved the capsule (a push is
    // longer than MAX_PEN_DEPTH: it changes the bits of any coordinate a world has)
    DbgRecoverOut o;
    int calls = 0, pushes = 0;
    V3 last = pos;
    recover_up_to_5<NC, OBB, BALL>(col, pos, [&](V3 now) {
        if (calls < 5) { o.pos[calls][0] = now.x; o.pos[calls][1] = now.y; o.pos[calls][2] = now.z; }
        if (__float_as_uint(now.x) != __float_as_uint(last.x) || __float_as_uint(now.y) != __float_as_uint(last.y) ||
            __float_as_uint(now.z) != __float_as_uint(last.z))
            ++pushes;
        last = now;
        ++calls;
    });
    for (int k = calls; k < 5; ++k) { o.pos[k][0] = pos.x; o.pos[k][1] = pos.y; o.pos[k][2] = pos.z; }
    o.pushes = pushes;
    if (idx < n && lane_id() == 0) out[idx] = o;
}

template <int NC, bool OBB, bool BALL>
__global__ __launch_bounds__(64 * DBG_WAVES) void debug_player_step_kernel(const DbgCol *cols, int n_cols, const DbgAgent *in, int n, DbgAgent *out)
{
    const int idx = blockIdx.x * DBG_WAVES + (int)(threadIdx.x >> 6);
    Col col[NC];
    debug_load_cols<NC>(cols, n_cols, col);
    const DbgAgent r = in[min(idx, n - 1)];
    AgentState a = {};
    a.pos[0] = r.pos[0]; a.pos[1] = r.pos[1]; a.pos[2] = r.pos[2];
    a.hvx = r.hvx; a.hvz = r.hvz; a.vvel = r.vvel; a.voffset = r.voffset; a.step_offset = r.step_offset; a.jump_speed = r.jump_speed;
    a.was_jumping = r.was_jumping;
    float reach2 = 0.0f;
    player_step<NC, OBB, BALL>(a, col, DT, &reach2);
    if (idx < n && lane_id() == 0) {
        DbgAgent o;
        o.pos[0] = a.pos[0]; o.pos[1] = a.pos[1]; o.pos[2] = a.pos[2];
        o.hvx = a.hvx; o.hvz = a.hvz; o.vvel = a.vvel; o.voffset = a.voffset; o.step_offset = a.step_offset; o.jump_speed = a.jump_speed;
        o.was_jumping = a.was_jumping; o.reach2 = reach2;
        out[idx] = o;
    }
}

struct DevBuf {   // a device allocation that ends with its scope
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct Variant { int nc; bool obb, ball; };
constexpr Variant VARIANTS[5] = {{1, false, false}, {2, false, false}, {4, false, false}, {1, true, false}, {1, false, true}};

// the colliders a variant's step kernels can hold: its kinds and at most 64 NC of them
int check_cols(const char *who, int variant, const void *cols, int n_cols)
{
    if (variant < 0 || variant > 4) return fail(std::string(who) + ": variant 0..4 (MV_PHYS_*)");
    if (n_cols < 0 || n_cols > 64 * VARIANTS[variant].nc || (n_cols && !cols)) return fail(std::string(who) + ": n_cols within 0..64 NC of the variant");
    const DbgCol *c = static_cast<const DbgCol *>(cols);
    for (int i = 0; i < n_cols; ++i) {
        const int k = c[i].kind;
        const bool ok = k == 0 || k == 1 || k == 2 || (VARIANTS[variant].obb && k >= 3 && k <= 5) || (VARIANTS[variant].ball && k == COL_BALL);
        if (!ok) return fail(std::string(who) + ": collider kind " + std::to_string(k) + " is not one this variant's kernels hold");
    }
    return 0;
}

// allocate, copy in, launch once, synchronise, copy back, free (mv_debug_math's shape)
template <class Launch>
int run_records(int device, const void *cols, int n_cols, const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch)
{
    HIP_TRY(hipSetDevice(device));
    DevBuf dcols, din, dout;
    HIP_TRY(hipMalloc(&dcols.p, std::max<size_t>((size_t)n_cols * sizeof(DbgCol), sizeof(DbgCol))));
    HIP_TRY(hipMalloc(&din.p, in_bytes));
    HIP_TRY(hipMalloc(&dout.p, out_bytes));
    if (n_cols) HIP_TRY(hipMemcpy(dcols.p, cols, (size_t)n_cols * sizeof(DbgCol), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dout.p, 0, out_bytes));
    launch(static_cast<const DbgCol *>(dcols.p), din.p, dout.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    return 0;
}

#define MV_DBG_LAUNCH(KERNEL, IN_T, OUT_T)                                                                                                  \
    [&](const DbgCol *dc, const void *di, void *dq) {                                                                                       \
        const dim3 grid((unsigned)((n + DBG_WAVES - 1) / DBG_WAVES)), block(64 * DBG_WAVES);                                                 \
        const IN_T *i_ = static_cast<const IN_T *>(di);                                                                                      \
        OUT_T *o_ = static_cast<OUT_T *>(dq);                                                                                                \
        switch (variant) {                                                                                                                   \
            case 0: hipLaunchKernelGGL((KERNEL<1, false, false>), grid, block, 0, nullptr, dc, n_cols, i_, n, o_); break;                    \
            case 1: hipLaunchKernelGGL((KERNEL<2, false, false>), grid, block, 0, nullptr, dc, n_cols, i_, n, o_); break;                    \
            case 2: hipLaunchKernelGGL((KERNEL<4, false, false>), grid, block, 0, nullptr, dc, n_cols, i_, n, o_); break;                    \
            case 3: hipLaunchKernelGGL((KERNEL<1, true, false>), grid, block, 0, nullptr, dc, n_cols, i_, n, o_); break;                     \
            default: hipLaunchKernelGGL((KERNEL<1, false, true>), grid, block, 0, nullptr, dc, n_cols, i_, n, o_); break;                    \
        }                                                                                                                                    \
    }

}  // namespace

extern "C" {

int mv_debug_sweep(int32_t device, int32_t variant, const void *cols, int32_t n_cols, const void *queries, int32_t n_queries, void *out)
{
    if (check_cols("mv_debug_sweep", variant, cols, n_cols)) return -1;
    if (n_queries < 0 || n_queries > (1 << 20) || (n_queries && (!queries || !out))) return fail("mv_debug_sweep: bad arguments (at most 2^20 queries)");
    if (n_queries == 0) return 0;
    const int n = n_queries;
    return run_records(device, cols, n_cols, queries, (size_t)n * sizeof(DbgQuery), out, (size_t)n * sizeof(DbgSweepOut),
                       MV_DBG_LAUNCH(debug_sweep_kernel, DbgQuery, DbgSweepOut));
}

int mv_debug_recover(int32_t device, int32_t variant, const void *cols, int32_t n_cols, const float *positions, int32_t n, void *out)
{
    if (check_cols("mv_debug_recover", variant, cols, n_cols)) return -1;
    if (n < 0 || n > (1 << 20) || (n && (!positions || !out))) return fail("mv_debug_recover: bad arguments (at most 2^20 positions)");
    if (n == 0) return 0;
    return run_records(device, cols, n_cols, positions, (size_t)n * 3 * sizeof(float), out, (size_t)n * sizeof(DbgRecoverOut),
                       MV_DBG_LAUNCH(debug_recover_kernel, float, DbgRecoverOut));
}

int mv_debug_player_step(int32_t device, int32_t variant, const void *cols, int32_t n_cols, const void *agents_in, int32_t n, void *agents_out)
{
    if (check_cols("mv_debug_player_step", variant, cols, n_cols)) return -1;
    if (n < 0 || n > (1 << 20) || (n && (!agents_in || !agents_out))) return fail("mv_debug_player_step: bad arguments (at most 2^20 records)");
    if (n == 0) return 0;
    return run_records(device, cols, n_cols, agents_in, (size_t)n * sizeof(DbgAgent), agents_out, (size_t)n * sizeof(DbgAgent),
                       MV_DBG_LAUNCH(debug_player_step_kernel, DbgAgent, DbgAgent));
}

}  // extern "C"
