// megaverse_amd/csrc/mv_raster.h -- host interface of the observation pass (mv_raster.hip)
#pragma once
#include <hip/hip_runtime.h>

#include "mv_overview.h"
#include "mv_types.h"

namespace mv {

// frame setup (+ frame sort, exact mode) + raster of every agent's W x H observation into `obs` on `stream`; `between` (optional) is
// recorded between the setup/sort kernels and the raster kernel; -1 if W/H are too large.  fast = 1: raster_fast_kernel (hardware
// reciprocals, frames looked up from the cost bins in its prologue; pixels within the tolerance DESIGN.md states), 0: the bit-exact
// raster_kernel behind frame_order_kernel.  setup_done = 1: the frame lists were built by the step kernel (mv_frame.h).
// publish (fast kernel only): the step's staged rewards / dones / true objectives (gv.rewards ...) are copied into these public arrays by the
// first workgroups of the raster launch -- ordered, on `stream`, with the observations (pipelined steps, mv_api.hip)
struct PublishTo { float *rewards; uint8_t *done; float *true_objective; };
// done: an event that completes when the pass does.  The fast kernels carry it as the completion signal of their own dispatch packet
// (hipExtLaunchKernelGGL's stop event) -- a separate hipEventRecord is one more packet the queue works off between two passes, ~5 us.
// The planes of one tick's entry beside its colours, each null where its stream is not attached: the gym's depth entry [N*A][H][W] in depth_format
// (mv_set_depth_obs; mv_depth_obs.h), its label entry [N*A][H][W] in seg_format (mv_set_seg_obs; mv_seg_obs.h), its normal entry [N*A][H][W][4] in
// normal_format (mv_set_normal_obs; mv_normal_obs.h).
struct PlaneOuts {
    void *depth = nullptr; int depth_format = 0;
    void *seg = nullptr; int seg_format = 0;
    void *normal = nullptr; int normal_format = 0;
    bool any() const { return depth || seg || normal; }
};
// planes (fast = 0 only; null or all null: none): the exact pass becomes the instantiation that stores every given plane beside the colours: one trace, every
// output, no further launch.  A fast pass stores no plane: its kernels stay what they are, and the caller follows it with launch_raster_planes.
int launch_raster(const GymView &gv, uint32_t *obs, int W, int H, hipStream_t stream, hipEvent_t between = nullptr, int fast = 1, int setup_done = 0,
                  const PublishTo *publish = nullptr, hipEvent_t done = nullptr, const PlaneOuts *planes = nullptr);

// The planes of every frame of gv -- its lists already set up -- with ONE launch of the exact trace without the shading, whichever of the seven non-empty sets
// of {depth, labels, normals} po names: never two.  Depth alone, labels alone and depth + labels: the kernels they always had; a set with normals: the
// normal kernel, which takes the other two by their pointers.  Frames in identity order; an undrawn or still frame (mv_frame.h: frame_skip) writes nothing.
// -1: W / H too large, no plane, an unknown format.
int launch_raster_planes(const GymView &gv, const PlaneOuts &po, int W, int H, hipStream_t stream);

// Overview cameras (mv_overview.h): the frame setup of every env from its camera ov.cams[env], the frame order from the overview's own cost bins and the exact
// pass into obs [N][H][W] RGBA, three launches on `stream`.  gv: a view whose vis_prims / vis_rects / vis_count / vis_stride / lpt_bucket / lpt_order / vis_hdr
// are the overview's own arrays -- nothing of a stepping call's passes is read or written.  -1: bad size.
// cost_order = false: no frame-order launch -- gv.lpt_order already holds the order to draw in (the identity: MV_OVERVIEW_ORDER=0, a measurement's switch).
int launch_overview(const GymView &gv, const OverviewArgs &ov, uint32_t *obs, int W, int H, hipStream_t stream, bool cost_order = true);

// the fast observation pass of n gyms of one job (frame lists already built by their step kernels) with at most two launches; publish: n
// entries or null; -1 if W / H / n are too large
int launch_raster_union(const GymView *views, uint32_t *const *obs, const PublishTo *publish, int n,
                        int W, int H, hipStream_t stream, hipEvent_t between = nullptr,
                        hipEvent_t done = nullptr);

// the fast observation passes of k ticks of ONE gym (a batched call; views[j] / obs[j] / publish[j] of tick j, the observation slabs distinct) with one
// launch: the next tick's expensive frames run in the tail of the previous tick's pass; 0: launched, 1: not applicable (the caller launches tick by tick)
int launch_raster_batch(const GymView *views, uint32_t *const *obs, const PublishTo *publish, int k,
                        int W, int H, hipStream_t stream, hipEvent_t done = nullptr);

// the fast observation passes of k ticks of n gyms of one job (a batched group call; views / obs / publish tick-major: [j * n + i]) with ONE launch.
// raster_union_batch_applicable: decided before the step launch (its frame setups leave the clearing of the cost histograms to the passes);
// launch_raster_union_batch: 0 launched, 1 not applicable, -1 / -2 bad sizes / views that are not one hand-over slot apart per tick
bool raster_union_batch_applicable(int k, int n, int W, int H);
int launch_raster_union_batch(const GymView *views, uint32_t *const *obs, const PublishTo *publish, int k,
                              int n, int W, int H, hipStream_t stream, hipEvent_t done = nullptr);

// The frame-order tables of the k <= MAX_STEP_TICKS ticks of a batched one-gym call, on the stream of its step launches and directly behind them: one small
// kernel writes order[position] = frame into every tick's GymView::lpt_forder (not null) and zeroes the tick's cost histogram; the views are marked
// (lpt_forder_on) so that the passes launched from them read the table.  done: completes with the kernel, carried by its dispatch packet.
void launch_frame_order_ticks(GymView *views, int k, hipStream_t stream, hipEvent_t done = nullptr);

// What the fast kernels need of the observation size alone, computed ONCE on the host -- with the single-precision expressions the kernels used to
// evaluate in every workgroup, operation for operation (IEEE division is correctly rounded on both sides, the host build contracts nothing): the same bits
// (tests/test_launch_constants.py).
// sx, ox, sy, oy: a ray's camera-space abscissae as affine functions of the pixel, dcx = sx i + ox, dcy = sy j + oy (classify_tiles);
// tiles_x_inv: raster_div_magic(tilesX), the reciprocal of tile / tilesX
struct RasterConsts { float sx, ox, sy, oy; uint32_t tiles_x_inv; };
RasterConsts raster_launch_consts(int W, int H);
// dcx[W] then dcy[H]: the abscissae themselves, as the prologue's tables hold them (GymView::ray_tab)
void raster_ray_table(int W, int H, float *out);
// n / d as a multiplication: m = ceil(2^32 / d), n / d == (n m) >> 32 while n d < 2^32.  d = 1 has no such m in 32 bits: 0 stands for it (n / 1 = n).
inline uint32_t raster_div_magic(uint32_t d) { return d <= 1u ? 0u : (uint32_t)((0x100000000ull + d - 1u) / d); }
inline uint32_t raster_div_by_magic(uint32_t n, uint32_t m) { return m ? (uint32_t)(((uint64_t)n * m) >> 32) : n; }

}  // namespace mv
