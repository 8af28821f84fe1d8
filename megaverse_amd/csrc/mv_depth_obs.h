// megaverse_amd/csrc/mv_depth_obs.h -- depth observations (mv_set_depth_obs, include/megaverse_hip.h): the record and its rule, stated once for the kernels
// that store it (mv_raster.hip: raster_depth_kernel) and for the host twin (mv_debug_depth_pack_host, mv_depth_obs.hip).
//
// The record: ONE value per pixel of a frame, a single plane [H][W] in the frame's own pixel order -- row 0 is the bottom row, as in the RGBA frame -- whatever
// the colour layout (mv_set_obs_layout) is.  The value is the ray parameter t of the pixel's nearest hit, the very float the shading works from.  Every ray has
// the camera-space direction dc = (x, y, -1) and every primitive frame keeps t, so t is the PLANAR camera-space depth -z_cam in world units, within
// [NEAR_Z, FAR_Z] = [0.01, 120].  A pixel whose ray hits nothing holds 0: hits are >= NEAR_Z > 0, so 0 is unambiguous in both formats.
//   DEPTH_F32: the bits of t.
//   DEPTH_F16: t rounded to nearest-even (__float2half_rn); 120 is far inside the half range and 0.01 far above its subnormals.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace mv {

enum : int { DEPTH_F32 = 0, DEPTH_F16 = 1 };

__host__ __device__ inline bool depth_format_known(int format) { return format == DEPTH_F32 || format == DEPTH_F16; }
__host__ __device__ inline size_t depth_value_bytes(int format) { return format == DEPTH_F16 ? 2u : 4u; }
// one frame's plane, the whole gym's entry
__host__ __device__ inline size_t depth_plane_bytes(int W, int H, int format) { return (size_t)W * H * depth_value_bytes(format); }

// the 32 bits of a DEPTH_F32 value
__host__ __device__ inline uint32_t depth_bits_f32(float t, bool hit)
{
    if (!hit) return 0u;
    uint32_t b;
    __builtin_memcpy(&b, &t, sizeof b);
    return b;
}

// the 16 bits of a DEPTH_F16 value
__host__ __device__ inline uint16_t depth_bits_f16(float t, bool hit)
{
    if (!hit) return (uint16_t)0;
    const __half h = __float2half_rn(t);
    uint16_t b;
    __builtin_memcpy(&b, &h, sizeof b);
    return b;
}

// a DEPTH_F16 value widened again (exact: every half is a float)
__host__ __device__ inline float depth_f16_to_f32(uint16_t b)
{
    __half h;
    __builtin_memcpy(&h, &b, sizeof b);
    return __half2float(h);
}

// n values -> out, as the kernels store them (hit[i] == 0: no surface)
inline void depth_pack_host(const float *t, const uint8_t *hit, int n, int format, void *out)
{
    for (int i = 0; i < n; ++i) {
        if (format == DEPTH_F16) reinterpret_cast<uint16_t *>(out)[i] = depth_bits_f16(t[i], hit[i] != 0);
        else reinterpret_cast<uint32_t *>(out)[i] = depth_bits_f32(t[i], hit[i] != 0);
    }
}

}  // namespace mv
