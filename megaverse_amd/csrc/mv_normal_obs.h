// megaverse_amd/csrc/mv_normal_obs.h -- normal observations (mv_set_normal_obs, include/megaverse_hip.h): the record and its rule, stated once for the kernels
// that store it (mv_raster.hip: raster_normal_kernel) and for the host twin (mv_debug_normal_pack_host, mv_obs_planes.hip).
//
// The record: ONE value of four components per pixel of a frame, a plane [H][W][4] in the frame's own pixel order -- row 0 is the bottom row, as in the RGBA
// frame -- whatever the colour layout (mv_set_obs_layout) is.  The value is the unit outward normal of the surface the pixel shows, in the VIEWER's camera frame
// (x right, y up, z back: the columns of the camera matrix) -- the very vector N the exact pass shades with, the same floats: a box in the world frame gives
// sgn * row `axis` of the camera matrix, a box in the viewer's own frame +-e_axis, a box in another frame C^T F n; a capsule, cone or scaled shape its kept hit
// normal, carried the same way.  Only entry faces are hit, so the normal faces the viewer.  The 4th component is 1 where there is a surface; a pixel whose ray
// hits nothing is four zeros, exactly where the depth plane holds 0 and the label plane holds 0.
//   NORMAL_F16:    four halves (x, y, z, 1), each component rounded to nearest-even (__float2half_rn): 8 bytes.
//   NORMAL_SNORM8: four signed bytes (q(x), q(y), q(z), 127), q(v) = (int)(127 clamp(v, -1, 1) + (v >= 0 ? 0.5f : -0.5f)): 4 bytes.  The product and the sum
//                  are two single-precision roundings (the library is built with -ffp-contract=off); a byte b reads back as b / 127.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace mv {

enum : int { NORMAL_F16 = 0, NORMAL_SNORM8 = 1 };

__host__ __device__ inline bool normal_format_known(int format) { return format == NORMAL_F16 || format == NORMAL_SNORM8; }
__host__ __device__ inline size_t normal_value_bytes(int format) { return format == NORMAL_SNORM8 ? 4u : 8u; }   // one pixel: four components
// one frame's plane, the whole gym's entry
__host__ __device__ inline size_t normal_plane_bytes(int W, int H, int format) { return (size_t)W * H * normal_value_bytes(format); }

__host__ __device__ inline uint32_t normal_half_bits(float v)
{
    const __half h = __float2half_rn(v);
    uint16_t b;
    __builtin_memcpy(&b, &h, sizeof b);
    return b;
}

// the 64 bits of a NORMAL_F16 value: x in the lowest half, then y, z, and 1.0 (0x3c00)
__host__ __device__ inline uint64_t normal_bits_f16(float x, float y, float z, bool hit)
{
    if (!hit) return 0ull;
    const uint32_t lo = normal_half_bits(x) | (normal_half_bits(y) << 16), hi = normal_half_bits(z) | (0x3c00u << 16);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// q of the rule: one component as a signed byte (NaN: 0)
__host__ __device__ inline int normal_snorm8(float v)
{
    const float c = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
    if (!(c == c)) return 0;
    return (int)(127.0f * c + (v >= 0.0f ? 0.5f : -0.5f));
}

// the 32 bits of a NORMAL_SNORM8 value: q(x) in the lowest byte, then q(y), q(z), and 127
__host__ __device__ inline uint32_t normal_bits_snorm8(float x, float y, float z, bool hit)
{
    if (!hit) return 0u;
    return ((uint32_t)normal_snorm8(x) & 255u) | (((uint32_t)normal_snorm8(y) & 255u) << 8) | (((uint32_t)normal_snorm8(z) & 255u) << 16) | (127u << 24);
}

// the values widened again: a half (exact: every half is a float), a signed byte as b / 127
__host__ __device__ inline float normal_f16_to_f32(uint16_t b)
{
    __half h;
    __builtin_memcpy(&h, &b, sizeof b);
    return __half2float(h);
}
__host__ __device__ inline float normal_snorm8_to_f32(int8_t b) { return (float)b / 127.0f; }

// n values (xyz[3 i ..]) -> out, as the kernels store them (hit[i] == 0: no surface)
inline void normal_pack_host(const float *xyz, const uint8_t *hit, int n, int format, void *out)
{
    for (int i = 0; i < n; ++i) {
        if (format == NORMAL_SNORM8) reinterpret_cast<uint32_t *>(out)[i] = normal_bits_snorm8(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], hit[i] != 0);
        else {
            const uint64_t b = normal_bits_f16(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], hit[i] != 0);
            __builtin_memcpy(reinterpret_cast<uint8_t *>(out) + 8 * (size_t)i, &b, sizeof b);
        }
    }
}

// one stored value of either format -> four floats (mv_get_normal_observation)
inline void normal_widen_host(const uint8_t *value, int format, float *out4)
{
    if (format == NORMAL_SNORM8)
        for (int c = 0; c < 4; ++c) out4[c] = normal_snorm8_to_f32((int8_t)value[c]);
    else
        for (int c = 0; c < 4; ++c) { uint16_t b; __builtin_memcpy(&b, value + 2 * c, 2); out4[c] = normal_f16_to_f32(b); }
}

}  // namespace mv
