// megaverse_amd/csrc/mv_scan_obs.h -- scan observations (include/megaverse_hip.h: mv_set_scan_obs): the rule, stated once for the kernel that writes the record
// (mv_scan_obs.hip: scan_obs_kernel) and for the host twin the tests compare it with (mv_debug_scan_host).
//
// The record: per drawn FRAME (one agent's view) SCAN_OBS_PLANES = 3 planes of K int16, [N*A][3][K], K = beams: a fan of K beams over the frame's horizontal
// field of view, beam 0 leftmost.  No ray is cast: the fan is binned out of the depth and label planes the pass already wrote, as a depth-image-to-laser-scan
// node does it, so a scan sees what the agent's camera sees and nothing behind an occluder the frame does not show.  Every pixel (px, py) of the frame whose
// depth t (mv_depth_obs.h) is not 0 and whose class (mv_seg_obs.h) is not SEG_HUD is unprojected exactly as a map observation's (mv_map_obs.h, line by line as
// far as u, f and hgt):
//   pc  = (x(px) t, y(py) t, -t)                 the hit in camera space (map_ray_x / map_ray_y: the pass's own abscissae)
//   d   = c pc                                   c: the viewer's 3x3 basis of the frame's header (row-major, columns right / up / back)
//   R   = (c[0], c[3], c[6])                     the right axis.  The cameras have no roll, R.y = 0, so (R.x, R.z) is a unit vector of the ground plane and
//                                                (R.z, -R.x) the unit horizontal heading -- no trigonometry, no normalisation.  R.y is not read: were a header
//                                                to hold a rolled camera, (R.x, R.z) would be shorter than 1 and every range shorter by that factor; the beams
//                                                would not change (u / f is a ratio)
//   u   = d.x R.x + d.z R.z                      lateral        f = d.x R.z - d.z R.x    forward        hgt = d.y    height over the eye
//   kept iff f > 0 and h_lo <= hgt <= h_hi       the height band over the eye: it takes the floor and the ceiling out.  Compared as floats; a NaN is dropped
//   s   = u / f,  fb = floor(s bscale)           bscale = float(K / 2) / TAN_HALF_FOV, formed once on the host (scan_bscale): the beams are evenly spaced on
//                                                the image plane -- uniform in the TANGENT of the bearing -- and with a level camera and K == W beam i is column i
//   beam = (int)fb + K/2                         kept iff -K/2 <= fb < K/2, compared as floats before any conversion
//   r   = sqrt(u u + f f)                        the horizontal distance from the eye
//   rq  = clamp(floor(r * 64), 0, 32767)         in 1/64 world units (SCAN_RANGE_SCALE)
//   key = rq << 4 | (15 - cls)                   cls: the label plane's class (map_class_of)
// Per beam, over the pixels kept in it: ONE minimum over key (an empty beam: SCAN_EMPTY_KEY) and one sum, both independent of the order the pixels come in.
//   plane 0 range: key >> 4 of the least key, -1 where no pixel was kept;  plane 1 class: 15 - (key & 15) of it -- the class of the nearest pixel, among pixels
//   of equal rq the greatest class --, 0 where none;  plane 2 count: the pixels kept, saturated at 32767.
// Every product, sum, division and square root below is one fp32 operation in the order written (the library is built with -ffp-contract=off, as the other rule
// headers need it); the division and the square root are correctly rounded on both sides (hipcc's default for fp32 `/` and sqrtf, which map_ray_x relies on too).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mv_map_obs.h"

namespace mv {

enum : int { SCAN_OBS_PLANES = 3, SCAN_BEAMS_MIN = 8, SCAN_BEAMS_MAX = 256, SCAN_BEAMS_STEP = 8, SCAN_RANGE_SCALE = 64, SCAN_SATURATED = 32767 };
constexpr uint32_t SCAN_EMPTY_KEY = 0xFFFFFFFFu;
static_assert(SEG_NUM_CLASSES <= 16 && (SCAN_SATURATED << 4 | 15) < 0x7FFFFFFF, "a key of a kept pixel is never SCAN_EMPTY_KEY");

__host__ __device__ inline bool scan_beams_known(int beams) { return beams >= SCAN_BEAMS_MIN && beams <= SCAN_BEAMS_MAX && beams % SCAN_BEAMS_STEP == 0; }
__host__ __device__ inline size_t scan_frame_values(int beams) { return (size_t)SCAN_OBS_PLANES * beams; }
inline float scan_bscale(int beams) { return float(beams / 2) / TAN_HALF_FOV; }   // (host: formed once per attach / per debug call)

// THE RULE: one pixel -> its beam and key; false: the pixel enters no beam.  c: the basis, 9 floats.
__host__ __device__ inline bool scan_pixel(const float *c, float x, float y, float t, int cls, float bscale, int K, float h_lo, float h_hi, int &beam, uint32_t &key)
{
    if (t == 0.0f || cls == SEG_HUD) return false;
    const float pcx = x * t, pcy = y * t, pcz = -t;
    const float dx = (c[0] * pcx + c[1] * pcy) + c[2] * pcz;   // (mat_mul's order, mv_frame.h)
    const float dy = (c[3] * pcx + c[4] * pcy) + c[5] * pcz;
    const float dz = (c[6] * pcx + c[7] * pcy) + c[8] * pcz;
    const float u = dx * c[0] + dz * c[6], f = dx * c[6] - dz * c[0];
    if (!(f > 0.0f && dy >= h_lo && dy <= h_hi)) return false;   // (a NaN is dropped)
    const float s = u / f;
    const float fb = floorf(s * bscale), half = float(K / 2);
    if (!(fb >= -half && fb < half)) return false;   // (compared as floats: no conversion of a value no int holds)
    const float r = sqrtf(u * u + f * f);
    const float rq = fminf(fmaxf(floorf(r * float(SCAN_RANGE_SCALE)), 0.0f), float(SCAN_SATURATED));
    beam = (int)fb + K / 2;
    key = (uint32_t)(int)rq << 4 | (uint32_t)(15 - cls);
    return true;
}

// one beam's three values from its accumulated key and count: the int16s' bits, each in the low half of a word (the kernel packs them two to a register)
__host__ __device__ inline void scan_beam_bits(uint32_t key, uint32_t count, uint32_t &range, uint32_t &cls, uint32_t &n)
{
    range = count ? key >> 4 : 0xffffu;   // (-1: no pixel was kept)
    cls = count ? 15u - (key & 15u) : 0u;
    n = count < (uint32_t)SCAN_SATURATED ? count : (uint32_t)SCAN_SATURATED;
}

// one frame's [3][K] from its planes [h][w] and the 12 camera floats eye(3) c(9), on the host: the loops.  key, count: K words of scratch each
inline void scan_obs_host(const void *depth, int depth_format, const void *seg, int seg_format, int w, int h, const float *cam12, int K, float h_lo, float h_hi,
                          uint32_t *key, uint32_t *count, int16_t *out)
{
    const float bscale = scan_bscale(K);
    for (int i = 0; i < K; ++i) { key[i] = SCAN_EMPTY_KEY; count[i] = 0u; }
    for (int py = 0; py < h; ++py) {
        const float y = map_ray_y(py, h);
        for (int px = 0; px < w; ++px) {
            const size_t i = (size_t)py * w + px;
            int beam;
            uint32_t k;
            if (!scan_pixel(cam12 + 3, map_ray_x(px, w), y, map_depth_at(depth, depth_format, i), map_class_of(map_label_at(seg, seg_format, i), seg_format), bscale,
                            K, h_lo, h_hi, beam, k))
                continue;
            ++count[beam];
            key[beam] = k < key[beam] ? k : key[beam];
        }
    }
    for (int i = 0; i < K; ++i) {
        uint32_t v[SCAN_OBS_PLANES];
        scan_beam_bits(key[i], count[i], v[0], v[1], v[2]);
        for (int q = 0; q < SCAN_OBS_PLANES; ++q) out[q * K + i] = (int16_t)(uint16_t)v[q];
    }
}

}  // namespace mv
