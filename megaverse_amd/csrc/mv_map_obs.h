// megaverse_amd/csrc/mv_map_obs.h -- map observations (include/megaverse_hip.h: mv_set_map_obs): the rule, stated once for the kernel that writes the record
// (mv_map_obs.hip: map_obs_kernel) and for the host twin the tests compare it with (mv_debug_map_host).
//
// The record: per drawn FRAME (one agent's view) MAP_OBS_PLANES = 3 planes of M x M int16, [N*A][3][M][M], M = cells: an egocentric top-down grid of square cells
// of cell_size world units.  The eye sits at the middle of the grid's bottom edge: row 0 is the nearest row, column M/2 begins at the eye's lateral 0, rows
// grow along the viewer's horizontal heading and columns along its right axis.  Every pixel (px, py) of the frame whose depth t (mv_depth_obs.h) is not 0 and
// whose class (mv_seg_obs.h) is not SEG_HUD is unprojected with the camera the pass drew it with and dropped into the cell below it:
//   pc  = (x(px) t, y(py) t, -t)                 the hit in camera space: the ray's direction is (x, y, -1) and t its parameter (mv_depth_obs.h); x and y are
//                                                the pass's own abscissae (mv_raster.hip: raster_ray_table's expressions, map_ray_x / map_ray_y below)
//   d   = c pc                                   c: the viewer's 3x3 basis of the frame's header (mv_frame.h: FH_CAM + FH_CAM_STRIDE * agent, floats 3 .. 11;
//                                                row-major, columns right / up / back): the hit relative to the eye in world axes
//   R   = (c[0], c[3], c[6])                     the right axis.  The cameras have no roll, R.y = 0, so (R.x, R.z) is a unit vector of the ground plane and
//                                                (R.z, -R.x) the unit horizontal heading -- no trigonometry, no normalisation.  R.y is not read: were a header
//                                                to hold a rolled camera, (R.x, R.z) would be shorter than 1 and the grid's cells larger by that factor; nothing
//                                                else would change
//   u   = d.x R.x + d.z R.z                      lateral        f = d.x R.z - d.z R.x    forward        hgt = d.y    height over the eye
//   col = floor(u inv) + M/2,  row = floor(f inv),  inv = 1.0f / cell_size formed once on the host; a pixel outside [0, M) x [0, M) is dropped
//   hq  = clamp(floor(hgt * 32), -32767, 32767)  in 1/32 world units (MAP_HEIGHT_SCALE)
//   cls = the label plane's byte (its low four bits: the classes are < SEG_NUM_CLASSES = 15), or word >> 12 of the instance format
// Per cell, over the pixels that fall in it:  plane 0 count, saturated at 32767;  plane 1 height, the greatest hq;  plane 2 class, the cls of a pixel with that
// greatest hq, among equals the greatest cls.  That is ONE maximum over key = (hq + 32768) << 4 | cls (>= 16 for every pixel: 0 says "nobody") and one sum,
// both independent of the order the pixels come in.  A cell no pixel fell in is three zeros.
// Every product and sum below is one fp32 operation in the order written (the library is built with -ffp-contract=off, as the other rule headers need it).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mv_depth_obs.h"
#include "mv_frame.h"
#include "mv_seg_obs.h"

namespace mv {

enum : int { MAP_OBS_PLANES = 3, MAP_CELLS_MIN = 8, MAP_CELLS_MAX = 64, MAP_CELLS_STEP = 8, MAP_HEIGHT_SCALE = 32, MAP_SATURATED = 32767, MAP_CAM_FLOATS = 12 };
static_assert(SEG_NUM_CLASSES <= 16 && SEG_INSTANCE_BITS == 12, "a class fits the key's low four bits");

__host__ __device__ inline bool map_cells_known(int cells) { return cells >= MAP_CELLS_MIN && cells <= MAP_CELLS_MAX && cells % MAP_CELLS_STEP == 0; }
__host__ __device__ inline size_t map_frame_values(int cells) { return (size_t)MAP_OBS_PLANES * cells * cells; }

// the pass's abscissae (mv_raster.hip: raster_ray_table, fast_prologue, raster_body -- the same expressions, the same bits)
__host__ __device__ inline float map_ray_x(int px, int W) { return (((float(px) + 0.5f) / float(W)) * 2.0f - 1.0f) * TAN_HALF_FOV; }
__host__ __device__ inline float map_ray_y(int py, int H) { return (((float(py) + 0.5f) / float(H)) * 2.0f - 1.0f) * TAN_HALF_FOV_Y; }

// a label value's class: fmt is uniform wherever this is called
__host__ __device__ inline int map_class_of(uint32_t label, int seg_format) { return seg_format == SEG_INSTANCE_U16 ? (int)(label >> SEG_INSTANCE_BITS) & 15 : (int)(label & 15u); }

// THE RULE: one pixel -> its cell (row * M + col) and key; false: the pixel enters no cell.  c: the basis, 9 floats.
__host__ __device__ inline bool map_pixel(const float *c, float x, float y, float t, int cls, float inv, int M, int &cell, uint32_t &key)
{
    if (t == 0.0f || cls == SEG_HUD) return false;
    const float pcx = x * t, pcy = y * t, pcz = -t;
    const float dx = (c[0] * pcx + c[1] * pcy) + c[2] * pcz;   // (mat_mul's order, mv_frame.h)
    const float dy = (c[3] * pcx + c[4] * pcy) + c[5] * pcz;
    const float dz = (c[6] * pcx + c[7] * pcy) + c[8] * pcz;
    const float u = dx * c[0] + dz * c[6], f = dx * c[6] - dz * c[0];
    const float fc = floorf(u * inv), fr = floorf(f * inv);
    const float half = float(M / 2);
    if (!(fc >= -half && fc < half && fr >= 0.0f && fr < float(M))) return false;   // (compared as floats: no conversion of a value no int holds; a NaN is dropped)
    const float fh = fminf(fmaxf(floorf(dy * float(MAP_HEIGHT_SCALE)), -32767.0f), 32767.0f);
    cell = (int)fr * M + ((int)fc + M / 2);
    key = (uint32_t)((int)fh + 32768) << 4 | (uint32_t)cls;
    return true;
}

// one cell's three values from its accumulated key and count: the int16s' bits, each in the low half of a word (the kernel packs them two to a register)
__host__ __device__ inline void map_cell_bits(uint32_t key, uint32_t count, uint32_t &n, uint32_t &height, uint32_t &cls)
{
    n = count < (uint32_t)MAP_SATURATED ? count : (uint32_t)MAP_SATURATED;
    height = count ? ((key >> 4) - 32768u) & 0xffffu : 0u;   // (two's complement: hq's low 16 bits)
    cls = count ? key & 15u : 0u;
}

// one plane value widened: depth -> t, labels -> the value map_class_of takes
__host__ __device__ inline float map_depth_at(const void *depth, int depth_format, size_t i)
{
    return depth_format == DEPTH_F16 ? depth_f16_to_f32(reinterpret_cast<const uint16_t *>(depth)[i]) : reinterpret_cast<const float *>(depth)[i];
}
__host__ __device__ inline uint32_t map_label_at(const void *seg, int seg_format, size_t i)
{
    return seg_format == SEG_INSTANCE_U16 ? (uint32_t) reinterpret_cast<const uint16_t *>(seg)[i] : (uint32_t) reinterpret_cast<const uint8_t *>(seg)[i];
}

// one frame's [3][M][M] from its planes [h][w] and the 12 camera floats eye(3) c(9), on the host: the loops.  key, count: M * M words of scratch each
inline void map_obs_host(const void *depth, int depth_format, const void *seg, int seg_format, int w, int h, const float *cam12, int M, float cell_size,
                         uint32_t *key, uint32_t *count, int16_t *out)
{
    const float inv = 1.0f / cell_size;
    for (int i = 0; i < M * M; ++i) key[i] = count[i] = 0u;
    for (int py = 0; py < h; ++py) {
        const float y = map_ray_y(py, h);
        for (int px = 0; px < w; ++px) {
            const size_t i = (size_t)py * w + px;
            int cell;
            uint32_t k;
            if (!map_pixel(cam12 + 3, map_ray_x(px, w), y, map_depth_at(depth, depth_format, i), map_class_of(map_label_at(seg, seg_format, i), seg_format), inv,
                           M, cell, k))
                continue;
            ++count[cell];
            key[cell] = k > key[cell] ? k : key[cell];
        }
    }
    for (int i = 0; i < M * M; ++i) {
        uint32_t v[MAP_OBS_PLANES];
        map_cell_bits(key[i], count[i], v[0], v[1], v[2]);
        for (int q = 0; q < MAP_OBS_PLANES; ++q) out[q * M * M + i] = (int16_t)(uint16_t)v[q];
    }
}

}  // namespace mv
