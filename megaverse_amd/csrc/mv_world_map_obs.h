// megaverse_amd/csrc/mv_world_map_obs.h -- world map observations (include/megaverse_hip.h: mv_set_world_map_obs): the rule, stated once for the kernel that
// merges a frame into an agent's grid (mv_world_map_obs.hip: world_map_obs_kernel) and for the host twin the tests compare it with (mv_debug_world_map_host).
//
// The record: ONE grid per agent, MAP_OBS_PLANES = 3 planes of M x M int16, [N*A][3][M][M], M = cells under map_cells_known's rule (mv_map_obs.h): an
// ALLOCENTRIC top-down grid of square cells of cell_size world units that is kept over an episode.  There is no entries dimension: every tick of every call
// merges into the same grid, in stream order, whatever the output ring's count.  The orientation is fixed: columns grow along world x from origin_x, rows
// along world z from origin_z, the grid covers M * cell_size world units each way, and nothing depends on the agent's heading.
// Every pixel (px, py) of a drawn frame whose depth t is not 0 and whose class is not SEG_HUD is unprojected exactly as map_pixel does (mv_map_obs.h):
//   pc  = (x(px) t, y(py) t, -t)                 map_ray_x / map_ray_y: the pass's own abscissae
//   d   = c pc                                   c: the viewer's 3x3 basis, floats 3 .. 11 of the camera record, in mat_mul's order
//   P   = eye + d                                eye: floats 0 .. 2 of the camera record; one fp32 add per axis: the hit in WORLD axes
//   col = floor((P.x - origin_x) inv),  row = floor((P.z - origin_z) inv),  inv = 1.0f / cell_size formed once on the host; the bounds are compared as floats:
//                                                a pixel outside [0, M) on either axis is dropped, and so is a NaN
//   hq  = clamp(floor(P.y * 32), -32767, 32767)  WORLD height in 1/32 world units (MAP_HEIGHT_SCALE), not height over the eye
//   key = (hq + 32768) << 4 | cls
// Per cell the planes keep MAP_OBS_FIELDS' meaning: the count, saturated at 32767; the greatest hq; the class at that height, among equal heights the greatest.
// THE BUFFER IS THE WHOLE STATE.  A cell's accumulated count is its stored count and its accumulated key is rebuilt from planes 1 and 2 when the count is not 0
// (world_map_cell_state: the inverse of map_cell_bits).  Merging a frame works per cell: count = min(old + new, 32767), key = max(old, new).  Both are
// independent of the order the pixels come in, and the merge is exact under saturation (min(min(a, S) + b, S) = min(a + b, S)), so the grids are reproducible
// byte for byte.  A consequence: a caller who zeroes an agent's grid on the gym's stream has cleared it, and a caller who copies one grid onto another has
// moved it -- what the user of mv_fork_envs does for the destination envs.  No clear or copy entry point is needed, and there is none.
// A grid is cleared (read as zeros) before a frame is merged exactly when that frame is the first of a new episode; mv_world_map_obs.hip says which frames are.
// Every product and sum below is one fp32 operation in the order written (the library is built with -ffp-contract=off).
#pragma once
#include "mv_map_obs.h"

namespace mv {

// THE RULE: one pixel -> its cell (row * M + col) and key; false: the pixel enters no cell.  cam: eye(3) c(9)
__host__ __device__ inline bool world_map_pixel(const float *cam, float x, float y, float t, int cls, float inv, float ox, float oz, int M, int &cell, uint32_t &key)
{
    if (t == 0.0f || cls == SEG_HUD) return false;
    const float *c = cam + 3;
    const float pcx = x * t, pcy = y * t, pcz = -t;
    const float dx = (c[0] * pcx + c[1] * pcy) + c[2] * pcz;   // (mat_mul's order, mv_frame.h)
    const float dy = (c[3] * pcx + c[4] * pcy) + c[5] * pcz;
    const float dz = (c[6] * pcx + c[7] * pcy) + c[8] * pcz;
    const float Px = cam[0] + dx, Py = cam[1] + dy, Pz = cam[2] + dz;
    const float fc = floorf((Px - ox) * inv), fr = floorf((Pz - oz) * inv);
    if (!(fc >= 0.0f && fc < float(M) && fr >= 0.0f && fr < float(M))) return false;   // (compared as floats: no conversion of a value no int holds; a NaN is dropped)
    const float fh = fminf(fmaxf(floorf(Py * float(MAP_HEIGHT_SCALE)), -32767.0f), 32767.0f);
    cell = (int)fr * M + (int)fc;
    key = (uint32_t)((int)fh + 32768) << 4 | (uint32_t)cls;
    return true;
}

// one cell's accumulated key and count from its three stored values, each the int16's bits in the low half of a word: map_cell_bits backwards.  (A stored count
// is at most 32767; whatever else a caller's bytes hold reads as a count past saturation and comes out as 32767.)
__host__ __device__ inline void world_map_cell_state(uint32_t n, uint32_t height, uint32_t cls, uint32_t &key, uint32_t &count)
{
    count = n & 0xffffu;
    key = count ? (((height + 32768u) & 0xffffu) << 4 | (cls & 15u)) : 0u;   // (two's complement: hq + 32768 in [1, 65535])
}

// one frame merged into one agent's grid [3][M][M] on the host: the loops.  clear: the grid is read as zeros.  key, count: M * M words of scratch each
inline void world_map_obs_host(const void *depth, int depth_format, const void *seg, int seg_format, int w, int h, const float *cam12, int M, float cell_size,
                               float ox, float oz, bool clear, uint32_t *key, uint32_t *count, int16_t *grid)
{
    const float inv = 1.0f / cell_size;
    const int cells = M * M;
    for (int i = 0; i < cells; ++i) {
        key[i] = count[i] = 0u;
        if (!clear) world_map_cell_state((uint16_t)grid[i], (uint16_t)grid[cells + i], (uint16_t)grid[2 * cells + i], key[i], count[i]);
    }
    for (int py = 0; py < h; ++py) {
        const float y = map_ray_y(py, h);
        for (int px = 0; px < w; ++px) {
            const size_t i = (size_t)py * w + px;
            int cell;
            uint32_t k;
            if (!world_map_pixel(cam12, map_ray_x(px, w), y, map_depth_at(depth, depth_format, i), map_class_of(map_label_at(seg, seg_format, i), seg_format),
                                 inv, ox, oz, M, cell, k))
                continue;
            ++count[cell];
            key[cell] = k > key[cell] ? k : key[cell];
        }
    }
    for (int i = 0; i < cells; ++i) {
        uint32_t v[MAP_OBS_PLANES];
        map_cell_bits(key[i], count[i], v[0], v[1], v[2]);
        for (int q = 0; q < MAP_OBS_PLANES; ++q) grid[q * cells + i] = (int16_t)(uint16_t)v[q];
    }
}

}  // namespace mv
