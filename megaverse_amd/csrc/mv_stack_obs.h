// megaverse_amd/csrc/mv_stack_obs.h -- stack observations (include/megaverse_hip.h: mv_set_stack_obs): the rule, stated once for the kernel that writes an
// agent's frame stack (mv_stack_obs.hip: stack_obs_kernel) and for the host twin the tests compare it with (mv_debug_stack_host).
//
// The record: per agent S = frames planes-sets of C channels of h x w bytes, [N*A][S][C][h][w] uint8, h = H / factor, w = W / factor; plane-set S - 1 is the
// newest frame, 0 the oldest; row 0 is the frame's row 0 (the bottom row).  C = 1 (STACK_GRAY_U8) or 3 (STACK_RGB_U8: planes R, G, B).
// The image of a frame: output pixel (Y, X) is made of the factor x factor block of frame pixels (Y factor + r, X factor + q); R, G, B: the block's sums of
// the three colour bytes (the RGBA layout's alpha byte is not read into any sum), each at most 16 * 255:
//   RGB   c_out = (sum_c + factor^2 / 2) / factor^2                        the mean, rounded half up (factor 1: the byte itself)
//   grey  (77 R + 150 G + 29 B + 128 factor^2) >> (8 + 2 log2 factor)     77 + 150 + 29 = 256: ONE rounding over weights and mean together; at most 255
// Integers only: at most 256 * 16 * 255 + 2048 < 2^21, no overflow, nothing to round twice, so a stack is reproducible byte for byte with no tolerance.
// The stack of a drawn frame:
//   the frame is the first of a new episode    every one of the S plane-sets is the image
//   otherwise                                  out[i] = prev[i + 1] for i < S - 1, out[S - 1] = the image
//   a frame drawn again (mv_render)            out[S - 1] = the image, nothing else is touched
// prev is the agent's stack in the entry the previous drawn tick wrote; with one entry it is out itself, and the shift is then in place: position p of
// plane-set i + 1 is read and position p of plane-set i is written by the SAME worker, i ascending, so no worker reads what another has overwritten.
// mv_stack_obs.hip says which frames are the first of a new episode (the world map's condition) and how its lanes share the positions.
#pragma once
#include <cstdint>
#include <cstring>

#include <hip/hip_runtime.h>

namespace mv {

enum : int { STACK_GRAY_U8 = 0, STACK_RGB_U8 = 1 };   // include/megaverse_hip.h: MV_STACK_GRAY_U8, MV_STACK_RGB_U8
enum : int { STACK_RGBA = 0, STACK_CHW = 1 };         // the frames' layout: MV_OBS_RGBA, MV_OBS_RGB_PLANAR
enum : int { STACK_FRAMES_MAX = 8, STACK_GRAY_R = 77, STACK_GRAY_G = 150, STACK_GRAY_B = 29 };
static_assert(STACK_GRAY_R + STACK_GRAY_G + STACK_GRAY_B == 256, "the grey weights are 8-bit fixed point");

__host__ __device__ inline bool stack_format_known(int format) { return format == STACK_GRAY_U8 || format == STACK_RGB_U8; }
__host__ __device__ inline int stack_channels(int format) { return format == STACK_RGB_U8 ? 3 : 1; }
// log2 factor for factor 1, 2, 4; -1: no such factor
__host__ __device__ inline int stack_factor_log2(int factor) { return factor == 1 ? 0 : factor == 2 ? 1 : factor == 4 ? 2 : -1; }
// one agent's stack in bytes
__host__ __device__ inline size_t stack_frame_bytes(int S, int format, int w, int h) { return (size_t)S * stack_channels(format) * w * h; }

// THE RULE, one output pixel: a channel's sum over the factor x factor block -> its byte; the three sums -> the grey byte.  lg = log2 factor
__host__ __device__ inline uint32_t stack_mean(uint32_t sum, int lg) { return (sum + ((1u << (2 * lg)) >> 1)) >> (2 * lg); }
__host__ __device__ inline uint32_t stack_gray(uint32_t R, uint32_t G, uint32_t B, int lg)
{
    return (STACK_GRAY_R * R + STACK_GRAY_G * G + STACK_GRAY_B * B + (128u << (2 * lg))) >> (8 + 2 * lg);
}

// byte c (0: R, 1: G, 2: B) of frame pixel (py, px) of a W x H frame in either layout
__host__ __device__ inline uint32_t stack_frame_byte(const uint8_t *frame, int layout, int W, int H, int py, int px, int c)
{
    return layout == STACK_CHW ? frame[((size_t)c * H + py) * W + px] : frame[((size_t)py * W + px) * 4 + c];
}

// what every entry point refuses of the stack's own arguments; null: fine, else the text behind "<who>: "
inline const char *stack_args_refusal(int W, int H, int S, int factor, int format)
{
    if (!stack_format_known(format)) return "unknown format (MV_STACK_GRAY_U8, MV_STACK_RGB_U8)";
    if (S < 1 || S > STACK_FRAMES_MAX) return "frames must lie in [1, 8]";
    if (stack_factor_log2(factor) < 0) return "factor must be 1, 2 or 4";
    if (W < 1 || H < 1 || W % factor || H % factor) return "the frame's width and height must be multiples of factor";
    if ((W / factor) % 4) return "the stack's width, the frame's over factor, must be a multiple of 4 (a lane writes four pixels as one word)";
    return nullptr;
}

// one frame -> one agent's stack on the host: the loops.  clear != 0: the frame is the first of a new episode.  prev == out: in place
inline void stack_obs_host(const uint8_t *frame, int layout, int W, int H, int S, int factor, int format, bool clear, const uint8_t *prev, uint8_t *out)
{
    const int lg = stack_factor_log2(factor), w = W / factor, h = H / factor, C = stack_channels(format);
    const size_t P = (size_t)C * w * h;
    if (!clear)
        for (int i = 0; i + 1 < S; ++i) std::memmove(out + i * P, prev + (i + 1) * P, P);
    uint8_t *img = out + (size_t)(S - 1) * P;
    for (int Y = 0; Y < h; ++Y)
        for (int X = 0; X < w; ++X) {
            uint32_t sum[3] = {0u, 0u, 0u};
            for (int r = 0; r < factor; ++r)
                for (int q = 0; q < factor; ++q)
                    for (int c = 0; c < 3; ++c) sum[c] += stack_frame_byte(frame, layout, W, H, Y * factor + r, X * factor + q, c);
            const size_t at = (size_t)Y * w + X;
            if (format == STACK_GRAY_U8) img[at] = (uint8_t)stack_gray(sum[0], sum[1], sum[2], lg);
            else
                for (int c = 0; c < 3; ++c) img[(size_t)c * w * h + at] = (uint8_t)stack_mean(sum[c], lg);
        }
    if (clear)
        for (int i = 0; i + 1 < S; ++i) std::memcpy(out + i * P, img, P);
}

}  // namespace mv
