// megaverse_amd/csrc/mv_seg_obs.h -- segmentation observations (mv_set_seg_obs, include/megaverse_hip.h): the record and its rule, stated once for the kernels
// that store it (mv_raster.hip: raster_seg_kernel) and for the host twins (mv_debug_seg_rule_host, mv_debug_seg_pack_host, mv_seg_obs.hip).
//
// The record: ONE label per pixel of a frame, a single plane [H][W] in the frame's own pixel order -- row 0 is the bottom row, as in the RGBA frame and the
// depth plane -- whatever the colour layout (mv_set_obs_layout) is.  The label names the drawable whose hit the pixel shows (the nearest hit, the very list
// position the shading works from): its CLASS, and the index of its record within its class's record array.
//   SEG_CLASS_U8:     one byte, the class.
//   SEG_INSTANCE_U16: one 16-bit word, class << 12 | instance; instance < 4096 (the capacities of mv_types.h, asserted below).  The whole word is 0 where the
//                     ray hits nothing; its class nibble is the U8 plane's byte, bit for bit.
//
// The classes follow the drawable groups of frame_setup_body (mv_frame.h), which packs the slots in the order the reference emits drawables:
//   layout boxes | "terrain" slots | movable objects | collectables | 3 per agent (capsule, eye box, time bar)
//
//   class          value  what it covers                                                                                 instance
//   NONE             0    the ray hits nothing: exactly where the depth is 0
//   FLOOR            1    a layout box drawn in the layout colour (LayoutBox.slot == 0)                                  box index
//   STRUCTURE        2    every other layout box; every hex_boxes record of the Hex scenarios, BoxAGone and Football     box index
//   EXIT             3    exit pad (TERRAIN_EXIT), Sokoban goal pad                                                      terrain index / cell index
//   LAVA             4    lava slab (every terrain box that is no exit: frame_setup_body draws it red)                   terrain index
//   BUILDING_ZONE    5    TowerBuilding's zone slab                                                                      0
//   FURNITURE        6    Rearrange's raised floor and pedestals, Sokoban's wall caps                                    static index / cell index
//   TARGET           7    Rearrange's target arrangement on the left pedestal                                            item index
//   MOVABLE          8    a movable object resting in the world (tower box, Sokoban box, Rearrange item)                 object index
//   CARRIED          9    a movable object in an agent's hands (state > 0)                                               object index
//   COLLECTABLE     10    Obstacles' diamonds, Collect's +1 diamonds, every Hex collectable (all of its parts)           record index, not the part
//   HAZARD          11    Collect's -1 (red) diamonds                                                                    reward index
//   BALL            12    Football's ball (its hex_objs records)                                                         record index (0)
//   AGENT           13    another agent's capsule and its eye box                                                        agent k
//   HUD             14    the time bar                                                                                   agent k whose camera frame it sits in
// HexMemory's good / bad is hidden state: it is no input of the rule, so both kinds carry the same word.
//
// The rule is a function of the scenario, the slot, the group boundaries and -- where a group has sub-types -- ONE value of the record the slot names:
//   layout boxes: LayoutBox.slot;  Obstacles' terrain: TerrainBox.type;  Sokoban's cells: the cell byte;  movable objects and diamonds: MovableObject.state.
// The kernels take the sub-type from the frame's own list where the list carries it (seg_subtype_of_prim: the primitive's frame says carried, its colour says
// exit / lava, wall cap / goal pad, red / green), so that only the boundaries and LayoutBox.slot are read from the env's records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mv_types.h"

namespace mv {

enum : int { SEG_CLASS_U8 = 0, SEG_INSTANCE_U16 = 1 };
enum : int {
    SEG_NONE = 0, SEG_FLOOR = 1, SEG_STRUCTURE = 2, SEG_EXIT = 3, SEG_LAVA = 4, SEG_BUILDING_ZONE = 5, SEG_FURNITURE = 6, SEG_TARGET = 7, SEG_MOVABLE = 8,
    SEG_CARRIED = 9, SEG_COLLECTABLE = 10, SEG_HAZARD = 11, SEG_BALL = 12, SEG_AGENT = 13, SEG_HUD = 14, SEG_NUM_CLASSES = 15,
};
enum : int { SEG_INSTANCE_BITS = 12, SEG_MAX_INSTANCES = 1 << SEG_INSTANCE_BITS };
static_assert(SEG_NUM_CLASSES <= 16, "a class is four bits of the U16 word");
static_assert(MAX_BOXES <= SEG_MAX_INSTANCES && COLLECT_MAX_BOXES <= SEG_MAX_INSTANCES && HEX_MAX_BOXES <= SEG_MAX_INSTANCES && HEX_MAX_OBJS <= SEG_MAX_INSTANCES
                  && MAX_OBJECTS <= SEG_MAX_INSTANCES && MAX_TERRAIN <= SEG_MAX_INSTANCES && MAX_REWARDS <= SEG_MAX_INSTANCES && COLLECT_MAX_REWARDS <= SEG_MAX_INSTANCES
                  && SOKO_DIM * SOKO_DIM <= SEG_MAX_INSTANCES && NUM_STATIC + MAX_ITEMS <= SEG_MAX_INSTANCES && MAX_AGENTS <= SEG_MAX_INSTANCES,
              "every record array's indices fit the instance field");

__host__ __device__ inline bool seg_format_known(int format) { return format == SEG_CLASS_U8 || format == SEG_INSTANCE_U16; }
__host__ __device__ inline size_t seg_value_bytes(int format) { return format == SEG_INSTANCE_U16 ? 2u : 1u; }
// one frame's plane
__host__ __device__ inline size_t seg_plane_bytes(int W, int H, int format) { return (size_t)W * H * seg_value_bytes(format); }

inline const char *seg_class_name(int cls)
{
    static const char *const names[SEG_NUM_CLASSES] = {"NONE", "FLOOR", "STRUCTURE", "EXIT", "LAVA", "BUILDING_ZONE", "FURNITURE", "TARGET", "MOVABLE",
                                                       "CARRIED", "COLLECTABLE", "HAZARD", "BALL", "AGENT", "HUD"};
    return cls >= 0 && cls < SEG_NUM_CLASSES ? names[cls] : nullptr;
}

// the 16-bit word of (class, instance); class NONE is the whole word 0
__host__ __device__ inline uint16_t seg_word(int cls, int instance)
{
    return cls == SEG_NONE ? (uint16_t)0 : (uint16_t)((cls << SEG_INSTANCE_BITS) | (instance & (SEG_MAX_INSTANCES - 1)));
}
__host__ __device__ inline int seg_class_of(uint16_t word) { return word >> SEG_INSTANCE_BITS; }
__host__ __device__ inline int seg_instance_of(uint16_t word) { return word & (SEG_MAX_INSTANCES - 1); }

// The group boundaries of an env's slots: [0, terrain) layout boxes, [terrain, objects) terrain slots, [objects, rewards) movable objects,
// [rewards, agents) collectables' parts, [agents, end) three per agent.  frame_setup_body's own arithmetic (mv_frame.h), from the env header's counts.
struct SegBounds { int32_t terrain, objects, rewards, agents, end; };
__host__ __device__ inline bool seg_hex_records(int scen) { return scen == SCN_HEX_MEMORY || scen == SCN_HEX_EXPLORE || scen == SCN_BOXAGONE || scen == SCN_FOOTBALL; }
__host__ __device__ inline SegBounds seg_bounds(int scen, int L, int Wroom, int num_boxes, int num_terrain, int num_objects, int num_rewards, int num_agents)
{
    const bool hex = seg_hex_records(scen);
    const int sokoW = Wroom > 1 ? Wroom : 1;
    const int nTerrain = scen == SCN_TOWER ? 1 : scen == SCN_REARRANGE ? NUM_STATIC + num_terrain : scen == SCN_SOKOBAN ? L * sokoW : hex ? 0 : num_terrain;
    const int nRewards = scen == SCN_TOWER ? 0 : hex ? 3 * num_rewards : 2 * num_rewards;
    SegBounds b;
    b.terrain = num_boxes;
    b.objects = b.terrain + nTerrain;
    b.rewards = b.objects + num_objects;
    b.agents = b.rewards + nRewards;
    b.end = b.agents + 3 * num_agents;
    return b;
}
__host__ __device__ inline SegBounds seg_bounds(const EnvHeader &h, int num_agents)
{
    return seg_bounds(h.scenario, h.L, h.W, h.num_boxes, h.num_terrain, h.num_objects, h.num_rewards, num_agents);
}

// THE RULE: slot -> word.  subtype: the one value of the slot's record that tells its group's sub-types apart (above); ignored where a group has none.
__host__ __device__ inline uint16_t seg_rule(int scen, int slot, const SegBounds &b, int subtype)
{
    if (slot < 0 || slot >= b.end) return 0;
    const bool hex = seg_hex_records(scen);
    if (slot < b.terrain) return seg_word(!hex && subtype == 0 ? SEG_FLOOR : SEG_STRUCTURE, slot);
    if (slot < b.objects) {
        const int j = slot - b.terrain;
        if (scen == SCN_TOWER) return seg_word(SEG_BUILDING_ZONE, 0);
        if (scen == SCN_REARRANGE) return j < NUM_STATIC ? seg_word(SEG_FURNITURE, j) : seg_word(SEG_TARGET, j - NUM_STATIC);
        if (scen == SCN_SOKOBAN) return seg_word(subtype == SOKO_WALL ? SEG_FURNITURE : subtype == SOKO_GOAL ? SEG_EXIT : SEG_NONE, j);
        return seg_word(subtype == TERRAIN_EXIT ? SEG_EXIT : SEG_LAVA, j);
    }
    if (slot < b.rewards) return seg_word(subtype > 0 ? SEG_CARRIED : SEG_MOVABLE, slot - b.objects);
    if (slot < b.agents) {
        const int q = slot - b.rewards;
        if (hex) return seg_word(scen == SCN_FOOTBALL ? SEG_BALL : SEG_COLLECTABLE, q / 3);
        return seg_word(scen == SCN_COLLECT && subtype == 2 ? SEG_HAZARD : SEG_COLLECTABLE, q >> 1);
    }
    const int q = slot - b.agents, k = q / 3;
    return seg_word(q - 3 * k == 2 ? SEG_HUD : SEG_AGENT, k);
}

// The sub-type of a slot as the frame's own list carries it: the primitive's frame of reference (a carried object lives in its carrier's camera frame,
// 1 + k = its state) and its colour (the constants frame_setup_body draws with, named once in mv_types.h: COLOR_EXIT_PAD, COLOR_SOKO_WALL_CAP, COLOR_DIAMOND_RED).
// Layout boxes: not in the list -- layout_slot is LayoutBox.slot of the box (read by the caller for the non-hex scenarios' layout slots only).
__host__ __device__ inline int seg_subtype_of_prim(int scen, int slot, const SegBounds &b, int frame_of_reference, uint32_t color, int layout_slot)
{
    if (slot < b.terrain) return layout_slot;
    if (slot < b.objects) {
        if (scen == SCN_SOKOBAN) return color == COLOR_SOKO_WALL_CAP ? (int)SOKO_WALL : (int)SOKO_GOAL;
        return color == COLOR_EXIT_PAD ? (int)TERRAIN_EXIT : (int)TERRAIN_LAVA;
    }
    if (slot < b.rewards) return frame_of_reference;
    if (slot < b.agents) return color == COLOR_DIAMOND_RED ? 2 : 1;
    return 0;
}

// what a plane of `format` holds for a word
__host__ __device__ inline uint8_t seg_bits_u8(uint16_t word) { return (uint8_t)seg_class_of(word); }

// n (class, instance) pairs -> out, as the kernels store them
inline void seg_pack_host(const int32_t *cls, const int32_t *instance, int n, int format, void *out)
{
    for (int i = 0; i < n; ++i) {
        const uint16_t w = seg_word(cls[i], instance[i]);
        if (format == SEG_INSTANCE_U16) reinterpret_cast<uint16_t *>(out)[i] = w;
        else reinterpret_cast<uint8_t *>(out)[i] = seg_bits_u8(w);
    }
}

}  // namespace mv
