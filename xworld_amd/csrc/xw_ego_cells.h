// xw_ego_cells.h -- what the r x r cells in front of an egocentric agent show (XMap::to_image with visible_radius > 0,
// xmap.cpp:148-200): the wall shadows of XMap::image_masking and the table view cell -> image.  Device code shared by the
// one-workgroup-per-env frame render (kernels_xworld_ego.hip, xw_render_ego_kernel), the native-resolution view
// (kernels_xworld_view.hip) and the symbolic observation (kernels_xworld_symbolic.hip): one wavefront walks one env, its
// scratch arrays live in LDS.
#pragma once
#include "xwb_common.h"

namespace xwb {
namespace {

// What one cell of the view shows: a 64 x 64 image (block icon, this env's warped goal image, the agent icon turned for
// its heading -- the three turned copies of every agent icon are appended to the atlas at create time) or one constant
// pixel (mask = 0).  The table makes the per-pixel lookup branch-free: one 16-byte LDS read, an AND and an add.
struct EgoCell {
    const uint32_t *img;
    int mask;                    // -1: index the image; 0: a constant pixel
    int tab;                     // frame of the interior-pixel table that shows this cell's image, -1: none (a goal)
};

// What one view cell shows.  dir: heading; tab: -1 for goals (their images are per env)
__device__ __forceinline__ EgoCell ego_icon_cell(const uint8_t *icon_type, const uint32_t *agent_rot, const uint32_t *atlas4,
                                                 int icon, int dir) {
    EgoCell c{atlas4 + (size_t)icon * 4096, -1, icon * 4 + dir};
    // the agent: XItem::get_item_image turns its icon by 90 - yaw deg
    if (icon_type[icon] == 2 && dir != 1) c.img = atlas4 + agent_rot[icon] + (size_t)(dir == 0 ? 0 : (dir == 2 ? 1 : 2)) * 4096;
    return c;
}

// the view window on the padded map: view cell (cx, cy) shows map cell (x_st - r + cx, y_st - r + cy)
struct EgoWindow { int x_st, y_st; };

__device__ __forceinline__ void ego_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }

// XMap::image_masking (xmap.cpp:273-362) by the lanes `tid` < 64 of one wavefront: s_shadow[view cell] = 1 behind a wall.
// is_block(x, y): map cell (x, y) holds a block (false outside the map).  s_ray [r]: scratch, all 1 on entry.
template <class IsBlock>
__device__ __forceinline__ EgoWindow ego_image_masking(int r, int ax, int ay, int dir, int tid, uint8_t *s_ray, uint8_t *s_shadow,
                                                       IsBlock is_block) {
    int major_x = 0, major_y = 0, minor_x = 0, minor_y = 0, scan_x0 = 0, scan_y0 = 0, xa = ax + r, ya = ay + r;
    if (dir == 0) { xa += r / 2; major_y = 1; minor_x = 1; }
    else if (dir == 3) { ya -= r / 2; major_x = 1; minor_y = -1; scan_y0 = r - 1; }
    else if (dir == 2) { xa -= r / 2; major_y = 1; minor_x = -1; scan_x0 = r - 1; }
    else { ya += r / 2; major_x = 1; minor_y = 1; }
    const int x_st = xa - r / 2, y_st = ya - r / 2;
    ego_wave_sync();
    if (tid < 2) {                                      // rays to either side of the agent
        const int o = tid ? 1 : -1;
        bool block = false;
        int rx = ax, ry = ay;
        for (int k = 1; k <= r / 2; ++k) {
            rx += o * major_x; ry += o * major_y;
            if (block) s_ray[r / 2 + o * k] = 0;
            if (is_block(rx, ry)) block = true;
        }
    }
    ego_wave_sync();
    if (tid < r) {                                      // one scan line per lane
        bool block = !s_ray[tid];
        int cx = scan_x0 + tid * major_x, cy = scan_y0 + tid * major_y;
        for (int j = 0; j < r; ++j) {
            s_shadow[cy * r + cx] = block ? 1 : 0;
            if (is_block(x_st - r + cx, y_st - r + cy)) block = true;
            cx = (cx + minor_x + r) % r;
            cy = (cy + minor_y + r) % r;
        }
    }
    ego_wave_sync();
    return EgoWindow{x_st, y_st};
}

// The quarter turn of the view undone (cv::warpAffine by 90 + yaw degrees, an exact integer map): pixel (row vr, column vc) of
// the turned S x S view shows pixel (*sx, *sy) of the window; an index S falls outside and leaves one black row / column.
//   up (3): sx = vc, sy = vr;  right (0): sx = S - vr, sy = vc;  down (1): sx = S - vc, sy = S - vr;  left (2): sx = vr, sy = S - vc
__device__ __forceinline__ void ego_view_source(int dir, int S, int vr, int vc, int *sx, int *sy) {
    const int fr = (dir == 3 || dir == 2) ? vr : S - vr, fc = (dir == 3 || dir == 0) ? vc : S - vc;
    const bool row_is_y = dir == 3 || dir == 1;
    *sx = row_is_y ? fc : fr;
    *sy = row_is_y ? fr : fc;
}

// What view cell k shows.  code / type: the env's grid (target bit stripped) and the type of the entity in each cell (3 = none);
// gc: its goal slot -> cell table; gimg: its warped goal images.  *slot: the goal slot of a goal, -1 for everything else.
__device__ __forceinline__ EgoCell ego_window_cell(const XwParams &p, const uint32_t *atlas4, const uint8_t *icon_type,
                                                   const uint32_t *agent_rot, const uint16_t *code, const uint8_t *type,
                                                   const uint8_t *shadow, const uint8_t *gc, const uint32_t *gimg, EgoWindow w,
                                                   int k, int dir, int *slot) {
    const int r = p.visible_radius, D = p.max_dim;
    const uint32_t *white = atlas4 + (size_t)p.n_icons * 4096, *black = white + 1;
    const int gx = w.x_st - r + k % r, gy = w.y_st - r + k / r;
    EgoCell c{black, 0, (p.n_icons + 1) * 4 + dir};     // outside the map, or in a wall's shadow
    *slot = -1;
    if ((unsigned)gx < (unsigned)D && (unsigned)gy < (unsigned)D && !(shadow[k] && !p.no_wall_shadow)) {
        const int cd = code[gy * D + gx];
        if (cd == 0) { c.img = white; c.tab = p.n_icons * 4 + dir; }
        else {
            c = ego_icon_cell(icon_type, agent_rot, atlas4, cd - 1, dir);
            if (type[gy * D + gx] == 0) {               // a goal: this env's warped copy
                // the FIRST slot that holds the cell: cell 255 of a 16 x 16 map reads like the empty slots' 0xff, which all
                // come after the real ones (xwb_common.h, xw_goal_slot_of)
                const int found = xw_goal_slot_of(gc, gy * D + gx), s = found < 0 ? 0 : found;
                c.img = gimg + s * 4096;
                c.tab = -1;
                *slot = s;
            }
        }
    }
    return c;
}

// Which entry of the table frames a view cell shows (EgoCell::tab without the heading): icon i < n_icons, n_icons = an empty
// cell, n_icons + 1 = a black one (outside the map, a wall's shadow); -1: a goal
__device__ __forceinline__ int ego_cell_entry(const EgoCell &c) { return c.tab >> 2; }

}  // namespace
}  // namespace xwb
