// xworld_amd/csrc/kernels_xworld_symbolic.hip -- symbolic observations of an XWorld2D batch (xwb_xw_symbolic, include/xwb.h):
// what each square of an env's newest frame shows, as ids -- int16 [n][3][S][S], planes KIND, ICON, NAME.
//   full observation   S = max_dim, square (i, j) = map cell (x = j, y = i).  A gather: the cell code the frame was drawn from
//                      (xw_frame_code, the selection of xwb_xw_pack_grids and xwb_xw_render_view) through icon_type and
//                      icon_name.  One lane per cell; a wavefront stores runs of a plane.
//   egocentric         S = r, square (i, j) of the TURNED frame.  Shadows, window and cell table are the frame render's own
//                      (xw_ego_cells.h: ego_image_masking, ego_window_cell -- the table entry is turned into ids here instead
//                      of pixels), the quarter turn is the view kernel's map (ego_view_source) at the square's centre pixel.
//                      One wavefront per env, four envs per workgroup; the 6 r^2 bytes of an env are staged in LDS so that
//                      the workgroup stores ONE contiguous run (54 bytes per env at r = 3: twelve stores of 18 bytes otherwise).
// The output is small (294 bytes per env at r = 7): the call is bound by its launch and by the latency of the loads behind
// the scan, not by its stores.  One launch per call; nothing is written but `out`.
#include "xwb_common.h"
#include "xw_device.h"
#include "xw_ego_cells.h"

namespace xwb {

namespace {

constexpr int SYM_BS = 256, SYM_WAVES = SYM_BS / 64;
// include/xwb.h XWB_SYM_*: the KIND of an icon is its XWB_ICON_* type + 1
enum : int { SYM_EMPTY = 0, SYM_DARK = 4 };

struct SymCell { int16_t kind, icon, name; };

// code: icon + 1, 0 = empty, the target bit stripped
__device__ __forceinline__ SymCell sym_of_code(const XwParams &p, uint32_t code) {
    if (code == 0) return SymCell{(int16_t)SYM_EMPTY, (int16_t)-1, (int16_t)-1};
    const int icon = (int)code - 1;
    return SymCell{(int16_t)(p.icon_type[icon] + 1), (int16_t)icon, p.icon_name[icon]};
}

}  // namespace

// src: PACK_SRC_*
__global__ __launch_bounds__(SYM_BS) void xw_symbolic_full_kernel(XwParams p, int src, int16_t *out) {
    const int cells = p.max_dim * p.max_dim;
    const size_t gi = (size_t)blockIdx.x * SYM_BS + threadIdx.x;
    if (gi >= (size_t)p.n * cells) return;
    const int e = (int)(gi / cells), c = (int)(gi - (size_t)e * cells);
    const SymCell s = sym_of_code(p, xw_frame_code(p, xw_frame_is_term(p, src, e), gi));
    int16_t *o = out + (size_t)e * 3 * cells + c;
    o[0] = s.kind; o[cells] = s.icon; o[2 * cells] = s.name;
}

__global__ __launch_bounds__(SYM_BS) void xw_symbolic_ego_kernel(XwParams p, int16_t *out) {
    const int r = p.visible_radius, rr = r * r, D = p.max_dim, cells = D * D;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint16_t s_code[SYM_WAVES][XW_MAX_DIM * XW_MAX_DIM];
    __shared__ uint8_t s_type[SYM_WAVES][XW_MAX_DIM * XW_MAX_DIM], s_shadow[SYM_WAVES][XW_MAX_DIM * XW_MAX_DIM], s_ray[SYM_WAVES][XW_MAX_DIM],
        s_gc[SYM_WAVES][XW_MAX_GOALS];
    __shared__ int16_t s_out[SYM_WAVES * 3 * XW_MAX_DIM * XW_MAX_DIM];
    const size_t e0 = (size_t)blockIdx.x * SYM_WAVES, e = e0 + wave;
    if (e < (size_t)p.n) {                                                      // (wave-uniform)
        const int dir = p.agent_dir[e] & 3, axy = p.agent_xy[e], ax = axy & 0xffff, ay = axy >> 16;
        uint16_t *code = s_code[wave];
        uint8_t *type = s_type[wave];
        for (int c = lane; c < cells; c += 64) {                                // the live state, as the frame render and the view read it
            const int cd = p.grid[e * cells + c] & CELL_ICON_MASK;
            code[c] = (uint16_t)cd;
            type[c] = cd ? p.icon_type[cd - 1] : (uint8_t)3;
        }
        if (lane < XW_MAX_GOALS) s_gc[wave][lane] = p.goal_cells[e * XW_MAX_GOALS + lane];
        if (lane < r) s_ray[wave][lane] = 1;
        auto is_block = [&](int x, int y) { return (unsigned)x < (unsigned)D && (unsigned)y < (unsigned)D && type[y * D + x] == 1; };
        const EgoWindow win = ego_image_masking(r, ax, ay, dir, lane, s_ray[wave], s_shadow[wave], is_block);
        int16_t *o = s_out + wave * 3 * rr;
        const uint32_t *atlas4 = reinterpret_cast<const uint32_t *>(p.atlas64), *gimg = p.goal_img + e * p.num_goals * 4096;
        for (int k = lane; k < rr; k += 64) {                                   // square k of the turned frame
            const int i = k / r, j = k - i * r;
            int sx, sy, slot;
            ego_view_source(dir, 64 * r, 64 * i + 32, 64 * j + 32, &sx, &sy);   // its centre pixel: never on the black line
            // the window cell it shows, as the renders' cell table has it (no pixel is read: the images are only named)
            const EgoCell cell = ego_window_cell(p, atlas4, p.icon_type, p.ego_agent_rot, code, type, s_shadow[wave], s_gc[wave], gimg, win,
                                                 (sy >> 6) * r + (sx >> 6), dir, &slot);
            const int entry = ego_cell_entry(cell);
            SymCell s{(int16_t)SYM_DARK, (int16_t)-1, (int16_t)-1};
            if (entry < 0) s = sym_of_code(p, code[s_gc[wave][slot]]);          // a goal: its cell holds the icon
            else if (entry <= p.n_icons) s = sym_of_code(p, entry < p.n_icons ? (uint32_t)entry + 1u : 0u);
            o[k] = s.kind; o[rr + k] = s.icon; o[2 * rr + k] = s.name;
        }
    }
    __syncthreads();
    const size_t left = (size_t)p.n - e0;                                       // envs of this workgroup: one contiguous run of the output
    const int count = 3 * rr * (int)(left < (size_t)SYM_WAVES ? left : (size_t)SYM_WAVES);
    int16_t *dst = out + e0 * 3 * rr;
    for (int t = tid; t < count; t += SYM_BS) dst[t] = s_out[t];
}

hipError_t launch_xw_symbolic(const XwParams &p, int src, int16_t *out, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    if (p.visible_radius) {
        hipLaunchKernelGGL(xw_symbolic_ego_kernel, dim3((unsigned)((p.n + SYM_WAVES - 1) / SYM_WAVES)), dim3(SYM_BS), 0, s, p, out);
    } else {
        const size_t total = (size_t)p.n * p.max_dim * p.max_dim;
        hipLaunchKernelGGL(xw_symbolic_full_kernel, dim3((unsigned)((total + SYM_BS - 1) / SYM_BS)), dim3(SYM_BS), 0, s, p, src, out);
    }
    return hipGetLastError();
}

}  // namespace xwb
