// xworld_amd/csrc/kernels_xworld_view.hip -- XWorld2D views at native resolution (xwb_xw_render_view): the image
// XWorldSimulator's resizes start from, 64 pixels per cell, interleaved B,G,R, uint8.
//   full observation   XMap::to_image(agent, false, 0), xmap.cpp:125-146: a white [64 D][64 D] canvas, every cell's item image
//                      copied in.  A cell row is 192 bytes = twelve 16-byte pieces and cell origins are 16-byte aligned in the
//                      frame, so with a 3-byte-per-pixel atlas (view_atlas: entry 0 a white cell, entry i + 1 icon i) the
//                      render is an aligned gather: cell code -> piece.
//   egocentric         XMap::to_image(agent, false, r), xmap.cpp:148-200: the [64 r][64 r] window in front of the agent, wall
//                      shadows black, turned by 90 + yaw degrees.  The cell table is the frame render's (xw_ego_cells.h); a
//                      view pixel is ONE source pixel: undo the quarter turn (the integer map of ego_pixel,
//                      xw_ego_pixel.h: source index S falls outside and leaves one black row / column), look the cell
//                      up, load one dword of atlas64 / goal_img.  Sources hold 4 bytes per pixel, the view 3: a lane makes
//                      four pixels = three dwords, one 12-byte store; a wavefront stores 768 contiguous bytes of a row.
// Both are pure store streams (786 KB per env at 8 x 8, 307 KB at r = 5) whose sources stay in the caches; stores are
// non-temporal like those of the frame renders.  One launch per call, one workgroup per (slot of the output, band of 64 view
// rows).  A slot whose env index lies outside the batch is zero-filled.
#include "xwb_common.h"
#include "xw_device.h"
#include "xw_ego_cells.h"

namespace xwb {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 px4_t __attribute__((aligned(4)));                               // four B,G,R pixels: twelve bytes at a dword boundary

constexpr int VIEW_BS = 256;

// the env of output slot `slot`, -1: not an env of this batch
__device__ __forceinline__ int view_env(const XwParams &p, const int32_t *envs, int slot) {
    const int e = envs ? envs[slot] : slot;
    return (unsigned)e < (unsigned)p.n ? e : -1;
}

}  // namespace

// src: PACK_SRC_* -- the same selection as xw_pack_grids_kernel (kernels_xworld.hip)
__global__ __launch_bounds__(VIEW_BS) void xw_view_full_kernel(XwParams p, int src, const int32_t *envs, const u32x4 *atlas3, u32x4 *out) {
    const int D = p.max_dim, cells = D * D, tid = threadIdx.x;
    const unsigned slot = blockIdx.x / (unsigned)D, cy = blockIdx.x - slot * (unsigned)D;
    const int row_pieces = 12 * D, band_pieces = 64 * row_pieces;               // pieces of one frame row, of this band
    const int e = view_env(p, envs, (int)slot);
    u32x4 *dst = out + (size_t)blockIdx.x * band_pieces;
    if (e < 0) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (int t = tid; t < band_pieces; t += VIEW_BS) __builtin_nontemporal_store(zero, dst + t);
        return;
    }
    __shared__ uint32_t s_entry[XW_MAX_DIM];                                    // atlas entry of each cell of this cell row
    if (tid < D) {
        const bool term = xw_frame_is_term(p, src, e);
        const size_t gi = (size_t)e * cells + cy * (unsigned)D + tid;
        s_entry[tid] = xw_frame_code(p, term, gi) * (64u * 12u);
    }
    __syncthreads();
    // piece t of the band: pixel row t / row_pieces, piece j = t % row_pieces of that row (advanced without a division)
    const int dj = VIEW_BS % row_pieces, dr = VIEW_BS / row_pieces;
    int py = tid / row_pieces, j = tid - py * row_pieces;
    for (int t = tid; t < band_pieces; t += VIEW_BS) {
        const int cx = (j * 171) >> 11, sub = j - cx * 12;                      // j / 12, exact for j < 192
        const u32x4 v = atlas3[s_entry[cx] + py * 12 + sub];
        __builtin_nontemporal_store(v, dst + t);
        j += dj; py += dr;
        if (j >= row_pieces) { j -= row_pieces; py += 1; }
    }
}

__global__ __launch_bounds__(VIEW_BS) void xw_view_ego_kernel(XwParams p, const int32_t *envs, const uint32_t *atlas4, uint32_t *out) {
    const int r = p.visible_radius, S = 64 * r, D = p.max_dim, cells = D * D, tid = threadIdx.x;
    const int row_quads = 16 * r, band_quads = 64 * row_quads;                  // groups of four pixels
    const unsigned slot = blockIdx.x / (unsigned)r, band = blockIdx.x - slot * (unsigned)r;
    const int e = view_env(p, envs, (int)slot);
    uint32_t *dst = out + (size_t)blockIdx.x * band_quads * 3;
    if (e < 0) {
        const u32x3 zero = {0u, 0u, 0u};
        for (int t = tid; t < band_quads; t += VIEW_BS) __builtin_nontemporal_store(zero, reinterpret_cast<px4_t *>(dst + 3 * t));
        return;
    }
    __shared__ EgoCell s_cells[XW_MAX_DIM * XW_MAX_DIM];
    __shared__ uint16_t s_code[XW_MAX_DIM * XW_MAX_DIM];
    __shared__ uint8_t s_type[XW_MAX_DIM * XW_MAX_DIM], s_shadow[XW_MAX_DIM * XW_MAX_DIM], s_ray[XW_MAX_DIM], s_gc[XW_MAX_GOALS];
    const int dir = p.agent_dir[e] & 3;
    if (tid < 64) {                                                             // the cell table: one wavefront (xw_ego_cells.h)
        const int axy = p.agent_xy[e], ax = axy & 0xffff, ay = axy >> 16;
        for (int c = tid; c < cells; c += 64) {
            const int code = p.grid[(size_t)e * cells + c] & CELL_ICON_MASK;
            s_code[c] = (uint16_t)code;
            s_type[c] = code ? p.icon_type[code - 1] : (uint8_t)3;
        }
        if (tid < XW_MAX_GOALS) s_gc[tid] = p.goal_cells[(size_t)e * XW_MAX_GOALS + tid];
        if (tid < r) s_ray[tid] = 1;
        auto is_block = [&](int x, int y) { return (unsigned)x < (unsigned)D && (unsigned)y < (unsigned)D && s_type[y * D + x] == 1; };
        const EgoWindow win = ego_image_masking(r, ax, ay, dir, tid, s_ray, s_shadow, is_block);
        const uint32_t *gimg = p.goal_img + (size_t)e * p.num_goals * 4096;
        for (int k = tid; k < r * r; k += 64) {
            int slot;
            s_cells[k] = ego_window_cell(p, atlas4, p.icon_type, p.ego_agent_rot, s_code, s_type, s_shadow, s_gc, gimg, win, k, dir, &slot);
        }
    }
    __syncthreads();
    const uint32_t *black = atlas4 + (size_t)p.n_icons * 4096 + 1;
    typedef const uint32_t __attribute__((address_space(1))) *global_u32;       // (pointers out of LDS: say they are global)
    const int dq = VIEW_BS % row_quads, dr = VIEW_BS / row_quads;
    int vr = tid / row_quads, q = tid - vr * row_quads;
    vr += 64 * (int)band;
    for (int t = tid; t < band_quads; t += VIEW_BS) {
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int sx, sy;
            ego_view_source(dir, S, vr, 4 * q + i, &sx, &sy);
            const bool inview = (unsigned)sx < (unsigned)S && (unsigned)sy < (unsigned)S;
            const EgoCell cell = s_cells[inview ? (sy >> 6) * r + (sx >> 6) : 0];
            const uint32_t *src = inview ? cell.img + ((((sy & 63) << 6) | (sx & 63)) & cell.mask) : black;
            v[i] = *(global_u32)src;
        }
        // B,G,R,0 x 4 -> twelve bytes
        const u32x3 o = {(v[0] & 0xffffffu) | v[1] << 24, ((v[1] >> 8) & 0xffffu) | v[2] << 16, ((v[2] >> 16) & 0xffu) | v[3] << 8};
        __builtin_nontemporal_store(o, reinterpret_cast<px4_t *>(dst + 3 * t));
        q += dq; vr += dr;
        if (q >= row_quads) { q -= row_quads; vr += 1; }
    }
}

hipError_t launch_xw_view(const XwParams &p, int src, const int32_t *envs, int n, const void *view_atlas, void *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (p.visible_radius) {
        hipLaunchKernelGGL(xw_view_ego_kernel, dim3((unsigned)p.visible_radius * (unsigned)n), dim3(VIEW_BS), 0, s, p, envs,
                           reinterpret_cast<const uint32_t *>(p.atlas64), static_cast<uint32_t *>(out));
    } else {
        hipLaunchKernelGGL(xw_view_full_kernel, dim3((unsigned)p.max_dim * (unsigned)n), dim3(VIEW_BS), 0, s, p, src, envs,
                           static_cast<const u32x4 *>(view_atlas), static_cast<u32x4 *>(out));
    }
    return hipGetLastError();
}

}  // namespace xwb
