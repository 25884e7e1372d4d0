// xworld_amd/csrc/kernels_xworld_ego.hip -- the egocentric observation of XWorld2D (FLAGS_visible_radius = r > 0): the render
// with ONE WORKGROUP PER ENV, and launch_xw_render_ego, the entry point that chooses between it and the span path.
//
// xw_ego_pixel.h has the reference pipeline and the pixel routine both renders share.  Here (round 1's kernel; the fallback for
// r = 1 and r >= 9, and what the span path, kernels_xworld_ego_span.hip, is tested against) a workgroup assembles its env's
// frame in LDS: interior pixels copied from table frames "every cell shows icon i" (xw_ego_build_tab_kernel), border pixels and
// goal cells evaluated, goal cells kept in a per-env cache.
#include "xw_ego_pixel.h"

namespace xwb {

#ifdef XWB_EGO_PROF
__device__ unsigned long long g_ego_prof[12];      // stage stamps of xw_render_ego_kernel; 8-10: goal cells, misses, frames with goals
#define EGO_T0() unsigned long long t_last = wall_clock64()
#define EGO_T(i) do { if (tid == 0) { const unsigned long long now = wall_clock64(); atomicAdd(&g_ego_prof[i], now - t_last); t_last = now; } } while (0)
#else
#define EGO_T0()
#define EGO_T(i)
#endif

namespace {

// The pixels that are evaluated one by one: FAST: every pixel of the border rows, of the border columns, and of the
// cells that show a goal (goal_k: their view-cell ids); otherwise every pixel of the frame.
template <int CH, int DIR, int BS, bool FAST>
__device__ __forceinline__ void ego_pixels(const EgoCtx &c, const EgoTap (*s_row)[3], const EgoTap (*s_col)[3],
                                           uint8_t *s_frame, int O, int tid, const EgoLayout &l, const uint8_t *goal_k, int n_goal) {
    const float inv_O = __builtin_amdgcn_rcpf((float)O);         // 1 ulp: far inside ego_div's margin
    if (!FAST) {
        for (int i = tid; i < O * O; i += BS) {
            const int oy = ego_div(i, inv_O);
            ego_pixel<CH, DIR, false>(c, s_row, s_col, s_frame, O * O, i, i - oy * O, oy, 0);
        }
        return;
    }
    const int cw2 = l.cw * l.cw, n_row_px = l.nbr * O, n_border_px = n_row_px + l.nbc * O;
    const float inv_cw = __builtin_amdgcn_rcpf((float)l.cw), inv_cw2 = __builtin_amdgcn_rcpf((float)cw2);
    // border rows and columns: any of the sixteen view pixels may belong to another cell, or to none
    for (int i = tid; i < n_border_px; i += BS) {
        int ox, oy;
        bool ok = true;
        if (i < n_row_px) {
            const int q = ego_div(i, inv_O);
            oy = l.br[q]; ox = i - q * O;
        } else {
            const int j = i - n_row_px, q = ego_div(j, inv_O);
            ox = l.bc[q]; oy = j - q * O;
            ok = !(l.rt[oy] & EGO_BORDER);                      // already done with its row
        }
        if (ok) ego_pixel<CH, DIR, false>(c, s_row, s_col, s_frame, O * O, oy * O + ox, ox, oy, 0);
    }
    // goal cells: interior pixels only
    for (int j = tid; j < n_goal * cw2; j += BS) {
        const int g = ego_div(j, inv_cw2), jj = j - g * cw2, k = goal_k[g];
        const uint16_t *rc = l.rect + 4 * k;
        const int py = ego_div(jj, inv_cw), px = jj - py * l.cw;
        bool ok = px < (int)rc[2] && py < (int)rc[3];
        const int ox = ok ? (int)rc[0] + px : 0, oy = ok ? (int)rc[1] + py : 0;
        const uint32_t fl = (uint32_t)l.rt[oy] | (uint32_t)l.ct[ox];
        ok = ok && !(fl & EGO_BORDER);
        if (ok) {
            if (fl & EGO_EDGE) ego_pixel<CH, DIR, false>(c, s_row, s_col, s_frame, O * O, oy * O + ox, ox, oy, 0);   // some taps are outside the view
            else ego_pixel<CH, DIR, true>(c, s_row, s_col, s_frame, O * O, oy * O + ox, ox, oy, k);
        }
    }
}

template <int CH, int BS, bool FAST>
__device__ __forceinline__ void ego_pixels_dir(int dir, const EgoCtx &ctx, const EgoTap (*s_row)[3], const EgoTap (*s_col)[3],
                                               uint8_t *s_frame, int O, int tid, const EgoLayout &l, const uint8_t *goal_k, int n_goal) {
    switch (dir) {
        case 0: ego_pixels<CH, 0, BS, FAST>(ctx, s_row, s_col, s_frame, O, tid, l, goal_k, n_goal); break;
        case 1: ego_pixels<CH, 1, BS, FAST>(ctx, s_row, s_col, s_frame, O, tid, l, goal_k, n_goal); break;
        case 2: ego_pixels<CH, 2, BS, FAST>(ctx, s_row, s_col, s_frame, O, tid, l, goal_k, n_goal); break;
        default: ego_pixels<CH, 3, BS, FAST>(ctx, s_row, s_col, s_frame, O, tid, l, goal_k, n_goal); break;
    }
}

// Interior pixels are copied from the table frame of the view cell they fall into.  The unit is a column segment: the
// dwords of one frame row (and plane) that show the same cell column -- 28 bytes at r = 3 -- fetched with dwordx4 / x3 /
// x2 loads (global loads only need dword alignment) instead of one gather per dword: 3.5 x fewer load instructions, which
// is what this phase is bound by (it was 44 % of the kernel).  All loads of an item are issued before its LDS writes;
// pixels of border rows / columns and of goal cells get whatever the table holds there and are overwritten by ego_pixels.
template <int CH, int BS>
__device__ __forceinline__ void ego_copy_interior(const EgoCell *s_cells, const EgoLayout &l, const uint8_t *tab, uint32_t frame_bytes,
                                                  uint8_t *s_frame, int O, int tid) {
    const int nseg = l.nseg, per_plane = O * nseg, items = CH * per_plane, rowd = O >> 2;
    const float inv_pp = __builtin_amdgcn_rcpf((float)per_plane), inv_ns = __builtin_amdgcn_rcpf((float)nseg);
    uint32_t *f32 = reinterpret_cast<uint32_t *>(s_frame);
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const unsigned int __attribute__((address_space(1))) *g_u32;
    typedef const u32x2 __attribute__((address_space(1))) *g_u32x2;
    typedef const u32x4 __attribute__((address_space(1))) *g_u32x4;
    for (int it = tid; it < items; it += BS) {
        const int ch = ego_div(it, inv_pp), rem = it - ch * per_plane;
        const int oy = ego_div(rem, inv_ns), sg = rem - oy * nseg;
        const int x4 = l.seg[3 * sg], ndw = l.seg[3 * sg + 1], cterm = l.seg[3 * sg + 2];
        const int cell = (int)(l.rt[oy] & EGO_TERM) + cterm;
        const int t = s_cells[cell].tab;
        const int d0 = ch * (O * rowd) + oy * rowd + x4;                      // dword index in the planar frame
        const uint8_t *src = tab + (uint32_t)(t < 0 ? 0 : t) * frame_bytes + 4u * (uint32_t)d0;
        u32x4 q[6];
#pragma unroll
        for (int pc = 0; pc < 6; ++pc) {
            const int left = ndw - 4 * pc;
            q[pc] = (u32x4)(0u);
            if (left >= 4) q[pc] = *(g_u32x4)(src + 16 * pc);
            else if (left == 3) { const u32x2 a = *(g_u32x2)(src + 16 * pc); q[pc].x = a.x; q[pc].y = a.y; q[pc].z = *(g_u32)(src + 16 * pc + 8); }
            else if (left == 2) { const u32x2 a = *(g_u32x2)(src + 16 * pc); q[pc].x = a.x; q[pc].y = a.y; }
            else if (left == 1) q[pc].x = *(g_u32)(src + 16 * pc);
        }
#pragma unroll
        for (int pc = 0; pc < 6; ++pc) {
            const int left = ndw - 4 * pc;
            if (left >= 1) f32[d0 + 4 * pc] = q[pc].x;
            if (left >= 2) f32[d0 + 4 * pc + 1] = q[pc].y;
            if (left >= 3) f32[d0 + 4 * pc + 2] = q[pc].z;
            if (left >= 4) f32[d0 + 4 * pc + 3] = q[pc].w;
        }
    }
}

}  // namespace

// The interior-pixel table: frame (slot, heading) = the frame of a view whose every cell shows slot's image; slots
// 0 .. n_icons - 1 = the icons, n_icons = an empty (white) cell, n_icons + 1 = a black cell.  One workgroup per frame.
template <int CH>
__global__ __launch_bounds__(256) void xw_ego_build_tab_kernel(XwParams p, const uint32_t *atlas4, const EgoTap *tap_h1,
                                                               const EgoTap *tap_v1, const EgoTap *tap_h2, const EgoTap *tap_v2,
                                                               uint8_t *tab, size_t frame_bytes) {
    extern __shared__ uint4 smem4[];
    const int r = p.visible_radius, O = p.out_dim;
    uint8_t *s_frame = reinterpret_cast<uint8_t *>(smem4);
    EgoCell *s_cells = reinterpret_cast<EgoCell *>(s_frame + ((CH * O * O + 15) & ~15));
    __shared__ EgoTap s_row[84][3], s_col[84][3];
    const int tid = threadIdx.x, slot = blockIdx.x >> 2, dir = blockIdx.x & 3;
    ego_compose_taps(s_row, s_col, tap_h1, tap_v1, tap_h2, tap_v2, O, tid, 256);
    const uint32_t *white = atlas4 + (size_t)p.n_icons * 4096, *black = white + 1;
    EgoCell c{slot == p.n_icons ? white : black, 0, -1};
    if (slot < p.n_icons) c = ego_icon_cell(p.icon_type, p.ego_agent_rot, atlas4, slot, dir);
    for (int k = tid; k < r * r; k += 256) s_cells[k] = c;
    __syncthreads();
    EgoCtx ctx{s_cells, white, black, r, 64 * r};
    ego_pixels_dir<CH, 256, false>(dir, ctx, s_row, s_col, s_frame, O, tid, EgoLayout{}, nullptr, 0);
    __syncthreads();
    uint8_t *out = tab + (size_t)blockIdx.x * frame_bytes;
    for (int i = tid; i < CH * O * O; i += 256) out[i] = s_frame[i];
}

// MODE 0: every env; 1: the compacted done list; 2: every env the last step did not finish (the rest is drawn from the list)
// BS threads per workgroup: 256 for the whole batch; 1024 for the short done list, where the latency of one env counts
// FAST: frame rows are whole dwords and cell boundaries fall on dwords (r <= 7): interior pixels are copied from the
// table and frames leave as 16-byte chunks.  Otherwise (r >= 9: 81, 77, 78, 75 pixel edges) every pixel is evaluated
// and frames leave element by element -- their byte size is not a multiple of 16.
template <int CH, int MODE, int BS, bool FAST>
__global__ __launch_bounds__(BS, 4) void xw_render_ego_kernel(XwParams p, const uint32_t *atlas4, const EgoTap *tap_h1,
                                                            const EgoTap *tap_v1, const EgoTap *tap_h2, const EgoTap *tap_v2,
                                                            const uint16_t *layout, const uint8_t *tab,
                                                            const int32_t *count_now) {
    extern __shared__ uint4 smem4[];
    const int r = p.visible_radius, S = 64 * r, D = p.max_dim, O = p.out_dim, O4 = (O + 3) & ~3;
    const uint32_t frame_bytes = (uint32_t)((CH * O * O + 15) & ~15);
    const int lw = ego_layout_words(O4, r);
    uint8_t *s_frame = reinterpret_cast<uint8_t *>(smem4);                       // CH * O * O, planar
    EgoCell *s_cells = reinterpret_cast<EgoCell *>(s_frame + frame_bytes);
    uint16_t *s_layout = reinterpret_cast<uint16_t *>(s_cells + r * r);          // FAST: the four headings' layout tables
    uint32_t *s_rot = reinterpret_cast<uint32_t *>(s_layout + (FAST ? 4 * lw : 0));   // [n_icons] ego_agent_rot
    uint8_t *s_itype = reinterpret_cast<uint8_t *>(s_rot + p.n_icons);           // [n_icons] icon_type
    uint8_t *s_type = s_itype + ((p.n_icons + 3) & ~3);                          // [D * D] type of the entity in a cell, 3 = none
    uint8_t *s_shadow = s_type + ((D * D + 3) & ~3);
    uint8_t *s_ray = s_shadow + ((r * r + 3) & ~3);
    uint8_t *s_gc = s_ray + ((r + 3) & ~3);
    uint8_t *s_goal_k = s_gc + XW_MAX_GOALS;                                     // [XW_MAX_GOALS] view cells that show a goal
    uint8_t *s_goal_slot = s_goal_k + XW_MAX_GOALS;                              // [XW_MAX_GOALS] their goal slots
    uint8_t *s_miss_k = s_goal_slot + XW_MAX_GOALS;                              // [XW_MAX_GOALS] those not in the cache yet
    uint8_t *s_miss_slot = s_miss_k + XW_MAX_GOALS;
    // composed taps of one output row / column: the two intermediate indices' taps and the output tap (static: O <= 84)
    __shared__ EgoTap s_row[84][3], s_col[84][3];
    __shared__ uint16_t s_code[XW_MAX_DIM * XW_MAX_DIM];                         // the env's grid, target bit stripped
    __shared__ int s_ngoal, s_nmiss;
    __shared__ uint32_t s_valid[64];                                             // the env's cache bits (ego_cache_words <= 64)
    const int tid = threadIdx.x;
    const int n_items = MODE == 1 ? *count_now : p.n;
    if ((int)blockIdx.x >= n_items) return;                    // the done list is short: most of its workgroups leave here
    ego_compose_taps(s_row, s_col, tap_h1, tap_v1, tap_h2, tap_v2, O, tid, BS);
    for (int i = tid; i < p.n_icons; i += BS) { s_itype[i] = p.icon_type[i]; s_rot[i] = p.ego_agent_rot[i]; }
    if (FAST) for (int i = tid; i < 4 * lw; i += BS) s_layout[i] = layout[i];
    const int cells = D * D;
    // Everything the env's setup reads from global memory is fetched one env ahead and staged in LDS, so the serial part
    // -- shadow rays, scan lines, cell table -- never waits for HBM / L2.  The setup is the first wavefront's job alone
    // (its lanes hold the grid: cells <= 256 = 4 per lane): it is scalar-heavy code that every wavefront would otherwise
    // repeat, and inside one wavefront its phases need no workgroup barrier (LDS operations of a wave complete in order).
    constexpr int CPL = XW_MAX_DIM * XW_MAX_DIM / 64;           // grid cells per lane of the first wavefront
    const bool wave0 = tid < 64;
    struct Fetch { int e, axy, dir, skip; uint32_t code[CPL], gc, valid; };
    auto fetch = [&](int item) {
        Fetch f;
        f.e = MODE == 1 ? p.done_list[item] : item;
        f.skip = MODE == 2 ? (int)p.term_flag[f.e] : 0;      // finished by this step: drawn from the list instead
        f.axy = p.agent_xy[f.e]; f.dir = p.agent_dir[f.e];
#pragma unroll
        for (int k = 0; k < CPL; ++k) f.code[k] = wave0 && tid + 64 * k < cells ? (uint32_t)p.grid[(size_t)f.e * cells + tid + 64 * k] : 0u;
        f.gc = tid < XW_MAX_GOALS ? (uint32_t)p.goal_cells[(size_t)f.e * XW_MAX_GOALS + tid] : 0xffu;
        // the env's goal-cell cache bits, lane i = word i (fetched with the rest, one env ahead: the look-up never waits)
        f.valid = (FAST && p.ego_cache_valid && tid < (int)p.ego_cache_words && tid < 64) ? p.ego_cache_valid[(size_t)f.e * p.ego_cache_words + tid] : 0u;
        return f;
    };
    Fetch nxt{};
    if ((int)blockIdx.x < n_items) nxt = fetch(blockIdx.x);
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const Fetch f = nxt;
        const int e = f.e, ax = f.axy & 0xffff, ay = f.axy >> 16, dir = f.dir;
        __syncthreads();                                        // the previous env's frame has left LDS
        EGO_T0();
        if (wave0) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int c = tid + 64 * k;
                if (c < cells) {
                    const int code = (int)(f.code[k] & CELL_ICON_MASK);
                    s_code[c] = (uint16_t)code;
                    s_type[c] = code ? s_itype[code - 1] : (uint8_t)3;
                }
            }
            if (tid < XW_MAX_GOALS) s_gc[tid] = (uint8_t)f.gc;
            if (FAST && tid < (int)p.ego_cache_words) s_valid[tid] = f.valid;
            if (tid < r) s_ray[tid] = 1;
            if (tid == 0) s_ngoal = 0;
        }
        if (item + (int)gridDim.x < n_items) nxt = fetch(item + gridDim.x);
        if (f.skip) continue;
        EgoLayout lay{};
        if (FAST) lay = ego_layout(s_layout + dir * lw, O4, r);
        const uint32_t *white = atlas4 + (size_t)p.n_icons * 4096, *black = white + 1;
        if (wave0) {
            auto is_block = [&](int x, int y) {
                return (unsigned)x < (unsigned)D && (unsigned)y < (unsigned)D && s_type[y * D + x] == 1;
            };
            const EgoWindow win = ego_image_masking(r, ax, ay, dir, tid, s_ray, s_shadow, is_block);
            const uint32_t *gimg = p.goal_img + (size_t)e * p.num_goals * 4096;
            for (int k = tid; k < r * r; k += 64) {             // what each view cell shows
                int slot;
                const EgoCell c = ego_window_cell(p, atlas4, s_itype, s_rot, s_code, s_type, s_shadow, s_gc, gimg, win, k, dir, &slot);
                if (FAST && slot >= 0) { const int j = atomicAdd(&s_ngoal, 1); s_goal_k[j] = (uint8_t)k; s_goal_slot[j] = (uint8_t)slot; }
                s_cells[k] = c;
            }
        }
        __syncthreads();
        EGO_T(3);
        EgoCtx ctx{s_cells, white, black, r, S};
        if (FAST) {
            ego_copy_interior<CH, BS>(s_cells, lay, tab, frame_bytes, s_frame, O, tid);
            __syncthreads();
            EGO_T(4);
        }
        const uint8_t *eval_k = s_goal_k;
        int n_eval = s_ngoal;
        // (four frames in five show no goal at all: nothing to look up, nothing to evaluate, no barrier)
        const bool cached = FAST && p.ego_cache != nullptr && p.ego_cellinfo == nullptr && s_ngoal > 0;   // (the span path keeps another entry layout)
        uint8_t *cache_env = nullptr;
        uint32_t *valid_env = nullptr;
        if (cached) {
            // goal cells: copy the ones this env has already rendered in this place and heading, evaluate the rest (and keep them)
            cache_env = p.ego_cache + (size_t)e * p.num_goals * (r * r * 4) * p.ego_cache_entry;
            valid_env = p.ego_cache_valid + (size_t)e * p.ego_cache_words;
            if (tid == 0) {
                int nm = 0;
                for (int j = 0; j < s_ngoal; ++j) {
                    const int bit = (s_goal_slot[j] * r * r + s_goal_k[j]) * 4 + dir;
                    if (!((s_valid[bit >> 5] >> (bit & 31)) & 1u)) { s_miss_k[nm] = s_goal_k[j]; s_miss_slot[nm] = s_goal_slot[j]; nm++; s_goal_k[j] = 0xff; }
                }
                s_nmiss = nm;
            }
            __syncthreads();
            for (int j = 0; j < s_ngoal; ++j) {
                const int k = s_goal_k[j];
                if (k == 0xff) continue;                                 // a miss
                const uint16_t *rc = lay.rect + 4 * k;
                const int x0 = rc[0], y0 = rc[1], w = rc[2], h = rc[3], wh = w * h;
                const uint8_t *src = cache_env + (size_t)((s_goal_slot[j] * r * r + k) * 4 + dir) * p.ego_cache_entry;
                for (int i = tid; i < wh * CH; i += BS) {
                    const int ch = i / wh, rem = i - ch * wh, py = rem / w, px = rem - py * w;
                    s_frame[ch * O * O + (y0 + py) * O + x0 + px] = src[i];
                }
            }
            eval_k = s_miss_k;
            n_eval = s_nmiss;
#ifdef XWB_EGO_PROF
            if (tid == 0) { atomicAdd(&g_ego_prof[8], (unsigned long long)s_ngoal); atomicAdd(&g_ego_prof[9], (unsigned long long)s_nmiss); atomicAdd(&g_ego_prof[10], 1ull); }
#endif
        }
        ego_pixels_dir<CH, BS, FAST>(dir, ctx, s_row, s_col, s_frame, O, tid, lay, eval_k, n_eval);
        __syncthreads();
        if (cached && n_eval > 0) {
            for (int j = 0; j < n_eval; ++j) {
                const int k = s_miss_k[j];
                const uint16_t *rc = lay.rect + 4 * k;
                const int x0 = rc[0], y0 = rc[1], w = rc[2], h = rc[3], wh = w * h;
                const int entry = (s_miss_slot[j] * r * r + k) * 4 + dir;
                uint8_t *dst = cache_env + (size_t)entry * p.ego_cache_entry;
                for (int i = tid; i < wh * CH; i += BS) {
                    const int ch = i / wh, rem = i - ch * wh, py = rem / w, px = rem - py * w;
                    dst[i] = s_frame[ch * O * O + (y0 + py) * O + x0 + px];
                }
                if (tid == 0) atomicOr(valid_env + (entry >> 5), 1u << (entry & 31));
            }
        }
        EGO_T(5);
        const int flag = p.context > 1 ? (MODE == 1 ? p.list_flag : (int)p.fresh[e]) : 1;
        const float scale = (float)(1 / 255.0);   // float32 frames: pixel * (1 / 255.0f), the product py_simulator.cpp:262-272 computes
        if (FAST) {
            const int cpf = CH * O * O / (p.obs_f32 ? 4 : 16);  // 16-byte chunks per frame: 16 uint8 pixels, or 4 float32 ones
            uint4 *frame0 = reinterpret_cast<uint4 *>(p.obs) + (size_t)e * p.context * cpf;
            if (p.obs_f32) {
                for (int cc = tid; cc < cpf; cc += BS) {
                    const uchar4 b = reinterpret_cast<const uchar4 *>(s_frame)[cc];
                    const float f0 = (float)b.x * scale, f1 = (float)b.y * scale, f2 = (float)b.z * scale, f3 = (float)b.w * scale;
                    xw_store_chunk(frame0, cc, cpf, p.context, flag,
                                   make_uint4(__float_as_uint(f0), __float_as_uint(f1), __float_as_uint(f2), __float_as_uint(f3)));
                }
            } else {
                for (int cc = tid; cc < cpf; cc += BS) xw_store_chunk(frame0, cc, cpf, p.context, flag, smem4[cc]);
            }
        } else if (flag != 0) {
            // shift_context / init_screen element by element (simulator.cpp:36-85)
            const int F = CH * O * O, ctxn = p.context;
            if (p.obs_f32) {
                float *q = reinterpret_cast<float *>(p.obs) + (size_t)e * ctxn * F;
                for (int i = tid; i < F; i += BS) {
                    for (int f = 0; f + 1 < ctxn; ++f) q[(size_t)f * F + i] = flag == 2 ? 0.f : q[(size_t)(f + 1) * F + i];
                    q[(size_t)(ctxn - 1) * F + i] = (float)s_frame[i] * scale;
                }
            } else {
                uint8_t *q = p.obs + (size_t)e * ctxn * F;
                for (int i = tid; i < F; i += BS) {
                    for (int f = 0; f + 1 < ctxn; ++f) q[(size_t)f * F + i] = flag == 2 ? (uint8_t)0 : q[(size_t)(f + 1) * F + i];
                    q[(size_t)(ctxn - 1) * F + i] = s_frame[i];
                }
            }
        }
        EGO_T(6);
        if (MODE == 1 && tid == 0 && p.list_flag == 2) { p.fresh[e] = 0; if (p.auto_reset == AUTO_RESET_BY_LIST) p.done[e] = 0; }
    }
}


// ------------------------------------------------------------------------------------------------- host side ----
static size_t ego_frame_bytes(const XwParams &p) { return (size_t)((p.channels * p.out_dim * p.out_dim + 15) & ~15); }

// bytes of one cache entry: the largest cell rectangle of any heading, all channels
size_t xw_ego_cache_entry_bytes(const XwParams &p, int cell_edge) { return (size_t)((cell_edge * cell_edge * p.channels + 15) & ~15); }

size_t xw_ego_tab_bytes(const XwParams &p) { return (size_t)(p.n_icons + 2) * 4 * ego_frame_bytes(p); }

// fills p.ego_tab (xw_ego_tab_bytes) -- once per batch, after the atlas and the taps are on the device
hipError_t launch_xw_ego_build_tab(const XwParams &p, hipStream_t s) {
    const EgoTables t = ego_tables_of(p);
    const int r = p.visible_radius;
    const size_t fb = ego_frame_bytes(p), lds = fb + (size_t)r * r * sizeof(EgoCell);
    const unsigned blocks = (unsigned)(p.n_icons + 2) * 4;
    const uint32_t *a4 = reinterpret_cast<const uint32_t *>(p.atlas64);
    uint8_t *tab = const_cast<uint8_t *>(p.ego_tab);
    ego_with_channels(p.channels, [&](auto ch) {
        hipLaunchKernelGGL((xw_ego_build_tab_kernel<decltype(ch)::value>), dim3(blocks), dim3(256), lds, s, p, a4, t.h1, t.v1, t.h2, t.v2, tab, fb);
    });
    return hipGetLastError();
}

hipError_t launch_xw_render_ego(const XwParams &p, RenderMode mode, hipStream_t s, hipEvent_t ev_front, hipEvent_t ev_list, hipEvent_t ev_cells) {
    // the span path, where the geometry allows: the whole batch / a step's frames, or the done list (whole or in parts:
    // xwb_reset_done runs the parts on two queues)
    const bool list_mode = mode == RENDER_LIST || mode > RENDER_SPAN_STEP;
    if (!list_mode && xw_ego_span(p)) return launch_xw_ego_span_render(p, mode, s, ev_front, ev_list, ev_cells);
    if (list_mode && xw_ego_span(p) && p.ego_cellsrc_list) return launch_xw_ego_span_render_list(p, mode, s);
    if (mode >= RENDER_SPAN_STEP) return hipErrorInvalidValue;   // (only the span path draws a step's terminal frames itself)
    const EgoTables t = ego_tables_of(p);
    const int r = p.visible_radius, O = p.out_dim, O4 = (O + 3) & ~3, D = p.max_dim;
    const bool fast = p.ego_fast != 0;
    const size_t lds = ego_frame_bytes(p) + (size_t)r * r * sizeof(EgoCell) + (fast ? (size_t)ego_layout_words(O4, r) * 8 : 0) +
                       (size_t)p.n_icons * 4 + (size_t)((p.n_icons + 3) & ~3) + (size_t)((D * D + 3) & ~3) +
                       (size_t)((r * r + 3) & ~3) + (size_t)((r + 3) & ~3) + 5 * XW_MAX_GOALS + 16;
    // whole batch: looping workgroups, each with its next env's state in flight, so the per-workgroup prologue (taps and
    // layout tables -> LDS) is amortised; 8192 of them rather than the 1024 that are resident at once: a shorter tail, and
    // a reset_done running on the side stream finds free slots (MI355X, C4 batch: 0.518 ms per step with 1024, 0.494 with 8192)
    const bool list = mode == RENDER_LIST;
    const unsigned blocks = list ? 2048u : (unsigned)(p.n < 8192 ? p.n : 8192);
    const int32_t *cnt = (const int32_t *)p.done_count;
    const uint32_t *a4 = reinterpret_cast<const uint32_t *>(p.atlas64);
    ego_with_channels(p.channels, [&](auto ch) {
        ego_with_bool(fast, [&](auto fast_c) {
            // the kernel's MODE (0: every env, 1: the done list, 2: the envs the last step did not finish) and workgroup size
            auto launch = [&](auto kmode, auto bs) {
                constexpr int CH = decltype(ch)::value, MODE = decltype(kmode)::value, BS = decltype(bs)::value;
                hipLaunchKernelGGL((xw_render_ego_kernel<CH, MODE, BS, decltype(fast_c)::value>), dim3(blocks), dim3(BS), lds, s, p, a4,
                                   t.h1, t.v1, t.h2, t.v2, t.lut, p.ego_tab, cnt);
            };
            if (list && p.ego_list_beside) launch(ego_int<1>{}, ego_int<256>{});
            else if (list) launch(ego_int<1>{}, ego_int<1024>{});
            else if (mode == RENDER_ALIVE) launch(ego_int<2>{}, ego_int<256>{});
            else launch(ego_int<0>{}, ego_int<256>{});
        });
    });
    return hipGetLastError();
}

}  // namespace xwb

#ifdef XWB_EGO_PROF
extern "C" __attribute__((visibility("default"))) int xwb_debug_ego_prof(unsigned long long *out) {
    unsigned long long z[12] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(xwb::g_ego_prof), sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(xwb::g_ego_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
