// xw_ego_pixel.h -- the egocentric observation of XWorld2D (FLAGS_visible_radius = r > 0): the pixel routine and the
// tables (resize taps, per-heading layouts, square maps) that both of its renders share, and nothing else.
//
// Reference pipeline, per env and per call (all on 8-bit BGR images):
//   XMap::to_image            xmap.cpp:125-206    world canvas from 64x64 item images, r cells of black padding, crop of
//                                                 the r x r cells in front of the agent, wall shadows (image_masking,
//                                                 :273-362) painted black, rotation by 90 + yaw degrees (cv::warpAffine)
//   XItem::get_item_image     xitem.cpp:33-63     every item image is warped by its own (yaw, scale, offset)
//   get_screen_rgb            xworld_simulator.cpp:287-307   cv::resize of the (64 r)^2 view to the (64 max_dim)^2 canvas size
//   down_sample_image         :508-545            cv::resize to (r * (84 / r))^2, optional BGR2GRAY, planar output
// Nothing here is materialised except the final frame: every output pixel is the fixed-point bilinear blend
// (cv::resize: 11-bit coefficients, the intermediate image rounded to 8 bits exactly as OpenCV does) of 2 x 2 pixels of
// the intermediate image, each of which blends 2 x 2 view pixels; a view pixel is found by undoing the quarter-turn view
// rotation (exact integer map, one border row / column), the cell lookup, and for goals the inverse affine warp with
// cv::remap's 5-bit sub-pixel bilinear weights.  Evaluating all 84^2 pixels that way is instruction-bound (16 view pixels
// and ~400 VALU operations each), so only the pixels that need it are: an output pixel whose 4 x 4 view pixels all lie
// inside ONE view cell depends on nothing but that cell's image, its position in the frame and the heading, and for
// blocks, the agent, empty cells and black cells that image is one of a few constants.
//
// Two renders share that pixel code (both bit-exact against the oracle and against each other):
//   - the SPAN PATH (kernels_xworld_ego_span.hip; r = 3, 5, 7): cell table -> evaluated pixels -> a gather of 16-byte pieces
//     from tables of whole squares; what draws the whole batch and the done list whenever the geometry allows;
//   - ONE WORKGROUP PER ENV (kernels_xworld_ego.hip, xw_render_ego_kernel; round 1's kernel and the fallback): the frame is
//     assembled in LDS from table frames "every cell shows icon i" (xw_ego_build_tab_kernel) plus evaluated border pixels and
//     goal cells.
// launch_xw_render_ego (kernels_xworld_ego.hip) chooses between them; xwb_ego_tables.hip builds the tables on the host.
//
// OpenCV 3.2 arithmetic restated (third party, cmake/opencv.cmake:5-6; DESIGN.md lists the pieces): the tests compare
// these kernels bit for bit with a CPU restatement of the same pipeline; pixel parity with the real library is unpinned.
#pragma once
#include "xwb_common.h"
#include "xw_device.h"
#include "xw_ego_cells.h"

#include <type_traits>

namespace xwb {

struct EgoTap { int16_t s0, s1, w0, w1; };        // cv::resize: source indices and 11-bit weights of one output index

namespace {

struct EgoCtx {
    const EgoCell *cells;        // LDS, r * r
    const uint32_t *white, *black;
    int r, S;
    int dir;                     // the heading, where it is not a template argument (ego_pixel<.., -1, ..>)
};

// cv::resize INTER_LINEAR on 8-bit data, one output value: HResizeLinear (11-bit) then VResizeLinear<uchar>
__device__ __forceinline__ int vresize(int b0, int h0, int b1, int h1) {
    // operands < 2^24 and products < 2^31: v_mul_u32_u24 is exact and full rate
    return (int)((((__umul24((unsigned)b0, (unsigned)(h0 >> 4))) >> 16) + ((__umul24((unsigned)b1, (unsigned)(h1 >> 4))) >> 16) + 2u) >> 2);
}

// One output pixel.  DIR = the agent's heading: cv::warpAffine(view, rot(centre S/2, 90 + yaw deg)) is undone per tap
// row / column -- quarter turns are exact integer maps, separable in x and y; the source index S falls outside and
// leaves one black row / column (borderValue 0).
// (DIR = -1: the heading is c.dir, a run-time value -- the same arithmetic with selects, for lanes of mixed headings)
// ONE: all sixteen view pixels lie in the view cell `one` (an interior pixel of that cell, whose image is indexed: a goal)
template <int CH, int DIR, bool ONE>
__device__ __forceinline__ void ego_pixel(const EgoCtx &c, const EgoTap (*s_row)[3], const EgoTap (*s_col)[3],
                                          uint8_t *s_frame, int plane, int o, int ox, int oy, int one) {
    const int S = c.S;
    {
        // the 2 x 2 intermediate pixels this output pixel blends, and the 4 x 4 view pixels behind them
        const EgoTap ty = s_row[oy][2], tx = s_col[ox][2];
        const EgoTap my[2] = {s_row[oy][0], s_row[oy][1]}, mx[2] = {s_col[ox][0], s_col[ox][1]};
        const int R[4] = {my[0].s0, my[0].s1, my[1].s0, my[1].s1}, C[4] = {mx[0].s0, mx[0].s1, mx[1].s0, mx[1].s1};
        // source coordinate contributed by a view row (vr) and by a view column (vc):
        //   up (3): sx = vc, sy = vr;  right (0): sx = S - vr, sy = vc;  down (1): sx = S - vc, sy = S - vr;  left (2): sx = vr, sy = S - vc
        int fr[4], fc[4];                                   // coordinate from the row index, from the column index
        const int dir = DIR >= 0 ? DIR : c.dir;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fr[i] = (dir == 3 || dir == 2) ? R[i] : S - R[i];
            fc[i] = (dir == 3 || dir == 0) ? C[i] : S - C[i];
        }
        // fr is sy for headings up / down and sx for right / left (and fc the other one)
        const bool ROW_IS_Y = dir == 3 || dir == 1;
        const uint32_t *src[16];
        if (ONE) {
            const uint32_t *img = c.cells[one].img;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = k >> 2, j = k & 3;
                const int px = (ROW_IS_Y ? fc[j] : fr[i]) & 63, py = (ROW_IS_Y ? fr[i] : fc[j]) & 63;
                src[k] = img + (py * 64 + px);
            }
        } else {
            int cr[4], cc[4], pr[4], pc[4];
            bool okr[4], okc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                okr[i] = (unsigned)fr[i] < (unsigned)S; okc[i] = (unsigned)fc[i] < (unsigned)S;
                cr[i] = ROW_IS_Y ? __mul24(fr[i] >> 6, c.r) : (fr[i] >> 6);
                cc[i] = ROW_IS_Y ? (fc[i] >> 6) : __mul24(fc[i] >> 6, c.r);
                pr[i] = fr[i] & 63; pc[i] = fc[i] & 63;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = k >> 2, j = k & 3;
                const bool inview = okr[i] && okc[j];
                const EgoCell cell = c.cells[inview ? cr[i] + cc[j] : 0];
                const int px = ROW_IS_Y ? pc[j] : pr[i], py = ROW_IS_Y ? pr[i] : pc[j];
                const uint32_t *q = cell.img + ((py * 64 + px) & cell.mask);
                src[k] = inview ? q : c.black;
            }
        }
        // the descriptors come from LDS, so the compiler cannot tell these pointers are global: say so (global_load instead
        // of flat_load, which would also wait on the LDS counter)
        typedef const uint32_t __attribute__((address_space(1))) *global_u32;
        uint32_t v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = *(global_u32)src[k];
        int out[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int hB[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {                  // intermediate row a
                int A[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {              // intermediate column b
                    const int h0 = __mul24((int)((v[(2 * a) * 4 + 2 * b] >> (8 * ch)) & 255u), mx[b].w0) +
                                   __mul24((int)((v[(2 * a) * 4 + 2 * b + 1] >> (8 * ch)) & 255u), mx[b].w1);
                    const int h1 = __mul24((int)((v[(2 * a + 1) * 4 + 2 * b] >> (8 * ch)) & 255u), mx[b].w0) +
                                   __mul24((int)((v[(2 * a + 1) * 4 + 2 * b + 1] >> (8 * ch)) & 255u), mx[b].w1);
                    A[b] = vresize(my[a].w0, h0, my[a].w1, h1);
                }
                hB[a] = __mul24(A[0], tx.w0) + __mul24(A[1], tx.w1);
            }
            out[ch] = vresize(ty.w0, hB[0], ty.w1, hB[1]);
        }
        if (CH == 3) {
            s_frame[o] = (uint8_t)out[0]; s_frame[plane + o] = (uint8_t)out[1]; s_frame[2 * plane + o] = (uint8_t)out[2];
        } else {
            s_frame[o] = (uint8_t)((out[0] * 1868 + out[1] * 9617 + out[2] * 4899 + (1 << 13)) >> 14);   // cvtColor BGR2GRAY
        }
    }
}

// The per-heading layout tables (xw_ego_tables builds them; uint16 words):
//   [0, O4)            row term: the view-cell index part every interior pixel of this output row adds (cell row * r, or
//                      the cell column for the sideways headings); bit 15: the row touches a cell border or the black
//                      border the quarter turn leaves -- all of its pixels are evaluated one by one
//   [O4, 2 O4)         column term, same
//   [2 O4, 2 O4 + Q)   column term per group of four columns (cell boundaries fall on multiples of four here, else the
//                      table is not used at all), Q = O4 / 4 rounded up to a multiple of 4
//   then 4 words       number of border rows, of border columns, largest edge of a cell's pixel rectangle, 0
//   then O4, O4        the border rows, the border columns
//   then r * r * 4     per view cell: x0, y0, width, height of its interior pixels in the frame
//   then 3 * (O4 / 4)  column segments (x4 start, dwords, column term): maximal runs of dwords of a frame row that show the
//                      same view-cell column -- the unit of the interior copy; their number is the header's 4th word
// Term flags: 0x8000 = border (the taps straddle two cells: every pixel evaluated), 0x4000 = edge (some taps fall outside
// the view -- the black line the quarter turn leaves -- but the rest lie in ONE cell: still a function of that cell's image
// alone, so the table frame of that image holds the pixel; only goal cells, whose images are per env, evaluate it).
struct EgoLayout {
    const uint16_t *rt, *ct, *ct4, *br, *bc, *rect, *seg;
    int nbr, nbc, cw, nseg;
};
constexpr uint32_t EGO_BORDER = 0x8000u, EGO_EDGE = 0x4000u, EGO_TERM = 0x3fffu;
// where each array of a heading's layout table starts (words), in the order above -- the one statement of that order: the host
// writes the table through it (xw_ego_tables) and the kernels read it through it
struct EgoLayoutAt { int rt, ct, ct4, hd, br, bc, rect, seg, words; };
__host__ __device__ constexpr EgoLayoutAt ego_layout_at(int O4, int r) {
    EgoLayoutAt a{};
    a.rt = 0; a.ct = a.rt + O4; a.ct4 = a.ct + O4; a.hd = a.ct4 + ((O4 / 4 + 3) & ~3);
    a.br = a.hd + 4; a.bc = a.br + O4; a.rect = a.bc + O4; a.seg = a.rect + 4 * r * r; a.words = a.seg + 3 * (O4 / 4);
    return a;
}
__host__ __device__ constexpr int ego_layout_words(int O4, int r) { return ego_layout_at(O4, r).words; }
__device__ __forceinline__ EgoLayout ego_layout(const uint16_t *base, int O4, int r) {
    const EgoLayoutAt a = ego_layout_at(O4, r);
    EgoLayout l;
    // (each array from the one before it, not from the base: the order of the additions decides the code of the per-env kernel)
    l.rt = base + a.rt; l.ct = l.rt + (a.ct - a.rt); l.ct4 = base + a.ct4;
    const uint16_t *h = l.ct4 + (a.hd - a.ct4);
    l.nbr = h[0]; l.nbc = h[1]; l.cw = h[2]; l.nseg = h[3];
    l.br = h + (a.br - a.hd); l.bc = l.br + (a.bc - a.br); l.rect = l.bc + (a.rect - a.bc); l.seg = l.rect + (a.seg - a.rect);
    return l;
}

__device__ __forceinline__ int ego_div(int i, float inv_n) { return (int)(((float)i + 0.5f) * inv_n); }   // i / n, exact: i < 2^16, n <= 84 * 84

__device__ __forceinline__ void ego_compose_taps(EgoTap (*s_row)[3], EgoTap (*s_col)[3], const EgoTap *tap_h1, const EgoTap *tap_v1,
                                                 const EgoTap *tap_h2, const EgoTap *tap_v2, int O, int tid, int bs) {
    for (int i = tid; i < O; i += bs) {
        const EgoTap ty = tap_v2[i], tx = tap_h2[i];
        s_row[i][0] = tap_v1[ty.s0]; s_row[i][1] = tap_v1[ty.s1]; s_row[i][2] = ty;
        s_col[i][0] = tap_h1[tx.s0]; s_col[i][1] = tap_h1[tx.s1]; s_col[i][2] = tx;
    }
}

// The square maps of the span path (bytes; 0xff where the geometry rules the span path out), the frame being r x r squares of
// U = O / r pixels:
//   cell [heading][square fy * r + fx]   the view cell the square shows
//   rows [heading][fy]                   which border row (its place in the layout's list) frame row fy * U is, 0xff: none
//   cols [heading][fx]                   the same for frame column fx * U
//   inv  [heading][view cell]            the square that shows the view cell (the inverse of `cell`)
struct EgoMapAt { int cell, rows, cols, inv, used, bytes; };
__host__ __device__ constexpr EgoMapAt ego_map_at(int r) {
    EgoMapAt a{};
    a.cell = 0; a.rows = a.cell + 4 * r * r; a.cols = a.rows + 4 * r; a.inv = a.cols + 4 * r; a.used = a.inv + 4 * r * r; a.bytes = (a.used + 15) & ~15;
    return a;
}

// The one blob of tables an egocentric batch keeps on the device (XwParams::ego_taps; xw_ego_tables builds and uploads it):
//   h1, v1 [64 * max_dim]   taps of the first resize (view -> canvas size), columns and rows
//   h2, v2 [out_dim]        taps of the second (canvas size -> frame)
//   lay    [4][lay.words]   the four headings' layout tables (EgoLayout)
//   map    [map.bytes]      the square maps (EgoMapAt)
//   comp   [2][out_dim][3]  the composed taps of an output row, then of an output column (ego_compose_taps: the two
//                           intermediate indices' taps and the output tap), for kernels that want them in ONE read
// The offsets are bytes from the start of the blob.
struct EgoBlob {
    int O4;                             // the frame edge rounded up to whole dwords (what the layout tables are sized by)
    EgoLayoutAt lay;
    EgoMapAt map;
    size_t at_h1, at_v1, at_h2, at_v2, at_lay, at_map, at_comp, bytes;
};
__host__ __device__ constexpr EgoBlob ego_blob(int r, int max_dim, int out_dim) {
    EgoBlob b{};
    const size_t n1 = (size_t)64 * max_dim * sizeof(EgoTap), n2 = (size_t)out_dim * sizeof(EgoTap);
    b.O4 = (out_dim + 3) & ~3; b.lay = ego_layout_at(b.O4, r); b.map = ego_map_at(r);
    b.at_h1 = 0; b.at_v1 = b.at_h1 + n1; b.at_h2 = b.at_v1 + n1; b.at_v2 = b.at_h2 + n2; b.at_lay = b.at_v2 + n2;
    b.at_map = b.at_lay + (size_t)4 * b.lay.words * sizeof(uint16_t); b.at_comp = b.at_map + b.map.bytes; b.bytes = b.at_comp + 6 * n2;
    return b;
}

// the blob's arrays as pointers (T = uint8_t: the host's buffer while xw_ego_tables fills it; const uint8_t: a reader)
template <class T, class Tap, class U16>
struct EgoTablesOf { Tap *h1, *v1, *h2, *v2; U16 *lut; T *map; Tap *comp; };
typedef EgoTablesOf<const uint8_t, const EgoTap, const uint16_t> EgoTables;
template <class T, class Tap, class U16>
inline EgoTablesOf<T, Tap, U16> ego_tables_at(T *blob, const EgoBlob &b) {
    return {reinterpret_cast<Tap *>(blob + b.at_h1), reinterpret_cast<Tap *>(blob + b.at_v1), reinterpret_cast<Tap *>(blob + b.at_h2),
            reinterpret_cast<Tap *>(blob + b.at_v2), reinterpret_cast<U16 *>(blob + b.at_lay), blob + b.at_map,
            reinterpret_cast<Tap *>(blob + b.at_comp)};
}
inline EgoTables ego_tables_of(const XwParams &p) {
    return ego_tables_at<const uint8_t, const EgoTap, const uint16_t>(reinterpret_cast<const uint8_t *>(p.ego_taps),
                                                                    ego_blob(p.visible_radius, p.max_dim, p.out_dim));
}

// A run-time value as a template argument: f is a generic lambda and gets a std::integral_constant.
template <class F> inline auto ego_with_bool(bool v, F f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
template <int N> using ego_int = std::integral_constant<int, N>;
// the image planes of a frame: 3 (BGR) or 1 (grey)
template <class F> inline auto ego_with_channels(int channels, F f) { return channels == 3 ? f(ego_int<3>{}) : f(ego_int<1>{}); }

}  // namespace

}  // namespace xwb
