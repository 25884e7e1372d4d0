// xworld_amd/csrc/xwb_ego_tables.hip -- the tables of an egocentric geometry (r, map size, frame size), built on the host once
// per batch and uploaded as one blob: cv::resize's taps, the per-heading layout tables, the span path's square maps.  Host
// code only; xw_ego_pixel.h (EgoBlob, EgoLayoutAt, EgoMapAt) says where everything lies, for this writer and for the kernels.
#include "xw_ego_pixel.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace xwb {

static void resize_taps(int src, int dst, EgoTap *h, EgoTap *v) {
    // cv::resize INTER_LINEAR (imgwarp.cpp): fx = (dx + 0.5) * scale - 0.5 in float; left edge: sx < 0 -> (0, fx = 0);
    // right edge: columns from the first one with sx + 1 >= src on take the single tap S[min(sx, src - 1)] * 2048;
    // rows are clipped instead; coefficients = cvRound(c * 2048) as short
    const double scale = (double)src / dst;
    int xmax = dst;
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= s;
        {   // vertical
            const float fy = f;
            const int r0 = s < 0 ? 0 : (s >= src ? src - 1 : s), r1 = s + 1 < 0 ? 0 : (s + 1 >= src ? src - 1 : s + 1);
            v[d] = EgoTap{(int16_t)r0, (int16_t)r1, (int16_t)lrintf((1.f - fy) * 2048), (int16_t)lrintf(fy * 2048)};
        }
        float fx = f;
        int sx = s;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= src) {
            if (d < xmax) xmax = d;
            if (sx >= src - 1) { fx = 0; sx = src - 1; }
        }
        if (d >= xmax) h[d] = EgoTap{(int16_t)sx, (int16_t)sx, 2048, 0};
        else h[d] = EgoTap{(int16_t)sx, (int16_t)(sx + 1), (int16_t)lrintf((1.f - fx) * 2048), (int16_t)lrintf(fx * 2048)};
    }
}

// The blob EgoBlob describes: the taps of both resizes (h1, v1: view -> canvas size; h2, v2: canvas size -> frame), the four
// headings' layout tables (EgoLayout), the square maps and the composed taps.  An output row is interior when the four view
// rows behind it exist and lie in one cell row (or column, for the sideways headings).  *fast_out: frame rows are whole dwords and no dword holds interior pixels of two
// cells -- the condition for copying interior pixels from the table.
hipError_t xw_ego_tables(int r, int max_dim, int out_dim, EgoTap **dev_out, int *fast_out, int *cell_edge_out, int *span_out) {
    int cell_edge = 1;
    // span path: the frame as r x r squares of U = O / r pixels, described by the square maps (cmap; EgoMapAt).  Possible when
    // the only rows / columns that straddle two cells are first rows / columns of a square.
    const int U = out_dim / r;
    bool span = (r == 3 || r == 5 || r == 7) && out_dim == r * (84 / r) && U % 4 == 0;
    const EgoBlob B = ego_blob(r, max_dim, out_dim);
    std::vector<uint8_t> blob(B.bytes, 0);
    const auto T = ego_tables_at<uint8_t, EgoTap, uint16_t>(blob.data(), B);
    uint8_t *const cmap = T.map;
    memset(cmap, 0xff, (size_t)B.map.bytes);
    const EgoTap *const h1 = T.h1, *const v1 = T.v1, *const h2 = T.h2, *const v2 = T.v2;
    resize_taps(64 * r, 64 * max_dim, T.h1, T.v1);
    resize_taps(64 * max_dim, out_dim, T.h2, T.v2);
    const int O = out_dim, O4 = B.O4, S = 64 * r;
    bool fast = (O & 3) == 0 && r * r <= 64;
    for (int dir = 0; dir < 4; ++dir) {
        uint16_t *L = T.lut + (size_t)dir * B.lay.words;
        uint16_t *rt = L + B.lay.rt, *ct = L + B.lay.ct, *ct4 = L + B.lay.ct4, *hd = L + B.lay.hd, *br = L + B.lay.br, *bc = L + B.lay.bc;
        uint16_t *rect = L + B.lay.rect, *seg = L + B.lay.seg;
        const bool row_is_y = dir == 3 || dir == 1;
        std::vector<int> cell_of[2];                           // per axis: the cell coordinate of an interior row / column, -1 border
        for (int axis = 0; axis < 2; ++axis) {                 // 0: output rows, 1: output columns
            const EgoTap *t1 = axis ? h1 : v1, *t2 = axis ? h2 : v2;
            const bool flip = axis ? !(dir == 3 || dir == 0) : !(dir == 3 || dir == 2);
            const bool times_r = axis ? !row_is_y : row_is_y;
            cell_of[axis].assign(O, -1);
            uint16_t *term = axis ? ct : rt, *border = axis ? bc : br;
            int nb = 0;
            for (int o = 0; o < O; ++o) {
                const int idx[4] = {t1[t2[o].s0].s0, t1[t2[o].s0].s1, t1[t2[o].s1].s0, t1[t2[o].s1].s1};
                int cell = -1;
                bool ok = true, edge = false;
                for (int i = 0; i < 4; ++i) {
                    const int f = flip ? S - idx[i] : idx[i];
                    if (f < 0 || f >= S) { edge = true; continue; }       // outside the view: black whatever the cells show
                    if (cell < 0) cell = f >> 6;
                    else if (cell != (f >> 6)) ok = false;
                }
                if (cell < 0) cell = 0;                                   // (all four outside: cannot happen, taps are adjacent pairs)
                if (ok) { term[o] = (uint16_t)((times_r ? cell * r : cell) | (edge ? EGO_EDGE : 0u)); cell_of[axis][o] = cell; }
                else { term[o] = (uint16_t)EGO_BORDER; border[nb++] = (uint16_t)o; }
            }
            hd[axis] = (uint16_t)nb;
        }
        for (int x4 = 0; x4 < O4 / 4; ++x4) {                  // the column term of a dword
            int term = -1;
            for (int j = 0; j < 4 && 4 * x4 + j < O; ++j) {
                if (ct[4 * x4 + j] & EGO_BORDER) continue;
                const int tj = ct[4 * x4 + j] & EGO_TERM;
                if (term < 0) term = tj;
                else if (term != tj) fast = false;
            }
            ct4[x4] = (uint16_t)(term < 0 ? 0 : term);
        }
        {   // column segments: maximal runs of dwords with the same column term (at most 24 dwords: six x4 loads per item)
            int ns = 0;
            for (int x4 = 0; x4 < O4 / 4; ++x4) {
                if (ns > 0 && seg[3 * (ns - 1) + 2] == ct4[x4] && seg[3 * (ns - 1) + 1] < 24) seg[3 * (ns - 1) + 1]++;
                else { seg[3 * ns] = (uint16_t)x4; seg[3 * ns + 1] = 1; seg[3 * ns + 2] = ct4[x4]; ns++; }
            }
            hd[3] = (uint16_t)ns;
        }
        int cw = 1;
        for (int k = 0; k < r * r; ++k) {                       // view cell k = vy * r + vx: where its interior pixels are
            const int vx = k % r, vy = k / r;
            const int row_cell = row_is_y ? vy : vx, col_cell = row_is_y ? vx : vy;
            int y0 = O, y1 = -1, x0 = O, x1 = -1;
            for (int o = 0; o < O; ++o) {
                if (cell_of[0][o] == row_cell) { if (o < y0) y0 = o; if (o > y1) y1 = o; }
                if (cell_of[1][o] == col_cell) { if (o < x0) x0 = o; if (o > x1) x1 = o; }
            }
            const int w = x1 >= x0 ? x1 - x0 + 1 : 0, h = y1 >= y0 ? y1 - y0 + 1 : 0;
            rect[4 * k] = (uint16_t)(w ? x0 : 0); rect[4 * k + 1] = (uint16_t)(h ? y0 : 0);
            rect[4 * k + 2] = (uint16_t)w; rect[4 * k + 3] = (uint16_t)h;
            if (w > cw) cw = w;
            if (h > cw) cw = h;
        }
        if (span) {
            for (int axis = 0; axis < 2; ++axis) {
                int nb = 0;
                for (int o = 0; o < O; ++o) {
                    if (cell_of[axis][o] < 0) {
                        if (o % U != 0 || o == 0) span = false;
                        else cmap[(axis ? B.map.cols : B.map.rows) + dir * r + o / U] = (uint8_t)nb;
                        nb++;
                    } else if (cell_of[axis][o] != cell_of[axis][(o / U) * U + U / 2]) {
                        span = false;
                    }
                }
            }
            for (int fy = 0; fy < r && span; ++fy)
                for (int fx = 0; fx < r; ++fx) {
                    const int rc = cell_of[0][fy * U + U / 2], cc = cell_of[1][fx * U + U / 2];
                    cmap[B.map.cell + dir * r * r + fy * r + fx] = (uint8_t)(row_is_y ? rc * r + cc : cc * r + rc);
                }
        }
        hd[2] = (uint16_t)cw;
        if (cw > cell_edge) cell_edge = cw;
    }
    for (int i = 0; i < 4 * r * r; ++i) {
        const uint8_t k = cmap[B.map.cell + i];
        if (k == 0xff || k >= r * r) { span = false; continue; }                  // (a permutation per heading, or no span path)
        cmap[B.map.inv + (i / (r * r)) * r * r + k] = (uint8_t)(i % (r * r));
    }
    // the composed taps of an output row / column (ego_compose_taps: the two intermediate indices' taps and the output tap), so
    // that a kernel whose workgroups live for one chain of dependent reads gets them in ONE read instead of two
    EgoTap *const comp = T.comp;
    for (int i = 0; i < O; ++i) {
        comp[(size_t)3 * i + 0] = v1[v2[i].s0]; comp[(size_t)3 * i + 1] = v1[v2[i].s1]; comp[(size_t)3 * i + 2] = v2[i];
        comp[(size_t)3 * (O + i) + 0] = h1[h2[i].s0]; comp[(size_t)3 * (O + i) + 1] = h1[h2[i].s1]; comp[(size_t)3 * (O + i) + 2] = h2[i];
    }
    uint8_t *d = nullptr;
    hipError_t err = hipMalloc(&d, blob.size());
    if (err != hipSuccess) return err;
    err = hipMemcpy(d, blob.data(), blob.size(), hipMemcpyHostToDevice);
    *dev_out = reinterpret_cast<EgoTap *>(d);
    *fast_out = fast ? 1 : 0;
    if (span_out) *span_out = fast && span ? 1 : 0;
    if (cell_edge_out) *cell_edge_out = cell_edge;
    return err;
}

}  // namespace xwb
