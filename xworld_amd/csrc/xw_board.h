// xw_board.h -- one XWorld2D board as bit masks held in registers (device code: the reset path, kernels_xworld_reset.hip).
// Cell c = y * D + x of the D x D board is bit c of a Mask<NW> (NW x 64 bits); Board<NW> knows where the board sits in the
// env's max_dim x max_dim grid row and offers the whole-board shift operations map generation is written in.
#pragma once
#include <stdint.h>

namespace xwb {

template <int NW>
struct Mask {
    uint64_t w[NW];
    Mask() = default;
    __device__ __forceinline__ explicit Mask(int b) { clear(); set(b); }      // the one cell b
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 0;
    }
    __device__ __forceinline__ bool test(int b) const {
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) v = ((b >> 6) == i) ? w[i] : v;
        return (v >> (b & 63)) & 1ull;
    }
    __device__ __forceinline__ void set(int b) {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] |= ((b >> 6) == i) ? (1ull << (b & 63)) : 0ull;
    }
    __device__ __forceinline__ void reset(int b) {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] &= ((b >> 6) == i) ? ~(1ull << (b & 63)) : ~0ull;
    }
    __device__ __forceinline__ bool any() const {
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) v |= w[i];
        return v != 0;
    }
    __device__ __forceinline__ bool equals(const Mask &o) const {
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) v |= w[i] ^ o.w[i];
        return v == 0;
    }
    __device__ __forceinline__ int count() const {
        int n = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) n += __popcll(w[i]);
        return n;
    }
    // number of set bits below bit b (any b: <= 0 counts none, >= 64 * NW counts all)
    __device__ __forceinline__ int count_below(int b) const {
        int n = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int k = b - i * 64;
            const uint64_t lowmask = k <= 0 ? 0ull : (k >= 64 ? ~0ull : ((1ull << k) - 1ull));
            n += __popcll(w[i] & lowmask);
        }
        return n;
    }
    // index of the k-th (0-based) set bit in ascending bit order
    __device__ __forceinline__ int select(int k) const {
        int base = 0;
        uint64_t word = 0;
        bool found = false;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int c = __popcll(w[i]);
            if (!found) {
                if (k < c) { word = w[i]; base = i * 64; found = true; }
                else k -= c;
            }
        }
        int pos = 0;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const int c = __popcll(word & ((1ull << s) - 1ull));
            if (k >= c) { k -= c; word >>= s; pos += s; }
        }
        return base + pos;
    }
    __device__ __forceinline__ Mask shl(int s) const {      // 1 <= s <= 63
        Mask r;
#pragma unroll
        for (int i = NW - 1; i >= 0; --i) r.w[i] = (w[i] << s) | (i > 0 ? (w[i - 1] >> (64 - s)) : 0ull);
        return r;
    }
    __device__ __forceinline__ Mask shr(int s) const {
        Mask r;
#pragma unroll
        for (int i = 0; i < NW; ++i) r.w[i] = (w[i] >> s) | (i + 1 < NW ? (w[i + 1] << (64 - s)) : 0ull);
        return r;
    }
    __device__ __forceinline__ Mask operator&(const Mask &o) const {
        Mask r;
#pragma unroll
        for (int i = 0; i < NW; ++i) r.w[i] = w[i] & o.w[i];
        return r;
    }
    __device__ __forceinline__ Mask operator|(const Mask &o) const {
        Mask r;
#pragma unroll
        for (int i = 0; i < NW; ++i) r.w[i] = w[i] | o.w[i];
        return r;
    }
    __device__ __forceinline__ Mask andnot(const Mask &o) const {      // this & ~o
        Mask r;
#pragma unroll
        for (int i = 0; i < NW; ++i) r.w[i] = w[i] & ~o.w[i];
        return r;
    }
};

// The actual D x D board of an env, centred in its MD x MD grid row (cpp_get_entities shifts by the padding offset).
template <int NW>
struct Board {
    int D, MD, off;
    Mask<NW> valid, col0, colN;                            // every cell; the cells of column 0; of column D - 1
    __device__ __forceinline__ Board(int D_, int MD_) : D(D_), MD(MD_), off((MD_ - D_) / 2) {
        valid.clear(); col0.clear(); colN.clear();
        for (int y = 0; y < D; ++y) { col0.set(y * D); colN.set(y * D + D - 1); }
        for (int c = 0; c < D * D; ++c) valid.set(c);
    }
    __device__ __forceinline__ int grid_index(int c) const { return (c / D + off) * MD + (c % D + off); }
    __device__ __forceinline__ int cell_at(int gx, int gy) const { return (gy - off) * D + (gx - off); }   // grid_index's inverse
    // the four neighbours of every cell of m, clipped to the board
    __device__ __forceinline__ Mask<NW> neighbours(const Mask<NW> &m) const {
        Mask<NW> r = m.andnot(colN).shl(1) | m.andnot(col0).shr(1) | m.shl(D) | m.shr(D);
        return r & valid;
    }
    // the cells 4-connected to `seed` through `open` cells (the seed itself included, open or not)
    __device__ __forceinline__ Mask<NW> flood(int seed, const Mask<NW> &open) const {
        Mask<NW> m(seed);
        for (int it = 0; it < D * D; ++it) {
            const Mask<NW> grown = m | (neighbours(m) & open);
            if (grown.equals(m)) break;
            m = grown;
        }
        return m;
    }
};

}  // namespace xwb
