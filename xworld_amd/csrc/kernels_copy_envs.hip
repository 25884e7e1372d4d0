// kernels_copy_envs.hip -- xwb_copy_envs: envs of one batch become copies of envs of the same or of another batch, on the device.
//
// The work of one pair (destination env, source env) is every per-env array of the two batches (CopyEnvsParams, xwb_common.h):
// a few dozen arrays of 1 .. 64 bytes per env, and a handful of large ones -- the frames (27 648 bytes at 8 x 8 colour), the
// egocentric goal images (16 KB per goal), the grid.  Workgroup (chunk, pair): chunk 0 copies all the small arrays, eight
// lanes per array, so their loads are in flight together instead of one round trip after the other; every other chunk is
// COPY_CHUNK bytes of one large array, 16 bytes per lane where both addresses allow, byte-wise otherwise (odd frame sizes: the
// per-env egocentric radii, SimpleGame).  A small list therefore still spreads over pairs x chunks workgroups.  Plain loads
// and stores: the kernel boundary orders them against the verbs around it.
//
// An index outside its batch: the pair is skipped whole (every workgroup of it takes the same decision from the same two
// words) and counted once in the destination's error counter.  A destination env named twice, or named as a source as well, is
// written / read by several workgroups in no order: its contents are unspecified, every access stays inside the arrays.
#include "xwb_common.h"

namespace xwb {

namespace {

// `len` bytes from src (null: zeros) to dst by the whole workgroup: whole 16-byte pieces first when both addresses are aligned
__device__ __forceinline__ void copy_span(uint8_t *dst, const uint8_t *src, uint32_t len, int tid) {
    const bool zero = src == nullptr;
    const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
    const uint32_t pieces = vec ? len >> 4 : 0u;                               // (<= COPY_BS: one per lane)
    if ((uint32_t)tid < pieces) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (!zero) v = reinterpret_cast<const uint4 *>(src)[tid];
        reinterpret_cast<uint4 *>(dst)[tid] = v;
    }
    // the rest (everything, for unaligned addresses) byte-wise: a lane's sixteen loads first, then its stores
    const uint32_t at = pieces * 16u + (uint32_t)tid;
    uint8_t v[COPY_CHUNK / COPY_BS];
#pragma unroll
    for (int j = 0; j < COPY_CHUNK / COPY_BS; ++j) {
        const uint32_t i = at + (uint32_t)j * COPY_BS;
        v[j] = !zero && i < len ? src[i] : (uint8_t)0;
    }
#pragma unroll
    for (int j = 0; j < COPY_CHUNK / COPY_BS; ++j) {
        const uint32_t i = at + (uint32_t)j * COPY_BS;
        if (i < len) dst[i] = v[j];
    }
}

}  // namespace

__global__ __launch_bounds__(COPY_BS) void xw_copy_envs_kernel(CopyEnvsParams p) {
    const int chunk = (int)blockIdx.x, tid = (int)threadIdx.x;
    for (int pair = (int)blockIdx.y; pair < p.n_pairs; pair += (int)gridDim.y) {
        const int d = p.dst_envs[pair], s = p.src_envs[pair];
        if ((unsigned)d >= (unsigned)p.n_dst || (unsigned)s >= (unsigned)p.n_src) {
            if (chunk == 0 && tid == 0) atomicAdd(p.err_count, 1);
            continue;
        }
        if (p.same && d == s) continue;
        if (chunk == 0) {
            // array k of the small ones: lanes 8 k .. 8 k + 7, word-wise where its size allows (the bases are allocations)
            const int k = tid >> 3, sub = tid & 7;
            CopyArray a{nullptr, nullptr, 0u, 0u};
            for (int j = 0; j < p.n_small; ++j) if (j == k) a = p.small[j];    // (a scalar read per array, no per-lane table index)
            uint8_t *dst = a.dst + (size_t)d * a.bytes;
            const uint8_t *src = a.src ? a.src + (size_t)s * a.bytes : nullptr;
            if ((a.bytes & 3u) == 0 && ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 3u) == 0) {
                for (uint32_t i = (uint32_t)sub; i < (a.bytes >> 2); i += 8u)
                    reinterpret_cast<uint32_t *>(dst)[i] = src ? reinterpret_cast<const uint32_t *>(src)[i] : 0u;
            } else {
                for (uint32_t i = (uint32_t)sub; i < a.bytes; i += 8u) dst[i] = src ? src[i] : (uint8_t)0;
            }
        } else {
            CopyArray a = p.big[0];
            for (int j = 1; j < p.n_big; ++j) if ((uint32_t)chunk >= p.big[j].chunk0) a = p.big[j];
            const uint32_t off = ((uint32_t)chunk - a.chunk0) * (uint32_t)COPY_CHUNK;
            if (off >= a.bytes) continue;                                      // (a grid larger than the table asks for)
            const uint32_t len = a.bytes - off < (uint32_t)COPY_CHUNK ? a.bytes - off : (uint32_t)COPY_CHUNK;
            copy_span(a.dst + (size_t)d * a.bytes + off, a.src ? a.src + (size_t)s * a.bytes + off : nullptr, len, tid);
        }
    }
}

hipError_t launch_copy_envs(const CopyEnvsParams &p, hipStream_t s) {
    if (p.n_pairs <= 0 || p.chunks <= 0) return hipSuccess;
    const dim3 grid((unsigned)p.chunks, (unsigned)(p.n_pairs < 65535 ? p.n_pairs : 65535));
    hipLaunchKernelGGL(xw_copy_envs_kernel, grid, dim3(COPY_BS), 0, s, p);
    return hipGetLastError();
}

}  // namespace xwb
