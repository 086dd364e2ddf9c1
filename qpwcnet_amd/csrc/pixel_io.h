// What the kernels that write pictures share (augment.hip, triplet.hip, vis.hip, review.hip): the store of a workgroup's
// tile of pixels, staged through LDS or element by element, and the launchers' step from run-time form flags to
// template arguments.
#pragma once
#include <type_traits>

#include "common.h"

namespace qpwc {

typedef float pix_f32x4 __attribute__((ext_vector_type(4)));

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// f(std::true_type) or f(std::false_type)
template <class F>
inline void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// f(std::integral_constant<int, QPWC_NHWC or QPWC_NCHW>)
template <class F>
inline void dispatch_layout(int layout, F&& f) {
    if (layout == QPWC_NHWC) f(std::integral_constant<int, QPWC_NHWC>{});
    else f(std::integral_constant<int, QPWC_NCHW>{});
}

// The store of TILE consecutive pixels (row-major, from pixel `base` of an image of ohw pixels) of one (B,oh,ow,C) /
// (B,C,oh,ow) tensor of T = float or uint8_t by a workgroup of THREADS lanes.  `img` is the image's first pixel,
// n * ohw; t is a pixel's place in the tile.
//   element-wise  put() writes channel c of pixel base + t to the tensor; nothing more is needed.
//   STAGED        put() writes it to `stage`, kElems elements of LDS that hold the tile in the tensor's own memory
//                 order.  After a barrier, flush() moves the cnt = min(TILE, ohw - base) pixels that exist, in pieces
//                 of 16 bytes (float) or 4 bytes (uint8_t), each lane a piece per trip.  It requires ohw % 4 == 0 and a
//                 tensor aligned to a piece: cnt and base are then multiples of 4, so a channels-last tile is cnt * C / 4
//                 whole pieces in one run, a plane's share of a channels-first tile is cnt / 4 of them, and every
//                 image, plane and tile starts on a piece.
template <bool STAGED, int LAYOUT, int C, int TILE, int THREADS, class T>
struct TileStore {
    static_assert(TILE % 4 == 0 && (std::is_same<T, float>::value || std::is_same<T, uint8_t>::value), "");
    using Piece = std::conditional_t<std::is_same<T, float>::value, pix_f32x4, uint32_t>;
    static constexpr int kElems = TILE * C, kPieces = kElems / 4;

    static __device__ __forceinline__ int stage_index(int t, int c) { return LAYOUT == QPWC_NHWC ? t * C + c : c * TILE + t; }

    static __device__ __forceinline__ void put(T* stage, T* out, int64_t img, int ohw, int base, int t, int c, T x) {
        if (STAGED) stage[stage_index(t, c)] = x;
        else out[LAYOUT == QPWC_NHWC ? (img + base + t) * C + c : (img * C + (int64_t)c * ohw) + base + t] = x;
    }

    static __device__ __forceinline__ void flush(const T* stage, T* out, int64_t img, int ohw, int base, int cnt) {
        const Piece* s = reinterpret_cast<const Piece*>(stage);
        Piece* o = reinterpret_cast<Piece*>(out);
        constexpr int kPlane = TILE / 4;   // pieces of one plane of the tile
#pragma unroll
        for (int i0 = 0; i0 < kPieces; i0 += THREADS) {
            const int i = i0 + (int)threadIdx.x;
            if (LAYOUT == QPWC_NHWC) {
                if (i < cnt * C / 4) o[(img + base) * C / 4 + i] = s[i];
            } else {
                const int c = i / kPlane, j = i - c * kPlane;
                if (i < kPieces && 4 * j < cnt) o[(img * C + (int64_t)c * ohw + base) / 4 + j] = s[i];
            }
        }
    }
};

}  // namespace qpwc
