// warp_core.h -- one destination pixel of cv2.warpPerspective(img, M, dsize, INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit
// BGR frames: PerspectiveTransformation.transformToBirdView / transformToFrontalView (perspectiveTransformation.py:89-117).
//
// cv2.warpPerspective is third-party arithmetic (opencv-python==4.5.4.60) and cv2 is not available here: this restates
// OpenCV 4.5's reference path (imgproc/src/imgwarp.cpp, WarpPerspectiveInvoker + remapBilinear<FixedPtCast<int, uchar, 15>>)
// and is checked against the same restatement in NumPy (tests/warp_ref.py).  Parity with a real cv2 build is UNPINNED.
//   * the matrix maps destination to source (OpenCV inverts M on the host unless WARP_INVERSE_MAP is given);
//   * OpenCV walks the destination in blocks of bw columns and evaluates the homogeneous coordinate at the block's first
//     column bx, then adds M*x1 for the column inside the block: (X0 + M0*x1) with X0 = M0*bx + M1*y + M2 is not the same
//     double as M0*x + M1*y + M2, so bx is part of the arithmetic;
//   * coordinates are rounded (ties to even) to 1/32 pixel; the four bilinear weights are integers that sum to 2^15:
//     (32-ax)*(32-ay)*32 and so on.  Whether OpenCV's 16-bit weight table stores its (0,0) entry differently is not known
//     here; this definition makes the identity warp exact;
//   * a tap outside the source reads 0 in every channel.
// All coordinate arithmetic is IEEE fp64 in the association written below, contraction off (the unit is compiled with
// -ffp-contract=off).  Like post_core.h / lane_core.h the header also compiles for the host (tests/hostemu/emu_warp.cpp).
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#if !defined(ADAS_HD)
#if defined(__HIPCC__)
#define ADAS_DEV __device__ __forceinline__
#define ADAS_HD __host__ __device__ inline
#pragma clang fp contract(off)
#else
#define ADAS_DEV inline
#define ADAS_HD inline
#endif
#endif

namespace adas {

#define ADAS_WARP_MAX_ROWS 4320   // both images: keeps the 1/32-pixel coordinates of in-range taps far inside int32 and
#define ADAS_WARP_MAX_COLS 16384  // the tap columns inside the 16-bit saturation of the map

// width of OpenCV's destination blocks: BLOCK_SZ = 32, bh0 = min(BLOCK_SZ/2, height), bw0 = min(BLOCK_SZ*BLOCK_SZ/bh0, width)
ADAS_HD int warp_block_width(int dst_h, int dst_w) {
    const int bh0 = dst_h < 16 ? dst_h : 16;
    const int bw0 = 1024 / bh0;
    return bw0 < dst_w ? bw0 : dst_w;
}

// adjugate / determinant of a row-major 3x3 matrix (cv::invert, DECOMP_LU's closed form for 3x3); false when det == 0
ADAS_HD bool warp_invert3x3(const double* m, double* o) {
    const double c0 = m[4] * m[8] - m[5] * m[7];
    const double c1 = m[3] * m[8] - m[5] * m[6];
    const double c2 = m[3] * m[7] - m[4] * m[6];
    double d = m[0] * c0 - m[1] * c1 + m[2] * c2;   // first-row expansion
    if (d == 0.0) return false;
    d = 1.0 / d;
    o[0] = c0 * d;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * d;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    o[3] = (m[5] * m[6] - m[3] * m[8]) * d;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * d;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    o[6] = c2 * d;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * d;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    return true;
}

struct WarpTap {
    int sx, sy;   // top-left tap, saturated to int16
    int ax, ay;   // 1/32-pixel fractions, 0 .. 31
};

ADAS_HD int warp_sat_s16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// std::max((double)INT_MIN, std::min((double)INT_MAX, v)) with the comparisons of <algorithm> (a NaN becomes INT_MAX)
ADAS_HD double warp_clamp_int(double v) {
    const double hi = 2147483647.0, lo = -2147483648.0;
    const double t = v < hi ? v : hi;
    return lo < t ? t : lo;
}

// source coordinate of destination pixel (x, y); M maps destination to source, bw = warp_block_width(dst_h, dst_w)
ADAS_HD WarpTap warp_coord(const double* M, int bw, int x, int y) {
    const int bx = (x / bw) * bw, x1 = x - bx;
    const double X0 = M[0] * bx + M[1] * y + M[2];
    const double Y0 = M[3] * bx + M[4] * y + M[5];
    const double W0 = M[6] * bx + M[7] * y + M[8];
    double W = W0 + M[6] * x1;
    W = W != 0.0 ? 32.0 / W : 0.0;   // INTER_TAB_SIZE / W
    const double fX = warp_clamp_int((X0 + M[0] * x1) * W);
    const double fY = warp_clamp_int((Y0 + M[3] * x1) * W);
    const int X = (int)rint(fX), Y = (int)rint(fY);   // cvRound: ties to even; in range after the clamp
    WarpTap t;
    t.sx = warp_sat_s16(X >> 5);
    t.sy = warp_sat_s16(Y >> 5);
    t.ax = X & 31;
    t.ay = Y & 31;
    return t;
}

ADAS_HD int warp_blend(int p00, int p01, int p10, int p11, int w00, int w01, int w10, int w11) {
    return (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
}

// the three channels of one destination pixel from frame `src` (HWC u8, src_h x src_w x 3)
ADAS_HD void warp_sample(const uint8_t* __restrict__ src, int src_h, int src_w, const WarpTap t, int out[3]) {
    const int w00 = (32 - t.ax) * (32 - t.ay) * 32, w01 = t.ax * (32 - t.ay) * 32;
    const int w10 = (32 - t.ax) * t.ay * 32, w11 = t.ax * t.ay * 32;
    const int sx = t.sx, sy = t.sy;
    if (sx >= 0 && sy >= 0 && sy + 1 < src_h && sx * 3 + 8 <= src_w * 3) {
        // all four taps inside, and 8 bytes from the left tap stay inside the row: the two taps of a row are 6 consecutive
        // bytes, read as one (unaligned) 8-byte load per row instead of six byte loads
        const uint8_t* r0 = src + ((size_t)sy * src_w + sx) * 3;
        unsigned long long a, b;
        memcpy(&a, r0, 8);
        memcpy(&b, r0 + (size_t)src_w * 3, 8);
        for (int c = 0; c < 3; ++c)
            out[c] = warp_blend((int)((a >> (8 * c)) & 0xff), (int)((a >> (8 * (3 + c))) & 0xff), (int)((b >> (8 * c)) & 0xff),
                                (int)((b >> (8 * (3 + c))) & 0xff), w00, w01, w10, w11);
        return;
    }
    const bool x0 = sx >= 0 && sx < src_w, x1 = sx + 1 >= 0 && sx + 1 < src_w;
    const bool y0 = sy >= 0 && sy < src_h, y1 = sy + 1 >= 0 && sy + 1 < src_h;
    if (!((x0 || x1) && (y0 || y1))) {   // every tap outside: the border value
        out[0] = out[1] = out[2] = 0;
        return;
    }
    // a row / column index that is outside is replaced by 0 so that every address formed lies inside the frame; its tap reads 0
    const uint8_t* r0 = src + ((size_t)(y0 ? sy : 0) * src_w) * 3;
    const uint8_t* r1 = src + ((size_t)(y1 ? sy + 1 : 0) * src_w) * 3;
    const int c0 = (x0 ? sx : 0) * 3, c1 = (x1 ? sx + 1 : 0) * 3;
    for (int c = 0; c < 3; ++c) {
        const int p00 = (y0 && x0) ? r0[c0 + c] : 0, p01 = (y0 && x1) ? r0[c1 + c] : 0;
        const int p10 = (y1 && x0) ? r1[c0 + c] : 0, p11 = (y1 && x1) ? r1[c1 + c] : 0;
        out[c] = warp_blend(p00, p01, p10, p11, w00, w01, w10, w11);
    }
}

}  // namespace adas
