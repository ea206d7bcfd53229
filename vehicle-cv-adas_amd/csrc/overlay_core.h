// overlay_core.h -- the pixel rules of the lane overlay: the part of the reference's Draw* block that needs nothing but pixels
// (UltrafastLaneDetectorV2.DrawDetectedOnFrame / DrawAreaOnFrame, ultrafastLaneDetectorV2.py:196-218, the discs of
// SingleCamDistanceMeasure.DrawDetectedOnFrame, distanceMeasure.py:98, and PerspectiveTransformation.DrawDetectedOnBirdView,
// perspectiveTransformation.py:217-226): cv2.addWeighted on u8, filled cv2.circle, cv2.fillPoly.
//
// cv2 is third-party arithmetic and is not available here: the rules below are modelled on OpenCV 4.5's drawing.cpp / arithm and are
// checked against their restatement in NumPy (tests/overlay_ref.py).  THE DEFINITIONS HERE ARE THE AUTHORITY; parity with a real cv2
// build is UNPINNED.  One known divergence: lines are NOT clipped to the image before they are walked (OpenCV clips the segment and
// restarts the error term); the pixels of the unclipped line that fall inside the image are drawn.
//   D1 blend   r = rintf((float)a * af + (float)b * bf), af = (float)alpha, bf = (float)(1.0 - (double)alpha): two separately rounded
//              fp32 products, one fp32 add, no fused multiply-add (the unit is compiled with -ffp-contract=off), ties to even, saturated;
//   D2 disc    row cy +- j covers cx - hw[j] .. cx + hw[j], hw from the midpoint walk (overlay_disc_halfwidths);
//   D3 line    8-connected, both end pixels, walked from the endpoint with the smaller x (a tie: the edge's first point); after k steps
//              the minor axis has moved floor((2 m k + M - 1) / (2 M)), so a row's run of a line is a closed form (overlay_line_row);
//   D4 polygon every edge by D3, plus the even-odd interior from 16.16 fixed-point crossings X = (x0 << 16) + (y - y0) * D of the edges
//              active on a row (y0 <= y < y1), D = ((x1 - x0) << 16) / (y1 - y0) truncated toward zero; sorted crossings pair up and
//              a pair fills ceil(Xl / 65536) .. floor(Xr / 65536).  Pixel q of a row is inside some pair exactly when the number of
//              crossings below q * 65536 is odd or a crossing equals q * 65536 (the number of crossings of a closed contour on a row is
//              even), so no sort is needed: overlay_poly_edge_row toggles one bit per crossing and a prefix XOR over the row does the rest.
// Nothing here loops for a number of steps given by a coordinate; all coordinate arithmetic is int64.
// Like warp_core.h the header also compiles for the host (tests/hostemu/emu_overlay.cpp).
#pragma once
#include <stdint.h>
#include <math.h>

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

#define ADAS_OVERLAY_MAX_RADIUS 64     // hw tables are [ADAS_OVERLAY_MAX_RADIUS + 1]
#define ADAS_OVERLAY_COORD_MAX 32767   // a polygon vertex beyond it in |x| or |y| skips the frame's fill (ADAS_OVERLAY_POLY_RANGE)

// coverage bits of one pixel
#define OV_BIT_LANE0 1u    // lanes 0..3: bits 0..3
#define OV_BIT_AREA 16u
#define OV_BIT_DIST 32u

// ---------------------------------------------------------------------------------------------------------------- D1
struct OverlayAlpha {
    float af, bf;
};
ADAS_HD OverlayAlpha overlay_alpha(double alpha) {
    OverlayAlpha a;
    a.af = (float)alpha;
    a.bf = (float)(1.0 - alpha);
    return a;
}
ADAS_HD int overlay_blend(int a, int b, const OverlayAlpha w) {
    const float pa = (float)a * w.af;
    const float pb = (float)b * w.bf;
    const float s = pa + pb;
    const float r = rintf(s);   // ties to even
    return r < 0.f ? 0 : (r > 255.f ? 255 : (int)r);
}

// ---------------------------------------------------------------------------------------------------------------- D2
// hw[0 .. r]; r in [0, ADAS_OVERLAY_MAX_RADIUS]
ADAS_HD void overlay_disc_halfwidths(int r, int* hw) {
    for (int i = 0; i <= r; ++i) hw[i] = 0;
    int dx = r, dy = 0, err = 0, plus = 1, minus = 2 * r - 1;
    while (dx >= dy) {
        if (hw[dy] < dx) hw[dy] = dx;
        if (hw[dx] < dy) hw[dx] = dy;
        ++dy;
        err += plus;
        plus += 2;
        if (err > 0) {
            err -= minus;
            --dx;
            minus -= 2;
        }
    }
}
// row cy + j (j in -r .. r, hwj = hw[|j|]) of the disc at (cx, cy) clipped to a W x H image: false when nothing of it is inside
ADAS_HD bool overlay_disc_row(int cx, int cy, int j, int hwj, int W, int H, int* y, int* xl, int* xr) {
    const long long yy = (long long)cy + j;
    if (yy < 0 || yy >= H) return false;
    long long l = (long long)cx - hwj, r = (long long)cx + hwj;
    if (l < 0) l = 0;
    if (r > W - 1) r = W - 1;
    if (l > r) return false;
    *y = (int)yy;
    *xl = (int)l;
    *xr = (int)r;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- D3
// the pixels of the line (ax, ay) -> (bx, by) on row y: false when it has none, else the run xl .. xr (unclipped in x)
ADAS_HD bool overlay_line_row(int ax, int ay, int bx, int by, int y, long long* xl, long long* xr) {
    long long xs = ax, ys = ay, xe = bx, ye = by;
    if (xe < xs) {   // start at the smaller x; on a tie the edge's first point stays the start
        xs = bx; ys = by; xe = ax; ye = ay;
    }
    const long long dx = xe - xs, dy = ye - ys, ady = dy < 0 ? -dy : dy;
    const long long j = dy < 0 ? ys - y : y - ys;   // rows moved from the start, in the line's direction
    if (j < 0 || j > ady) return false;
    if (ady > dx) {   // the major axis is y: one pixel per row, after k = j steps
        const long long M = ady, m = dx;
        *xl = *xr = xs + (2 * m * j + M - 1) / (2 * M);
        return true;
    }
    const long long M = dx, m = ady;
    if (m == 0) {   // horizontal (M == 0: a single point)
        *xl = xs;
        *xr = xe;
        return true;
    }
    // the steps k in [0, M] with floor((2 m k + M - 1) / (2 M)) == j
    const long long lo = 2 * M * j - M + 1;
    long long k0 = lo <= 0 ? 0 : (lo + 2 * m - 1) / (2 * m);
    long long k1 = (2 * M * j + M) / (2 * m);
    if (k1 > M) k1 = M;
    if (k0 > k1) return false;
    *xl = xs + k0;
    *xr = xs + k1;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- D4
// the 16.16 crossing of edge (ax, ay) - (bx, by) with row y: false when the edge is horizontal or not active on the row
ADAS_HD bool overlay_edge_crossing(int ax, int ay, int bx, int by, int y, long long* X) {
    if (ay == by) return false;
    long long x0 = ax, y0 = ay, x1 = bx, y1 = by;
    if (y1 < y0) {
        x0 = bx; y0 = by; x1 = ax; y1 = ay;
    }
    if (y < y0 || y >= y1) return false;
    const long long D = ((x1 - x0) * 65536) / (y1 - y0);   // truncated toward zero
    *X = x0 * 65536 + (y - y0) * D;
    return true;
}
ADAS_HD bool overlay_poly_in_range(const int* pts, int n) {
    for (int i = 0; i < 2 * n; ++i)
        if (pts[i] > ADAS_OVERLAY_COORD_MAX || pts[i] < -ADAS_OVERLAY_COORD_MAX) return false;
    return true;
}
// What edge e (p_e -> p_(e+1), the last one back to p_0) of the contour pts[n][2] contributes to row y of a W-column image:
//   ops.fill(xl, xr)  the columns of its line on the row, clipped to the image;
//   ops.set(q)        a crossing exactly on column q;
//   ops.toggle(t)     columns t .. W - 1 change parity (t in [0, W - 1]).
// overlay_row_resolve turns a row's toggle bits into the interior.  Contours of fewer than 3 points have no interior.
template <class Ops>
ADAS_HD void overlay_poly_edge_row(const int* pts, int n, int e, int y, int W, Ops& ops) {
    const int e1 = e + 1 == n ? 0 : e + 1;
    const int ax = pts[2 * e], ay = pts[2 * e + 1], bx = pts[2 * e1], by = pts[2 * e1 + 1];
    long long xl, xr;
    if (overlay_line_row(ax, ay, bx, by, y, &xl, &xr)) {
        if (xl < 0) xl = 0;
        if (xr > W - 1) xr = W - 1;
        if (xl <= xr) ops.fill((int)xl, (int)xr);
    }
    long long X;
    if (n >= 3 && overlay_edge_crossing(ax, ay, bx, by, y, &X)) {
        const long long q = X >> 16;   // floor
        if ((X & 0xffff) == 0 && q >= 0 && q < W) ops.set((int)q);
        const long long t = q + 1 < 0 ? 0 : q + 1;
        if (t < W) ops.toggle((int)t);
    }
}
// inclusive prefix XOR of a word's bits (bit i of the result = parity of bits 0 .. i); carry = parity entering the word (0 / 1)
ADAS_HD uint32_t overlay_prefix_xor(uint32_t w, uint32_t carry) {
    w ^= w << 1;
    w ^= w << 2;
    w ^= w << 4;
    w ^= w << 8;
    w ^= w << 16;
    return carry ? ~w : w;
}
// bits lo .. hi (inclusive, 0 <= lo <= hi) that fall into word `word` of a row
ADAS_HD uint32_t overlay_word_mask(int lo, int hi, int word) {
    const int b0 = word * 32, b1 = b0 + 31;
    if (hi < b0 || lo > b1) return 0u;
    const int l = lo > b0 ? lo - b0 : 0, h = hi < b1 ? hi - b0 : 31;
    return (0xffffffffu >> (31 - h)) & (0xffffffffu << l);
}

// ---------------------------------------------------------------------------------------------------------------- D5
struct OverlayStyle {            // one frame's resolved colours, channel c in bits 8c .. 8c + 7
    uint32_t lane[4];            // per lane, after the offset rule
    uint32_t area;
    uint32_t dist;
    OverlayAlpha lane_w, area_w;
    int lane_direct;             // the bird view: discs are written, not blended
};
// channel c of one pixel: s = the source byte, bits = its coverage (OV_BIT_*)
ADAS_HD uint32_t overlay_pack_bgr(const uint8_t* c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }
ADAS_HD int overlay_pixel(int s, uint32_t bits, int c, const OverlayStyle& st) {
    if (bits & OV_BIT_DIST) return (int)((st.dist >> (8 * c)) & 0xffu);
    int v = s;
    if (bits & 15u) {   // the last disc drawn wins: lanes are drawn in order
        const uint32_t col = (bits & 8u) ? st.lane[3] : (bits & 4u) ? st.lane[2] : (bits & 2u) ? st.lane[1] : st.lane[0];
        const int k = (int)((col >> (8 * c)) & 0xffu);
        v = st.lane_direct ? k : overlay_blend(k, v, st.lane_w);
    }
    if (bits & OV_BIT_AREA) v = overlay_blend(v, (int)((st.area >> (8 * c)) & 0xffu), st.area_w);
    return v;
}

}  // namespace adas
