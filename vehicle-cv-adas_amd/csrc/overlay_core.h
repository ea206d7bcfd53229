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
// The object layer (boxes of the detector and of the tracker: ObjectDetectBase.cornerRect, ObjectDetector/core.py:94-113, and the box part of
// ObjectTrackBase.plot_bbox, ObjectTracker/core.py:226-245) adds, under the same terms (the definitions are the authority, parity unpinned):
//   D6 thick   axis-aligned segment (ax, ay) - (bx, by) of thickness t >= 2, R = (t + 1) >> 1: the body, the segment's pixels along its axis
//              (both ends) by -R .. +R across it, plus a D2 disc of radius R on each endpoint (OpenCV 4.5's ThickLine: a quad of half-width
//              t / 2 filled with both borders, end caps of radius (t * 32768 + 32768) >> 16).  A zero-length segment is its two coinciding
//              discs.  On a row the body and the caps are one run (overlay_seg_row).  t == 1 is the D3 line: R = 0 gives the same pixels;
//   D7 outline the edges (x1,y1)-(x2,y1), (x2,y1)-(x2,y2), (x2,y2)-(x1,y2), (x1,y2)-(x1,y1): D3 lines for t == 1, D6 segments for t >= 2;
//   D8 tint    r = rintf(((float)a * af + (float)b * bf) + g), a the pixel, b the colour, af = (float)0.6, bf = (float)0.4 (given, not
//              1 - af), g = 1.0f: two separately rounded products, two adds in that order, no contraction, ties to even, saturated;
//   D9 fold    v0 = the pixel after AREA.  Detections in order: inside detection i's outline or corner arms, v = colour_i.  Tracks in order:
//              inside track k's outline v = colour_k, then inside its tint region v = D8(v, colour_k).  DISTANCE still overrides everything.
//              Where boxes overlap the result is this sequential fold (overlay_object_ops / overlay_object_channel per record).
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

#if !defined(ADAS_HDI)   // the object layer's rules are inlined into the kernels: a box passed by reference must not end up in scratch
#if defined(__HIPCC__)
#define ADAS_HDI __host__ __device__ __forceinline__
#else
#define ADAS_HDI inline
#endif
#endif

namespace adas {

#define ADAS_OVERLAY_MAX_RADIUS 64     // hw tables are [ADAS_OVERLAY_MAX_RADIUS + 1]
#define ADAS_OVERLAY_COORD_MAX 32767   // a polygon vertex beyond it in |x| or |y| skips the frame's fill (ADAS_OVERLAY_POLY_RANGE)

// coverage bits of one pixel
#define OV_BIT_LANE0 1u    // lanes 0..3: bits 0..3
#define OV_BIT_AREA 16u
#define OV_BIT_DIST 32u
#define OV_BIT_DET 64u     // some detection draws here
#define OV_BIT_TRK 128u    // some track draws or tints here

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

// ---------------------------------------------------------------------------------------------------------------- D6
#define ADAS_OVERLAY_MAX_THICKNESS (2 * ADAS_OVERLAY_MAX_RADIUS - 1)   // R = (t + 1) >> 1 <= ADAS_OVERLAY_MAX_RADIUS
ADAS_HDI int overlay_seg_radius(int t) { return t >= 2 ? (t + 1) >> 1 : 0; }   // t == 1: the thin line (D3); axis-aligned, R = 0 gives its pixels
// the pixels of the segment (ax, ay) - (bx, by), ax == bx or ay == by, on row y: false when it has none, else the run xl .. xr (unclipped).
// hw: overlay_disc_halfwidths(R).  Body and caps of a row are one run: a horizontal body ax .. bx grows by the caps' hw[|y - ay|] on either
// side; a vertical body is -R .. +R on its rows and a cap's row beyond its ends.
ADAS_HDI bool overlay_seg_row(long long ax, long long ay, long long bx, long long by, int R, const int* hw, long long y, long long* xl,
                             long long* xr) {
    if (ay == by) {   // horizontal, or zero length: two coinciding discs
        const long long j = y < ay ? ay - y : y - ay;
        if (j > R) return false;
        *xl = (ax < bx ? ax : bx) - hw[j];
        *xr = (ax < bx ? bx : ax) + hw[j];
        return true;
    }
    const long long y0 = ay < by ? ay : by, y1 = ay < by ? by : ay;
    if (y >= y0 && y <= y1) {
        *xl = ax - R;
        *xr = ax + R;
        return true;
    }
    const long long j = y < y0 ? y0 - y : y - y1;
    if (j > R) return false;
    *xl = ax - hw[j];
    *xr = ax + hw[j];
    return true;
}
ADAS_HDI bool overlay_seg_hit(long long ax, long long ay, long long bx, long long by, int R, const int* hw, int x, int y) {
    long long xl, xr;
    return overlay_seg_row(ax, ay, bx, by, R, hw, y, &xl, &xr) && x >= xl && x <= xr;
}

// ---------------------------------------------------------------------------------------------------------------- D7
// edge k (0 .. 3) of the outline through (x1, y1), (x2, y1), (x2, y2), (x1, y2)
ADAS_HDI void overlay_rect_edge(long long x1, long long y1, long long x2, long long y2, int k, long long* ax, long long* ay, long long* bx,
                               long long* by) {
    *ax = (k == 0 || k == 3) ? x1 : x2;
    *ay = k < 2 ? y1 : y2;
    *bx = k < 2 ? x2 : x1;
    *by = (k == 0 || k == 3) ? y1 : y2;
}

// ---------------------------------------------------------------------------------------------------------------- D8
ADAS_HDI int overlay_tint(int a, int b) {
    const float af = (float)0.6, bf = (float)0.4, g = 1.0f;
    const float pa = (float)a * af;
    const float pb = (float)b * bf;
    const float s = pa + pb;
    const float t = s + g;
    const float r = rintf(t);   // ties to even
    return r < 0.f ? 0 : (r > 255.f ? 255 : (int)r);
}

// ---------------------------------------------------------------------------------------------------------------- D9
#define OV_OBJ_NONE 0    // nothing is drawn (a track that is not activated, or fails the area gate)
#define OV_OBJ_DET 1     // cornerRect: the outline (thickness rect_t) and eight corner arms of length l (thickness arm_t), written
#define OV_OBJ_TRACK 2   // plot_bbox: the outline (thickness track_t), written, then the region x1 .. x2 - 1, y1 .. y2 - 1 tinted
struct OverlayObject {           // one box, 48 bytes
    int kind;
    int x1, y1, x2, y2;          // a detection's RectInfo.tolist(); a track's clamped corners
    int l;                       // the arms' length (detections)
    uint32_t colour;             // packed as overlay_pack_bgr does
    int bx0, by0, bx1, by1;      // every pixel the box can touch, inside the image; empty (bx0 > bx1) when it touches none
    int pad;
};
#define OV_SEG_RECT 0     // a detection's outline
#define OV_SEG_ARM 1      // its corner arms
#define OV_SEG_TRACK 2    // a track's outline
struct OverlayObjStyle {
    int radii;            // overlay_seg_radius of the three thicknesses, 8 bits each: OV_SEG_RECT lowest (one word: chosen by a shift)
    const int* hw;        // their overlay_disc_halfwidths: table w at hw + w * hw_stride
    int hw_stride;
};
ADAS_HDI int overlay_obj_radii(int rect_t, int arm_t, int track_t) {
    return overlay_seg_radius(rect_t) | (overlay_seg_radius(arm_t) << 8) | (overlay_seg_radius(track_t) << 16);
}
ADAS_HDI int overlay_obj_radius(const OverlayObjStyle& s, int which) { return (s.radii >> (8 * which)) & 0xff; }
ADAS_HDI int overlay_trunc_i32(double v) {        // astype(int) for what an image can hold: toward zero, saturated, NaN -> 0
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return (int)v;
}
ADAS_HDI uint32_t overlay_class_colour(int cls, const uint32_t* table, int n) {   // outside the table: 'unknown', black
    return (table && cls >= 0 && cls < n) ? table[cls] : 0u;
}
ADAS_HDI void overlay_object_bounds(OverlayObject* o, long long grow, int W, int H) {
    long long x0 = (o->x1 < o->x2 ? o->x1 : o->x2) - grow, x1 = (o->x1 < o->x2 ? o->x2 : o->x1) + grow;
    long long y0 = (o->y1 < o->y2 ? o->y1 : o->y2) - grow, y1 = (o->y1 < o->y2 ? o->y2 : o->y1) + grow;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > W - 1) x1 = W - 1;
    if (y1 > H - 1) y1 = H - 1;
    if (x0 > x1 || y0 > y1) {
        x0 = y0 = 1;
        x1 = y1 = 0;
    }
    o->bx0 = (int)x0; o->by0 = (int)y0; o->bx1 = (int)x1; o->by1 = (int)y1;
}
// cornerRect's box: l = max(1, int(min(ymax - ymin, xmax - xmin) * 0.2)), an fp64 product truncated toward zero
ADAS_HDI OverlayObject overlay_make_detection(const int* xyxy, uint32_t colour, const OverlayObjStyle& s, int W, int H) {
    OverlayObject o;
    o.kind = OV_OBJ_DET;
    o.x1 = xyxy[0]; o.y1 = xyxy[1]; o.x2 = xyxy[2]; o.y2 = xyxy[3];
    const long long dy = (long long)o.y2 - o.y1, dx = (long long)o.x2 - o.x1;
    const double p = (double)(dy < dx ? dy : dx) * 0.2;
    const int l = (int)p;   // |p| < 2^30
    o.l = l < 1 ? 1 : l;
    o.colour = colour;
    o.pad = 0;
    const int rr = overlay_obj_radius(s, OV_SEG_RECT), ra = overlay_obj_radius(s, OV_SEG_ARM);
    overlay_object_bounds(&o, (long long)o.l + (rr > ra ? rr : ra), W, H);
    return o;
}
// plot_bbox's box of a track that is activated: tlwh.astype(int), clamped to the image; OV_OBJ_NONE when tlwh[2] * tlwh[3] > min_box_area fails
ADAS_HDI OverlayObject overlay_make_track(const double* tlwh, int activated, double min_box_area, uint32_t colour, const OverlayObjStyle& s, int W,
                                         int H) {
    OverlayObject o;
    o.kind = OV_OBJ_NONE;
    o.x1 = o.y1 = o.x2 = o.y2 = o.l = o.pad = 0;
    o.colour = colour;
    o.bx0 = o.by0 = 1;
    o.bx1 = o.by1 = 0;
    if (!activated || !(tlwh[2] * tlwh[3] > min_box_area)) return o;
    const long long tx = overlay_trunc_i32(tlwh[0]), ty = overlay_trunc_i32(tlwh[1]), tw = overlay_trunc_i32(tlwh[2]), th = overlay_trunc_i32(tlwh[3]);
    const long long lo = -2147483647LL - 1;
    long long x2 = tx + tw < W ? tx + tw : W, y2 = ty + th < H ? ty + th : H;
    if (x2 < lo) x2 = lo;
    if (y2 < lo) y2 = lo;
    o.kind = OV_OBJ_TRACK;
    o.x1 = (int)(tx > 0 ? tx : 0); o.y1 = (int)(ty > 0 ? ty : 0); o.x2 = (int)x2; o.y2 = (int)y2;
    overlay_object_bounds(&o, overlay_obj_radius(s, OV_SEG_TRACK), W, H);
    return o;
}
// segment k of a box: 0 .. 3 the outline's edges (D7), for a detection 4 .. 11 the corner arms in cornerRect's order.  Returns the segment's
// radius and its half-widths in *hw.
ADAS_HDI int overlay_object_segments(const OverlayObject& o) { return o.kind == OV_OBJ_DET ? 12 : (o.kind == OV_OBJ_TRACK ? 4 : 0); }
ADAS_HDI int overlay_object_segment(const OverlayObject& o, int k, const OverlayObjStyle& s, long long* ax, long long* ay, long long* bx,
                                    long long* by, const int** hw) {
    const long long x1 = o.x1, y1 = o.y1, x2 = o.x2, y2 = o.y2, l = o.l;   // every field is read before any is chosen
    int which = o.kind == OV_OBJ_DET ? OV_SEG_RECT : OV_SEG_TRACK;
    if (k < 4) {
        overlay_rect_edge(x1, y1, x2, y2, k, ax, ay, bx, by);
    } else {
        const int a = k - 4, corner = a >> 1;                        // corners: top left, top right, bottom left, bottom right
        const long long cx = (corner & 1) ? x2 : x1, cy = (corner & 2) ? y2 : y1;
        *ax = cx; *ay = cy; *bx = cx; *by = cy;
        if (a & 1) *by = (corner & 2) ? cy - l : cy + l;            // the vertical arm, into the box
        else *bx = (corner & 1) ? cx - l : cx + l;                  // the horizontal arm
        which = OV_SEG_ARM;
    }
    *hw = s.hw + which * s.hw_stride;
    return overlay_obj_radius(s, which);
}
// what box o does to pixel (x, y), in this order: bit 0 its colour is written, bit 1 the pixel is tinted with it
ADAS_HDI int overlay_object_ops(const OverlayObject& o, int x, int y, const OverlayObjStyle& s) {
    if (x < o.bx0 || x > o.bx1 || y < o.by0 || y > o.by1) return 0;
    int ops = 0;
    // every segment lies on one of the lines x = x1, x = x2, y = y1, y = y2 and reaches at most its radius across it (a cap is a disc on a
    // point of its line): a pixel farther than the largest radius from all four lines is in no segment -- the box's interior, mostly
    const long long g = o.kind == OV_OBJ_DET ? (overlay_obj_radius(s, OV_SEG_RECT) > overlay_obj_radius(s, OV_SEG_ARM) ? overlay_obj_radius(s, OV_SEG_RECT)
                                                                                                                     : overlay_obj_radius(s, OV_SEG_ARM))
                                             : overlay_obj_radius(s, OV_SEG_TRACK);
    const long long dx1 = (long long)x - o.x1, dx2 = (long long)x - o.x2, dy1 = (long long)y - o.y1, dy2 = (long long)y - o.y2;
    const bool near = (dx1 >= -g && dx1 <= g) || (dx2 >= -g && dx2 <= g) || (dy1 >= -g && dy1 <= g) || (dy2 >= -g && dy2 <= g);
    const int n = near ? overlay_object_segments(o) : 0;
    for (int k = 0; k < n && !ops; ++k) {
        long long ax, ay, bx, by;
        const int* hw;
        const int R = overlay_object_segment(o, k, s, &ax, &ay, &bx, &by, &hw);
        if (overlay_seg_hit(ax, ay, bx, by, R, hw, x, y)) ops = 1;
    }
    if (o.kind == OV_OBJ_TRACK && x >= o.x1 && x < o.x2 && y >= o.y1 && y < o.y2) ops |= 2;
    return ops;
}
ADAS_HDI int overlay_object_channel(int v, int ops, uint32_t colour, int c) {
    const int k = (int)((colour >> (8 * c)) & 0xffu);
    if (ops & 1) v = k;
    if (ops & 2) v = overlay_tint(v, k);
    return v;
}

}  // namespace adas
