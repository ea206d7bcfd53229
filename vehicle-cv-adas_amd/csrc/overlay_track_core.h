// overlay_track_core.h -- what BYTETracker.DrawTrackedOnFrame(frame, show_box=False, show_traject=True) puts on the frame for a track
// (byteTracker.py:202-215): plot_trajectories' growing circles (ObjectTracker/core.py:188-197) and plot_directions' lock-on rectangle or
// shadowed arrow (core.py:57-66,105-171, strack.py:145-149).  Two parts, under overlay_core.h's terms (the definitions are the authority,
// parity with a real cv2 build UNPINNED, int64 coordinate arithmetic, no loop whose trip count is a coordinate, compiles for the host):
//
// The per-track arithmetic (overlay_track_prims), fp64, no contraction: a track is drawn iff it is activated and tlwh[2] * tlwh[3] >
// min_box_area.  T = its trajectory, oldest first.
//   circles    if len(T) > 1, for i = 0 .. len - 1: centre (int((x1 + x2) / 2), int(y2)), radius int(sqrt(i + 1) * 0.5), thickness
//              int(sqrt(i + 1) * 1.2) (the 30 pairs come from overlay_mark_table), class colour;
//   directions O = the boxes of T with x1 >= 10, y1 >= 10, x2 <= W - 10, y2 <= H - 10; per consecutive pair shift = |min(next - cur)| and
//              dir = next centre - cur centre if shift >= 2 else (0, 0); n = len(O) - 1.  With len(O) > 1, cx = tlwh[0] + tlwh[2] / 2,
//              cy = tlwh[1] + tlwh[3] / 2, rate = tlwh[2] / tlwh[3], h = tlwh[3], w = h * rate:
//   n < 5      fw = floor(w / 2), rw_ = (cx - (cx - fw)) / 5, sx = int((cx - fw) + rw_ * n), ex = int((cx + fw) - rw_ * n), the same in y:
//              the D7 outline (sx, sy) - (ex, ey) of thickness 2 in max(0, c - 10) per channel;
//   n >= 5     L = 1000 * min(h * w / (H * W), 0.02), md = the per-component median of the n directions (even n: (a + b) / 2 of the two
//              middle values), start = (int(cx), int(cy)), end = (int(cx + md.x * L), int(cy + md.y * L)), three D12 arrows:
//              (start.x - 2, start.y + 2) -> (end.x - 2, end.y + 2) in (100, 100, 100), t = 5, tip 0.3; start -> (end.x - 1, end.y - 1), white,
//              t = 2, tip 0.3 - 0.1; start -> end, white, t = 3, tip 0.3.
// int() is overlay_trunc_i32.  A track gives at most 30 circles + 9 segments: ADAS_OVERLAY_TRACK_PRIMS slots.
//
// The pixel rules:
//   D10 circle  (cx, cy, r, t), R = overlay_seg_radius(t): the union of D2 discs of radius R centred on every outline pixel, the outline being
//              the eight reflections of each (dx, dy) the midpoint walk of overlay_disc_halfwidths visits.  t == 1 (R = 0) is the outline
//              itself, r == 0 one pixel (with t = 2 a plus sign).  This is D6's "caps on the vertices" applied to the polyline OpenCV's
//              EllipseEx would draw.  A row may hold two runs (r > R): rows are ORed outline pixel by outline pixel.
//   D11 segment (a, b, t >= 2) of any slope, R = overlay_seg_radius(t): a D2 disc of radius R on each endpoint plus the body, the pixels p
//              with 0 <= v.d <= d.d and |v.x d.y - v.y d.x| <= Tq, d = b - a, v = p - a, Tq = floor(sqrt(R^2 d.d)) the exact integer square
//              root (the same set as cross^2 <= R^2 d.d).  A zero-length segment is its disc; t == 1 is the D3 line.  PROPERTY: for an
//              axis-aligned segment these are D6's pixels exactly (d = (L, 0): 0 <= v.x <= L, |v.y| L <= R L).  An endpoint with |x| or
//              |y| > ADAS_OVERLAY_COORD_MAX skips the primitive (ADAS_OVERLAY_TRACK_RANGE): every product then fits int64 with room to spare.
//   D12 arrow  (p1 -> p2, t, tip): the D11 segments p1 - p2, qa - p2, qb - p2 with u = p1 - p2, k = tip * 0.70710678118654752440,
//              qa = (rint(p2.x + k (u.x - u.y)), rint(p2.y + k (u.x + u.y))), qb = (rint(p2.x + k (u.x + u.y)), rint(p2.y + k (u.y - u.x))):
//              one multiply, one add and one rint (ties to even) per component.  This is OpenCV's pt2 + |u| tip (cos, sin)(atan2(u) +- pi / 4)
//              with the trigonometry removed algebraically -- deliberately, so that host and device cannot disagree in a transcendental.
//   fold       extends D9: per track in list order its outline and tint (TRACKS), then its circles in order, then its indicator; every
//              primitive writes its colour.  A pixel some primitive covers therefore ends as the colour of the LAST primitive that hits it
//              (track k), folded through the outline / tint of tracks k + 1 .. (overlay_object_ops / overlay_object_channel) when TRACKS is
//              on -- no earlier value of the pixel is needed.  DISTANCE still overrides everything.
#pragma once
#include <string.h>
#include "overlay_core.h"

namespace adas {

#define ADAS_OVERLAY_TRACK_PRIMS 40    // slots of one track: 30 circles + 9 segments
#define ADAS_OVERLAY_TRACK_RING 30     // a trajectory's depth (ADAS_TRAJECTORY_LEN)
#define ADAS_OVERLAY_TRACK_MAX_R 3     // largest disc radius of a primitive: thicknesses are the reference's, at most 6
#define ADAS_OVERLAY_TRACK_HW 8        // ints of one half-width table (radius 0 .. 3, padded)

#define OV_PRIM_NONE 0
#define OV_PRIM_CIRCLE 1
#define OV_PRIM_EDGE 2      // an edge of the lock-on rectangle: four in a row, D7's order
#define OV_PRIM_SHAFT 3     // an arrow's p1 - p2; its two tips follow
#define OV_PRIM_TIP 4       // q - p2
struct OverlayPrim {         // 64 bytes
    int kind;
    int ax, ay, bx, by;      // a circle's centre in (ax, ay); a segment's endpoints
    int r, t;                // a circle's radius; the thickness
    uint32_t colour;         // packed as overlay_pack_bgr does
    long long tq;            // a segment's Tq
    int x0, y0, x1, y1;      // every pixel it can touch, inside the image; empty (x0 > x1) when it touches none or is skipped
    int skip;                // 1: an endpoint out of range, not drawn
    int pad;
};
struct OverlayTrackHead {    // one track's list, 32 bytes
    int n;                   // primitives in its slots
    int x0, y0, x1, y1;      // the union of their boxes (empty: x0 > x1)
    int range;               // 1: some primitive was skipped
    int pad[2];
};
struct OverlayTrackStyle {
    const int* hw;           // overlay_disc_halfwidths of radius R at hw + R * ADAS_OVERLAY_TRACK_HW, R = 0 .. ADAS_OVERLAY_TRACK_MAX_R
};

// the (radius, thickness) of circle i, i = 0 .. 29: host only (sqrt is the host's correctly rounded one), uploaded with the launch
inline void overlay_mark_table(int* r, int* t) {
    for (int i = 0; i < ADAS_OVERLAY_TRACK_RING; ++i) {
        const double s = sqrt((double)(i + 1));
        const double a = s * 0.5, b = s * 1.2;
        r[i] = (int)a;
        t[i] = (int)b;
    }
}

ADAS_HDI void overlay_track_halfwidths(int R, int* hw_all) { overlay_disc_halfwidths(R, hw_all + R * ADAS_OVERLAY_TRACK_HW); }

// floor(sqrt(v)), exact; v < 2^62
ADAS_HDI long long overlay_isqrt(long long v) {
    if (v <= 0) return 0;
    long long s = (long long)sqrt((double)v);   // within one of the answer below 2^52; the two corrections make it exact
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}
ADAS_HDI long long overlay_floor_div(long long a, long long b) {   // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
ADAS_HDI long long overlay_ceil_div(long long a, long long b) {    // b > 0
    const long long q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}
ADAS_HDI bool overlay_coord_in_range(long long v) { return v <= ADAS_OVERLAY_COORD_MAX && v >= -ADAS_OVERLAY_COORD_MAX; }
ADAS_HDI int overlay_sat_i32(long long v) { return v > 2147483647LL ? 2147483647 : (v < -2147483647LL - 1 ? -2147483647 - 1 : (int)v); }

ADAS_HDI void overlay_prim_bounds(OverlayPrim* p, long long xa, long long ya, long long xb, long long yb, int W, int H) {
    if (xa < 0) xa = 0;
    if (ya < 0) ya = 0;
    if (xb > W - 1) xb = W - 1;
    if (yb > H - 1) yb = H - 1;
    if (xa > xb || ya > yb) {
        xa = ya = 1;
        xb = yb = 0;
    }
    p->x0 = (int)xa; p->y0 = (int)ya; p->x1 = (int)xb; p->y1 = (int)yb;
}
ADAS_HDI OverlayPrim overlay_make_circle(int cx, int cy, int r, int t, uint32_t colour, int W, int H) {
    OverlayPrim p;
    p.kind = OV_PRIM_CIRCLE;
    p.ax = cx; p.ay = cy; p.bx = cx; p.by = cy;
    p.r = r; p.t = t; p.colour = colour;
    p.tq = 0; p.skip = 0; p.pad = 0;
    const long long g = (long long)r + overlay_seg_radius(t);
    overlay_prim_bounds(&p, (long long)cx - g, (long long)cy - g, (long long)cx + g, (long long)cy + g, W, H);
    return p;
}
// D11's record; an endpoint out of range: kept for the record list, never drawn
ADAS_HDI OverlayPrim overlay_make_segment(int kind, long long ax, long long ay, long long bx, long long by, int t, uint32_t colour, int W, int H) {
    OverlayPrim p;
    p.kind = kind;
    p.ax = overlay_sat_i32(ax); p.ay = overlay_sat_i32(ay); p.bx = overlay_sat_i32(bx); p.by = overlay_sat_i32(by);
    p.r = 0; p.t = t; p.colour = colour;
    p.tq = 0; p.pad = 0;
    p.skip = !(overlay_coord_in_range(ax) && overlay_coord_in_range(ay) && overlay_coord_in_range(bx) && overlay_coord_in_range(by));
    p.x0 = p.y0 = 1;
    p.x1 = p.y1 = 0;
    if (p.skip) return p;
    const long long R = overlay_seg_radius(t), dx = bx - ax, dy = by - ay;
    p.tq = overlay_isqrt(R * R * (dx * dx + dy * dy));
    overlay_prim_bounds(&p, (ax < bx ? ax : bx) - R, (ay < by ? ay : by) - R, (ax < bx ? bx : ax) + R, (ay < by ? by : ay) + R, W, H);
    return p;
}
// D12's two tip points
ADAS_HDI void overlay_arrow_tips(long long p1x, long long p1y, long long p2x, long long p2y, double tip, long long* q) {
    const double k = tip * 0.70710678118654752440;
    const long long ux = p1x - p2x, uy = p1y - p2y;
    const double m0 = k * (double)(ux - uy), m1 = k * (double)(ux + uy), m2 = k * (double)(uy - ux);
    const double s0 = (double)p2x + m0, s1 = (double)p2y + m1, s2 = (double)p2x + m1, s3 = (double)p2y + m2;
    q[0] = overlay_trunc_i32(rint(s0)); q[1] = overlay_trunc_i32(rint(s1));
    q[2] = overlay_trunc_i32(rint(s2)); q[3] = overlay_trunc_i32(rint(s3));
}
ADAS_HDI int overlay_make_arrow(OverlayPrim* out, long long p1x, long long p1y, long long p2x, long long p2y, int t, double tip, uint32_t colour, int W,
                                int H) {
    long long q[4];
    overlay_arrow_tips(p1x, p1y, p2x, p2y, tip, q);
    out[0] = overlay_make_segment(OV_PRIM_SHAFT, p1x, p1y, p2x, p2y, t, colour, W, H);
    out[1] = overlay_make_segment(OV_PRIM_TIP, q[0], q[1], p2x, p2y, t, colour, W, H);
    out[2] = overlay_make_segment(OV_PRIM_TIP, q[2], q[3], p2x, p2y, t, colour, W, H);
    return 3;
}
ADAS_HDI uint32_t overlay_colour_minus(uint32_t c, int by) {   // max(0, channel - by): cv2 saturates the negative scalar
    uint32_t o = 0u;
    for (int k = 0; k < 3; ++k) {
        const int v = (int)((c >> (8 * k)) & 0xffu) - by;
        o |= (uint32_t)(v < 0 ? 0 : v) << (8 * k);
    }
    return o;
}
ADAS_HDI void overlay_sort_small(double* v, int n, int ws) {   // insertion sort where the values lie (element j at v[j * ws]), n <= 29
    for (int i = 1; i < n; ++i) {
        const double x = v[i * ws];
        int j = i - 1;
        while (j >= 0 && v[j * ws] > x) {
            v[(j + 1) * ws] = v[j * ws];
            --j;
        }
        v[(j + 1) * ws] = x;
    }
}
ADAS_HDI double overlay_median_sorted(const double* v, int n, int ws) {   // np.median: the mean of the two middle values for an even count
    if (n & 1) return v[(n / 2) * ws];
    const double s = v[(n / 2 - 1) * ws] + v[(n / 2) * ws];
    return s / 2.0;
}

// One track's primitives into out[ADAS_OVERLAY_TRACK_PRIMS], in drawing order; returns their number.  ring: the trajectory's boxes (tlbr),
// entry i (oldest first) at ring + ((start + i) % ADAS_OVERLAY_TRACK_RING) * 4, len of them; tab_r / tab_t: overlay_mark_table;
// work: 2 * (ADAS_OVERLAY_TRACK_RING - 1) doubles, element j at work[j * ws].
ADAS_HDI int overlay_track_prims(const double* tlwh, int activated, double min_box_area, uint32_t colour, const double* ring, int start, int len,
                                 const int* tab_r, const int* tab_t, int W, int H, double* work, int ws, OverlayPrim* out, int* range) {
    *range = 0;
    if (!activated || !(tlwh[2] * tlwh[3] > min_box_area)) return 0;
    len = len < 0 ? 0 : (len > ADAS_OVERLAY_TRACK_RING ? ADAS_OVERLAY_TRACK_RING : len);
    int n = 0;
    int m = 0;   // boxes that passed the border filter so far
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
    const int NW = ADAS_OVERLAY_TRACK_RING - 1;
    for (int i = 0; i < len; ++i) {
        const double* b = ring + (size_t)((start + i) % ADAS_OVERLAY_TRACK_RING) * 4;
        const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
        if (len > 1) {
            const double sx = b0 + b2;
            out[n++] = overlay_make_circle(overlay_trunc_i32(sx / 2.0), overlay_trunc_i32(b3), tab_r[i], tab_t[i], colour, W, H);
        }
        if (b0 >= 10.0 && b1 >= 10.0 && b2 <= (double)(W - 10) && b3 <= (double)(H - 10)) {
            if (m > 0) {
                const double d0 = b0 - p0, d1 = b1 - p1, d2 = b2 - p2, d3 = b3 - p3;
                double mn = d0;
                if (d1 < mn) mn = d1;
                if (d2 < mn) mn = d2;
                if (d3 < mn) mn = d3;
                double dx = 0.0, dy = 0.0;
                if (fabs(mn) >= 2.0) {
                    const double ncx = (b0 + b2) / 2.0, ncy = (b1 + b3) / 2.0, ccx = (p0 + p2) / 2.0, ccy = (p1 + p3) / 2.0;
                    dx = ncx - ccx;
                    dy = ncy - ccy;
                }
                work[(m - 1) * ws] = dx;
                work[(NW + m - 1) * ws] = dy;
            }
            p0 = b0; p1 = b1; p2 = b2; p3 = b3;
            ++m;
        }
    }
    if (m > 1) {
        const int nd = m - 1;
        const double hx = tlwh[2] / 2.0, hy = tlwh[3] / 2.0;
        const double cx = tlwh[0] + hx, cy = tlwh[1] + hy, rate = tlwh[2] / tlwh[3], h = tlwh[3];
        const double w = h * rate;
        if (nd < 5) {
            const double fw = floor(w / 2.0), fh = floor(h / 2.0);
            const double lx = cx - fw, ly = cy - fh, ux = cx + fw, uy = cy + fh;
            const double rw_ = (cx - lx) / 5.0, rh_ = (cy - ly) / 5.0;
            const double ax = rw_ * (double)nd, ay = rh_ * (double)nd;
            const long long sx = overlay_trunc_i32(lx + ax), sy = overlay_trunc_i32(ly + ay), ex = overlay_trunc_i32(ux - ax), ey = overlay_trunc_i32(uy - ay);
            const uint32_t c = overlay_colour_minus(colour, 10);
            for (int k = 0; k < 4; ++k) {
                long long ea, eb, ec, ed;
                overlay_rect_edge(sx, sy, ex, ey, k, &ea, &eb, &ec, &ed);
                out[n++] = overlay_make_segment(OV_PRIM_EDGE, ea, eb, ec, ed, 2, c, W, H);
            }
        } else {
            const double hwp = h * w, fr = (double)H * (double)W;
            const double q = hwp / fr;
            const double L = 1000.0 * (0.02 < q ? 0.02 : q);
            overlay_sort_small(work, nd, ws);   // the medians: each component sorted where it lies
            overlay_sort_small(work + (size_t)NW * ws, nd, ws);
            const double mdx = overlay_median_sorted(work, nd, ws), mdy = overlay_median_sorted(work + (size_t)NW * ws, nd, ws);
            const double tx = mdx * L, ty = mdy * L;
            const long long s0 = overlay_trunc_i32(cx), s1 = overlay_trunc_i32(cy), e0 = overlay_trunc_i32(cx + tx), e1 = overlay_trunc_i32(cy + ty);
            const uint32_t white = 0xffffffu, grey = 100u | (100u << 8) | (100u << 16);
            const double tip = 0.3, tip2 = tip - 0.1;
            n += overlay_make_arrow(out + n, s0 - 2, s1 + 2, e0 - 2, e1 + 2, 5, tip, grey, W, H);
            n += overlay_make_arrow(out + n, s0, s1, e0 - 1, e1 - 1, 2, tip2, white, W, H);
            n += overlay_make_arrow(out + n, s0, s1, e0, e1, 3, tip, white, W, H);
        }
    }
    for (int i = 0; i < n; ++i)
        if (out[i].skip) *range = 1;
    return n;
}
ADAS_HDI OverlayTrackHead overlay_track_head(const OverlayPrim* p, int n, int range) {
    OverlayTrackHead h;
    h.n = n; h.range = range; h.pad[0] = h.pad[1] = 0;
    h.x0 = h.y0 = 1;
    h.x1 = h.y1 = 0;
    for (int i = 0; i < n; ++i) {
        if (p[i].x0 > p[i].x1) continue;
        if (h.x0 > h.x1) {
            h.x0 = p[i].x0; h.y0 = p[i].y0; h.x1 = p[i].x1; h.y1 = p[i].y1;
        } else {
            h.x0 = p[i].x0 < h.x0 ? p[i].x0 : h.x0; h.y0 = p[i].y0 < h.y0 ? p[i].y0 : h.y0;
            h.x1 = p[i].x1 > h.x1 ? p[i].x1 : h.x1; h.y1 = p[i].y1 > h.y1 ? p[i].y1 : h.y1;
        }
    }
    return h;
}

// One track's primitives as the public record list (M: adas_overlay_track_mark; kinds 1 circle, 2 rectangle, 3 arrow): a rectangle is four
// edges in a row, an arrow a shaft and two tips.  Marks [n, ...) are appended while they fit max_marks; returns the new total.  Host only.
template <class M>
inline int overlay_track_marks(const OverlayPrim* p, int np, int track, M* marks, int max_marks, int n) {
    np = np < 0 ? 0 : (np > ADAS_OVERLAY_TRACK_PRIMS ? ADAS_OVERLAY_TRACK_PRIMS : np);
    for (int i = 0; i < np;) {
        M m;
        memset(&m, 0, sizeof(m));
        m.track = track;
        m.x1 = p[i].ax; m.y1 = p[i].ay; m.x2 = p[i].bx; m.y2 = p[i].by;
        m.radius = p[i].r; m.thickness = p[i].t;
        for (int c = 0; c < 3; ++c) m.color[c] = (uint8_t)(p[i].colour >> (8 * c));
        int span = 1;
        if (p[i].kind == OV_PRIM_CIRCLE) {
            m.kind = 1;
        } else if (p[i].kind == OV_PRIM_EDGE && i + 3 < np) {
            m.kind = 2;
            m.x2 = p[i + 1].bx; m.y2 = p[i + 1].by;   // edges (x1, y1) - (x2, y1), (x2, y1) - (x2, y2), ...
            span = 4;
        } else if (p[i].kind == OV_PRIM_SHAFT && i + 2 < np) {
            m.kind = 3;
            m.tip[0] = p[i + 1].ax; m.tip[1] = p[i + 1].ay; m.tip[2] = p[i + 2].ax; m.tip[3] = p[i + 2].ay;
            span = 3;
        }
        for (int j = 0; j < span; ++j) m.skipped |= (uint8_t)(p[i + j].skip ? 1 << j : 0);
        if (n < max_marks) marks[n] = m;
        ++n;
        i += span;
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------- pixels
ADAS_HDI bool overlay_disc_has(long long ddx, long long ddy, int R, const int* hw) {   // (ddx, ddy) from the centre of a D2 disc of radius R
    const long long j = ddy < 0 ? -ddy : ddy, i = ddx < 0 ? -ddx : ddx;
    return j <= R && i <= hw[j];
}
struct OverlayWalk {   // the midpoint walk of overlay_disc_halfwidths, one (dx, dy) per step
    int dx, dy, err, plus, minus;
};
ADAS_HDI void overlay_walk_begin(OverlayWalk* w, int r) {
    w->dx = r; w->dy = 0; w->err = 0; w->plus = 1; w->minus = 2 * r - 1;
}
ADAS_HDI bool overlay_walk_live(const OverlayWalk& w) { return w.dx >= w.dy; }
ADAS_HDI void overlay_walk_step(OverlayWalk* w) {
    ++w->dy;
    w->err += w->plus;
    w->plus += 2;
    if (w->err > 0) {
        w->err -= w->minus;
        --w->dx;
        w->minus -= 2;
    }
}
// reflection k (0 .. 7) of the walk's (dx, dy)
ADAS_HDI void overlay_walk_reflect(const OverlayWalk& w, int k, long long* ox, long long* oy) {
    const long long a = (k & 4) ? w.dy : w.dx, b = (k & 4) ? w.dx : w.dy;
    *ox = (k & 1) ? -a : a;
    *oy = (k & 2) ? -b : b;
}
// D10
ADAS_HDI bool overlay_circle_hit(const OverlayPrim& p, const OverlayTrackStyle& s, int x, int y) {
    const int R = overlay_seg_radius(p.t);
    const int* hw = s.hw + R * ADAS_OVERLAY_TRACK_HW;
    const long long X = (long long)x - p.ax, Y = (long long)y - p.ay;
    OverlayWalk w;
    for (overlay_walk_begin(&w, p.r); overlay_walk_live(w); overlay_walk_step(&w))   // at most r + 1 steps, r <= ADAS_OVERLAY_MAX_RADIUS
        for (int k = 0; k < 8; ++k) {
            long long ox, oy;
            overlay_walk_reflect(w, k, &ox, &oy);
            if (overlay_disc_has(X - ox, Y - oy, R, hw)) return true;
        }
    return false;
}
// the circle's runs on row y, clipped to the image: ops.fill(xl, xr) per outline pixel whose disc meets the row
template <class Ops>
ADAS_HDI void overlay_circle_row(const OverlayPrim& p, const OverlayTrackStyle& s, int y, int W, Ops& ops) {
    const int R = overlay_seg_radius(p.t);
    const int* hw = s.hw + R * ADAS_OVERLAY_TRACK_HW;
    OverlayWalk w;
    for (overlay_walk_begin(&w, p.r); overlay_walk_live(w); overlay_walk_step(&w))
        for (int k = 0; k < 8; ++k) {
            long long ox, oy;
            overlay_walk_reflect(w, k, &ox, &oy);
            long long j = (long long)y - ((long long)p.ay + oy);
            if (j < 0) j = -j;
            if (j > R) continue;
            long long xl = (long long)p.ax + ox - hw[j], xr = (long long)p.ax + ox + hw[j];
            if (xl < 0) xl = 0;
            if (xr > W - 1) xr = W - 1;
            if (xl <= xr) ops.fill((int)xl, (int)xr);
        }
}
// D11
ADAS_HDI bool overlay_segment_hit(const OverlayPrim& p, const OverlayTrackStyle& s, int x, int y) {
    if (p.t < 2) {   // the D3 line
        long long xl, xr;
        return overlay_line_row(p.ax, p.ay, p.bx, p.by, y, &xl, &xr) && x >= xl && x <= xr;
    }
    const int R = overlay_seg_radius(p.t);
    const int* hw = s.hw + R * ADAS_OVERLAY_TRACK_HW;
    const long long vx = (long long)x - p.ax, vy = (long long)y - p.ay;
    if (overlay_disc_has(vx, vy, R, hw) || overlay_disc_has((long long)x - p.bx, (long long)y - p.by, R, hw)) return true;
    const long long dx = (long long)p.bx - p.ax, dy = (long long)p.by - p.ay;
    const long long dd = dx * dx + dy * dy;
    if (dd == 0) return false;
    const long long dot = vx * dx + vy * dy;
    if (dot < 0 || dot > dd) return false;
    const long long cr = vx * dy - vy * dx;
    return (cr < 0 ? -cr : cr) <= p.tq;
}
// the integers v with lo <= k v + c <= hi, intersected with [*l, *r]: false when none is left
ADAS_HDI bool overlay_lin_range(long long k, long long c, long long lo, long long hi, long long* l, long long* r) {
    if (k == 0) return lo <= c && c <= hi;
    if (k < 0) {
        const long long nlo = -hi, nhi = -lo;
        k = -k; c = -c; lo = nlo; hi = nhi;
    }
    const long long a = overlay_ceil_div(lo - c, k), b = overlay_floor_div(hi - c, k);
    if (a > *l) *l = a;
    if (b < *r) *r = b;
    return *l <= *r;
}
template <class Ops>
ADAS_HDI void overlay_segment_row(const OverlayPrim& p, const OverlayTrackStyle& s, int y, int W, Ops& ops) {
    long long xl, xr;
    if (p.t < 2) {
        if (!overlay_line_row(p.ax, p.ay, p.bx, p.by, y, &xl, &xr)) return;
        if (xl < 0) xl = 0;
        if (xr > W - 1) xr = W - 1;
        if (xl <= xr) ops.fill((int)xl, (int)xr);
        return;
    }
    const int R = overlay_seg_radius(p.t);
    const int* hw = s.hw + R * ADAS_OVERLAY_TRACK_HW;
    for (int e = 0; e < 2; ++e) {   // the end discs
        const long long cx = e ? p.bx : p.ax, cy = e ? p.by : p.ay;
        long long j = (long long)y - cy;
        if (j < 0) j = -j;
        if (j > R) continue;
        xl = cx - hw[j]; xr = cx + hw[j];
        if (xl < 0) xl = 0;
        if (xr > W - 1) xr = W - 1;
        if (xl <= xr) ops.fill((int)xl, (int)xr);
    }
    const long long dx = (long long)p.bx - p.ax, dy = (long long)p.by - p.ay;
    const long long dd = dx * dx + dy * dy;
    if (dd == 0) return;
    const long long vy = (long long)y - p.ay;
    long long l = -(long long)p.ax, r = (long long)(W - 1) - p.ax;   // v.x of the image's columns
    if (!overlay_lin_range(dx, vy * dy, 0, dd, &l, &r)) return;
    if (!overlay_lin_range(dy, -vy * dx, -p.tq, p.tq, &l, &r)) return;
    ops.fill((int)(l + p.ax), (int)(r + p.ax));
}
ADAS_HDI bool overlay_prim_hit(const OverlayPrim& p, const OverlayTrackStyle& s, int x, int y) {
    if (x < p.x0 || x > p.x1 || y < p.y0 || y > p.y1) return false;
    return p.kind == OV_PRIM_CIRCLE ? overlay_circle_hit(p, s, x, y) : overlay_segment_hit(p, s, x, y);
}
template <class Ops>
ADAS_HDI void overlay_prim_row(const OverlayPrim& p, const OverlayTrackStyle& s, int y, int W, Ops& ops) {
    if (y < p.y0 || y > p.y1) return;
    if (p.kind == OV_PRIM_CIRCLE) overlay_circle_row(p, s, y, W, ops);
    else overlay_segment_row(p, s, y, W, ops);
}
// The fold at a pixel some primitive may cover.  heads [nt], prims [nt][ADAS_OVERLAY_TRACK_PRIMS]: the frame's lists; objs: the tracks'
// OverlayObject records, row k at objs[k], or null with TRACKS off.  Returns false when no primitive hits (the pixel stays); else bgr[3].
ADAS_HDI bool overlay_track_pixel(const OverlayTrackHead* heads, const OverlayPrim* prims, int nt, const OverlayTrackStyle& s, const OverlayObject* objs,
                                  const OverlayObjStyle& os, int x, int y, int* bgr) {
    for (int k = nt - 1; k >= 0; --k) {
        const OverlayTrackHead& h = heads[k];
        if (x < h.x0 || x > h.x1 || y < h.y0 || y > h.y1) continue;
        const OverlayPrim* p = prims + (size_t)k * ADAS_OVERLAY_TRACK_PRIMS;
        for (int i = h.n - 1; i >= 0; --i) {
            if (!overlay_prim_hit(p[i], s, x, y)) continue;
            const uint32_t c = p[i].colour;
            bgr[0] = (int)(c & 0xffu); bgr[1] = (int)((c >> 8) & 0xffu); bgr[2] = (int)((c >> 16) & 0xffu);
            if (objs)
                for (int j = k + 1; j < nt; ++j) {
                    const int ops = overlay_object_ops(objs[j], x, y, os);
                    if (!ops) continue;
                    for (int ch = 0; ch < 3; ++ch) bgr[ch] = overlay_object_channel(bgr[ch], ops, objs[j].colour, ch);
                }
            return true;
        }
    }
    return false;
}

}  // namespace adas
