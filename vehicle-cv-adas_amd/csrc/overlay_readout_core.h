// overlay_readout_core.h -- what PerspectiveTransformation.calcCurveAndOffset puts on the bird-view image it is handed
// (perspectiveTransformation.py:205-213): the white arrow at the vehicle's position, the grey arrow at the image centre and the two red
// strings 'Offset: %.1f m' and 'R : %.1f m'.  DrawDetectedOnBirdView's discs come on top (demo.py:292 before :299).  Compiled for the
// device (overlay_readout.hip) and for the host (tests/hostemu/emu_overlay_readout.cpp); restated in NumPy by tests/readout_ref.py.
// Under overlay_core.h's terms: int64 coordinate arithmetic, no loop whose trip count is a coordinate, fp64 without contraction, int() is
// overlay_trunc_i32; THE DEFINITIONS HERE ARE THE AUTHORITY, parity with a real cv2 build is UNPINNED.
// Per frame: direction (int32), veh_pos, curvature, offset (fp64), the bird size (Wb, Hb).
//   R0 gate    a frame is drawn only when direction != LANE_DIR_NONE (0).  STATED DIVERGENCE: the reference draws whenever both ego lanes
//              are non-empty; lane_core.h fits only when both have at least 3 points and Hb > 719.  A frame that fails is not touched.
//   R1 arrow A D12 arrow (int(veh_pos), Hb - 1) -> (int(veh_pos), int((double)Wb / 3)), colour (255, 255, 255), t = 5, tip 0.2.  The end
//              row uses the WIDTH: the reference writes img.shape[1] / 3.
//   R2 arrow B D12 arrow (int(Wb / 2.), Hb - 1) -> (int(Wb / 2.), int((double)Hb / 1.3)), colour (150, 150, 150), t = 10, tip 0.5: radius
//              5, above ADAS_OVERLAY_TRACK_MAX_R -- the readouts carry a half-width table of their own, radius 0 .. READOUT_MAX_R, in
//              overlay_track_core.h's layout (radius R at hw + R * ADAS_OVERLAY_TRACK_HW).
//   R3 strings "Offset: " + fmt1(offset) + " m" at (20, 80) and "R : " + fmt1(curvature) + " m" at (20, 180), colour (0, 0, 255); fmt1 is
//              T1's '%.1f' (nan / inf as Python prints them); finite |x| >= 2^30 skips that string and sets READOUT_FLAG_RANGE.
//   R4 zoom    the run is laid out at zoom 1 relative to its origin (T2 / T3): glyph pixel (u, v), u = (pen >> 16) + bearing_x + col,
//              v = row - baseline_row, covers the real pixels (x + z u + i, y + z v + j), i, j in 0 .. z - 1, with that glyph pixel's
//              coverage, blended per T4 and clipped per pixel.  z in 1 .. 4.  STATED DIVERGENCE: nearest-neighbour magnified glyphs (the
//              caller renders its atlas at fontScale 3 / z; a cell is at most 64 rows).
//   R5 order   arrow A, arrow B, string 1, string 2 (then the bird stage's discs): a byte ends as if they were painted one after another.
//              A primitive with an endpoint beyond ADAS_OVERLAY_COORD_MAX is skipped with READOUT_FLAG_RANGE (D11); NaN veh_pos truncates to 0.
//   R6 record  per frame: drawn, flags, the six D11 segments (two arrows: shaft, tip, tip) with their boxes and Tq, the two strings with
//              their origins, clipped boxes and characters, and the union box.
#pragma once
#include "overlay_track_core.h"
#include "overlay_text_core.h"

namespace adas {

constexpr int READOUT_MAX_R = 5;                                              // arrow B: t = 10
constexpr int READOUT_HW_INTS = (READOUT_MAX_R + 1) * ADAS_OVERLAY_TRACK_HW;  // the half-width tables of radius 0 .. 5
constexpr int READOUT_MAX_ZOOM = 4;
constexpr int READOUT_CHARS = 32;                                             // "Offset: " + at most 13 characters + " m"
constexpr int READOUT_FLAG_RANGE = 1;
constexpr int READOUT_DIR_NONE = 0;                                           // LANE_DIR_NONE
constexpr int READOUT_PRIMS = 6, READOUT_STRINGS = 2;

struct ReadoutStyle {   // adas_overlay_readout_style
    int32_t slot, zoom;
    int32_t offset_x, offset_y, radius_x, radius_y;   // the strings' origins: (20, 80), (20, 180)
    uint8_t text_color[3], arrow_a_color[3], arrow_b_color[3];
    uint8_t pad[3];
};

struct ReadoutString {   // 64 bytes
    int32_t x, y;                 // the origin
    int32_t bx0, by0, bx1, by1;   // every pixel it can touch, inside the image, half open; empty: bx0 >= bx1
    int32_t len;                  // 0: not drawn
    int32_t skipped;              // 1: out of range
    char text[READOUT_CHARS];
};

struct ReadoutRecord {   // one frame
    int32_t drawn, flags;
    int32_t x0, y0, x1, y1;       // the union of the items' boxes, inclusive; empty: x0 > x1
    int32_t pad[2];
    OverlayPrim prims[READOUT_PRIMS];
    ReadoutString str[READOUT_STRINGS];
};

ADAS_HDI void readout_default_style(ReadoutStyle* s) {
    s->slot = 10; s->zoom = 2;
    s->offset_x = 20; s->offset_y = 80; s->radius_x = 20; s->radius_y = 180;
    for (int c = 0; c < 3; ++c) {
        s->text_color[c] = c == 2 ? 255 : 0;
        s->arrow_a_color[c] = 255;
        s->arrow_b_color[c] = 150;
        s->pad[c] = 0;
    }
}

ADAS_HDI void readout_halfwidths(int* hw) {   // hw[READOUT_HW_INTS]
    for (int i = 0; i < READOUT_HW_INTS; ++i) hw[i] = 0;
    for (int R = 0; R <= READOUT_MAX_R; ++R) overlay_track_halfwidths(R, hw);
}

// R1 / R2: arrow k (0: A, 1: B) into out[3]
ADAS_HDI void readout_arrow(int k, double veh_pos, int Wb, int Hb, const ReadoutStyle& st, OverlayPrim* out) {
    if (k == 0) {
        const long long x = overlay_trunc_i32(veh_pos);
        const double third = (double)Wb / 3;
        overlay_make_arrow(out, x, (long long)Hb - 1, x, overlay_trunc_i32(third), 5, 0.2, overlay_pack_bgr(st.arrow_a_color), Wb, Hb);
    } else {
        const double half = (double)Wb / 2., low = (double)Hb / 1.3;
        const long long x = overlay_trunc_i32(half);
        overlay_make_arrow(out, x, (long long)Hb - 1, x, overlay_trunc_i32(low), 10, 0.5, overlay_pack_bgr(st.arrow_b_color), Wb, Hb);
    }
}

ADAS_HDI int readout_floor_div(int a, int z) {   // z > 0; a is a pixel minus an origin: |a| < 2^30 + 2^15
    const int q = a / z;
    return (a % z != 0 && a < 0) ? q - 1 : q;
}

// R3 / R4: string k (0: the offset, 1: the radius) of value v
ADAS_HDI void readout_string(int k, double v, int Wb, int Hb, const ReadoutStyle& st, const TextFont& f, ReadoutString* s) {
    s->x = k ? st.radius_x : st.offset_x;
    s->y = k ? st.radius_y : st.offset_y;
    s->bx0 = s->by0 = s->bx1 = s->by1 = 0;
    s->len = 0; s->skipped = 0;
    for (int i = 0; i < READOUT_CHARS; ++i) s->text[i] = 0;
    char num[16];
    const int nl = text_format_fixed(v, 1, num);
    if (nl < 0) { s->skipped = 1; return; }
    const char* head = k ? "R : " : "Offset: ";
    int n = 0;
    while (*head) s->text[n++] = *head++;
    for (int i = 0; i < nl; ++i) s->text[n++] = num[i];
    s->text[n++] = ' '; s->text[n++] = 'm';
    s->len = n;
    long long pen = 0, lo = 0, hi = 0;   // the run at zoom 1 relative to its origin
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const int g = text_glyph(s->text[i]);
        const long long gx0 = (pen >> 16) + f.bearing_x[g];
        if (f.glyph_w[g] > 0) {
            if (!any || gx0 < lo) lo = gx0;
            if (!any || gx0 + f.glyph_w[g] > hi) hi = gx0 + f.glyph_w[g];
            any = true;
        }
        pen += f.advance[g];
    }
    if (!any) return;
    const long long z = st.zoom;
    long long x0 = s->x + z * lo, x1 = s->x + z * hi, y0 = s->y - z * f.baseline_row, y1 = s->y + z * ((long long)f.cell_h - f.baseline_row);
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > Wb) x1 = Wb;
    if (y1 > Hb) y1 = Hb;
    if (x0 >= x1 || y0 >= y1) return;
    s->bx0 = (int32_t)x0; s->by0 = (int32_t)y0; s->bx1 = (int32_t)x1; s->by1 = (int32_t)y1;
}

// item k of the frame's record: 0, 1 the arrows, 2, 3 the strings (independent of one another: a lane each on the device)
ADAS_HDI void readout_item(int k, double veh_pos, double curvature, double offset, int Wb, int Hb, const ReadoutStyle& st, const TextFont& f,
                           ReadoutRecord* r) {
    if (k < 2) readout_arrow(k, veh_pos, Wb, Hb, st, r->prims + 3 * k);
    else readout_string(k - 2, k == 2 ? offset : curvature, Wb, Hb, st, f, r->str + (k - 2));
}

// R0 for a frame that fails the gate: an empty record
ADAS_HDI void readout_clear(ReadoutRecord* r) {
    r->drawn = 0; r->flags = 0;
    r->x0 = r->y0 = 1; r->x1 = r->y1 = 0;
    r->pad[0] = r->pad[1] = 0;
    for (int i = 0; i < READOUT_PRIMS; ++i) {
        OverlayPrim& p = r->prims[i];
        p.kind = OV_PRIM_NONE; p.ax = p.ay = p.bx = p.by = 0; p.r = p.t = 0; p.colour = 0u; p.tq = 0;
        p.x0 = p.y0 = 1; p.x1 = p.y1 = 0; p.skip = 0; p.pad = 0;
    }
    for (int k = 0; k < READOUT_STRINGS; ++k) {
        ReadoutString& s = r->str[k];
        s.x = s.y = s.bx0 = s.by0 = s.bx1 = s.by1 = s.len = s.skipped = 0;
        for (int i = 0; i < READOUT_CHARS; ++i) s.text[i] = 0;
    }
}

// the head of a drawn frame's record, after its four items: flags and the union box
ADAS_HDI void readout_finish(ReadoutRecord* r) {
    r->drawn = 1; r->flags = 0;
    r->pad[0] = r->pad[1] = 0;
    int x0 = 1, y0 = 1, x1 = 0, y1 = 0;
    for (int i = 0; i < READOUT_PRIMS + READOUT_STRINGS; ++i) {
        int a, b, c, d;
        if (i < READOUT_PRIMS) {
            const OverlayPrim& p = r->prims[i];
            if (p.skip) r->flags |= READOUT_FLAG_RANGE;
            a = p.x0; b = p.y0; c = p.x1; d = p.y1;
        } else {
            const ReadoutString& s = r->str[i - READOUT_PRIMS];
            if (s.skipped) r->flags |= READOUT_FLAG_RANGE;
            a = s.bx0; b = s.by0; c = s.bx1 - 1; d = s.by1 - 1;
        }
        if (a > c || b > d) continue;
        if (x0 > x1) { x0 = a; y0 = b; x1 = c; y1 = d; }
        else {
            x0 = a < x0 ? a : x0; y0 = b < y0 ? b : y0;
            x1 = c > x1 ? c : x1; y1 = d > y1 ? d : y1;
        }
    }
    r->x0 = x0; r->y0 = y0; r->x1 = x1; r->y1 = y1;
}

// one frame's record, the items one after another (the host's form; the device gives items 0 .. 3 a lane each)
ADAS_HDI void readout_layout(int direction, double veh_pos, double curvature, double offset, int Wb, int Hb, const ReadoutStyle& st, const TextFont& f,
                             ReadoutRecord* r) {
    if (direction == READOUT_DIR_NONE) { readout_clear(r); return; }
    for (int k = 0; k < 4; ++k) readout_item(k, veh_pos, curvature, offset, Wb, Hb, st, f, r);
    readout_finish(r);
}

// the bytes [*c0, *c1) of a row that the items whose boxes meet rows [r0, r1) span; false: none does (a draw workgroup's band: the union
// box of the whole record would have it walk the empty rows and columns between a string at the top and an arrow at the bottom)
ADAS_HDI bool readout_band_span(const ReadoutRecord& r, int r0, int r1, int* c0, int* c1) {
    int x0 = 0x7fffffff, x1 = -1;
    for (int i = 0; i < READOUT_PRIMS; ++i) {
        const OverlayPrim& p = r.prims[i];
        if (p.x0 > p.x1 || p.y0 >= r1 || p.y1 < r0) continue;
        x0 = p.x0 < x0 ? p.x0 : x0;
        x1 = p.x1 > x1 ? p.x1 : x1;
    }
    for (int k = 0; k < READOUT_STRINGS; ++k) {
        const ReadoutString& s = r.str[k];
        if (s.bx0 >= s.bx1 || s.by0 >= r1 || s.by1 <= r0) continue;
        x0 = s.bx0 < x0 ? s.bx0 : x0;
        x1 = s.bx1 - 1 > x1 ? s.bx1 - 1 : x1;
    }
    if (x0 > x1) return false;
    *c0 = x0 * 3;
    *c1 = (x1 + 1) * 3;
    return true;
}

// does some item's box meet bytes [lo, hi) of row `row`
ADAS_HDI bool readout_meets(const ReadoutRecord& r, int row, int lo, int hi) {
    for (int i = 0; i < READOUT_PRIMS; ++i) {
        const OverlayPrim& p = r.prims[i];
        if (p.x0 <= p.x1 && row >= p.y0 && row <= p.y1 && p.x0 * 3 < hi && (p.x1 + 1) * 3 > lo) return true;
    }
    for (int k = 0; k < READOUT_STRINGS; ++k) {
        const ReadoutString& s = r.str[k];
        if (s.bx0 < s.bx1 && row >= s.by0 && row < s.by1 && s.bx0 * 3 < hi && s.bx1 * 3 > lo) return true;
    }
    return false;
}

// R5 on one 16-byte piece: w holds bytes [b0, b0 + 16) of row `row` of the frame's bird image (b0 relative to the row's first byte, any
// sign); only bytes [lo, hi) of the row are the caller's.  The bytes some item paints are replaced; returns whether any was.
// The pixels of a piece are independent of one another, so the order R5 gives each of them is kept by painting item after item over the
// whole piece: the arrows (a written colour: the last primitive that hits a pixel decides), then string 1 and string 2 glyph by glyph -- a
// glyph whose columns miss the piece is passed over with two comparisons.
ADAS_HDI bool readout_fold_piece(const ReadoutRecord& r, const ReadoutStyle& st, const TextFont& f, const int* hw, int row, int b0, int lo, int hi,
                                 uint32_t w[4]) {
    if (lo >= hi) return false;
    bool any = false;
    const int p0 = lo / 3, p1 = (hi - 1) / 3;   // lo >= 0: at most 6 pixels
    bool prims = false;
    for (int i = 0; i < READOUT_PRIMS; ++i) {
        const OverlayPrim& p = r.prims[i];
        prims = prims || (p.x0 <= p.x1 && row >= p.y0 && row <= p.y1 && p.x0 <= p1 && p.x1 >= p0);
    }
    if (prims) {
        const OverlayTrackStyle ts = {hw};
        for (int px = p0; px <= p1; ++px)
            for (int i = READOUT_PRIMS - 1; i >= 0; --i) {
                const OverlayPrim& p = r.prims[i];
                if (!overlay_prim_hit(p, ts, px, row)) continue;   // a skipped primitive has an empty box
                for (int ch = 0; ch < 3; ++ch) {
                    const int b = px * 3 + ch, j = b - b0;
                    if (b < lo || b >= hi) continue;
                    w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (((p.colour >> (8 * ch)) & 0xffu) << (8 * (j & 3)));
                    any = true;
                }
                break;
            }
    }
    const int z = st.zoom;
    for (int k = 0; k < READOUT_STRINGS; ++k) {
        const ReadoutString& s = r.str[k];
        if (row < s.by0 || row >= s.by1 || s.bx0 > p1 || s.bx1 <= p0) continue;
        const int ar = readout_floor_div(row - s.y, z) + f.baseline_row;
        if (ar < 0 || ar >= f.cell_h) continue;
        const uint8_t* arow = f.atlas + (long long)ar * f.atlas_w;
        const int q0 = p0 > s.bx0 ? p0 : s.bx0, q1 = p1 < s.bx1 - 1 ? p1 : s.bx1 - 1;   // the string's pixels of the piece
        const long long u0 = readout_floor_div(q0 - s.x, z), u1 = readout_floor_div(q1 - s.x, z);
        long long pen = 0;
        for (int i = 0; i < s.len; ++i) {
            const int g = text_glyph(s.text[i]);
            const long long gx0 = (pen >> 16) + f.bearing_x[g];
            pen += f.advance[g];
            const int gw = f.glyph_w[g];
            if (gw <= 0 || gx0 + gw <= u0 || gx0 > u1) continue;
            const uint8_t* gp = arow + f.glyph_x[g];
            for (int px = q0; px <= q1; ++px) {
                const long long col = readout_floor_div(px - s.x, z) - gx0;
                if (col < 0 || col >= gw) continue;
                const uint32_t cov = gp[col];
                if (!cov) continue;
                for (int ch = 0; ch < 3; ++ch) {
                    const int b = px * 3 + ch, j = b - b0;
                    if (b < lo || b >= hi) continue;
                    const uint32_t dst = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (text_blend(dst, st.text_color[ch], cov) << (8 * (j & 3)));
                    any = true;
                }
            }
        }
    }
    return any;
}

}  // namespace adas
