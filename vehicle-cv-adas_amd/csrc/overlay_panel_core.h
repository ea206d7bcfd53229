// overlay_panel_core.h -- the pixel and state rules of the demo's three UI panels (ControlPanel.DisplayBirdViewPanel, DisplaySignsPanel,
// DisplayCollisionPanel, demo.py:101-214, called in that order at demo.py:307-309) without their putText lines: slice arithmetic on u8 pixels,
// one cv2.resize, and the curve_status latch that keeps a turn sign or the straight sign on screen.  THE DEFINITIONS HERE ARE THE AUTHORITY.
// The signs and collision panels and the bird panel's placement restate the reference's own NumPy lines (pinned by tests/golden/panels.json.gz);
// the resize inside the bird panel is rule P5, the project's restatement of OpenCV's 8-bit INTER_LINEAR, parity with a real cv2 build UNPINNED.
//   P1 geometry  W = int(src_w * ratio), H = int(src_h * ratio) on doubles (the host computes them once).  Bird panel: rows 0 .. H + 2b - 1,
//                columns src_w - W - 2b .. src_w - 1 (b: the border).  Signs widget: rows 0 .. sh - 1, columns 0 .. sw - 1.  Collision widget:
//                rows H + 2b .. 2H - 1, the bird panel's columns.
//   P2 widget    every byte v of a widget becomes v >> 1; then the border colour goes to widget rows 0..2, the two rows before the last, widget
//                columns 0..2 and the two columns before the last (NumPy's [0:3] and [-3:-1]: the last row and column stay only dimmed).
//   P3 sprite    pixel (y, x) of a BGRA sprite placed at (y0, x0) is written -- its channels 0..2 -- where its mask channel is non-zero: alpha
//                for the FCWS sprites, the turn signs, straight and warn; channel 2 for the two LTA sprites (the reference tests [:, :, 2]).
//                Signs: y0 = the signs row offset, x0 = sw / 2 - w / 2.  Collision: y0 = H + its row offset, x0 = src_w - W - its column offset.
//   P4 latch     panel_choose_signs: the two if-chains of DisplaySignsPanel over (latch, offset type, curvature type); up to two sprites in
//                paint order and the latch after the frame.  A type outside its enum is UNKNOWN.
//   P5 resize    destination (ry, rx) reads f = (float)((d + 0.5) * scale - 0.5), scale = 1.0 / ((double)dsize / ssize); s = floor(f); the
//                coefficients are rint((1 - f) * 2048) and rint(f * 2048) in fp32; horizontal taps outside the image collapse onto the border
//                pixel with weight 2048, vertical taps are clamped; h = p[x0] * a0 + p[x1] * a1 per row and
//                v = ((b0 * (h0 >> 4)) >> 16 + (b1 * (h1 >> 4)) >> 16 + 2) >> 2, saturated.  The same size is a copy.  This is the rule of
//                pre_kernels.hip and of oracle.preprocess.cv_resize_linear_u8.
//   P6 fold      a frame byte takes, in this order: the bird panel (0 on its border, the resized bird pixel inside), the signs widget (P2),
//                the first and the second sign sprite, the collision widget (P2), the collision sprite.  Later panels read what earlier ones
//                left, so where rectangles overlap (narrow frames) the result is the reference's sequential painting.  A byte outside every
//                panel and every sprite is not written.
// Nothing here loops for a number of steps given by a coordinate.  Like overlay_core.h the header also compiles for the host
// (tests/hostemu/emu_overlay_panels.cpp).
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

#if !defined(ADAS_HDI)
#if defined(__HIPCC__)
#define ADAS_HDI __host__ __device__ __forceinline__
#else
#define ADAS_HDI inline
#endif
#endif

namespace adas {

// panel bits, sprite slots, latch codes: the values of ADAS_PANEL_* in adas_hip.h
#define PANEL_BIRD 1
#define PANEL_SIGNS 2
#define PANEL_COLLISION 4
#define PANEL_SPRITES 9
#define PANEL_SPRITE_FCWS_WARNING 0
#define PANEL_SPRITE_FCWS_PROMPT 1
#define PANEL_SPRITE_FCWS_NORMAL 2
#define PANEL_SPRITE_LEFT 3
#define PANEL_SPRITE_RIGHT 4
#define PANEL_SPRITE_STRAIGHT 5
#define PANEL_SPRITE_WARN 6
#define PANEL_SPRITE_LTA_LEFT 7
#define PANEL_SPRITE_LTA_RIGHT 8
#define PANEL_LATCH_NONE 0
#define PANEL_LATCH_LEFT 1
#define PANEL_LATCH_RIGHT 2
#define PANEL_LATCH_STRAIGHT 3
#define PANEL_MAX_W 7680   // widest bird panel interior: its column taps are one LDS table of 8 bytes per column

// the message enums as the analysis stage stores them (ADAS_COLLISION_* / ADAS_OFFSET_* / ADAS_CURVATURE_*)
enum { PN_COLL_UNKNOWN = 0, PN_COLL_NORMAL = 1, PN_COLL_PROMPT = 2, PN_COLL_WARNING = 3 };
enum { PN_OFF_UNKNOWN = 0, PN_OFF_RIGHT = 1, PN_OFF_LEFT = 2, PN_OFF_CENTER = 3 };
enum { PN_CUR_UNKNOWN = 0, PN_CUR_STRAIGHT = 1, PN_CUR_EASY_LEFT = 2, PN_CUR_HARD_LEFT = 3, PN_CUR_EASY_RIGHT = 4, PN_CUR_HARD_RIGHT = 5 };

struct PanelSprite {
    int off;          // first pixel in the atlas
    int w, h;         // 0 x 0: empty, draws nothing
    int x0, y0;       // where pixel (0, 0) lands in the frame
    int mask_shift;   // bit position of the mask channel in a BGRA word: 24 alpha, 16 channel 2
};

struct PanelGeom {
    int src_h, src_w;
    int W, H, border;
    int bird_h, bird_w;         // the bird-view image the panel resizes (0: the handle has none)
    int bx0;                    // src_w - W - 2 * border: first column of the bird panel and of the collision widget
    int bird_rows;              // H + 2 * border
    int sw, sh;                 // the signs widget
    int cy0, cy1;               // the collision widget's rows [cy0, cy1)
    int identity;               // the bird image already is W x H: a copy
    uint32_t colour;            // the border colour, B | G << 8 | R << 16
    double scale_x, scale_y;    // P5
    PanelSprite sp[PANEL_SPRITES];
};

struct PanelRecord {            // adas_overlay_panel_record
    int sign[2];                // sprite slot of the first / second chain, -1: none
    int collision;              // sprite slot, -1: none
    int latch;                  // after the frame
    int offset_type, curvature_type, collision_type;   // as read
    int reserved;
};

// ---------------------------------------------------------------------------------------------------------------- P1
struct PanelParams {            // adas_overlay_panel_params
    double show_ratio;
    int border, signs_w, signs_h, signs_sprite_row, collision_sprite_row, collision_sprite_col;
    uint8_t border_color[3], reserved;
};

// what panel_geometry refuses: the panel, and for a sprite its slot
#define PANEL_FIT_OK 0
#define PANEL_FIT_PARAMS 1      // a parameter out of range, or a frame under 6 columns
#define PANEL_FIT_BIRD 2        // the bird panel leaves the frame, or W is outside 1 .. PANEL_MAX_W
#define PANEL_FIT_SIGNS 3       // the signs widget leaves the frame
#define PANEL_FIT_COLLISION 4   // the collision widget is empty (H <= 2 * border) or leaves the frame
#define PANEL_FIT_SIGN_SPRITE 5
#define PANEL_FIT_COLLISION_SPRITE 6   // e.g. W + collision_sprite_col < its width
#define PANEL_FIT_SPRITE_SIZE 7

// Host side, once: the geometry of a src_h x src_w frame under p, with sprites of sizes sprite_w[k] x sprite_h[k] (0: empty) laid out one
// behind the other in the atlas.  Every rectangle and every sprite placement must lie wholly inside the frame: the reference would clip
// silently, wrap to the other edge (a negative index) or raise.  Returns PANEL_FIT_*; *slot: the offending sprite.
inline int panel_geometry(int src_h, int src_w, int bird_h, int bird_w, const PanelParams& p, const int* sprite_w, const int* sprite_h, PanelGeom* out,
                          int* slot) {
    *slot = -1;
    if (!(p.show_ratio > 0.0 && p.show_ratio <= 1.0) || p.border < 0 || p.border > 4096 || p.signs_w <= 0 || p.signs_h <= 0 || p.signs_sprite_row < 0 ||
        p.collision_sprite_row < 0 || p.collision_sprite_col < 0 || src_w < 6 || src_h < 1)
        return PANEL_FIT_PARAMS;
    PanelGeom g;
    g.src_h = src_h; g.src_w = src_w;
    g.W = (int)((double)src_w * p.show_ratio);   // Python's int(src * ratio)
    g.H = (int)((double)src_h * p.show_ratio);
    g.border = p.border;
    g.bird_h = bird_h; g.bird_w = bird_w;
    g.bx0 = src_w - g.W - 2 * g.border;
    g.bird_rows = g.H + 2 * g.border;
    g.sw = p.signs_w; g.sh = p.signs_h;
    g.cy0 = g.H + 2 * g.border; g.cy1 = 2 * g.H;
    g.colour = (uint32_t)p.border_color[0] | ((uint32_t)p.border_color[1] << 8) | ((uint32_t)p.border_color[2] << 16);
    g.identity = bird_h == g.H && bird_w == g.W;
    g.scale_x = g.scale_y = 1.0;
    for (int k = 0; k < PANEL_SPRITES; ++k) {
        g.sp[k].off = g.sp[k].w = g.sp[k].h = g.sp[k].x0 = g.sp[k].y0 = 0;
        g.sp[k].mask_shift = (k == PANEL_SPRITE_LTA_LEFT || k == PANEL_SPRITE_LTA_RIGHT) ? 16 : 24;
    }
    *out = g;
    if (g.W < 1 || g.H < 1 || g.W > PANEL_MAX_W || g.bx0 < 0 || g.bird_rows > src_h) return PANEL_FIT_BIRD;
    if (g.sw > src_w || g.sh > src_h) return PANEL_FIT_SIGNS;
    if (g.cy1 <= g.cy0 || g.cy1 > src_h) return PANEL_FIT_COLLISION;
    if (bird_h > 0 && bird_w > 0) {
        g.scale_x = 1.0 / ((double)g.W / (double)bird_w);
        g.scale_y = 1.0 / ((double)g.H / (double)bird_h);
    }
    long long pixels = 0;
    for (int k = 0; k < PANEL_SPRITES; ++k) {
        PanelSprite& s = g.sp[k];
        if (sprite_w[k] == 0 && sprite_h[k] == 0) continue;
        *slot = k;
        if (sprite_w[k] < 1 || sprite_h[k] < 1 || sprite_w[k] > 16384 || sprite_h[k] > 4320) return PANEL_FIT_SPRITE_SIZE;
        s.w = sprite_w[k]; s.h = sprite_h[k];
        s.off = (int)pixels;
        pixels += (long long)s.w * s.h;
        if (pixels > (1ll << 28)) return PANEL_FIT_SPRITE_SIZE;
        if (k <= PANEL_SPRITE_FCWS_NORMAL) {
            s.y0 = g.H + p.collision_sprite_row;
            s.x0 = src_w - g.W - p.collision_sprite_col;
            if (s.x0 < 0 || s.x0 + s.w > src_w || s.y0 + s.h > src_h) { *out = g; return PANEL_FIT_COLLISION_SPRITE; }
        } else {
            s.y0 = p.signs_sprite_row;
            s.x0 = g.sw / 2 - s.w / 2;
            if (s.x0 < 0 || s.x0 + s.w > src_w || s.y0 + s.h > src_h) { *out = g; return PANEL_FIT_SIGN_SPRITE; }
        }
    }
    *slot = -1;
    *out = g;
    return PANEL_FIT_OK;
}

// ---------------------------------------------------------------------------------------------------------------- P4
ADAS_HD int panel_enum(int v, int n) { return (v < 0 || v >= n) ? 0 : v; }

ADAS_HD void panel_choose_signs(int latch, int offset_type, int curvature_type, int* s0, int* s1, int* latch_out) {
    const int off = panel_enum(offset_type, 4), cur = panel_enum(curvature_type, 6);
    int a = -1, b = -1;
    if (cur == PN_CUR_UNKNOWN && (off == PN_OFF_UNKNOWN || off == PN_OFF_CENTER)) {
        a = PANEL_SPRITE_WARN;
        latch = PANEL_LATCH_NONE;
    } else if ((cur == PN_CUR_HARD_LEFT || latch == PANEL_LATCH_LEFT) && cur != PN_CUR_EASY_RIGHT && cur != PN_CUR_HARD_RIGHT) {
        a = PANEL_SPRITE_LEFT;
        latch = PANEL_LATCH_LEFT;
    } else if ((cur == PN_CUR_HARD_RIGHT || latch == PANEL_LATCH_RIGHT) && cur != PN_CUR_EASY_LEFT && cur != PN_CUR_HARD_LEFT) {
        a = PANEL_SPRITE_RIGHT;
        latch = PANEL_LATCH_RIGHT;
    }
    if (off == PN_OFF_RIGHT) {
        b = PANEL_SPRITE_LTA_LEFT;
    } else if (off == PN_OFF_LEFT) {
        b = PANEL_SPRITE_LTA_RIGHT;
    } else if (cur == PN_CUR_STRAIGHT || latch == PANEL_LATCH_STRAIGHT) {
        b = PANEL_SPRITE_STRAIGHT;
        latch = PANEL_LATCH_STRAIGHT;
    }
    *s0 = a;
    *s1 = b;
    *latch_out = latch;
}

ADAS_HD int panel_choose_collision(int collision_type) {
    const int c = panel_enum(collision_type, 4);
    return c == PN_COLL_WARNING ? PANEL_SPRITE_FCWS_WARNING : (c == PN_COLL_PROMPT ? PANEL_SPRITE_FCWS_PROMPT : (c == PN_COLL_NORMAL ? PANEL_SPRITE_FCWS_NORMAL : -1));
}

// one frame of the state walk: the record of a frame with types (off, cur, col) under `panels`, from the latch before it
ADAS_HD PanelRecord panel_step(int panels, int latch, int off, int cur, int col) {
    PanelRecord r;
    r.sign[0] = r.sign[1] = r.collision = -1;
    r.latch = latch;
    r.offset_type = off; r.curvature_type = cur; r.collision_type = col;
    r.reserved = 0;
    if (panels & PANEL_SIGNS) panel_choose_signs(latch, off, cur, &r.sign[0], &r.sign[1], &r.latch);
    if (panels & PANEL_COLLISION) r.collision = panel_choose_collision(col);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- P5
ADAS_HD double panel_scale(int dsize, int ssize) { return 1.0 / ((double)dsize / (double)ssize); }

ADAS_HD void panel_lin_coef(int d, double scale, int ssize, bool horizontal, int* s0, int* s1, int* c0, int* c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (horizontal) {   // out-of-range taps collapse onto the border pixel with weight 1
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    }
    *c0 = (int)rintf((1.f - f) * 2048.f);
    *c1 = (int)rintf(f * 2048.f);
    int a = s, b = s + 1;
    a = a < 0 ? 0 : (a > ssize - 1 ? ssize - 1 : a);
    b = b < 0 ? 0 : (b > ssize - 1 ? ssize - 1 : b);
    *s0 = a;
    *s1 = b;
}

struct PanelTap {
    short s0, s1, c0, c1;   // source taps (<= 16383) and their 11-bit coefficients (<= 2048)
};
ADAS_HD PanelTap panel_col_tap(int rx, double scale_x, int sw) {
    int x0, x1, a0, a1;
    panel_lin_coef(rx, scale_x, sw, true, &x0, &x1, &a0, &a1);
    PanelTap t;
    t.s0 = (short)x0; t.s1 = (short)x1; t.c0 = (short)a0; t.c1 = (short)a1;
    return t;
}
ADAS_HD PanelTap panel_row_tap(int ry, double scale_y, int sh) {
    int y0, y1, b0, b1;
    panel_lin_coef(ry, scale_y, sh, false, &y0, &y1, &b0, &b1);
    PanelTap t;
    t.s0 = (short)y0; t.s1 = (short)y1; t.c0 = (short)b0; t.c1 = (short)b1;
    return t;
}
// the resized pixel from its two source rows, packed B | G << 8 | R << 16
ADAS_HDI uint32_t panel_resize_taps(const uint8_t* r0, const uint8_t* r1, int b0, int b1, const PanelTap c) {
    const int x0 = c.s0 * 3, x1 = c.s1 * 3, a0 = c.c0, a1 = c.c1;
    uint32_t out = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const int h0 = r0[x0 + ch] * a0 + r0[x1 + ch] * a1;
        const int h1 = r1[x0 + ch] * a0 + r1[x1 + ch] * a1;
        int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        out |= (uint32_t)v << (8 * ch);
    }
    return out;
}
// pixel (ry, rx) of the bird image [sh][sw][3] resized to dh x dw
ADAS_HD uint32_t panel_resize_px(const uint8_t* src, int sh, int sw, int dh, int dw, int ry, int rx) {
    if (dh == sh && dw == sw) {
        const uint8_t* p = src + ((size_t)ry * sw + rx) * 3;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    const PanelTap r = panel_row_tap(ry, panel_scale(dh, sh), sh);
    return panel_resize_taps(src + (size_t)r.s0 * sw * 3, src + (size_t)r.s1 * sw * 3, r.c0, r.c1, panel_col_tap(rx, panel_scale(dw, sw), sw));
}

// ---------------------------------------------------------------------------------------------------------------- P2, P3, P6
// widget row / column r of n takes the border colour: NumPy's [0:3] and [-3:-1]
ADAS_HD bool panel_border_index(int r, int n) { return r < 3 || (r >= n - 3 && r <= n - 2); }

ADAS_HD uint32_t panel_widget(uint32_t v, int r, int c, int h, int w, uint32_t colour) {
    return (panel_border_index(r, h) || panel_border_index(c, w)) ? colour : ((v >> 1) & 0x7f7f7fu);
}

// sprite `s` over pixel (row, col): true and *v = its channels 0..2 where its mask channel is non-zero
ADAS_HDI bool panel_sprite(const PanelSprite& s, const uint32_t* atlas, int row, int col, uint32_t* v) {
    const int y = row - s.y0, x = col - s.x0;
    if (y < 0 || y >= s.h || x < 0 || x >= s.w) return false;
    const uint32_t px = atlas[s.off + y * s.w + x];
    if (!((px >> s.mask_shift) & 0xffu)) return false;
    *v = px & 0xffffffu;
    return true;
}

// P6 on pixel (row, col) of a frame whose record is rec; v: its bytes before the panels (B | G << 8 | R << 16; the rules are per channel, so a
// caller that knows only some of the three may pass anything in the others and drop them again).  bird(ry, rx): the resized bird pixel.
// Returns the bytes after the panels; *written = false when no panel or sprite covers the pixel.
template <class Bird>
ADAS_HDI uint32_t panel_fold_pixel(const PanelGeom& g, int panels, const PanelRecord& rec, const uint32_t* atlas, const PanelSprite* sp, int row, int col, uint32_t v,
                                   const Bird& bird, bool* written) {
    bool wr = false;
    const bool right = col >= g.bx0;
    if ((panels & PANEL_BIRD) && right && row < g.bird_rows) {
        const int ry = row - g.border, rx = col - g.bx0 - g.border;
        v = (ry >= 0 && ry < g.H && rx >= 0 && rx < g.W) ? bird(ry, rx) : 0u;
        wr = true;
    }
    if (panels & PANEL_SIGNS) {
        if (row < g.sh && col < g.sw) {
            v = panel_widget(v, row, col, g.sh, g.sw, g.colour);
            wr = true;
        }
        const int s0 = rec.sign[0], s1 = rec.sign[1];   // no loop over sign[]: an indexed record would live in scratch on the device
        if (s0 >= 0 && panel_sprite(sp[s0], atlas, row, col, &v)) wr = true;
        if (s1 >= 0 && panel_sprite(sp[s1], atlas, row, col, &v)) wr = true;
    }
    if (panels & PANEL_COLLISION) {
        if (right && row >= g.cy0 && row < g.cy1) {
            v = panel_widget(v, row - g.cy0, col - g.bx0, g.cy1 - g.cy0, g.src_w - g.bx0, g.colour);
            wr = true;
        }
        if (rec.collision >= 0 && panel_sprite(sp[rec.collision], atlas, row, col, &v)) wr = true;
    }
    *written = wr;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- the draw pass's rows
// What one run touches: per row at most a left span, columns [0, lw) on rows [0, lh) -- the signs widget and its sprites -- and a right span,
// columns [rx0, src_w) on rows [ry0, rh) -- the bird panel, the collision widget and its sprites.  Every pixel P6 can write lies in one of them.
struct PanelSpans {
    int lw, lh;
    int rx0, ry0, rh;
    int row0, row1;   // rows [row0, row1) hold a span
};

ADAS_HD PanelSpans panel_spans(const PanelGeom& g, int panels) {
    PanelSpans s;
    s.lw = s.lh = 0;
    s.rx0 = g.src_w; s.ry0 = g.src_h; s.rh = 0;
    if (panels & PANEL_SIGNS) {
        s.lw = g.sw; s.lh = g.sh;
        const int slots[6] = {PANEL_SPRITE_LEFT, PANEL_SPRITE_RIGHT, PANEL_SPRITE_STRAIGHT, PANEL_SPRITE_WARN, PANEL_SPRITE_LTA_LEFT, PANEL_SPRITE_LTA_RIGHT};
        for (int k = 0; k < 6; ++k) {
            const PanelSprite& p = g.sp[slots[k]];
            if (p.w <= 0 || p.h <= 0) continue;
            if (p.x0 + p.w > s.lw) s.lw = p.x0 + p.w;
            if (p.y0 + p.h > s.lh) s.lh = p.y0 + p.h;
        }
    }
    if (panels & PANEL_BIRD) {
        s.rx0 = g.bx0; s.ry0 = 0; s.rh = g.bird_rows;
    }
    if (panels & PANEL_COLLISION) {
        if (g.bx0 < s.rx0) s.rx0 = g.bx0;
        if (g.cy0 < s.ry0) s.ry0 = g.cy0;
        if (g.cy1 > s.rh) s.rh = g.cy1;
        for (int k = PANEL_SPRITE_FCWS_WARNING; k <= PANEL_SPRITE_FCWS_NORMAL; ++k) {
            const PanelSprite& p = g.sp[k];
            if (p.w <= 0 || p.h <= 0) continue;
            if (p.x0 < s.rx0) s.rx0 = p.x0;
            if (p.y0 < s.ry0) s.ry0 = p.y0;
            if (p.y0 + p.h > s.rh) s.rh = p.y0 + p.h;
        }
    }
    s.row0 = s.lh > 0 ? 0 : s.ry0;
    s.row1 = s.lh > s.rh ? s.lh : s.rh;
    if (s.row1 <= s.row0) s.row0 = s.row1 = 0;
    return s;
}

// the n (0..2) column intervals [c0(i), c1(i)) of a row, left to right, merged where they meet.  Named fields and selects, no arrays: an array
// indexed by a loop counter would live in scratch memory on the device
struct PanelRowSpans {
    int n, a0, a1, b0, b1;
    ADAS_HD int c0(int i) const { return i ? b0 : a0; }
    ADAS_HD int c1(int i) const { return i ? b1 : a1; }
};
ADAS_HD PanelRowSpans panel_row_spans(const PanelSpans& s, int src_w, int row) {
    PanelRowSpans o;
    o.n = o.a0 = o.a1 = o.b0 = o.b1 = 0;
    const bool l = row >= 0 && row < s.lh, r = row >= s.ry0 && row < s.rh;
    if (l && r && s.rx0 <= s.lw) {
        o.n = 1; o.a1 = src_w;
    } else if (l && r) {
        o.n = 2; o.a1 = s.lw; o.b0 = s.rx0; o.b1 = src_w;
    } else if (l) {
        o.n = 1; o.a1 = s.lw;
    } else if (r) {
        o.n = 1; o.a0 = s.rx0; o.a1 = src_w;
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- the draw pass's pieces
// The pass works on aligned 16-byte pieces of the frame buffer [frames][src_h][src_w][3], which may start on any address: piece P holds the
// buffer's bytes 16 P - align .. 16 P - align + 15 (align = the buffer's address & 15).  A span's pieces are the ones its bytes meet; a piece
// that two spans meet -- the end of a row and the start of the next, two spans of a row less than 16 bytes apart -- belongs to the first of
// them, whose lane folds every byte of it.  Rows hold at least 18 bytes (src_w >= 6), so a piece meets at most two rows.

// last piece of the last span of (frame, row); -1: the row has none
ADAS_HD long long panel_row_last_piece(const PanelSpans& sp, const PanelGeom& g, int align, long long frame, int row) {
    if (row < sp.row0 || row >= sp.row1) return -1;
    const PanelRowSpans rs = panel_row_spans(sp, g.src_w, row);
    if (!rs.n) return -1;
    const long long rowstart = (frame * g.src_h + row) * (long long)g.src_w * 3;
    return (rowstart + align + (long long)rs.c1(rs.n - 1) * 3 - 1) >> 4;
}
// last piece of the spans before (frame, row): the row above, or the last row of the frame before
ADAS_HD long long panel_prev_last_piece(const PanelSpans& sp, const PanelGeom& g, int align, long long frame, int row) {
    if (row > 0) return panel_row_last_piece(sp, g, align, frame, row - 1);
    return frame > 0 ? panel_row_last_piece(sp, g, align, frame - 1, g.src_h - 1) : -1;
}
// pieces [*p0, *p1] of columns [c0, c1) of (frame, row) that no span before owns; *prev_last: the last piece owned so far, updated
ADAS_HD void panel_span_pieces(const PanelGeom& g, int align, long long frame, int row, int c0, int c1, long long* prev_last, long long* p0, long long* p1) {
    const long long rowstart = (frame * g.src_h + row) * (long long)g.src_w * 3;
    long long a = (rowstart + align + (long long)c0 * 3) >> 4;
    const long long b = (rowstart + align + (long long)c1 * 3 - 1) >> 4;
    if (a <= *prev_last) a = *prev_last + 1;
    if (b > *prev_last) *prev_last = b;
    *p0 = a;
    *p1 = b;
}

struct PanelPiece {   // 16 bytes as four little-endian words; named, not an array (see PanelRowSpans)
    uint32_t w0, w1, w2, w3;
};

// P6 on one piece.  d: the piece's first byte relative to the first byte of (frame f, row), -15 .. 3 src_w - 1; io: its 16 bytes (bytes outside
// the buffer: anything; they are not looked at).  Pixels of the row above or below, or of a neighbouring
// frame, that the piece holds are folded with their own coordinates and record (rec_f: recs[f], already loaded).  bird.frame(ff) selects frame ff's bird image.  Returns
// false when nothing was written (io is then unchanged).
template <class Bird>
ADAS_HDI bool panel_fold_piece(const PanelGeom& g, int panels, const PanelRecord* recs, const PanelRecord& rec_f, int frames, const uint32_t* atlas, const PanelSprite* sp, int f, int row, int d,
                               PanelPiece* io, Bird& bird) {
    const int px_first = d >= 0 ? d / 3 : -((2 - d) / 3);
    const int phase = d - 3 * px_first;   // 0..2: pixel px_first + k holds bytes 3k - phase .. 3k + 2 - phase of the piece
    const int sh = 8 * phase;
    uint32_t X[5];                        // the piece moved up by `phase` bytes: pixel k at bytes 3k .. 3k + 2
    X[0] = io->w0 << sh;
    X[1] = (uint32_t)((((unsigned long long)io->w1 << 32) | io->w0) >> (32 - sh));
    X[2] = (uint32_t)((((unsigned long long)io->w2 << 32) | io->w1) >> (32 - sh));
    X[3] = (uint32_t)((((unsigned long long)io->w3 << 32) | io->w2) >> (32 - sh));
    X[4] = (uint32_t)(((unsigned long long)io->w3) >> (32 - sh));
    bool any = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 6; ++k) {
        int c = px_first + k, r = row, ff = f;
        if (c < 0) {
            c += g.src_w;
            if (--r < 0) { r = g.src_h - 1; --ff; }
        } else if (c >= g.src_w) {
            c -= g.src_w;
            if (++r >= g.src_h) { r = 0; ++ff; }
        }
        if (ff < 0 || ff >= frames) continue;
        const int b = 3 * k, w = b >> 2, s = 8 * (b & 3);
        const unsigned long long pair = (((unsigned long long)(w + 1 < 5 ? X[w + 1] : 0u)) << 32) | X[w];
        const uint32_t v = (uint32_t)(pair >> s) & 0xffffffu;
        bird.frame(ff);
        bool wr;
        PanelRecord rec = rec_f;   // by value: a reference to one of the two would put the record in scratch
        if (ff != f) rec = recs[ff];
        const uint32_t nv = panel_fold_pixel(g, panels, rec, atlas, sp, r, c, v, bird, &wr);
        if (!wr) continue;
        any = true;
        const unsigned long long m = 0xffffffull << s, val = (unsigned long long)nv << s;
        X[w] = (X[w] & ~(uint32_t)m) | (uint32_t)val;
        if (w + 1 < 5) X[w + 1] = (X[w + 1] & ~(uint32_t)(m >> 32)) | (uint32_t)(val >> 32);
    }
    if (!any) return false;
    io->w0 = (uint32_t)((((unsigned long long)X[1] << 32) | X[0]) >> sh);
    io->w1 = (uint32_t)((((unsigned long long)X[2] << 32) | X[1]) >> sh);
    io->w2 = (uint32_t)((((unsigned long long)X[3] << 32) | X[2]) >> sh);
    io->w3 = (uint32_t)((((unsigned long long)X[4] << 32) | X[3]) >> sh);
    return true;
}

// columns ca .. cb of `row` meet sprite p
ADAS_HDI bool panel_sprite_meets(const PanelSprite& p, int row, int ca, int cb) { return row >= p.y0 && row < p.y0 + p.h && cb >= p.x0 && ca < p.x0 + p.w; }

// panel_fold_piece with the work a piece cannot need taken out first.  A piece that lies inside one row (all but the ones across a row's end)
// knows its columns ca .. cb: a panel whose rectangle and sprites they miss is dropped from the mask, a sprite they miss from the record; a
// piece wholly inside a widget's dimmed interior with no sprite over it is four word operations, (w >> 1) & 0x7f7f7f7f; a piece that only one
// panel can reach takes P6 compiled for that panel alone.  The bytes are those of panel_fold_piece: the host build runs this function too.
template <class Bird>
ADAS_HDI bool panel_fold_piece_fast(const PanelGeom& g, int panels, const PanelRecord* recs, const PanelRecord& rec_f, int frames, const uint32_t* atlas, const PanelSprite* sp, int f,
                                    int row, int d, PanelPiece* io, Bird& bird) {
    if (d < 0 || d + 16 > g.src_w * 3) return panel_fold_piece(g, panels, recs, rec_f, frames, atlas, sp, f, row, d, io, bird);
    const int ca = d / 3, cb = (d + 15) / 3;
    const bool right = cb >= g.bx0;
    int pm = panels;
    PanelRecord r = rec_f;
    if (!(right && row < g.bird_rows)) pm &= ~PANEL_BIRD;
    if (pm & PANEL_SIGNS) {
        if (!(r.sign[0] >= 0 && panel_sprite_meets(sp[r.sign[0] < 0 ? 0 : r.sign[0]], row, ca, cb))) r.sign[0] = -1;
        if (!(r.sign[1] >= 0 && panel_sprite_meets(sp[r.sign[1] < 0 ? 0 : r.sign[1]], row, ca, cb))) r.sign[1] = -1;
        if (!(row < g.sh && ca < g.sw) && r.sign[0] < 0 && r.sign[1] < 0) pm &= ~PANEL_SIGNS;
    }
    if (pm & PANEL_COLLISION) {
        if (!(r.collision >= 0 && panel_sprite_meets(sp[r.collision < 0 ? 0 : r.collision], row, ca, cb))) r.collision = -1;
        if (!(right && row >= g.cy0 && row < g.cy1) && r.collision < 0) pm &= ~PANEL_COLLISION;
    }
    if (!pm) return false;
    const bool dim_signs = pm == PANEL_SIGNS && r.sign[0] < 0 && r.sign[1] < 0 && ca >= 3 && cb < g.sw - 3 && !panel_border_index(row, g.sh);
    const bool dim_coll = pm == PANEL_COLLISION && r.collision < 0 && ca >= g.bx0 + 3 && cb < g.src_w - 3 && !panel_border_index(row - g.cy0, g.cy1 - g.cy0);
    if (dim_signs || dim_coll) {
        io->w0 = (io->w0 >> 1) & 0x7f7f7f7fu; io->w1 = (io->w1 >> 1) & 0x7f7f7f7fu;
        io->w2 = (io->w2 >> 1) & 0x7f7f7f7fu; io->w3 = (io->w3 >> 1) & 0x7f7f7f7fu;
        return true;
    }
    if (pm == PANEL_BIRD) return panel_fold_piece(g, PANEL_BIRD, recs, r, frames, atlas, sp, f, row, d, io, bird);
    if (pm == PANEL_SIGNS) return panel_fold_piece(g, PANEL_SIGNS, recs, r, frames, atlas, sp, f, row, d, io, bird);
    if (pm == PANEL_COLLISION) return panel_fold_piece(g, PANEL_COLLISION, recs, r, frames, atlas, sp, f, row, d, io, bird);
    return panel_fold_piece(g, pm, recs, r, frames, atlas, sp, f, row, d, io, bird);
}

}  // namespace adas
