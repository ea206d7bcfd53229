// overlay_text_core.h -- the rules of the overlay's text (adas_overlay_*text*), compiled for the device (overlay_text.hip) and for the host
// (tests/hostemu/emu_overlay_text.cpp); restated in NumPy by tests/text_ref.py.  The font is caller data: a bitmap coverage atlas per slot
// with the metrics of characters 32..126; nothing here knows a typeface.  Every rule is integer arithmetic, or double arithmetic without
// contraction where the reference computes in Python floats.
//   T1  numbers: '%.2f' / '%.1f' of a double correctly rounded from its exact binary value (mantissa x 10^n in 64 bits, shifted by the
//       exponent, half to even on the exact remainder); the sign of negative zero and of what rounds to zero is kept; nan, inf, -inf as
//       Python prints them; finite |x| >= 2^30 is out of range (the item is skipped, ADAS_OVERLAY_TEXT_RANGE).  int32 in decimal.
//   T2  size: w = (sum of advances + size_w_extra + 0x8000) >> 16, h = size_h.
//   T3  pen: x accumulates in 16.16 from the origin; a glyph's columns start at (pen >> 16) + bearing_x; its rows are y - baseline_row ...
//   T4  pixel: out = (dst * (255 - c) + colour * c + 127) / 255 per channel; c == 0 writes nothing; clipped per pixel at the four edges.
//   T5  the items of a frame in paint order (text_candidate): detections, tracks, track ids, distances, the three panel strings, caller lines.
//   T6  at most max_items per frame, the rest dropped in paint order with ADAS_OVERLAY_TEXT_OVERFLOW.
//   T7  a frame's bytes are those of painting its items one after another, a run's glyphs one after another.
// A character outside 32..126 draws as '?'.  A ladder (a run of consecutive slots) picks the slot whose declared scale is nearest the
// reference's continuous fontScale, the smaller scale on a tie.
#pragma once
#include <stdint.h>
#include <math.h>

#if !defined(ADAS_HDI)
#if defined(__HIPCC__)
#define ADAS_HDI __host__ __device__ __forceinline__
#else
#define ADAS_HDI inline
#endif
#endif

namespace adas {

constexpr int TEXT_FONTS = 16;
constexpr int TEXT_GLYPHS = 95;        // characters 32 .. 126
constexpr int TEXT_MAX_CELL = 64;      // cell_h and glyph_w
constexpr int TEXT_MAX_CHARS = 47;
constexpr int TEXT_LABEL_BYTES = 32;   // a class name: at most 31 bytes and a 0
constexpr int TEXT_MAX_LINES = 8;
constexpr int TEXT_MAX_ITEMS = 1024;   // the most a handle's max_text_items may be
constexpr int TEXT_DETECTIONS = 1, TEXT_TRACKS = 2, TEXT_TRACK_IDS = 4, TEXT_DISTANCE = 8, TEXT_PANELS = 16, TEXT_LINES = 32;
constexpr int TEXT_ALL = 63;
constexpr int TEXT_FLAG_RANGE = 1, TEXT_FLAG_OVERFLOW = 2;
constexpr int TEXT_ITEM_RECT = 1, TEXT_ITEM_RUN = 2;
constexpr double TEXT_RANGE = 1073741824.0;   // 2^30

struct TextFont {   // adas_overlay_font, the atlas on the device
    const uint8_t* atlas;   // [cell_h][atlas_w] coverage
    int32_t atlas_w, cell_h;
    int32_t baseline_row;   // the cell's row that sits on the origin's y
    int32_t size_h;         // T2
    int32_t size_w_extra;   // 16.16
    int32_t set;            // the slot holds a font
    double scale;           // the declared fontScale: ladders only
    int32_t glyph_x[TEXT_GLYPHS], glyph_w[TEXT_GLYPHS], bearing_x[TEXT_GLYPHS], advance[TEXT_GLYPHS];
};

struct TextItem {   // adas_overlay_text_item
    int32_t kind;     // TEXT_ITEM_*
    int32_t source;   // the TEXT_* bit it belongs to
    int32_t x, y;     // a run's origin; a rectangle's first corner as cv2.rectangle is given it
    int32_t x1, y1;   // a rectangle's second corner (inclusive, either order); 0 for a run
    int32_t bx0, by0, bx1, by1;   // every pixel the item can touch, inside the frame, half open; empty: bx0 >= bx1
    int32_t slot;     // a run's font; -1 for a rectangle
    uint8_t color[3];
    uint8_t len;
    char text[TEXT_MAX_CHARS + 1];
};

struct TextLine {   // a caller line
    int32_t x, y, slot;
    uint8_t color[3];
    uint8_t len;
    char text[TEXT_MAX_CHARS + 1];
};

struct TextStyle {   // adas_overlay_text_style
    double show_ratio;      // 0.25: the FCWS string's column is src_w - int(src_w * show_ratio) + fcws_dx
    double min_box_area;    // 10: the gate of the tracks and their ids
    int32_t max_text_items; // 256
    int32_t det_size_slot, det_label_slot;   // the font the box is sized by; the font that is drawn
    int32_t det_label_dx, det_label_dy;      // (2, -7); EfficientDet's variant (0, -5)
    int32_t det_box_pad;                     // 3: the rectangle ends at ymin - th - 3
    int32_t track_slot, track_dy;            // -10
    int32_t id_first, id_count, id_shadow_first, id_shadow_count;   // ladders
    int32_t dist_size_first, dist_size_count, dist_first, dist_count, dist_shadow_first, dist_shadow_count;
    int32_t shadow_dx, shadow_dy;            // (2, 2)
    int32_t ldws_slot, lkas_slot, fcws_slot;
    int32_t ldws_x, ldws_y, lkas_x, lkas_y, fcws_dx, fcws_y;   // (10, 240), (10, 280), (100, 240)
    int32_t id_shadow_sub;                   // 30
    uint8_t label_color[3], dist_color[3], dist_shadow_color[3];   // white, white, (150, 150, 150)
    uint8_t offset_colors[4][3], curvature_colors[6][3], collision_colors[4][3];   // OffsetDict / CurvatureDict / CollisionDict
    uint8_t pad[5];
};

struct TextSrc {   // what the layout reads of frame q, where it already sits; null: that kind has no source
    const int32_t *det_xyxy, *det_cls, *det_cnt;   // [q][det_cap][4], [q][det_cap], the count at det_cnt[q * det_cnt_stride]
    // track row k of frame q, by byte strides (raw arrays, or the tracker's live table in the layout of adas_track): tlwh, 4 doubles at
    // trk_tlwh + q * trk_frame_bytes + k * trk_row_bytes, and is_activated, an int at the same strides (null: every row is); the class and
    // the id, ints at + q * trk_cls_frame_bytes + k * trk_cls_row_bytes; the rows of the frame, an int at trk_cnt + q * trk_cnt_bytes
    const unsigned char *trk_tlwh, *trk_act, *trk_cls, *trk_ids, *trk_cnt;
    long long trk_frame_bytes, trk_row_bytes, trk_cls_frame_bytes, trk_cls_row_bytes, trk_cnt_bytes;
    // its trajectory.  slot_ids null: the newest box (x1, y1, x2, y2), 4 doubles at ring + q * ring_frame_bytes + k * 32, and the length, an
    // int at len + q * len_frame_bytes + k * 4.  Else the tracker's rings: the row's slot, an int at slot_ids + q * slot_frame_bytes + k * 4;
    // the boxes ever appended n, an int at len + q * len_frame_bytes + slot * len_row_bytes; entry i of the list at ring + q *
    // ring_frame_bytes + slot * 960 + (i % 30) * 32: the length is min(n, 30), the newest box entry n - 1
    const unsigned char *ring, *slot_ids, *len;
    long long ring_frame_bytes, slot_frame_bytes, len_frame_bytes, len_row_bytes;
    const int32_t* dist_xy;                         // [q][dist_cap][2]
    const double* dist_d;                           // [q][dist_cap]
    const int32_t* dist_cnt;                        // the count at dist_cnt[q * dist_cnt_stride]
    const int32_t *offset, *curvature, *collision;  // the types at [q * msg_stride]
    int32_t det_cnt_stride, dist_cnt_stride, msg_stride;
    int32_t det_cap, trk_cap, dist_cap;
    int32_t src_w, src_h;
};

// the sources as raw arrays (adas_overlay_text_arrays)
ADAS_HDI TextSrc text_src_of_arrays(const int32_t* det_xyxy, const int32_t* det_cls, const int32_t* det_cnt, int det_cap, const double* trk_tlwh,
                                    const int32_t* trk_cls, const int32_t* trk_ids, const int32_t* trk_cnt, int trk_cap, const double* trk_last,
                                    const int32_t* traj_len, const int32_t* dist_xy, const double* dist_d, const int32_t* dist_cnt, int dist_cap,
                                    const int32_t* offset, const int32_t* curvature, const int32_t* collision) {
    TextSrc s = {};
    s.det_xyxy = det_xyxy; s.det_cls = det_cls; s.det_cnt = det_cnt; s.det_cnt_stride = 1; s.det_cap = det_cap;
    s.trk_tlwh = (const unsigned char*)trk_tlwh; s.trk_frame_bytes = (long long)trk_cap * 32; s.trk_row_bytes = 32;
    s.trk_cls = (const unsigned char*)trk_cls; s.trk_ids = (const unsigned char*)trk_ids; s.trk_cls_frame_bytes = (long long)trk_cap * 4; s.trk_cls_row_bytes = 4;
    s.trk_cnt = (const unsigned char*)trk_cnt; s.trk_cnt_bytes = 4; s.trk_cap = trk_cap;
    s.ring = (const unsigned char*)trk_last; s.ring_frame_bytes = (long long)trk_cap * 32;
    s.len = (const unsigned char*)traj_len; s.len_frame_bytes = (long long)trk_cap * 4;
    s.dist_xy = dist_xy; s.dist_d = dist_d; s.dist_cnt = dist_cnt; s.dist_cnt_stride = 1; s.dist_cap = dist_cap;
    s.offset = offset; s.curvature = curvature; s.collision = collision; s.msg_stride = 1;
    return s;
}

struct TextTables {   // what a handle holds on the device
    const TextFont* fonts;                 // [TEXT_FONTS]
    const char* det_names; int32_t n_det_names;   // [n][TEXT_LABEL_BYTES]
    const char* trk_names; int32_t n_trk_names;
    const uint32_t* det_colors; int32_t n_det_colors;   // packed b | g << 8 | r << 16; outside the table: black
    const uint32_t* trk_colors; int32_t n_trk_colors;
    const TextLine* lines; int32_t n_lines;
};

// ---- T1
ADAS_HDI uint64_t text_double_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return u;
}

// '%.<prec>f' of x, prec 1 or 2, into out (at most 16 bytes, no 0).  Returns the length, or -1: finite and |x| >= 2^30.
ADAS_HDI int text_format_fixed(double x, int prec, char* out) {
    const uint64_t u = text_double_bits(x);
    const int neg = (int)(u >> 63);
    const int be = (int)((u >> 52) & 0x7ff);
    const uint64_t frac = u & 0xfffffffffffffull;
    int n = 0;
    if (be == 0x7ff) {
        if (frac) { out[0] = 'n'; out[1] = 'a'; out[2] = 'n'; return 3; }
        if (neg) out[n++] = '-';
        out[n++] = 'i'; out[n++] = 'n'; out[n++] = 'f';
        return n;
    }
    if (be >= 1023 + 30) return -1;
    const uint64_t m = be ? (frac | (1ull << 52)) : frac;   // x = m * 2^(e), e = (be ? be : 1) - 1075 < 0
    const int s = 1075 - (be ? be : 1);                     // 23 .. 1074
    const uint64_t p10 = prec == 2 ? 100u : 10u;
    const uint64_t N = m * p10;                             // < 2^60
    uint64_t q = 0;
    if (s < 61) {
        q = N >> s;
        const uint64_t rem = N & ((1ull << s) - 1), half = 1ull << (s - 1);
        if (rem > half || (rem == half && (q & 1))) ++q;
    }   // else N < 2^60 <= half: rounds to zero
    if (neg) out[n++] = '-';
    const uint64_t ip = q / p10, fp = q % p10;
    char tmp[12];
    int k = 0;
    uint64_t v = ip;
    do { tmp[k++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
    while (k) out[n++] = tmp[--k];
    out[n++] = '.';
    if (prec == 2) out[n++] = (char)('0' + (int)(fp / 10));
    out[n++] = (char)('0' + (int)(fp % 10));
    return n;
}

ADAS_HDI int text_format_int(int32_t x, char* out) {   // at most 11 bytes
    int n = 0;
    uint32_t v = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;
    if (x < 0) out[n++] = '-';
    char tmp[10];
    int k = 0;
    do { tmp[k++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
    while (k) out[n++] = tmp[--k];
    return n;
}

ADAS_HDI int text_glyph(char c) {
    const unsigned char ch = (unsigned char)c;
    return (ch < 32 || ch > 126) ? '?' - 32 : ch - 32;
}

// ---- T2
ADAS_HDI void text_size(const TextFont& f, const char* s, int len, int* w, int* h) {
    long long sum = 0;
    for (int i = 0; i < len; ++i) sum += f.advance[text_glyph(s[i])];
    *w = (int)((sum + f.size_w_extra + 0x8000) >> 16);
    *h = f.size_h;
}

// the slot of the ladder [first, first + count) whose declared scale is nearest v: the smaller scale on a tie, then the lower slot
ADAS_HDI int text_ladder(const TextFont* fonts, int first, int count, double v) {
    int best = first;
    double bd = fabs(fonts[first].scale - v);
    for (int k = first + 1; k < first + count; ++k) {
        const double d = fabs(fonts[k].scale - v);
        if (d < bd || (d == bd && fonts[k].scale < fonts[best].scale)) { best = k; bd = d; }
    }
    return best;
}

ADAS_HDI void text_clip(TextItem* it, long long x0, long long y0, long long x1, long long y1, int W, int H) {   // half open in, clipped out
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > W) x1 = W;
    if (y1 > H) y1 = H;
    if (x0 >= x1 || y0 >= y1) x0 = y0 = x1 = y1 = 0;
    it->bx0 = (int)x0; it->by0 = (int)y0; it->bx1 = (int)x1; it->by1 = (int)y1;
}

// a glyph run at origin (x, y): T3 gives its box
ADAS_HDI void text_make_run(TextItem* it, const TextFont* fonts, int source, int slot, long long x, long long y, uint32_t colour, const char* s, int len,
                            int W, int H) {
    const TextFont& f = fonts[slot];
    it->kind = TEXT_ITEM_RUN; it->source = source;
    it->x = (int32_t)x; it->y = (int32_t)y; it->x1 = 0; it->y1 = 0;
    it->slot = slot;
    it->color[0] = (uint8_t)colour; it->color[1] = (uint8_t)(colour >> 8); it->color[2] = (uint8_t)(colour >> 16);
    if (len > TEXT_MAX_CHARS) len = TEXT_MAX_CHARS;
    it->len = (uint8_t)len;
    long long pen = x * 65536, lo = 0, hi = 0;
    bool any = false;
    for (int i = 0; i < TEXT_MAX_CHARS + 1; ++i) it->text[i] = i < len ? s[i] : 0;
    for (int i = 0; i < len; ++i) {
        const int g = text_glyph(s[i]);
        const long long gx0 = (pen >> 16) + f.bearing_x[g];
        if (f.glyph_w[g] > 0) {
            if (!any || gx0 < lo) lo = gx0;
            if (!any || gx0 + f.glyph_w[g] > hi) hi = gx0 + f.glyph_w[g];
            any = true;
        }
        pen += f.advance[g];
    }
    if (!any) lo = hi = 0;
    text_clip(it, lo, y - f.baseline_row, hi, y - f.baseline_row + f.cell_h, W, H);
}

ADAS_HDI void text_make_rect(TextItem* it, int source, long long xa, long long ya, long long xb, long long yb, uint32_t colour, int W, int H) {
    it->kind = TEXT_ITEM_RECT; it->source = source;
    it->x = (int32_t)xa; it->y = (int32_t)ya; it->x1 = (int32_t)xb; it->y1 = (int32_t)yb;
    it->slot = -1;
    it->color[0] = (uint8_t)colour; it->color[1] = (uint8_t)(colour >> 8); it->color[2] = (uint8_t)(colour >> 16);
    it->len = 0;
    for (int i = 0; i < TEXT_MAX_CHARS + 1; ++i) it->text[i] = 0;
    text_clip(it, xa < xb ? xa : xb, ya < yb ? ya : yb, (xa < xb ? xb : xa) + 1, (ya < yb ? yb : ya) + 1, W, H);
}

ADAS_HDI int text_append(char* dst, int n, const char* s) {
    while (*s && n < TEXT_MAX_CHARS) dst[n++] = *s++;
    return n;
}
ADAS_HDI int text_append_n(char* dst, int n, const char* s, int len) {
    for (int i = 0; i < len && n < TEXT_MAX_CHARS; ++i) dst[n++] = s[i];
    return n;
}

// the name of class cls: the table's, or 'unknown'
ADAS_HDI int text_class_name(char* dst, int n, int cls, const char* names, int n_names) {
    if (!names || cls < 0 || cls >= n_names) return text_append(dst, n, "unknown");
    const char* s = names + (long long)cls * TEXT_LABEL_BYTES;
    for (int i = 0; i < TEXT_LABEL_BYTES - 1 && s[i] && n < TEXT_MAX_CHARS; ++i) dst[n++] = s[i];
    return n;
}

ADAS_HDI uint32_t text_class_colour(int cls, const uint32_t* table, int n) { return (table && cls >= 0 && cls < n) ? table[cls] : 0u; }
ADAS_HDI uint32_t text_pack(const uint8_t* c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }
ADAS_HDI bool text_in_range(double v) { return fabs(v) < TEXT_RANGE; }   // false for nan
ADAS_HDI bool text_in_range_i(int32_t v) { return v > -(1 << 30) && v < (1 << 30); }

ADAS_HDI const char* text_offset_string(int t) {   // OffsetType (ufldDetector/utils.py:10-14) by ADAS_OFFSET_*
    return t == 1 ? "Please Keep Right" : t == 2 ? "Please Keep Left" : t == 3 ? "Good Lane Keeping" : "To Be Determined ...";
}
ADAS_HDI const char* text_curvature_string(int t) {   // CurvatureType (ufldDetector/utils.py:16-22) by ADAS_CURVATURE_*
    return t == 1 ? "Keep Straight Ahead" : t == 2 ? "Gentle Left Curve Ahead" : t == 3 ? "Hard Left Curve Ahead" : t == 4 ? "Gentle Right Curve Ahead"
         : t == 5 ? "Hard Right Curve Ahead" : "To Be Determined ...";
}
ADAS_HDI const char* text_collision_string(int t) {   // CollisionType (ObjectDetector/utils.py:8-12) by ADAS_COLLISION_*
    return t == 1 ? "Normal Risk" : t == 2 ? "Prompt Risk" : t == 3 ? "Warning Risk" : "Determined ...";
}

// the candidates of one kind in frame q, in paint order
ADAS_HDI int text_candidates(const TextSrc& s, const TextTables& t, int kind, long long q) {
    int n = 0;
    if (kind == TEXT_DETECTIONS) { n = s.det_cnt[q * s.det_cnt_stride]; n = n < 0 ? 0 : (n > s.det_cap ? s.det_cap : n); }
    else if (kind == TEXT_TRACKS || kind == TEXT_TRACK_IDS) { n = *(const int32_t*)(s.trk_cnt + q * s.trk_cnt_bytes); n = n < 0 ? 0 : (n > s.trk_cap ? s.trk_cap : n); }
    else if (kind == TEXT_DISTANCE) { n = s.dist_cnt[q * s.dist_cnt_stride]; n = n < 0 ? 0 : (n > s.dist_cap ? s.dist_cap : n); }
    else if (kind == TEXT_PANELS) n = 3;
    else if (kind == TEXT_LINES) n = t.n_lines;
    return n;
}

// T5: candidate c of `kind` in frame q.  Returns the items it paints (0 .. 2); with out != null writes the first `room` of them; a candidate
// that is out of range paints none and sets TEXT_FLAG_RANGE in *flags.
ADAS_HDI int text_candidate(const TextSrc& s, const TextTables& t, const TextStyle& st, int kind, long long q, int c, TextItem* out, int room, int* flags) {
    const int W = s.src_w, H = s.src_h;
    char buf[TEXT_MAX_CHARS + 1];
    int n = 0;
    if (kind == TEXT_DETECTIONS) {   // yoloDetector.py:180-191
        const int32_t* b = s.det_xyxy + (q * s.det_cap + c) * 4;
        const int xmin = b[0], ymin = b[1];
        if (!text_in_range_i(xmin) || !text_in_range_i(ymin)) { *flags |= TEXT_FLAG_RANGE; return 0; }
        if (!out) return 2;
        const int cls = s.det_cls[q * s.det_cap + c];
        n = text_class_name(buf, 0, cls, t.det_names, t.n_det_names);
        int tw, th;
        text_size(t.fonts[st.det_size_slot], buf, n, &tw, &th);
        const bool known = t.det_names && cls >= 0 && cls < t.n_det_names;
        if (room > 0) text_make_rect(out, kind, xmin, ymin, (long long)xmin + tw, (long long)ymin - th - st.det_box_pad,
                                     known ? text_class_colour(cls, t.det_colors, t.n_det_colors) : 0u, W, H);
        if (room > 1) text_make_run(out + 1, t.fonts, kind, st.det_label_slot, (long long)xmin + st.det_label_dx, (long long)ymin + st.det_label_dy,
                                    text_pack(st.label_color), buf, n, W, H);
        return 2;
    }
    if (kind == TEXT_TRACKS || kind == TEXT_TRACK_IDS) {
        const long long at = q * s.trk_frame_bytes + c * s.trk_row_bytes, cat = q * s.trk_cls_frame_bytes + c * s.trk_cls_row_bytes;
        const double* tl = (const double*)(s.trk_tlwh + at);
        if (s.trk_act && !*(const int32_t*)(s.trk_act + at)) return 0;   // byteTracker.py:203
        if (!(tl[2] * tl[3] > st.min_box_area)) return 0;
        const int cls = *(const int32_t*)(s.trk_cls + cat), tid = *(const int32_t*)(s.trk_ids + cat);
        const uint32_t colour = text_class_colour(cls, t.trk_colors, t.n_trk_colors);
        if (kind == TEXT_TRACKS) {   // core.py:235-239
            if (!text_in_range(tl[0]) || !text_in_range(tl[1])) { *flags |= TEXT_FLAG_RANGE; return 0; }
            if (!out) return 1;
            n = text_class_name(buf, 0, cls, t.trk_names, t.n_trk_names);
            n = text_append(buf, n, " : ");
            char num[12];
            n = text_append_n(buf, n, num, text_format_int(tid, num));
            if (room > 0) text_make_run(out, t.fonts, kind, st.track_slot, (long long)(int)tl[0], (long long)(int)tl[1] + st.track_dy, colour, buf, n, W, H);
            return 1;
        }
        const double* bx;   // the newest box of the row's trajectory; core.py:188: drawn when the list holds more than one
        if (!s.slot_ids) {
            if (*(const int32_t*)(s.len + q * s.len_frame_bytes + (long long)c * 4) <= 1) return 0;
            bx = (const double*)(s.ring + q * s.ring_frame_bytes + (long long)c * 32);
        } else {
            const int slot = *(const int32_t*)(s.slot_ids + q * s.slot_frame_bytes + (long long)c * 4);
            if (slot < 0 || slot >= s.trk_cap) return 0;   // not a slot of the table: no trajectory
            const int appended = *(const int32_t*)(s.len + q * s.len_frame_bytes + slot * s.len_row_bytes);
            if (appended <= 1) return 0;
            bx = (const double*)(s.ring + q * s.ring_frame_bytes + (long long)slot * 960 + ((appended - 1) % 30) * 32);
        }
        const double v = (bx[2] + bx[3]) * 6e-4;
        const double fs = v < 1.0 ? v : 1.0;
        const double ox = bx[0] + 10.0 * fs, oy = bx[1] + 30.0 * fs;
        if (!text_in_range(ox) || !text_in_range(oy)) { *flags |= TEXT_FLAG_RANGE; return 0; }
        if (!out) return 2;
        n = text_append(buf, 0, "ID: ");
        char num[12];
        n = text_append_n(buf, n, num, text_format_int(tid, num));
        uint32_t shadow = 0;
        for (int ch = 0; ch < 3; ++ch) {
            const int cv = (int)((colour >> (8 * ch)) & 255u) - st.id_shadow_sub;
            shadow |= (uint32_t)(cv < 0 ? 0 : (cv > 255 ? 255 : cv)) << (8 * ch);
        }
        const long long x = (long long)(int)ox, y = (long long)(int)oy;
        if (room > 0) text_make_run(out, t.fonts, kind, text_ladder(t.fonts, st.id_shadow_first, st.id_shadow_count, fs), x + st.shadow_dx, y + st.shadow_dy,
                                    shadow, buf, n, W, H);
        if (room > 1) text_make_run(out + 1, t.fonts, kind, text_ladder(t.fonts, st.id_first, st.id_count, fs), x, y, colour, buf, n, W, H);
        return 2;
    }
    if (kind == TEXT_DISTANCE) {   // distanceMeasure.py:97-115
        const long long at = q * s.dist_cap + c;
        const int x = s.dist_xy[at * 2], y = s.dist_xy[at * 2 + 1];
        const double d = s.dist_d[at];
        char num[16];
        const bool big = !(d < 0) && d == d && !text_in_range(d);   // T1: finite or infinite, |d| >= 2^30; a negative d prints no number
        if (big || !text_in_range_i(x) || !text_in_range_i(y)) { *flags |= TEXT_FLAG_RANGE; return 0; }
        const int nl = d < 0 ? 0 : text_format_fixed(d, 2, num);
        if (!out) return 2;
        n = text_append(buf, 0, " ");
        n = d < 0 ? text_append(buf, n, "unknown") : text_append_n(buf, n, num, nl);
        n = text_append(buf, n, " m");
        double fs = 1.0;   // d == 0 and nan: 1
        if (d != 0.0 && d == d) {
            const double r = 1.0 / d;
            const double m = r < 1.0 ? r : 1.0;
            fs = m > 0.4 ? m : 0.4;
        }
        int tw, th;
        text_size(t.fonts[text_ladder(t.fonts, st.dist_size_first, st.dist_size_count, fs)], buf, n, &tw, &th);
        const long long tx = (2LL * x - tw) / 2 + 1, ty = (long long)y + th + 5;   // int(x - tw / 2) + 1: towards zero
        if (room > 0) text_make_run(out, t.fonts, kind, text_ladder(t.fonts, st.dist_shadow_first, st.dist_shadow_count, fs), tx + st.shadow_dx,
                                    ty + st.shadow_dy, text_pack(st.dist_shadow_color), buf, n, W, H);
        if (room > 1) text_make_run(out + 1, t.fonts, kind, text_ladder(t.fonts, st.dist_first, st.dist_count, fs), tx, ty, text_pack(st.dist_color), buf, n, W, H);
        return 2;
    }
    if (kind == TEXT_PANELS) {   // demo.py:173-174, 212
        if (!out) return 1;
        if (room < 1) return 1;
        if (c == 0) {
            const int ty = s.offset[q * s.msg_stride];
            n = text_append(buf, text_append(buf, 0, "LDWS : "), text_offset_string(ty));
            text_make_run(out, t.fonts, kind, st.ldws_slot, st.ldws_x, st.ldws_y, text_pack(st.offset_colors[ty >= 1 && ty <= 3 ? ty : 0]), buf, n, W, H);
        } else if (c == 1) {
            const int ty = s.curvature[q * s.msg_stride];
            n = text_append(buf, text_append(buf, 0, "LKAS : "), text_curvature_string(ty));
            text_make_run(out, t.fonts, kind, st.lkas_slot, st.lkas_x, st.lkas_y, text_pack(st.curvature_colors[ty >= 1 && ty <= 5 ? ty : 0]), buf, n, W, H);
        } else {
            const int ty = s.collision[q * s.msg_stride];
            n = text_append(buf, text_append(buf, 0, "FCWS : "), text_collision_string(ty));
            text_make_run(out, t.fonts, kind, st.fcws_slot, (long long)W - (int)(W * st.show_ratio) + st.fcws_dx, st.fcws_y,
                          text_pack(st.collision_colors[ty >= 1 && ty <= 3 ? ty : 0]), buf, n, W, H);
        }
        return 1;
    }
    if (kind == TEXT_LINES) {
        if (!out || room < 1) return 1;
        const TextLine& l = t.lines[c];
        text_make_run(out, t.fonts, kind, l.slot, l.x, l.y, text_pack(l.color), l.text, l.len, W, H);
        return 1;
    }
    return 0;
}

// ---- T4
ADAS_HDI uint32_t text_blend(uint32_t dst, uint32_t colour, uint32_t c) { return (dst * (255u - c) + colour * c + 127u) / 255u; }

// T7 on one 16-byte piece: w holds bytes [b0, b0 + 16) of row `row` of the item's frame (b0 relative to the row's first byte, any sign);
// the bytes of the piece that item `it` paints are replaced.  Bytes outside the item's clipped box are never touched.  Returns whether any
// byte was.
ADAS_HDI bool text_fold_piece(const TextFont* fonts, const TextItem& it, int row, int b0, uint32_t w[4]) {
    if (row < it.by0 || row >= it.by1) return false;
    const int lo = it.bx0 * 3 > b0 ? it.bx0 * 3 : b0, hi = it.bx1 * 3 < b0 + 16 ? it.bx1 * 3 : b0 + 16;
    if (lo >= hi) return false;
    if (it.kind == TEXT_ITEM_RECT) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 16; ++j) {
            const int b = b0 + j;
            if (b < lo || b >= hi) continue;
            const uint32_t col = it.color[b % 3];
            w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (col << (8 * (j & 3)));
        }
        return true;
    }
    if (it.kind != TEXT_ITEM_RUN) return false;
    const TextFont& f = fonts[it.slot];
    const int ar = row - (it.y - f.baseline_row);   // 0 .. cell_h - 1 by the box
    if (ar < 0 || ar >= f.cell_h) return false;
    const uint8_t* arow = f.atlas + (long long)ar * f.atlas_w;
    long long pen = (long long)it.x * 65536;
    bool any = false;
    for (int i = 0; i < it.len; ++i) {
        const int g = text_glyph(it.text[i]);
        const long long gx0 = (pen >> 16) + f.bearing_x[g];
        pen += f.advance[g];
        const int gw = f.glyph_w[g];
        if (gw <= 0 || (gx0 + gw) * 3 <= lo || gx0 * 3 >= hi) continue;
        const uint8_t* gp = arow + f.glyph_x[g];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 16; ++j) {
            const int b = b0 + j;
            if (b < lo || b >= hi) continue;
            const int px = b / 3;   // b >= 0 here
            const long long k = px - gx0;
            if (k < 0 || k >= gw) continue;
            const uint32_t cov = gp[k];
            if (!cov) continue;
            const uint32_t dst = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            const uint32_t v = text_blend(dst, it.color[b - px * 3], cov);
            w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (v << (8 * (j & 3)));
            any = true;
        }
    }
    return any;
}

}  // namespace adas
