// scale_core.h -- finished BGR frames reduced to previews and a stream mosaic: the rules of adas_scale_* and the byte addresses of every load
// and store its work items make, shared by the HIP kernel (scale_kernels.hip) and a host build (tests/hostemu/emu_scale.cpp) so that an
// indexing mistake shows on the CPU.  What a caller's cv2.resize(frame_show, size, interpolation=INTER_AREA / INTER_LINEAR) and the NumPy
// slice assignments of a video wall do on host cores.  The rules below are the authority: parity with a real cv2 build is unpinned -- cv2 was
// not available where this was written; S4 is overlay_panel_core.h's P5 (itself unpinned), S5 is an exact box filter which cv2's INTER_AREA
// approximates in floating point, and tests/scale_ref.py restates S2-S6 independently in NumPy and Python integers.
//
//   S1 source      BGR u8 [batch][src_h][src_w][3], tightly packed: what the overlay, the step's camera frames, the JPEG decoder and the YUV
//                  converter hold.
//   S2 canvases    a tile is dst_w x dst_h; a canvas is cols x rows tiles, BGR u8 [rows * dst_h][cols * dst_w][3], tightly packed, canvas k
//                  at k * canvas_bytes.  cols = rows = 1 is one reduced frame per frame: there is no separate path without a mosaic.  With
//                  T = cols * rows, frame f goes to canvas f / T, cell f % T, tile row cell / cols, tile column cell % cols; a run of `batch`
//                  frames writes ceil(batch / T) canvases.
//   S3 write-once  every byte of those canvases is written exactly once per run; a cell without a frame (the last canvas of a batch that is
//                  no multiple of T) is filled with `background`, so nothing of an earlier run survives.  No byte outside those canvases is
//                  written, no byte outside a source frame is read.
//   S4 `linear`    rule P5 of overlay_panel_core.h, evaluated by calling panel_scale / panel_row_tap / panel_col_tap / panel_resize_taps on
//                  the four taps' twelve bytes -- not restated here.  Any source and destination size; equal sizes are a copy.
//   S5 `area`      an exact box filter in integers, reduction only (dst_w > src_w or dst_h > src_h is refused).  Destination column dx covers
//                  the source columns x with x * dst_w < (dx + 1) * src_w and (x + 1) * dst_w > dx * src_w, each with the weight
//                    wx = min((x + 1) * dst_w, (dx + 1) * src_w) - max(x * dst_w, dx * src_w),   sum wx = src_w;
//                  rows likewise with wy, sum wy = src_h.  With D = src_w * src_h a byte is
//                    (sum_y wy * (sum_x wx * p) + D / 2) / D   in floor division: round to nearest, ties up.
//                  D <= 2^23 is required.  uint32 then holds all of it: sum_x wx * p <= 255 * src_w, the double sum <= 255 * D, and the
//                  numerator <= 255 * D + D / 2 <= 255 * 2^23 + 2^22 = 2143289344 < 2^31 = 2147483648.  The sides are at most 16383, so
//                  every product of a coordinate and a side stays below 2^28.  At a ratio of exactly 2 this is (a + b + c + d + 2) >> 2; at
//                  equal sizes it is a copy.  The division is a plain uint32 one, on the device as on the host.
//   S6 border      with border > 0 (2 * border < min(dst_w, dst_h)) and a per-frame state array, the outermost `border` pixel rings of frame
//                  f's tile take border_bgr[state] in place of the resized pixels, state = the int32 at d_state + f * state_stride bytes (the
//                  form in which the panels read the analysis rows' collision column), indexed by ANA_COLLISION_*; a state outside 0..3
//                  counts as 0 (UNKNOWN).  No state array or border = 0: nothing is drawn.  Empty cells have no border.
//   S7 determinism a tile's bytes depend on its frame, its state and the parameters alone.
//   S8 addressing  scale_src_at (a source pixel's B byte inside its frame), scale_frame_bytes, scale_canvas_bytes and scale_item's own
//                  arithmetic give the byte offset of every access.  Work is numbered per canvas; scale_path decides for a whole run:
//                    staged block   (`area`, SCALE_PATH_STAGED) a workgroup per segment of a tile row: 16-byte source loads through LDS,
//                                   16-byte canvas stores; the section "`area`, staged" below says how.
//                    vector item    (`linear`, SCALE_PATH_PIECES) 16 consecutive bytes of one canvas row (5 1/3 pixels of one tile): byte
//                                   loads of the taps, one 16-byte store.
//                    generic item   (SCALE_PATH_GENERIC) one canvas pixel: byte loads, three byte stores, no alignment assumed.
//                  The two vector paths need scale_vector_ok: the tile's row bytes (dst_w * 3, hence the canvas row's bytes, every tile's
//                  offset in its row and canvas_bytes) and both base pointers are multiples of 16; the staged one also that a segment's
//                  source columns fit its LDS rows (scale_staged_plan: up to 16 KB of a source row for 256 tile pixels).  Every path writes
//                  the same bytes.  Loop counts come from the sizes, never from pixel data.
#pragma once
#include <stdint.h>
#include <string.h>
#include "overlay_panel_core.h"

namespace adas {

#define SCALE_MODE_AREA 0
#define SCALE_MODE_LINEAR 1
#define SCALE_MAX_DIM 16383
#define SCALE_MAX_D (1 << 23)

#define SCALE_OK 0
#define SCALE_BAD_MODE 1
#define SCALE_BAD_SIZE 2
#define SCALE_BAD_MOSAIC 3
#define SCALE_ENLARGE 4
#define SCALE_BIG_D 5
#define SCALE_BAD_BORDER 6
#define SCALE_BIG_CANVAS 7

// adas_scale_params, field for field (scale_kernels.hip asserts it)
struct ScaleParams {
    int32_t src_w, src_h;
    int32_t dst_w, dst_h;
    int32_t mode;
    int32_t cols, rows;
    int32_t border;
    uint8_t background[4];      // B, G, R, unused
    uint8_t border_bgr[4][4];   // [ANA_COLLISION_*] B, G, R, unused
};

ADAS_HDI long long scale_frame_bytes(const ScaleParams& p) { return (long long)p.src_w * p.src_h * 3; }
ADAS_HDI long long scale_canvas_row_bytes(const ScaleParams& p) { return (long long)p.cols * p.dst_w * 3; }
ADAS_HDI long long scale_canvas_bytes(const ScaleParams& p) { return scale_canvas_row_bytes(p) * p.rows * p.dst_h; }
ADAS_HDI int scale_canvases(const ScaleParams& p, int batch) {
    const int T = p.cols * p.rows;
    return (batch + T - 1) / T;
}

ADAS_HDI int scale_check(const ScaleParams& p) {
    if (p.mode != SCALE_MODE_AREA && p.mode != SCALE_MODE_LINEAR) return SCALE_BAD_MODE;
    if (p.src_w < 1 || p.src_h < 1 || p.dst_w < 1 || p.dst_h < 1) return SCALE_BAD_SIZE;
    if (p.src_w > SCALE_MAX_DIM || p.src_h > SCALE_MAX_DIM || p.dst_w > SCALE_MAX_DIM || p.dst_h > SCALE_MAX_DIM) return SCALE_BAD_SIZE;
    if (p.cols < 1 || p.rows < 1 || p.cols > SCALE_MAX_DIM || p.rows > SCALE_MAX_DIM) return SCALE_BAD_MOSAIC;
    if (p.mode == SCALE_MODE_AREA && (p.dst_w > p.src_w || p.dst_h > p.src_h)) return SCALE_ENLARGE;
    if (p.mode == SCALE_MODE_AREA && (long long)p.src_w * p.src_h > SCALE_MAX_D) return SCALE_BIG_D;
    if (p.border < 0 || 2 * (long long)p.border >= (p.dst_w < p.dst_h ? p.dst_w : p.dst_h)) return SCALE_BAD_BORDER;
    if ((long long)p.cols * p.dst_w > 0x7fffffffLL / 3 || scale_canvas_bytes(p) > 0x7fffffffLL) return SCALE_BIG_CANVAS;
    return SCALE_OK;
}

// ------------------------------------------------------------------------------------------------------------- S8: where the bytes are
// pixel (x, y)'s B byte inside its (tight) source frame
ADAS_HDI long long scale_src_at(const ScaleParams& p, int x, int y) { return ((long long)y * p.src_w + x) * 3; }
// the path of a whole run
ADAS_HDI bool scale_vector_ok(const ScaleParams& p, const void* src, const void* dst) {
    const long long m = (long long)(uintptr_t)src | (long long)(uintptr_t)dst | ((long long)p.dst_w * 3);
    return (m & 15) == 0;
}
// work items of one canvas: 16-byte pieces, or pixels (both fit 31 bits: scale_check's SCALE_BIG_CANVAS)
ADAS_HDI uint32_t scale_items_per_canvas(const ScaleParams& p, bool vec) {
    return vec ? (uint32_t)(scale_canvas_bytes(p) / 16) : (uint32_t)(scale_canvas_bytes(p) / 3);
}

// ------------------------------------------------------------------------------------------------------------------ memory accesses
// Every load and store of an item goes through these.  A host build that defines SCALE_AUDIT sees each one's address, width and required
// alignment (scale_audit; kind 0 a source load, 1 a canvas store, 2 a state load) before it happens, and an access it answers with false does
// not happen (a load then gives zero).
#if defined(SCALE_AUDIT) && !defined(__HIP_DEVICE_COMPILE__)
bool scale_audit(const void* p, int bytes, int align, int kind);
#define SCALE_AUDIT_CALL(p, n, a, k) scale_audit(p, n, a, k)
#else
#define SCALE_AUDIT_CALL(p, n, a, k) true
#endif

ADAS_HDI uint32_t scale_ld1(const uint8_t* p) {
    if (!SCALE_AUDIT_CALL(p, 1, 1, 0)) return 0;
    return *p;
}
ADAS_HDI void scale_st1(uint8_t* p, uint32_t v) {
    if (!SCALE_AUDIT_CALL(p, 1, 1, 1)) return;
    *p = (uint8_t)v;
}
// 16 bytes, lo's lowest byte first
ADAS_HDI void scale_st16(uint8_t* p, uint64_t lo, uint64_t hi) {
    if (!SCALE_AUDIT_CALL(p, 16, 16, 1)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint4*)p = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
#else
    const uint64_t w[2] = {lo, hi};   // little endian, as the device
    memcpy(p, w, 16);
#endif
}
ADAS_HDI int scale_ld_state(const uint8_t* p) {
    if (!SCALE_AUDIT_CALL(p, 4, 4, 2)) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const int32_t*)p;
#else
    int32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}

// ------------------------------------------------------------------------------------------------------------------ S4, S5: a pixel
// the first source index and the one behind the last that destination index d of `dn` covers in a side of `sn`
ADAS_HDI void scale_area_span(int d, int dn, int sn, int* lo, int* hi) {
    *lo = (d * sn) / dn;
    *hi = ((d + 1) * sn + dn - 1) / dn;
}
// S5's weight of source index s for destination index d
ADAS_HDI int scale_area_weight(int s, int d, int dn, int sn) {
    const int a = (s + 1) * dn, b = (d + 1) * sn, c = s * dn, e = d * sn;
    return (a < b ? a : b) - (c > e ? c : e);
}

// tile pixel (dx, dy) of frame `s` in `area`, packed B | G << 8 | R << 16; only the channels of chmask are loaded, the others are 0
ADAS_HDI uint32_t scale_area_px(const ScaleParams& p, const uint8_t* s, int dx, int dy, int chmask) {
    int x0, x1, y0, y1;
    scale_area_span(dx, p.dst_w, p.src_w, &x0, &x1);
    scale_area_span(dy, p.dst_h, p.src_h, &y0, &y1);
    const uint32_t D = (uint32_t)p.src_w * (uint32_t)p.src_h;
    uint32_t acc[3] = {0, 0, 0};
    for (int y = y0; y < y1; ++y) {
        const uint32_t wy = (uint32_t)scale_area_weight(y, dy, p.dst_h, p.src_h);
        uint32_t row[3] = {0, 0, 0};
        const uint8_t* q = s + scale_src_at(p, x0, y);
        for (int x = x0; x < x1; ++x, q += 3) {
            const uint32_t wx = (uint32_t)scale_area_weight(x, dx, p.dst_w, p.src_w);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                if ((chmask >> ch) & 1) row[ch] += wx * scale_ld1(q + ch);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += wy * row[ch];
    }
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        if ((chmask >> ch) & 1) out |= ((acc[ch] + D / 2) / D) << (8 * ch);
    return out;
}

// tile pixel (dx, dy) of frame `s` in `linear`: P5 on the four taps, gathered through the audited loads
ADAS_HDI uint32_t scale_linear_px(const ScaleParams& p, const uint8_t* s, int dx, int dy) {
    if (p.dst_w == p.src_w && p.dst_h == p.src_h) {
        const uint8_t* q = s + scale_src_at(p, dx, dy);
        return scale_ld1(q) | (scale_ld1(q + 1) << 8) | (scale_ld1(q + 2) << 16);
    }
    const PanelTap r = panel_row_tap(dy, panel_scale(p.dst_h, p.src_h), p.src_h);
    const PanelTap c = panel_col_tap(dx, panel_scale(p.dst_w, p.src_w), p.src_w);
    uint8_t r0[6], r1[6];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        r0[ch] = (uint8_t)scale_ld1(s + scale_src_at(p, c.s0, r.s0) + ch);
        r0[3 + ch] = (uint8_t)scale_ld1(s + scale_src_at(p, c.s1, r.s0) + ch);
        r1[ch] = (uint8_t)scale_ld1(s + scale_src_at(p, c.s0, r.s1) + ch);
        r1[3 + ch] = (uint8_t)scale_ld1(s + scale_src_at(p, c.s1, r.s1) + ch);
    }
    PanelTap t = c;
    t.s0 = 0;
    t.s1 = 1;
    return panel_resize_taps(r0, r1, r.c0, r.c1, t);
}

ADAS_HDI uint32_t scale_pack_bgr(const uint8_t* c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }
ADAS_HDI bool scale_on_border(const ScaleParams& p, int dx, int dy) {
    return dx < p.border || dy < p.border || dx >= p.dst_w - p.border || dy >= p.dst_h - p.border;
}
// S6: frame f's border colour, or -1 when nothing is drawn
ADAS_HDI int64_t scale_border_colour(const ScaleParams& p, const uint8_t* state, long long state_stride, int f) {
    if (p.border <= 0 || !state) return -1;
    int st = scale_ld_state(state + (long long)f * state_stride);
    if (st < 0 || st > 3) st = 0;
    return (int64_t)scale_pack_bgr(p.border_bgr[st]);
}
// S4-S6: tile pixel (dx, dy) of frame `s`; MODE is p.mode
template <int MODE>
ADAS_HDI uint32_t scale_tile_px(const ScaleParams& p, const uint8_t* s, int64_t border, int dx, int dy, int chmask) {
    if (border >= 0 && scale_on_border(p, dx, dy)) return (uint32_t)border;
    return MODE == SCALE_MODE_LINEAR ? scale_linear_px(p, s, dx, dy) : scale_area_px(p, s, dx, dy, chmask);
}

// ------------------------------------------------------------------------------------------------------------------ the work items
// item t (0 <= t < scale_items_per_canvas) of canvas k: src, state (or null) and dst are the run's base pointers; MODE is p.mode
template <int MODE>
ADAS_HDI void scale_item(const ScaleParams& p, bool vec, int batch, const uint8_t* src, const uint8_t* state, long long state_stride, uint8_t* dst,
                         int k, uint32_t t) {
    const int T = p.cols * p.rows, tile_rb = p.dst_w * 3;
    const long long row_rb = scale_canvas_row_bytes(p);
    uint8_t* canvas = dst + (long long)k * scale_canvas_bytes(p);
    if (vec) {
        const uint32_t per_row = (uint32_t)(row_rb / 16);
        const int y = (int)(t / per_row);
        const long long byte0 = 16LL * (t - (uint32_t)y * per_row);
        const int tcol = (int)(byte0 / tile_rb), tb = (int)(byte0 - (long long)tcol * tile_rb);   // tb + 15 < tile_rb: both multiples of 16
        const int trow = y / p.dst_h, dy = y - trow * p.dst_h;
        const int f = k * T + trow * p.cols + tcol;
        const bool empty = f >= batch;
        const uint8_t* s = src + (long long)(empty ? 0 : f) * scale_frame_bytes(p);
        const int64_t border = empty ? -1 : scale_border_colour(p, state, state_stride, f);
        const int px0 = tb / 3;
        uint64_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {   // 16 bytes touch at most 7 pixels
            const int dx = px0 + j, pos = 3 * dx - tb;   // pos in -2 .. 18: the pixel's B byte inside the piece
            int chmask = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                if (pos + ch >= 0 && pos + ch < 16) chmask |= 1 << ch;
            if (!chmask) continue;
            const uint32_t v = empty ? scale_pack_bgr(p.background) : scale_tile_px<MODE>(p, s, border, dx, dy, chmask);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int b = pos + ch;
                if (b < 0 || b >= 16) continue;
                const uint64_t byte = (v >> (8 * ch)) & 255u;
                if (b < 8)
                    lo |= byte << (8 * b);
                else
                    hi |= byte << (8 * (b - 8));
            }
        }
        scale_st16(canvas + (long long)y * row_rb + byte0, lo, hi);
        return;
    }
    const uint32_t cw = (uint32_t)(p.cols * p.dst_w);
    const int y = (int)(t / cw), x = (int)(t - (uint32_t)y * cw);
    const int tcol = x / p.dst_w, dx = x - tcol * p.dst_w, trow = y / p.dst_h, dy = y - trow * p.dst_h;
    const int f = k * T + trow * p.cols + tcol;
    uint32_t v;
    if (f >= batch)
        v = scale_pack_bgr(p.background);
    else
        v = scale_tile_px<MODE>(p, src + (long long)f * scale_frame_bytes(p), scale_border_colour(p, state, state_stride, f), dx, dy, 7);
    uint8_t* o = canvas + (long long)y * row_rb + 3LL * x;
    scale_st1(o, v & 255u);
    scale_st1(o + 1, (v >> 8) & 255u);
    scale_st1(o + 2, (v >> 16) & 255u);
}

// ------------------------------------------------------------------------------------------------------------------ `area`, staged
// The vector path of `area`: a workgroup of SCALE_BLOCK lanes owns one segment (at most SCALE_BLOCK pixels, a multiple of 16) of one tile
// row.  For every source row of that tile row's span it brings the segment's source columns into LDS in 16-byte pieces -- neighbouring
// lanes load neighbouring pieces, so a wavefront's loads of a source row are contiguous -- each lane adds the row's share to the three sums
// of its own pixel from LDS, and at the end the segment's bytes meet in LDS and leave in 16-byte stores.  A piece that is not wholly inside
// the columns the segment needs (the first and the last of a row) is loaded byte by byte, those columns' bytes alone, so nothing else is
// read.  The next row's pieces are loaded into registers in front of the current row's sums and written to the other LDS buffer behind them:
// one barrier per source row.  The phases below are one lane's part each; the kernel and the host build call them in the same order with a
// barrier (the host: the end of a loop over the lanes) between them.
#define SCALE_BLOCK 256
#define SCALE_STAGE_PIECES 4   // pieces of one source row a lane loads at most

struct ScaleStaged {
    int32_t n_seg, seg_px;   // segments of a tile row, pixels of every segment but the last
    int32_t lds_row;         // bytes of one staged source row: a multiple of 16
};
ADAS_HDI int scale_staged_lds_bytes(const ScaleStaged& s) { return 2 * s.lds_row + SCALE_BLOCK * 3; }

// the plan of a run; false when `area` cannot go this way (a tile width that is no multiple of 16, or columns too many to stage)
ADAS_HDI bool scale_staged_plan(const ScaleParams& p, ScaleStaged* s) {
    if (p.mode != SCALE_MODE_AREA || p.dst_w % 16) return false;
    const int n = (p.dst_w + SCALE_BLOCK - 1) / SCALE_BLOCK;
    s->seg_px = (((p.dst_w + n - 1) / n) + 15) & ~15;
    s->n_seg = (p.dst_w + s->seg_px - 1) / s->seg_px;
    int most = 0;
    for (int g = 0; g < s->n_seg; ++g) {
        const int px0 = g * s->seg_px, px1 = px0 + s->seg_px < p.dst_w ? px0 + s->seg_px : p.dst_w;
        int lo, hi, unused;
        scale_area_span(px0, p.dst_w, p.src_w, &lo, &unused);
        scale_area_span(px1 - 1, p.dst_w, p.src_w, &unused, &hi);
        if ((hi - lo) * 3 > most) most = (hi - lo) * 3;
    }
    s->lds_row = 16 * ((most + 30) / 16 + 1);   // the pieces that [o, o + most) touches for any o, and one to spare
    return s->lds_row / 16 <= SCALE_BLOCK * SCALE_STAGE_PIECES;
}
ADAS_HDI uint32_t scale_staged_blocks_per_canvas(const ScaleParams& p, const ScaleStaged& s) {
    return (uint32_t)(p.rows * p.dst_h) * (uint32_t)(p.cols * s.n_seg);   // < 2^31: fewer than a canvas has bytes
}

struct ScaleBlock {
    int dy, f, px0, npx;          // tile row, frame, first pixel and pixels of the segment
    int empty;                    // a cell without a frame
    int64_t border;               // S6's colour or -1
    int x_lo, x_hi, y_lo, y_hi;   // the source columns and rows the segment needs (hi: one behind)
    long long frame_off, out_off; // frame f inside the source, the segment's first byte inside the destination
};
// block b (0 <= b < scale_staged_blocks_per_canvas) of canvas k
ADAS_HDI ScaleBlock scale_block(const ScaleParams& p, const ScaleStaged& s, int batch, const uint8_t* state, long long state_stride, int k, uint32_t b) {
    ScaleBlock B;
    const uint32_t per_row = (uint32_t)(p.cols * s.n_seg);
    const int y = (int)(b / per_row), r = (int)(b - (uint32_t)y * per_row), tcol = r / s.n_seg, g = r - tcol * s.n_seg;
    const int trow = y / p.dst_h;
    B.dy = y - trow * p.dst_h;
    B.f = k * (p.cols * p.rows) + trow * p.cols + tcol;
    B.empty = B.f >= batch;
    B.px0 = g * s.seg_px;
    B.npx = B.px0 + s.seg_px < p.dst_w ? s.seg_px : p.dst_w - B.px0;
    B.border = B.empty ? -1 : scale_border_colour(p, state, state_stride, B.f);
    int unused;
    scale_area_span(B.px0, p.dst_w, p.src_w, &B.x_lo, &unused);
    scale_area_span(B.px0 + B.npx - 1, p.dst_w, p.src_w, &unused, &B.x_hi);
    scale_area_span(B.dy, p.dst_h, p.src_h, &B.y_lo, &B.y_hi);
    // nothing is read for a cell without a frame, or for a row that lies in the border as a whole
    if (B.empty || (B.border >= 0 && (B.dy < p.border || B.dy >= p.dst_h - p.border))) B.y_hi = B.y_lo;
    B.frame_off = (long long)(B.empty ? 0 : B.f) * scale_frame_bytes(p);
    B.out_off = (long long)k * scale_canvas_bytes(p) + (long long)y * scale_canvas_row_bytes(p) + 3LL * (tcol * p.dst_w + B.px0);
    return B;
}

struct ScalePiece {
    uint32_t w[4];
};
// phase 1, lane `tid`, its i-th piece of source row sy into registers
ADAS_HDI ScalePiece scale_stage_load(const ScaleParams& p, const ScaleBlock& B, const uint8_t* src, int sy, int tid, int i) {
    ScalePiece v;
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    const long long lo = B.frame_off + scale_src_at(p, B.x_lo, sy), hi = B.frame_off + scale_src_at(p, B.x_hi, sy);
    const long long a = (lo & ~15LL) + 16LL * (tid + SCALE_BLOCK * i);
    if (a >= hi) return v;
    if (a >= lo && a + 16 <= hi) {
        if (!SCALE_AUDIT_CALL(src + a, 16, 16, 0)) return v;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 q = *(const uint4*)(src + a);
        v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
#else
        memcpy(v.w, src + a, 16);
#endif
        return v;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)   // the first or the last piece of the row: the needed bytes alone
        if (a + j >= lo && a + j < hi) v.w[j >> 2] |= scale_ld1(src + a + j) << (8 * (j & 3));
    return v;
}
// phase 3, the same piece into the LDS row buffer
ADAS_HDI void scale_stage_write(const ScaleStaged& s, uint8_t* lds_row, int tid, int i, const ScalePiece& v) {
    const int q = tid + SCALE_BLOCK * i;
    if (q >= s.lds_row / 16) return;
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint4*)(lds_row + 16 * q) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
#else
    memcpy(lds_row + 16 * q, v.w, 16);   // little endian, as the device
#endif
}
// phase 2, lane `tid`: source row sy's share of its pixel's three sums, from the LDS row buffer that holds that row
ADAS_HDI void scale_block_accumulate(const ScaleParams& p, const ScaleBlock& B, const uint8_t* lds_row, int sy, int tid, uint32_t* acc) {
    if (tid >= B.npx) return;
    const int dx = B.px0 + tid;
    int x0, x1;
    scale_area_span(dx, p.dst_w, p.src_w, &x0, &x1);
    const long long lo = B.frame_off + scale_src_at(p, B.x_lo, sy);
    const uint8_t* q = lds_row + (int)(lo & 15) + 3 * (x0 - B.x_lo);
    uint32_t row[3] = {0, 0, 0};
    for (int x = x0; x < x1; ++x, q += 3) {
        const uint32_t wx = (uint32_t)scale_area_weight(x, dx, p.dst_w, p.src_w);
        row[0] += wx * q[0];
        row[1] += wx * q[1];
        row[2] += wx * q[2];
    }
    const uint32_t wy = (uint32_t)scale_area_weight(sy, B.dy, p.dst_h, p.src_h);
    acc[0] += wy * row[0];
    acc[1] += wy * row[1];
    acc[2] += wy * row[2];
}
// phase 4, lane `tid`: its pixel's three bytes into the LDS output row
ADAS_HDI void scale_block_finish(const ScaleParams& p, const ScaleBlock& B, uint8_t* lds_out, int tid, const uint32_t* acc) {
    if (tid >= B.npx) return;
    const uint32_t D = (uint32_t)p.src_w * (uint32_t)p.src_h;
    uint32_t v;
    if (B.empty)
        v = scale_pack_bgr(p.background);
    else if (B.border >= 0 && scale_on_border(p, B.px0 + tid, B.dy))
        v = (uint32_t)B.border;
    else
        v = ((acc[0] + D / 2) / D) | (((acc[1] + D / 2) / D) << 8) | (((acc[2] + D / 2) / D) << 16);
    lds_out[3 * tid] = (uint8_t)v;
    lds_out[3 * tid + 1] = (uint8_t)(v >> 8);
    lds_out[3 * tid + 2] = (uint8_t)(v >> 16);
}
// phase 5, lane `tid`: 16 bytes of the LDS output row into the canvas
ADAS_HDI void scale_block_store(const ScaleBlock& B, const uint8_t* lds_out, uint8_t* dst, int tid) {
    if (tid >= B.npx * 3 / 16) return;   // npx is a multiple of 16
    uint64_t w[2];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 q = *(const uint4*)(lds_out + 16 * tid);
    w[0] = q.x | ((uint64_t)q.y << 32);
    w[1] = q.z | ((uint64_t)q.w << 32);
#else
    memcpy(w, lds_out + 16 * tid, 16);
#endif
    scale_st16(dst + B.out_off + 16LL * tid, w[0], w[1]);
}

#define SCALE_PATH_GENERIC 0
#define SCALE_PATH_PIECES 1
#define SCALE_PATH_STAGED 2
// the path of a whole run (S8); *s is filled for SCALE_PATH_STAGED
ADAS_HDI int scale_path(const ScaleParams& p, const void* src, const void* dst, ScaleStaged* s) {
    if (!scale_vector_ok(p, src, dst)) return SCALE_PATH_GENERIC;
    if (p.mode == SCALE_MODE_LINEAR) return SCALE_PATH_PIECES;
    return scale_staged_plan(p, s) ? SCALE_PATH_STAGED : SCALE_PATH_GENERIC;
}

}  // namespace adas
