// Host build of the UI panels' rules (csrc/overlay_panel_core.h; g++, one thread): the choice functions, the resize and the per-byte fold the
// device kernels evaluate, composed the way the draw kernel composes them -- the geometry once, the row spans of a run, P6 on every pixel of a
// span -- so that the CPU suite can compare them record for record and byte for byte with tests/panels_ref.py.  Test scaffolding only; never
// loaded by the product.
#include <string.h>
#include <vector>
#include "overlay_panel_core.h"

using namespace adas;

namespace {

struct HostBird {   // P5 straight from the image: no table
    const uint8_t* img;
    const PanelGeom* g;
    const uint8_t* base = nullptr;   // [frames][bird_h][bird_w][3]
    void frame(int ff) { img = base ? base + (size_t)ff * g->bird_h * g->bird_w * 3 : nullptr; }
    uint32_t operator()(int ry, int rx) const { return panel_resize_px(img, g->bird_h, g->bird_w, g->H, g->W, ry, rx); }
};

}  // namespace

extern "C" {

// out: first sprite, second sprite, latch after
void emu_panel_choose(int latch, int offset_type, int curvature_type, int* out) { panel_choose_signs(latch, offset_type, curvature_type, out, out + 1, out + 2); }

int emu_panel_choose_collision(int collision_type) { return panel_choose_collision(collision_type); }

// src [sh][sw][3] -> dst [dh][dw][3]
void emu_panel_resize(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw) {
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            const uint32_t v = panel_resize_px(src, sh, sw, dh, dw, y, x);
            uint8_t* p = dst + ((size_t)y * dw + x) * 3;
            p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
        }
}

// PANEL_FIT_* of a frame size under params with the sprites' sizes; *slot: the offending sprite
int emu_panel_fit(int H, int W, const PanelParams* params, const int* sprite_w, const int* sprite_h, int* slot) {
    PanelGeom g;
    return panel_geometry(H, W, 0, 0, *params, sprite_w, sprite_h, &g, slot);
}

// One frame, in place: img [H][W][3]; bird [bh][bw][3] or null; sprites: nine [h][w][4] BGRA arrays (null: empty) with their sizes; rec: the
// frame's record, 8 ints (sign[2], collision, latch after, the three types, 0).  Returns PANEL_FIT_* of the geometry, or, with bit 30 set, the
// number of pixels P6 writes outside the row spans of the run (never expected).
int emu_panels_frame(uint8_t* img, int H, int W, const uint8_t* bird, int bh, int bw, const PanelParams* params, const uint8_t* const* sprites,
                     const int* sprite_w, const int* sprite_h, int panels, int latch, int offset_type, int curvature_type, int collision_type, int* rec) {
    PanelGeom g;
    int slot = -1;
    const int fit = panel_geometry(H, W, bird ? bh : 0, bird ? bw : 0, *params, sprite_w, sprite_h, &g, &slot);
    if (fit) return fit;
    size_t pixels = 0;
    for (int k = 0; k < PANEL_SPRITES; ++k) pixels += (size_t)g.sp[k].w * g.sp[k].h;
    std::vector<uint32_t> atlas(pixels ? pixels : 1);
    for (int k = 0; k < PANEL_SPRITES; ++k)
        if (g.sp[k].w > 0) memcpy(atlas.data() + g.sp[k].off, sprites[k], (size_t)g.sp[k].w * g.sp[k].h * 4);
    const PanelRecord r = panel_step(panels, latch, offset_type, curvature_type, collision_type);
    memcpy(rec, &r, sizeof(r));
    const PanelSpans sp = panel_spans(g, panels);
    HostBird hb;
    hb.img = bird;
    hb.g = &g;
    int stray = 0;
    for (int row = 0; row < H; ++row) {
        PanelRowSpans rs = panel_row_spans(sp, W, row);
        if (row < sp.row0 || row >= sp.row1) rs.n = 0;
        for (int col = 0; col < W; ++col) {
            bool in_span = false;
            for (int i = 0; i < rs.n; ++i) in_span = in_span || (col >= rs.c0(i) && col < rs.c1(i));
            uint8_t* p = img + ((size_t)row * W + col) * 3;
            for (int ch = 0; ch < 3; ++ch) {   // per byte: the other two channels of v are noise, as for a lane that holds part of a pixel
                bool wr = false;
                const uint32_t v = ((uint32_t)p[ch] << (8 * ch)) | (0x5aa55au & ~(0xffu << (8 * ch)));
                const uint32_t nv = panel_fold_pixel(g, panels, r, atlas.data(), g.sp, row, col, v, hb, &wr);
                if (wr && !in_span) ++stray;
                if (wr && in_span) p[ch] = (uint8_t)(nv >> (8 * ch));
            }
        }
    }
    return stray ? ((1 << 30) | stray) : 0;
}

// A whole run the way the two kernels do it: frames [n_streams * n_frames][H][W][3] in place, inside a buffer whose address is `align` mod 16
// (only the alignment is emulated: buf points at frame 0).  The state walk (frame b of stream s at b * n_streams + s, latch[s] in and out)
// fills recs [frames][8]; then every (frame, row, span) takes its pieces, a piece inside the buffer is 16 bytes at once, the buffer's first
// and last piece go byte by byte.  Returns PANEL_FIT_*, or with bit 30 set: 1 a piece was taken twice, 2 a piece outside the buffer.
int emu_panels_run(uint8_t* buf, int n_streams, int n_frames, int H, int W, int align, const uint8_t* bird, int bh, int bw, const PanelParams* params,
                   const uint8_t* const* sprites, const int* sprite_w, const int* sprite_h, int panels, int* latch, const int* offset_type,
                   const int* curvature_type, const int* collision_type, int* recs_out) {
    PanelGeom g;
    int slot = -1;
    const int fit = panel_geometry(H, W, bird ? bh : 0, bird ? bw : 0, *params, sprite_w, sprite_h, &g, &slot);
    if (fit) return fit;
    size_t pixels = 0;
    for (int k = 0; k < PANEL_SPRITES; ++k) pixels += (size_t)g.sp[k].w * g.sp[k].h;
    std::vector<uint32_t> atlas(pixels ? pixels : 1);
    for (int k = 0; k < PANEL_SPRITES; ++k)
        if (g.sp[k].w > 0) memcpy(atlas.data() + g.sp[k].off, sprites[k], (size_t)g.sp[k].w * g.sp[k].h * 4);
    const int frames = n_streams * n_frames;
    std::vector<PanelRecord> recs(frames);
    for (int s = 0; s < n_streams; ++s) {
        int l = latch[s];
        for (int b = 0; b < n_frames; ++b) {
            const int q = b * n_streams + s;
            recs[q] = panel_step(panels, l, offset_type ? offset_type[q] : 0, curvature_type ? curvature_type[q] : 0, collision_type ? collision_type[q] : 0);
            l = recs[q].latch;
        }
        latch[s] = l;
    }
    memcpy(recs_out, recs.data(), (size_t)frames * sizeof(PanelRecord));
    const PanelSpans sp = panel_spans(g, panels);
    const long long total = (long long)frames * H * W * 3;
    std::vector<char> taken((size_t)(total / 16 + 3), 0);
    HostBird hb;
    hb.g = &g;
    hb.base = bird;
    for (int f = 0; f < frames; ++f)
        for (int row = sp.row0; row < sp.row1; ++row) {
            const PanelRowSpans rs = panel_row_spans(sp, W, row);
            long long prev_last = panel_prev_last_piece(sp, g, align, f, row);
            const long long rowstart = ((long long)f * H + row) * W * 3;
            for (int i = 0; i < rs.n; ++i) {
                long long p0, p1;
                panel_span_pieces(g, align, f, row, rs.c0(i), rs.c1(i), &prev_last, &p0, &p1);
                for (long long P = p0; P <= p1; ++P) {
                    const long long o0 = P * 16 - align;
                    if (P < 0 || o0 + 16 <= 0 || o0 >= total) return (1 << 30) | 2;
                    if (taken[(size_t)P]++) return (1 << 30) | 1;
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    for (int j = 0; j < 16; ++j)
                        if (o0 + j >= 0 && o0 + j < total) w[j >> 2] |= (uint32_t)buf[o0 + j] << (8 * (j & 3));
                    PanelPiece io{w[0], w[1], w[2], w[3]};
                    if (!panel_fold_piece_fast(g, panels, recs.data(), recs[f], frames, atlas.data(), g.sp, f, row, (int)(o0 - rowstart), &io, hb)) continue;
                    w[0] = io.w0; w[1] = io.w1; w[2] = io.w2; w[3] = io.w3;
                    for (int j = 0; j < 16; ++j)
                        if (o0 + j >= 0 && o0 + j < total) buf[o0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
                }
            }
        }
    return 0;
}

}  // extern "C"
