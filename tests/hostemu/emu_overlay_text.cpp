// Host build of the overlay text's rules (csrc/overlay_text_core.h; g++, one thread): the formatter, the size and ladder rules, the layout of
// a frame's items and the per-piece fold, composed the way the two device kernels compose them -- candidates counted and placed kind by kind,
// then every band's aligned 16-byte pieces with only the bytes inside the span written -- so that the CPU suite can compare them item for
// item and byte for byte with tests/text_ref.py.  Test scaffolding only; never loaded by the product.
#include <string.h>
#include <vector>
#include "overlay_text_core.h"

using namespace adas;

struct EmuTextArrays {   // adas_overlay_text_arrays, host pointers
    const int32_t *det_xyxy, *det_cls, *det_counts;
    const double* trk_tlwh;
    const int32_t *trk_cls, *trk_ids, *trk_counts;
    const double* trk_last_tlbr;
    const int32_t* traj_len;
    const int32_t* dist_points;
    const double* dist_d;
    const int32_t* dist_counts;
    const int32_t *offset_type, *curvature_type, *collision_type;
    int32_t det_cap, trk_cap, dist_cap, reserved;
};

struct EmuTextTables {
    const TextFont* fonts;   // [TEXT_FONTS], atlas: host pointers
    const char* det_names; int32_t n_det_names;
    const char* trk_names; int32_t n_trk_names;
    const uint32_t* det_colors; int32_t n_det_colors;
    const uint32_t* trk_colors; int32_t n_trk_colors;
    const TextLine* lines; int32_t n_lines;
};

extern "C" {

int emu_text_format_fixed(double x, int prec, char* out) { return text_format_fixed(x, prec, out); }
int emu_text_format_int(int x, char* out) { return text_format_int(x, out); }
int emu_text_ladder(const TextFont* fonts, int first, int count, double v) { return text_ladder(fonts, first, count, v); }
void emu_text_size(const TextFont* font, const char* s, int len, int* wh) { text_size(*font, s, len, wh, wh + 1); }
int emu_text_sizeof(int what) { return what == 0 ? (int)sizeof(TextFont) : what == 1 ? (int)sizeof(TextItem) : what == 2 ? (int)sizeof(TextStyle) : (int)sizeof(TextLine); }

// The layout kernel's walk: items [frames][max_items], heads [frames][4] (count, flags, first row, end row)
void emu_text_layout(const EmuTextArrays* a, const EmuTextTables* tb, const TextStyle* st, int W, int H, int mask, int frames, int max_items, TextItem* items,
                     int* heads) {
    TextSrc s = text_src_of_arrays(a->det_xyxy, a->det_cls, a->det_counts, a->det_cap, a->trk_tlwh, a->trk_cls, a->trk_ids, a->trk_counts, a->trk_cap,
                                   a->trk_last_tlbr, a->traj_len, a->dist_points, a->dist_d, a->dist_counts, a->dist_cap, a->offset_type, a->curvature_type,
                                   a->collision_type);
    s.src_w = W; s.src_h = H;
    TextTables t = {};
    t.fonts = tb->fonts;
    t.det_names = tb->det_names; t.n_det_names = tb->n_det_names; t.trk_names = tb->trk_names; t.n_trk_names = tb->n_trk_names;
    t.det_colors = tb->det_colors; t.n_det_colors = tb->n_det_colors; t.trk_colors = tb->trk_colors; t.n_trk_colors = tb->n_trk_colors;
    t.lines = tb->lines; t.n_lines = tb->n_lines;
    for (long long q = 0; q < frames; ++q) {
        TextItem* out = items + q * max_items;
        int base = 0, flags = 0, r0 = 0x7fffffff, r1 = 0;
        for (int kind = 1; kind <= TEXT_LINES; kind <<= 1) {
            if (!(mask & kind)) continue;
            const int n = text_candidates(s, t, kind, q);
            for (int c = 0; c < n; ++c) {
                const int k = text_candidate(s, t, *st, kind, q, c, nullptr, 0, &flags);
                if (k > 0) {
                    if (base + k > max_items) flags |= TEXT_FLAG_OVERFLOW;
                    if (base < max_items) {
                        const int room = max_items - base;
                        text_candidate(s, t, *st, kind, q, c, out + base, room, &flags);
                        for (int i = 0; i < k && i < room; ++i)
                            if (out[base + i].bx0 < out[base + i].bx1) {
                                r0 = out[base + i].by0 < r0 ? out[base + i].by0 : r0;
                                r1 = out[base + i].by1 > r1 ? out[base + i].by1 : r1;
                            }
                    }
                }
                base += k;
            }
        }
        heads[q * 4] = base < max_items ? base : max_items;
        heads[q * 4 + 1] = flags;
        heads[q * 4 + 2] = r1 > r0 ? r0 : 0;
        heads[q * 4 + 3] = r1 > r0 ? r1 : 0;
    }
}

// The draw kernel's walk over buf = frames [frames][H][W][3] in place, inside a buffer whose address is `align` mod 16 (only the alignment is
// emulated: buf points at frame 0).  rows: the rows of a band.  Returns 0, or 1: a byte outside the buffer would be touched, 2: a byte was
// written twice, 3: a byte outside every item's box was written.
int emu_text_draw(uint8_t* buf, int frames, int H, int W, int align, const TextFont* fonts, const TextItem* all_items, const int* heads, int max_items,
                  int rows) {
    const long long row_bytes = (long long)W * 3, total = (long long)frames * H * row_bytes;
    std::vector<char> written((size_t)total, 0);
    for (int f = 0; f < frames; ++f) {
        const TextItem* items = all_items + (long long)f * max_items;
        const int* hd = heads + (long long)f * 4;
        for (int r0 = 0; r0 < H; r0 += rows) {
            const int r1 = r0 + rows < H ? r0 + rows : H;
            int n = hd[0];
            if (n <= 0 || r1 <= hd[2] || r0 >= hd[3]) continue;
            if (n > max_items) n = max_items;
            std::vector<int> bin;
            int s_c0 = 0x7fffffff, s_c1 = 0;
            for (int i = 0; i < n; ++i) {
                const TextItem& it = items[i];
                if (it.bx0 < it.bx1 && it.by0 < r1 && it.by1 > r0) {
                    bin.push_back(i);
                    s_c0 = it.bx0 < s_c0 ? it.bx0 : s_c0;
                    s_c1 = it.bx1 > s_c1 ? it.bx1 : s_c1;
                }
            }
            if (bin.empty()) continue;
            const int c0 = s_c0 * 3, c1 = s_c1 * 3;
            for (int row = r0; row < r1; ++row) {
                const long long rowstart = ((long long)f * H + row) * row_bytes;
                const long long P0 = (rowstart + align + c0) >> 4, P1 = (rowstart + align + c1 - 1) >> 4;
                for (long long P = P0; P <= P1; ++P) {
                    const long long o0 = P * 16 - align;
                    const int b0 = (int)(o0 - rowstart);
                    const int lo = b0 > c0 ? b0 : c0, hi = b0 + 16 < c1 ? b0 + 16 : c1;
                    bool meets = false;
                    for (int i : bin) meets = meets || (row >= items[i].by0 && row < items[i].by1 && items[i].bx0 * 3 < hi && items[i].bx1 * 3 > lo);
                    if (!meets) continue;
                    if (rowstart + lo < 0 || rowstart + hi > total) return 1;
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    for (int j = 0; j < 16; ++j)
                        if (b0 + j >= lo && b0 + j < hi) w[j >> 2] |= (uint32_t)buf[o0 + j] << (8 * (j & 3));
                    const uint32_t before[4] = {w[0], w[1], w[2], w[3]};
                    bool any = false;
                    for (int i : bin) any |= text_fold_piece(fonts, items[i], row, b0, w);
                    if (!any) continue;
                    for (int j = 0; j < 16; ++j) {
                        const int b = b0 + j;
                        const bool own = b >= lo && b < hi;
                        const bool changed = ((w[j >> 2] ^ before[j >> 2]) >> (8 * (j & 3))) & 0xffu;
                        if (!own) {
                            if (changed) return 3;
                            continue;
                        }
                        bool inside = false;
                        for (int i : bin) inside = inside || (row >= items[i].by0 && row < items[i].by1 && b >= items[i].bx0 * 3 && b < items[i].bx1 * 3);
                        if (changed && !inside) return 3;
                        if (written[(size_t)(o0 + j)]++) return 2;
                        buf[o0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
                    }
                }
            }
        }
    }
    return 0;
}

}  // extern "C"
