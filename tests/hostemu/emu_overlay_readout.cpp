// Host build of csrc/overlay_readout_core.h (g++, no HIP): the readouts' layout and the draw kernel's walk of aligned 16-byte pieces, so
// that the CPU suite can compare the device's rules R0-R6 with tests/readout_ref.py.  Also a one-thread run of lane_core.h's geometry that
// keeps veh_pos (the GPU suite compares the device's array with it, bit for bit).  Test scaffolding.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "adas_hip.h"
#define ADAS_LANE_HOST_TEAM 64   // lane_core.h's fits add their rows in the wave's order: the device's bits, not only its values
#include "post_core.h"  // ahead of the overlay's cores: it defines ADAS_HD / ADAS_DEV without a guard, they take an existing definition
#include "lane_core.h"
#include "overlay_readout_core.h"

using namespace adas;

static_assert(sizeof(ReadoutStyle) == sizeof(adas_overlay_readout_style), "ReadoutStyle");
static_assert(sizeof(ReadoutString) == sizeof(adas_overlay_readout_string), "ReadoutString");

extern "C" {

int emu_readout_sizeof(int k) {
    return k == 0 ? (int)sizeof(ReadoutStyle) : k == 1 ? (int)sizeof(ReadoutRecord) : k == 2 ? (int)sizeof(TextFont) : k == 3 ? (int)sizeof(adas_overlay_readout_record) : 0;
}

void emu_readout_default_style(ReadoutStyle* st) { readout_default_style(st); }

int emu_readout_format1(double x, char* out) { return text_format_fixed(x, 1, out); }

void emu_readout_tips(long long p1x, long long p1y, long long p2x, long long p2y, double tip, long long* q) { overlay_arrow_tips(p1x, p1y, p2x, p2y, tip, q); }

// the layout kernel: frame q from dir[q], veh[q], cur[q], off[q]
void emu_readout_layout(const int* dir, const double* veh, const double* cur, const double* off, int frames, int W, int H, const ReadoutStyle* st,
                        const TextFont* font, ReadoutRecord* recs) {
    for (int q = 0; q < frames; ++q) {
        if (dir[q] == READOUT_DIR_NONE) {
            readout_clear(recs + q);
            continue;
        }
        for (int k = 0; k < 4; ++k) readout_item(k, veh[q], cur[q], off[q], W, H, *st, *font, recs + q);   // a lane each on the device
        readout_finish(recs + q);
    }
}

// a record as adas_overlay_fetch_readout hands it out
void emu_readout_public(const ReadoutRecord* r, adas_overlay_readout_record* rec) {
    memset(rec, 0, sizeof(*rec));
    rec->drawn = r->drawn; rec->flags = r->flags;
    if (r->drawn)
        for (int k = 0; k < 2; ++k) (void)overlay_track_marks(r->prims + 3 * k, 3, k, &rec->arrows[k], 1, 0);
    memcpy(rec->strings, r->str, sizeof(rec->strings));
}

// The draw kernel's walk over buf = frames [frames][H][W][3] in place, inside a buffer whose address is `align` mod 16 (only the alignment is
// emulated: buf points at frame 0).  rows: the rows of a band.  Returns 0, or 1: a byte outside the buffer would be touched, 2: a byte was
// written twice, 3: a byte outside every item's box was written.
int emu_readout_draw(uint8_t* buf, int frames, int H, int W, int align, const ReadoutStyle* st, const TextFont* font, const ReadoutRecord* recs, int rows) {
    const long long row_bytes = (long long)W * 3, total = (long long)frames * H * row_bytes;
    std::vector<char> written((size_t)total, 0);
    int hw[READOUT_HW_INTS];
    readout_halfwidths(hw);
    for (int f = 0; f < frames; ++f) {
        const ReadoutRecord& r = recs[f];
        for (int r0 = 0; r0 < H; r0 += rows) {
            const int r1 = r0 + rows < H ? r0 + rows : H;
            if (!r.drawn || r.x0 > r.x1 || r1 <= r.y0 || r0 > r.y1) continue;
            int c0 = 0, c1 = 0;
            if (!readout_band_span(r, r0, r1, &c0, &c1)) continue;
            for (int row = r0; row < r1; ++row) {
                const long long rowstart = ((long long)f * H + row) * row_bytes;
                const long long P0 = (rowstart + align + c0) >> 4, P1 = (rowstart + align + c1 - 1) >> 4;
                for (long long P = P0; P <= P1; ++P) {
                    const long long o0 = P * 16 - align;
                    const int b0 = (int)(o0 - rowstart);
                    const int lo = b0 > c0 ? b0 : c0, hi = b0 + 16 < c1 ? b0 + 16 : c1;
                    if (!readout_meets(r, row, lo, hi)) continue;
                    if (rowstart + lo < 0 || rowstart + hi > total || lo < 0 || hi > row_bytes) return 1;
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    for (int j = 0; j < 16; ++j)
                        if (b0 + j >= lo && b0 + j < hi) w[j >> 2] |= (uint32_t)buf[o0 + j] << (8 * (j & 3));
                    const uint32_t before[4] = {w[0], w[1], w[2], w[3]};
                    if (!readout_fold_piece(r, *st, *font, hw, row, b0, lo, hi, w)) continue;
                    for (int j = 0; j < 16; ++j) {
                        const int b = b0 + j;
                        const bool own = b >= lo && b < hi;
                        const bool changed = ((w[j >> 2] ^ before[j >> 2]) >> (8 * (j & 3))) & 0xffu;
                        if (!own) {
                            if (changed) return 3;
                            continue;
                        }
                        if (changed && !readout_meets(r, row, b, b + 1)) return 3;
                        if (written[(size_t)(o0 + j)]++) return 2;
                        buf[o0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
                    }
                }
            }
        }
    }
    return 0;
}

// lane_core.h's geometry of one frame, one thread, keeping veh_pos
int emu_readout_lane_geometry(const int* lane_cnt, const int* lane_det, const int* lane_pts, int img_h, int bird_w, int bird_h, int adjust, const double* M,
                              int* hdr, double* vals, double* veh) {
    LaneGeomCfg cfg;
    cfg.img_h = img_h; cfg.bird_w = bird_w; cfg.bird_h = bird_h; cfg.adjust = adjust;
    for (int i = 0; i < 9; ++i) cfg.M[i] = M[i];
    std::vector<double> fx(2 * (size_t)img_h);
    std::vector<int> idx(2 * (size_t)img_h), area(4 * (size_t)img_h), bird(4 * ADAS_LANE_MAXPTS * 2);
    LaneGeomFrame f{lane_cnt, lane_det, lane_pts, hdr, vals, area.data(), bird.data(), fx.data(), idx.data(), veh};
    std::vector<double> lds(lane_lds_bytes(img_h, bird_h) / 8 + 2);
    Ctx c{0, 1};
    lane_geometry_frame(c, cfg, f, lds.data());
    return 0;
}

}  // extern "C"
