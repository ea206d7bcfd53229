// overlay_readout.hip -- the bird view's readouts on the device: the two arrows and the 'Offset: %.1f m' / 'R : %.1f m' strings that
// PerspectiveTransformation.calcCurveAndOffset draws on the bird-view image, from the geometry kernel's direction, curvature, offset and
// veh_pos where they lie in HBM.  The rules are overlay_readout_core.h (R0-R6); this file is the two kernels around them and the C ABI
// (adas_overlay_*readout*).  A run is
//   overlay_readout_layout_kernel  one wave per frame: the gate, then a lane each for arrow A, arrow B and the two strings ('%.1f' of the
//                                  device-resident doubles, the run's box at the style's zoom), then the record's flags and union box.
//   overlay_readout_draw_kernel    in place on the bird images.  A workgroup owns RO_ROWS rows of one frame and leaves after reading the
//                                  record's head when they miss its union box, or when no item's box meets them (the rows between the
//                                  strings and the arrows); otherwise its lanes take the aligned 16-byte pieces of the columns that the
//                                  items meeting its rows span, row by row: a piece no item's box meets is dropped without touching memory, else one
//                                  16-byte load, R5 over the eight items in order (readout_fold_piece), one 16-byte store.  A piece that
//                                  reaches outside the box's span of its row goes byte by byte, and only the bytes inside: no byte has two
//                                  writers and nothing outside the buffer is read or written at any alignment or row length.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "overlay_readout_core.h"

using namespace adas;

static_assert(sizeof(ReadoutStyle) == sizeof(adas_overlay_readout_style) && offsetof(ReadoutStyle, text_color) == offsetof(adas_overlay_readout_style, text_color) &&
                  offsetof(ReadoutStyle, arrow_b_color) == offsetof(adas_overlay_readout_style, arrow_b_color),
              "ReadoutStyle is adas_overlay_readout_style");
static_assert(sizeof(ReadoutString) == sizeof(adas_overlay_readout_string) && offsetof(ReadoutString, text) == offsetof(adas_overlay_readout_string, text) &&
                  offsetof(ReadoutString, bx0) == offsetof(adas_overlay_readout_string, box),
              "ReadoutString is adas_overlay_readout_string");
static_assert(READOUT_FLAG_RANGE == ADAS_OVERLAY_READOUT_RANGE && TEXT_FONTS == ADAS_TEXT_FONTS, "overlay_readout_core.h restates ADAS_OVERLAY_READOUT_*");
static_assert(sizeof(ReadoutRecord) % 4 == 0 && sizeof(TextFont) % 4 == 0, "copied to LDS word by word");

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_ROWS = 8;   // rows of a draw workgroup

struct RoLayout {
    overlay_readout_sources s;
    const TextFont* fonts;   // [TEXT_FONTS]
    ReadoutStyle st;
    int W, H;                // the bird image
    ReadoutRecord* recs;     // [frames]
};

__global__ __launch_bounds__(64) void overlay_readout_layout_kernel(const RoLayout a) {
    const long long q = blockIdx.x;
    const int lane = threadIdx.x;
    ReadoutRecord* rec = a.recs + q;
    if (a.s.dir[q * a.s.dir_stride] == READOUT_DIR_NONE) {   // R0, the whole wave
        if (lane == 0) readout_clear(rec);
        return;
    }
    if (lane < 4)
        readout_item(lane, a.s.veh[q], a.s.cur[q * a.s.val_stride], a.s.off[q * a.s.val_stride], a.W, a.H, a.st, a.fonts[a.st.slot], rec);
    __syncthreads();
    if (lane == 0) readout_finish(rec);
}

struct RoDraw {
    const ReadoutRecord* recs;
    const TextFont* fonts;
    ReadoutStyle st;
    uint8_t* dst;   // [frames][H][W][3], any alignment
    int W, H;
    int align;      // the buffer's address & 15
    int hw[READOUT_HW_INTS];
};

__global__ __launch_bounds__(RO_THREADS) void overlay_readout_draw_kernel(const RoDraw a) {
    __shared__ ReadoutRecord s_rec;
    __shared__ TextFont s_font;
    __shared__ int s_hw[READOUT_HW_INTS];
    const int f = blockIdx.y, t = threadIdx.x;
    const int r0 = blockIdx.x * RO_ROWS, r1 = r0 + RO_ROWS < a.H ? r0 + RO_ROWS : a.H;
    const ReadoutRecord* g = a.recs + f;
    if (!g->drawn || g->x0 > g->x1 || r1 <= g->y0 || r0 > g->y1) return;   // the whole workgroup
    {
        const uint32_t* src = (const uint32_t*)g;
        uint32_t* dst = (uint32_t*)&s_rec;
        for (int i = t; i < (int)(sizeof(ReadoutRecord) / 4); i += RO_THREADS) dst[i] = src[i];
        const uint32_t* fs = (const uint32_t*)(a.fonts + a.st.slot);
        uint32_t* fd = (uint32_t*)&s_font;
        for (int i = t; i < (int)(sizeof(TextFont) / 4); i += RO_THREADS) fd[i] = fs[i];
        if (t < READOUT_HW_INTS) s_hw[t] = a.hw[t];
    }
    __syncthreads();
    int c0 = 0, c1 = 0;   // the bytes of a row that the items meeting this band span
    if (!readout_band_span(s_rec, r0, r1, &c0, &c1)) return;   // the same in every lane
    const int maxnp = (c1 - c0 + 15) / 16 + 1;
    const long long row_bytes = (long long)a.W * 3;
    for (int idx = t; idx < (r1 - r0) * maxnp; idx += RO_THREADS) {
        const int row = r0 + idx / maxnp;
        const long long rowstart = ((long long)f * a.H + row) * row_bytes;   // in the buffer
        const long long P0 = (rowstart + a.align + c0) >> 4, P1 = (rowstart + a.align + c1 - 1) >> 4;
        const long long P = P0 + idx % maxnp;
        if (P > P1) continue;
        const long long o0 = P * 16 - a.align;     // the piece's first byte in the buffer
        const int b0 = (int)(o0 - rowstart);       // and in the row
        const int lo = b0 > c0 ? b0 : c0, hi = b0 + 16 < c1 ? b0 + 16 : c1;   // the bytes of the piece this lane owns
        if (!readout_meets(s_rec, row, lo, hi)) continue;
        const bool full = lo == b0 && hi == b0 + 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (full) {
            const uint4 v = *(const uint4*)(a.dst + o0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (b0 + j >= lo && b0 + j < hi) w[j >> 2] |= (uint32_t)a.dst[o0 + j] << (8 * (j & 3));
        }
        if (!readout_fold_piece(s_rec, a.st, s_font, s_hw, row, b0, lo, hi, w)) continue;
        if (full) {
            *(uint4*)(a.dst + o0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (b0 + j >= lo && b0 + j < hi) a.dst[o0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

}  // namespace

struct adas::overlay_readout {
    ReadoutStyle style;
    ReadoutRecord* recs = nullptr;   // [max_batch]
    int max_batch = 0, bird_w = 0, bird_h = 0;
    int hw[READOUT_HW_INTS];
    int run_frames = 0;
};

void adas::overlay_readout_free(adas::overlay_readout* s) {
    if (!s) return;
    if (s->recs) (void)hipFree(s->recs);
    delete s;
}

// the handle's readout state, made by the first adas_overlay_set_readout_style or the first run with the stage
static int readout_state(adas_overlay* h, adas::overlay_readout** out) {
    adas::overlay_readout** held = adas::overlay_readout_slot(h);
    if (*held) { *out = *held; return ADAS_OK; }
    adas::overlay_readout* s = new (std::nothrow) adas::overlay_readout();
    ADAS_REQUIRE(s, ADAS_ERR_INVALID, "out of host memory");
    readout_default_style(&s->style);
    readout_halfwidths(s->hw);
    int sh = 0, sw = 0;
    (void)adas::overlay_geometry(h, &sh, &sw, &s->bird_h, &s->bird_w, &s->max_batch);
    hipError_t e = hipMalloc((void**)&s->recs, (size_t)s->max_batch * sizeof(ReadoutRecord));
    if (e == hipSuccess) e = hipMemset(s->recs, 0, (size_t)s->max_batch * sizeof(ReadoutRecord));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        adas::overlay_readout_free(s);
        return hip_fail(e, "hipMalloc(overlay readout records)", __FILE__, __LINE__);
    }
    *held = s;
    *out = s;
    return ADAS_OK;
}

int adas::overlay_readout_reserve(adas_overlay* h) {
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "overlay_readout_reserve: null handle");
    adas::overlay_readout* s = nullptr;
    return readout_state(h, &s);
}

int adas::overlay_readout_check(const char* who, adas_overlay* h) {
    adas::overlay_readout* s = nullptr;
    int rc = readout_state(h, &s);
    if (rc) return rc;
    const void *d_fonts = nullptr, *h_fonts = nullptr;
    adas::overlay_text_font_tables(h, &d_fonts, &h_fonts);
    ADAS_REQUIRE(d_fonts && h_fonts && ((const TextFont*)h_fonts)[s->style.slot].set, ADAS_ERR_INVALID,
                 "%s: the readouts stage needs font slot %d, which is empty (adas_overlay_set_font; the slot is the readout style's)", who, s->style.slot);
    return ADAS_OK;
}

int adas::overlay_readout_launch(adas_overlay* h, const adas::overlay_readout_sources& src, uint8_t* d_bird, int frames, void* stream) {
    adas::overlay_readout* s = *adas::overlay_readout_slot(h);
    const void *d_fonts = nullptr, *h_fonts = nullptr;
    adas::overlay_text_font_tables(h, &d_fonts, &h_fonts);
    ADAS_REQUIRE(s && d_fonts && d_bird && frames > 0 && frames <= s->max_batch, ADAS_ERR_INVALID, "the readouts stage was not checked before its launch");
    hipStream_t strm = (hipStream_t)stream;
    RoLayout a = {};
    a.s = src;
    a.fonts = (const TextFont*)d_fonts;
    a.st = s->style;
    a.W = s->bird_w; a.H = s->bird_h;
    a.recs = s->recs;
    hipLaunchKernelGGL(overlay_readout_layout_kernel, dim3((unsigned)frames), dim3(64), 0, strm, a);
    ADAS_HIP_TRY(hipGetLastError());
    RoDraw d = {};
    d.recs = s->recs; d.fonts = a.fonts; d.st = s->style; d.dst = d_bird;
    d.W = s->bird_w; d.H = s->bird_h;
    d.align = (int)((uintptr_t)d_bird & 15);
    memcpy(d.hw, s->hw, sizeof(d.hw));
    hipLaunchKernelGGL(overlay_readout_draw_kernel, dim3((unsigned)((s->bird_h + RO_ROWS - 1) / RO_ROWS), (unsigned)frames), dim3(RO_THREADS), 0, strm, d);
    ADAS_HIP_TRY(hipGetLastError());
    s->run_frames = frames;
    return ADAS_OK;
}

extern "C" {

int adas_overlay_default_readout_style(adas_overlay_readout_style* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_overlay_default_readout_style: null argument");
    readout_default_style((ReadoutStyle*)p);
    return ADAS_OK;
}

int adas_overlay_set_readout_style(adas_overlay* h, const adas_overlay_readout_style* p) {
    const char* who = "adas_overlay_set_readout_style";
    ADAS_REQUIRE(h && p, ADAS_ERR_INVALID, "%s: bad argument", who);
    ReadoutStyle st;
    memcpy(&st, p, sizeof(st));
    ADAS_REQUIRE(st.zoom >= 1 && st.zoom <= READOUT_MAX_ZOOM, ADAS_ERR_INVALID, "%s: zoom %d (1 .. %d)", who, st.zoom, READOUT_MAX_ZOOM);
    ADAS_REQUIRE(st.slot >= 0 && st.slot < TEXT_FONTS, ADAS_ERR_INVALID, "%s: font slot %d (0 .. %d)", who, st.slot, TEXT_FONTS - 1);
    ADAS_REQUIRE(text_in_range_i(st.offset_x) && text_in_range_i(st.offset_y) && text_in_range_i(st.radius_x) && text_in_range_i(st.radius_y), ADAS_ERR_INVALID,
                 "%s: origins (%d, %d), (%d, %d)", who, st.offset_x, st.offset_y, st.radius_x, st.radius_y);
    adas::overlay_readout* s = nullptr;
    int rc = readout_state(h, &s);
    if (rc) return rc;
    s->style = st;
    adas::bump_config_generation();   // a captured step holds the style in its kernel arguments
    return ADAS_OK;
}

int adas_overlay_fetch_readout(adas_overlay* h, int frame, adas_overlay_readout_record* rec) {
    const char* who = "adas_overlay_fetch_readout";
    adas::overlay_readout* s = h ? *adas::overlay_readout_slot(h) : nullptr;
    ADAS_REQUIRE(s && rec, ADAS_ERR_INVALID, "%s: no readouts run on this handle, or a null argument", who);
    ADAS_REQUIRE(frame >= 0 && frame < s->run_frames, ADAS_ERR_INVALID, "%s: frame %d was not part of the last run with the readouts stage (%d frames)", who,
                 frame, s->run_frames);
    ADAS_HIP_TRY(hipDeviceSynchronize());
    ReadoutRecord r;
    ADAS_HIP_TRY(hipMemcpy(&r, s->recs + frame, sizeof(r), hipMemcpyDeviceToHost));
    memset(rec, 0, sizeof(*rec));
    rec->drawn = r.drawn; rec->flags = r.flags;
    if (r.drawn)
        for (int k = 0; k < 2; ++k) (void)overlay_track_marks(r.prims + 3 * k, 3, k, &rec->arrows[k], 1, 0);
    memcpy(rec->strings, r.str, sizeof(rec->strings));
    return ADAS_OK;
}

}  // extern "C"
