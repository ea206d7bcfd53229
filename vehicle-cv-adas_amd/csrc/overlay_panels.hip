// overlay_panels.hip -- the demo's three UI panels on the device (ControlPanel.DisplayBirdViewPanel / DisplaySignsPanel /
// DisplayCollisionPanel, demo.py:101-214) without their text.  The pixel and state rules are overlay_panel_core.h (P1-P6); this file is the
// two kernels around them and the C ABI (adas_overlay_*panel*).  A run is
//   overlay_panels_state_kernel  one lane per stream walks that stream's frames of the step in order (frame b of stream s is row
//                                b * n_streams + s), writes a record per frame -- the sprites chosen, the latch after the frame, the types
//                                read -- and stores the stream's latch in the handle's device memory: a replayed graph carries the state.
//   overlay_panels_draw_kernel   one pass over the rows and column spans of the panels (panel_spans): a workgroup owns a few rows of one frame
//                                (as many as give its lanes about one piece each), a lane one aligned 16-byte piece of the frame buffer at a
//                                time -- one 16-byte load, P6 on the up to six pixels that meet the piece (panel_fold_piece_fast: what the
//                                piece cannot meet is dropped first), one 16-byte store; bytes outside every panel go through unchanged.  Frames
//                                and rows start on every alignment: pieces are counted in the buffer's aligned address space, a piece that two
//                                spans meet (the end of a row and the start of the next, two spans less than 16 bytes apart) belongs to the
//                                first of them, and a piece that reaches outside the buffer goes byte by byte.  Every byte is written at most
//                                once with the whole fold, so workgroups need no order and overlapping panels no second pass.  The bird panel's
//                                column taps and the row taps of the workgroup's rows are tabulated once per workgroup in LDS; sprites are
//                                4-byte reads from one BGRA atlas that stays in the cache across frames.
// The yardstick is a device-to-device copy of the same frames (tools/bench_panels.py); as measured the pass is bound by its instructions, not
// by its bytes.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "overlay_panel_core.h"

using namespace adas;

static_assert(PANEL_BIRD == ADAS_PANEL_BIRD && PANEL_SIGNS == ADAS_PANEL_SIGNS && PANEL_COLLISION == ADAS_PANEL_COLLISION &&
                  PANEL_SPRITES == ADAS_PANEL_SPRITES && PANEL_SPRITE_LTA_RIGHT == ADAS_PANEL_SPRITE_LTA_RIGHT &&
                  PANEL_SPRITE_WARN == ADAS_PANEL_SPRITE_WARN && PANEL_LATCH_STRAIGHT == ADAS_PANEL_LATCH_STRAIGHT,
              "overlay_panel_core.h restates ADAS_PANEL_*");
static_assert(sizeof(PanelRecord) == sizeof(adas_overlay_panel_record) && offsetof(PanelRecord, latch) == offsetof(adas_overlay_panel_record, latch) &&
                  offsetof(PanelRecord, collision_type) == offsetof(adas_overlay_panel_record, collision_type),
              "PanelRecord is adas_overlay_panel_record");
static_assert(PN_OFF_CENTER == ADAS_OFFSET_CENTER && PN_OFF_RIGHT == ADAS_OFFSET_RIGHT && PN_CUR_HARD_RIGHT == ADAS_CURVATURE_HARD_RIGHT &&
                  PN_CUR_HARD_LEFT == ADAS_CURVATURE_HARD_LEFT && PN_CUR_STRAIGHT == ADAS_CURVATURE_STRAIGHT && PN_COLL_WARNING == ADAS_COLLISION_WARNING &&
                  PN_COLL_NORMAL == ADAS_COLLISION_NORMAL,
              "overlay_panel_core.h restates the message enums");

namespace {

constexpr int PN_THREADS = 256;
constexpr int PN_ROWS = 8;   // most rows of a draw workgroup (narrow spans: few pieces per row)

struct PnState {
    const int *offset, *curvature, *collision;   // frame q at [q * stride]; null: UNKNOWN
    int offset_stride, curvature_stride, collision_stride;
    int n_streams, n_frames, panels;
    int* latch;           // [n_streams]
    PanelRecord* recs;    // [n_streams * n_frames]
};

__global__ __launch_bounds__(64) void overlay_panels_state_kernel(const PnState a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n_streams) return;
    int latch = a.latch[s];
    if (latch < PANEL_LATCH_NONE || latch > PANEL_LATCH_STRAIGHT) latch = PANEL_LATCH_NONE;
    for (int b = 0; b < a.n_frames; ++b) {   // a stream's frames in temporal order
        const size_t q = (size_t)b * a.n_streams + s;
        const int off = a.offset ? a.offset[q * a.offset_stride] : 0;
        const int cur = a.curvature ? a.curvature[q * a.curvature_stride] : 0;
        const int col = a.collision ? a.collision[q * a.collision_stride] : 0;
        const PanelRecord r = panel_step(a.panels, latch, off, cur, col);
        latch = r.latch;
        a.recs[q] = r;
    }
    a.latch[s] = latch;
}

struct PnDraw {
    PanelGeom g;
    PanelSpans sp;
    int panels, frames;
    int align;                  // the buffer's address & 15
    int rows;                   // rows of a workgroup, 1 .. PN_ROWS
    uint8_t* dst;               // [frames][src_h][src_w][3], any alignment
    const uint8_t* bird;        // [frames][bird_h][bird_w][3]
    const uint32_t* atlas;
    const PanelSprite* sprites;  // g.sp in device memory: indexed per lane
    const PanelRecord* recs;
};

struct PnSeg {   // one span of one of the workgroup's rows: its pieces [p0, p0 + n)
    long long p0;
    int n, row;
};

struct PnBird {   // P5 from the workgroup's LDS tables: the column taps, and the row taps of its rows and of the row above and below them
    const uint8_t* base;   // [frames][bird_h][bird_w][3]
    const uint8_t* img;
    __device__ __forceinline__ void frame(int ff) { img = base + (size_t)ff * g->bird_h * g->bird_w * 3; }
    const PanelTap* tab;
    const PanelTap* row_tab;   // interior row ry at [ry - ry_base], PN_ROWS + 2 entries
    const PanelGeom* g;
    int ry_base;
    __device__ __forceinline__ uint32_t operator()(int ry, int rx) const {
        if (g->identity) {
            const uint8_t* p = img + ((size_t)ry * g->bird_w + rx) * 3;
            return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
        const unsigned k = (unsigned)(ry - ry_base);   // a piece meets its own row and at most the next or the one before
        const PanelTap r = k < (unsigned)(PN_ROWS + 2) ? row_tab[k] : panel_row_tap(ry, g->scale_y, g->bird_h);
        return panel_resize_taps(img + (size_t)r.s0 * g->bird_w * 3, img + (size_t)r.s1 * g->bird_w * 3, r.c0, r.c1, tab[rx]);
    }
};

// A workgroup owns a.rows consecutive rows of one frame (the host sizes a.rows so that their pieces are about one per lane): their spans'
// piece ranges are tabulated once, and the lanes take the pieces of all of them in one sweep -- a lane's chain of dependent memory accesses
// is one piece long, which is what the pass's time depends on.
__global__ __launch_bounds__(PN_THREADS) void overlay_panels_draw_kernel(const PnDraw a) {
    extern __shared__ PanelTap pn_tab[];
    __shared__ PnSeg seg[2 * PN_ROWS];
    __shared__ PanelTap row_tab[PN_ROWS + 2];
    const PanelGeom& g = a.g;
    const int bands = (a.sp.row1 - a.sp.row0 + a.rows - 1) / a.rows;
    const int f = blockIdx.x / bands;
    const int r_begin = a.sp.row0 + (blockIdx.x % bands) * a.rows;
    const int r_end = r_begin + a.rows < a.sp.row1 ? r_begin + a.rows : a.sp.row1;
    const bool resize = (a.panels & PANEL_BIRD) && !g.identity;
    const int t = threadIdx.x;
    // the bird panel's interior rows that the workgroup's rows, or a piece reaching one row further, can meet
    if (resize && r_end + 1 > g.border && r_begin - 1 < g.border + g.H) {
        for (int x = t; x < g.W; x += PN_THREADS) pn_tab[x] = panel_col_tap(x, g.scale_x, g.bird_w);
        if (t < PN_ROWS + 2) {
            const int ry = r_begin - 1 - g.border + t;
            row_tab[t] = panel_row_tap(ry < 0 ? 0 : (ry >= g.H ? g.H - 1 : ry), g.scale_y, g.bird_h);
        }
    }
    if (t >= 64 && t < 64 + PN_ROWS) {   // a lane of the second wave per row: its spans' pieces, less the ones the span before owns
        const int k = t - 64, row = r_begin + k;
        PnSeg s0 = {0, 0, row}, s1 = {0, 0, row};
        if (row < r_end) {
            const PanelRowSpans rs = panel_row_spans(a.sp, g.src_w, row);
            long long prev_last = panel_prev_last_piece(a.sp, g, a.align, f, row), p0, p1;
            if (rs.n > 0) {
                panel_span_pieces(g, a.align, f, row, rs.a0, rs.a1, &prev_last, &p0, &p1);
                s0.p0 = p0; s0.n = p1 >= p0 ? (int)(p1 - p0 + 1) : 0;
            }
            if (rs.n > 1) {
                panel_span_pieces(g, a.align, f, row, rs.b0, rs.b1, &prev_last, &p0, &p1);
                s1.p0 = p0; s1.n = p1 >= p0 ? (int)(p1 - p0 + 1) : 0;
            }
        }
        seg[2 * k] = s0;
        seg[2 * k + 1] = s1;
    }
    __syncthreads();
    const long long row_bytes = (long long)g.src_w * 3;
    const long long total = (long long)a.frames * g.src_h * row_bytes;
    const PanelRecord rec = a.recs[f];
    PnBird bird;
    bird.base = a.bird;
    bird.img = a.bird;
    bird.tab = pn_tab;
    bird.row_tab = row_tab;
    bird.g = &g;
    bird.ry_base = r_begin - 1 - g.border;
    int first = 0;   // pieces of the segments before segment j
    int j = 0;
    for (int i = t;; i += PN_THREADS) {
        while (j < 2 * PN_ROWS && i >= first + seg[j].n) first += seg[j++].n;   // at most 2 PN_ROWS steps over the whole sweep
        if (j >= 2 * PN_ROWS) break;
        const int row = seg[j].row;
        const long long P = seg[j].p0 + (i - first);
        const long long rowstart = ((long long)f * g.src_h + row) * row_bytes;
        const long long o0 = P * 16 - a.align;          // the piece's first byte in the buffer
        const bool full = o0 >= 0 && o0 + 16 <= total;  // else: the buffer's first or last piece, byte by byte
        PanelPiece io;
        if (full) {
            const uint4 q = *(const uint4*)(a.dst + o0);
            io.w0 = q.x; io.w1 = q.y; io.w2 = q.z; io.w3 = q.w;
        } else {
            unsigned long long lo = 0, hi = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (o0 + b >= 0 && o0 + b < total) lo |= (unsigned long long)a.dst[o0 + b] << (8 * b);
                if (o0 + 8 + b >= 0 && o0 + 8 + b < total) hi |= (unsigned long long)a.dst[o0 + 8 + b] << (8 * b);
            }
            io.w0 = (uint32_t)lo; io.w1 = (uint32_t)(lo >> 32); io.w2 = (uint32_t)hi; io.w3 = (uint32_t)(hi >> 32);
        }
        if (!panel_fold_piece_fast(g, a.panels, a.recs, rec, a.frames, a.atlas, a.sprites, f, row, (int)(o0 - rowstart), &io, bird)) continue;
        if (full) {
            *(uint4*)(a.dst + o0) = make_uint4(io.w0, io.w1, io.w2, io.w3);
        } else {
            const unsigned long long lo = ((unsigned long long)io.w1 << 32) | io.w0, hi = ((unsigned long long)io.w3 << 32) | io.w2;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (o0 + b >= 0 && o0 + b < total) a.dst[o0 + b] = (uint8_t)(lo >> (8 * b));
                if (o0 + 8 + b >= 0 && o0 + 8 + b < total) a.dst[o0 + 8 + b] = (uint8_t)(hi >> (8 * b));
            }
        }
    }
}

}  // namespace

struct adas::overlay_panels {
    PanelGeom g;
    uint32_t* atlas = nullptr;
    PanelSprite* sprites = nullptr;   // g.sp on the device
    int* latch = nullptr;        // [max_batch]
    PanelRecord* recs = nullptr; // [max_batch]
    int max_batch = 0;
    int run_frames = 0;          // frames of the last run
};

void adas::overlay_panels_free(adas::overlay_panels* s) {
    if (!s) return;
    for (void* q : {(void*)s->atlas, (void*)s->sprites, (void*)s->latch, (void*)s->recs})
        if (q) (void)hipFree(q);
    delete s;
}

bool adas::overlay_panels_ready(adas_overlay* h) { return h && *adas::overlay_panel_slot(h); }

// one run, from wherever the three types live (frame q at [q * stride] of each)
static int panels_launch(const char* who, adas_overlay* h, uint8_t* d_frames_bgr, const int* off, int off_stride, const int* cur, int cur_stride,
                         const int* col, int col_stride, const uint8_t* d_bird_bgr, int panels, int n_streams, int n_frames, void* stream) {
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "%s: null handle", who);
    ADAS_REQUIRE(!(panels & ~(ADAS_PANEL_BIRD | ADAS_PANEL_SIGNS | ADAS_PANEL_COLLISION)) && panels >= 0, ADAS_ERR_INVALID, "%s: unknown panel bits 0x%x", who,
                 panels);
    adas::overlay_panels* s = *adas::overlay_panel_slot(h);
    ADAS_REQUIRE(s, ADAS_ERR_INVALID, "%s: no panels set (call adas_overlay_set_panels first)", who);
    ADAS_REQUIRE(n_streams > 0 && n_frames > 0, ADAS_ERR_INVALID, "%s: bad argument (%d streams x %d frames)", who, n_streams, n_frames);
    const long long frames = (long long)n_streams * n_frames;
    ADAS_REQUIRE(frames <= s->max_batch, ADAS_ERR_INVALID, "%s: %d streams x %d frames, the handle holds %d frames", who, n_streams, n_frames, s->max_batch);
    ADAS_REQUIRE(!(panels & ADAS_PANEL_SIGNS) || (off && cur), ADAS_ERR_INVALID, "%s: the signs panel needs the offset and curvature types", who);
    ADAS_REQUIRE(!(panels & ADAS_PANEL_COLLISION) || col, ADAS_ERR_INVALID, "%s: the collision panel needs the collision types", who);
    ADAS_REQUIRE(!(panels & ADAS_PANEL_BIRD) || (s->g.bird_h > 0 && d_bird_bgr), ADAS_ERR_INVALID,
                 "%s: the bird panel needs a handle created with a bird-view size and a bird-view image", who);
    if (!d_frames_bgr) {
        int written = 0;
        int rc = adas::overlay_own_frames(h, &d_frames_bgr, &written);
        if (rc) return rc;
        ADAS_REQUIRE(frames <= written, ADAS_ERR_INVALID, "%s: %d frames, but the handle's own buffer holds %d drawn frames (run the overlay into it first)", who,
                     (int)frames, written);
    }
    hipStream_t st = (hipStream_t)stream;
    adas::overlay_note_stream(h, stream);
    s->run_frames = (int)frames;
    if (!panels) return ADAS_OK;
    PnState a = {};
    a.offset = off; a.curvature = cur; a.collision = col;
    a.offset_stride = off_stride; a.curvature_stride = cur_stride; a.collision_stride = col_stride;
    a.n_streams = n_streams; a.n_frames = n_frames; a.panels = panels;
    a.latch = s->latch; a.recs = s->recs;
    hipLaunchKernelGGL(overlay_panels_state_kernel, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    PnDraw d = {};
    d.g = s->g;
    d.sp = panel_spans(s->g, panels);
    d.panels = panels; d.frames = (int)frames;
    d.align = (int)((uintptr_t)d_frames_bgr & 15);
    d.dst = d_frames_bgr; d.bird = d_bird_bgr; d.atlas = s->atlas; d.sprites = s->sprites; d.recs = s->recs;
    const int rows = d.sp.row1 - d.sp.row0;
    if (rows > 0) {
        // about one piece per lane: the widest row of the run holds the left and the right span
        const int row_pieces = ((d.sp.lw + (s->g.src_w - d.sp.rx0)) * 3 + 15) / 16 + 2;
        d.rows = PN_THREADS / row_pieces < 1 ? 1 : (PN_THREADS / row_pieces > PN_ROWS ? PN_ROWS : PN_THREADS / row_pieces);
        const unsigned bands = (unsigned)((rows + d.rows - 1) / d.rows);
        const size_t lds = ((panels & ADAS_PANEL_BIRD) && !s->g.identity) ? (size_t)s->g.W * sizeof(PanelTap) : 0;
        hipLaunchKernelGGL(overlay_panels_draw_kernel, dim3(bands * (unsigned)frames), dim3(PN_THREADS), lds, st, d);
        ADAS_HIP_TRY(hipGetLastError());
    }
    return ADAS_OK;
}

int adas::overlay_run_panels(const char* who, adas_overlay* h, uint8_t* d_frames_bgr, const adas_analysis* analysis, const uint8_t* d_bird_bgr, int panels,
                             int n_streams, int n_frames, void* stream) {
    ADAS_REQUIRE(!(panels & (ADAS_PANEL_SIGNS | ADAS_PANEL_COLLISION)) || panels < 0 || (panels & ~7) || analysis, ADAS_ERR_INVALID,
                 "%s: the signs and collision panels need an analysis handle", who);
    const int *off = nullptr, *cur = nullptr, *col = nullptr;
    int stride = 0;
    if (analysis) {
        const int *fr, *pts;
        int maxp = 0, af = 0;
        ADAS_REQUIRE(adas::analysis_capacity(analysis, nullptr, &af) && (long long)n_streams * n_frames <= af, ADAS_ERR_INVALID,
                     "%s: %d streams x %d frames, the analysis handle holds %d frames", who, n_streams, n_frames, af);
        adas::analysis_frame_views(analysis, &fr, &stride, &pts, &maxp);
        off = fr + offsetof(adas_analysis_frame, offset_msg) / 4;
        cur = fr + offsetof(adas_analysis_frame, curvature_msg) / 4;
        col = fr + offsetof(adas_analysis_frame, collision_msg) / 4;
    }
    return panels_launch(who, h, d_frames_bgr, off, stride, cur, stride, col, stride, d_bird_bgr, panels, n_streams, n_frames, stream);
}

extern "C" {

int adas_overlay_default_panel_params(adas_overlay_panel_params* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_overlay_default_panel_params: null argument");
    memset(p, 0, sizeof(*p));
    p->show_ratio = 0.25;
    p->border = 10;
    p->signs_w = 400; p->signs_h = 365;
    p->signs_sprite_row = 10;
    p->collision_sprite_row = 50; p->collision_sprite_col = 5;
    p->border_color[0] = 0; p->border_color[1] = 0; p->border_color[2] = 255;
    return ADAS_OK;
}

int adas_overlay_set_panels(adas_overlay* h, const adas_overlay_panel_params* p, const adas_overlay_sprite sprites[ADAS_PANEL_SPRITES]) {
    const char* who = "adas_overlay_set_panels";
    ADAS_REQUIRE(h && p && sprites, ADAS_ERR_INVALID, "%s: bad argument", who);
    int src_h = 0, src_w = 0, bird_h = 0, bird_w = 0, max_batch = 0;
    (void)adas::overlay_geometry(h, &src_h, &src_w, &bird_h, &bird_w, &max_batch);
    static_assert(sizeof(PanelParams) == sizeof(adas_overlay_panel_params) && offsetof(PanelParams, border_color) == offsetof(adas_overlay_panel_params, border_color),
                  "PanelParams is adas_overlay_panel_params");
    PanelParams pp;
    memcpy(&pp, p, sizeof(pp));
    int sw[ADAS_PANEL_SPRITES], sh[ADAS_PANEL_SPRITES];
    for (int k = 0; k < ADAS_PANEL_SPRITES; ++k) {
        sw[k] = sprites[k].bgra ? sprites[k].w : 0;
        sh[k] = sprites[k].bgra ? sprites[k].h : 0;
        ADAS_REQUIRE(!sprites[k].bgra || (sw[k] > 0 && sh[k] > 0), ADAS_ERR_INVALID, "%s: sprite %d is %dx%d", who, k, sprites[k].w, sprites[k].h);
    }
    PanelGeom g;
    int slot = -1;
    const int fit = panel_geometry(src_h, src_w, bird_h, bird_w, pp, sw, sh, &g, &slot);
    ADAS_REQUIRE(fit != PANEL_FIT_PARAMS, ADAS_ERR_INVALID,
                 "%s: bad parameters (ratio %g, border %d, signs widget %dx%d, offsets %d, %d, %d) or a frame under 6 columns (%d)", who, p->show_ratio,
                 p->border, p->signs_w, p->signs_h, p->signs_sprite_row, p->collision_sprite_row, p->collision_sprite_col, src_w);
    ADAS_REQUIRE(fit != PANEL_FIT_BIRD, ADAS_ERR_INVALID, "%s: the bird panel (%dx%d inside a border of %d) does not fit a %dx%d frame (W in 1..%d)", who, g.W,
                 g.H, g.border, src_w, src_h, PANEL_MAX_W);
    ADAS_REQUIRE(fit != PANEL_FIT_SIGNS, ADAS_ERR_INVALID, "%s: the signs panel's widget (%dx%d) does not fit a %dx%d frame", who, g.sw, g.sh, src_w, src_h);
    ADAS_REQUIRE(fit != PANEL_FIT_COLLISION, ADAS_ERR_INVALID,
                 "%s: the collision panel's widget is rows H + %d .. 2H - 1 with H = %d: H must exceed %d and 2H fit the frame (%dx%d)", who, 2 * g.border, g.H,
                 2 * g.border, src_w, src_h);
    ADAS_REQUIRE(fit != PANEL_FIT_SPRITE_SIZE, ADAS_ERR_INVALID, "%s: sprite %d is %dx%d, or the sprites hold too many pixels", who, slot,
                 slot >= 0 ? sw[slot] : 0, slot >= 0 ? sh[slot] : 0);
    ADAS_REQUIRE(fit != PANEL_FIT_COLLISION_SPRITE, ADAS_ERR_INVALID,
                 "%s: the collision panel's sprite %d (%dx%d at column %d, row %d) would leave the %dx%d frame: W + %d = %d columns, %d rows below H", who, slot,
                 sw[slot < 0 ? 0 : slot], sh[slot < 0 ? 0 : slot], g.sp[slot < 0 ? 0 : slot].x0, g.sp[slot < 0 ? 0 : slot].y0, src_w, src_h,
                 p->collision_sprite_col, g.W + p->collision_sprite_col, src_h - g.H);
    ADAS_REQUIRE(fit != PANEL_FIT_SIGN_SPRITE, ADAS_ERR_INVALID, "%s: the signs panel's sprite %d (%dx%d at column %d, row %d) would leave the %dx%d frame", who,
                 slot, sw[slot < 0 ? 0 : slot], sh[slot < 0 ? 0 : slot], g.sp[slot < 0 ? 0 : slot].x0, g.sp[slot < 0 ? 0 : slot].y0, src_w, src_h);
    size_t pixels = 0;
    for (int k = 0; k < ADAS_PANEL_SPRITES; ++k) pixels += (size_t)g.sp[k].w * g.sp[k].h;
    uint32_t* host = new (std::nothrow) uint32_t[pixels ? pixels : 1];
    ADAS_REQUIRE(host, ADAS_ERR_INVALID, "out of host memory");
    for (int k = 0; k < ADAS_PANEL_SPRITES; ++k)
        if (g.sp[k].w > 0) memcpy(host + g.sp[k].off, sprites[k].bgra, (size_t)g.sp[k].w * g.sp[k].h * 4);
    adas::overlay_panels* s = new (std::nothrow) adas::overlay_panels();
    if (!s) {
        delete[] host;
        ADAS_REQUIRE(false, ADAS_ERR_INVALID, "out of host memory");
    }
    s->g = g;
    s->max_batch = max_batch;
    hipError_t e = hipMalloc((void**)&s->atlas, (pixels ? pixels : 1) * 4);
    if (e == hipSuccess) e = hipMemcpy(s->atlas, host, (pixels ? pixels : 1) * 4, hipMemcpyHostToDevice);
    delete[] host;
    if (e == hipSuccess) e = hipMalloc((void**)&s->sprites, sizeof(g.sp));
    if (e == hipSuccess) e = hipMemcpy(s->sprites, g.sp, sizeof(g.sp), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&s->latch, (size_t)max_batch * 4);
    if (e == hipSuccess) e = hipMemset(s->latch, 0, (size_t)max_batch * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&s->recs, (size_t)max_batch * sizeof(PanelRecord));
    if (e == hipSuccess) e = hipMemset(s->recs, 0, (size_t)max_batch * sizeof(PanelRecord));
    if (e == hipSuccess) e = hipDeviceSynchronize();   // a run in flight may still read the old tables
    if (e != hipSuccess) {
        adas::overlay_panels_free(s);
        return hip_fail(e, "hipMalloc(overlay panels)", __FILE__, __LINE__);
    }
    adas::overlay_panels** held = adas::overlay_panel_slot(h);
    adas::overlay_panels_free(*held);
    *held = s;
    adas::bump_config_generation();   // a captured step holds the old tables' addresses in its kernel arguments
    return ADAS_OK;
}

int adas_overlay_run_panels(adas_overlay* h, uint8_t* d_frames_bgr, const adas_analysis* analysis, const uint8_t* d_bird_bgr, int panels, int n_streams,
                            int n_frames, void* stream) {
    return adas::overlay_run_panels("adas_overlay_run_panels", h, d_frames_bgr, analysis, d_bird_bgr, panels, n_streams, n_frames, stream);
}

int adas_overlay_run_panels_arrays(adas_overlay* h, uint8_t* d_frames_bgr, const int32_t* d_offset_type, const int32_t* d_curvature_type,
                                   const int32_t* d_collision_type, const uint8_t* d_bird_bgr, int panels, int n_streams, int n_frames, void* stream) {
    return panels_launch("adas_overlay_run_panels_arrays", h, d_frames_bgr, d_offset_type, 1, d_curvature_type, 1, d_collision_type, 1, d_bird_bgr, panels,
                         n_streams, n_frames, stream);
}

int adas_overlay_reset_panels(adas_overlay* h, int stream_index) {
    adas::overlay_panels* s = h ? *adas::overlay_panel_slot(h) : nullptr;
    ADAS_REQUIRE(s, ADAS_ERR_INVALID, "adas_overlay_reset_panels: no panels set (call adas_overlay_set_panels first)");
    ADAS_REQUIRE(stream_index >= -1 && stream_index < s->max_batch, ADAS_ERR_INVALID, "adas_overlay_reset_panels: stream %d of %d", stream_index, s->max_batch);
    ADAS_HIP_TRY(hipDeviceSynchronize());   // the last run, on whichever stream
    if (stream_index < 0) ADAS_HIP_TRY(hipMemset(s->latch, 0, (size_t)s->max_batch * 4));
    else ADAS_HIP_TRY(hipMemset(s->latch + stream_index, 0, 4));
    ADAS_HIP_TRY(hipDeviceSynchronize());
    return ADAS_OK;
}

int adas_overlay_fetch_panel_record(adas_overlay* h, int frame, adas_overlay_panel_record* rec) {
    adas::overlay_panels* s = h ? *adas::overlay_panel_slot(h) : nullptr;
    ADAS_REQUIRE(s && rec, ADAS_ERR_INVALID, "adas_overlay_fetch_panel_record: no panels set, or a null argument");
    ADAS_REQUIRE(frame >= 0 && frame < s->run_frames, ADAS_ERR_INVALID, "adas_overlay_fetch_panel_record: frame %d was not part of the last panel run (%d frames)",
                 frame, s->run_frames);
    ADAS_HIP_TRY(hipDeviceSynchronize());
    ADAS_HIP_TRY(hipMemcpy(rec, s->recs + frame, sizeof(*rec), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

}  // extern "C"
