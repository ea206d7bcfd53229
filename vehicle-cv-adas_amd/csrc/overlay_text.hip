// overlay_text.hip -- the overlay's text on the device from caller-supplied glyph atlases: class labels on their filled background, the
// tracker's "name : id" and shadowed "ID: n", the shadowed distances, the three panel strings and up to eight caller lines.  The rules are
// overlay_text_core.h (T1-T7); this file is the two kernels around them and the C ABI (adas_overlay_*text*, adas_overlay_set_font).  A run is
//   overlay_text_layout_kernel  one wave per frame.  Kind by kind in paint order, 64 candidates at a time: a lane counts the items of its
//                               candidate, the counts are scanned in LDS, and the lane formats, sizes and places its items at their place in
//                               the frame's list (T5, T6) -- strings, '%.2f' of a distance, ids and class names never leave the device.
//                               The frame's head holds its count, its flags and the rows its items cover.
//   overlay_text_draw_kernel    in place on the frames.  A workgroup owns 8 rows of one frame: it leaves after reading the head when no item
//                               covers them; otherwise it bins the frame's items that meet its rows, in order, in LDS, and its lanes take the
//                               aligned 16-byte pieces of the columns the binned items span, row by row.  A lane drops a piece no item's box
//                               meets without touching memory; else one 16-byte load, T7 over the binned items in order (text_fold_piece),
//                               one 16-byte store.  A piece that reaches outside the span of its row goes byte by byte, and only the bytes
//                               inside: no byte has two writers, nothing outside an item's clipped box is written, and nothing outside the
//                               buffer is read or written at any alignment or row length.
// As measured the stage is far from what its bytes would allow, and what bounds it is not identified.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "overlay_text_core.h"

using namespace adas;

static_assert(sizeof(TextFont) == sizeof(adas_overlay_font) && offsetof(TextFont, glyph_x) == offsetof(adas_overlay_font, glyph_x) &&
                  offsetof(TextFont, scale) == offsetof(adas_overlay_font, scale) && offsetof(TextFont, advance) == offsetof(adas_overlay_font, advance),
              "TextFont is adas_overlay_font");
static_assert(sizeof(TextItem) == sizeof(adas_overlay_text_item) && offsetof(TextItem, text) == offsetof(adas_overlay_text_item, text) &&
                  offsetof(TextItem, color) == offsetof(adas_overlay_text_item, color),
              "TextItem is adas_overlay_text_item");
static_assert(sizeof(TextStyle) == sizeof(adas_overlay_text_style) && offsetof(TextStyle, offset_colors) == offsetof(adas_overlay_text_style, offset_colors) &&
                  offsetof(TextStyle, fcws_y) == offsetof(adas_overlay_text_style, fcws_y),
              "TextStyle is adas_overlay_text_style");
static_assert(sizeof(TextLine) == sizeof(adas_overlay_text_line) && offsetof(TextLine, text) == offsetof(adas_overlay_text_line, text),
              "TextLine is adas_overlay_text_line");
static_assert(TEXT_FONTS == ADAS_TEXT_FONTS && TEXT_DETECTIONS == ADAS_TEXT_DETECTIONS && TEXT_TRACKS == ADAS_TEXT_TRACKS &&
                  TEXT_TRACK_IDS == ADAS_TEXT_TRACK_IDS && TEXT_DISTANCE == ADAS_TEXT_DISTANCE && TEXT_PANELS == ADAS_TEXT_PANELS &&
                  TEXT_LINES == ADAS_TEXT_LINES && TEXT_FLAG_RANGE == ADAS_OVERLAY_TEXT_RANGE && TEXT_FLAG_OVERFLOW == ADAS_OVERLAY_TEXT_OVERFLOW &&
                  TEXT_MAX_LINES == ADAS_TEXT_MAX_LINES && TEXT_ITEM_RECT == ADAS_TEXT_ITEM_RECT && TEXT_ITEM_RUN == ADAS_TEXT_ITEM_RUN,
              "overlay_text_core.h restates ADAS_TEXT_*");

namespace {

constexpr int TX_THREADS = 256;
constexpr int TX_ROWS = 8;   // rows of a draw workgroup

struct TxLayout {
    TextSrc s;
    TextTables t;
    TextStyle st;
    int mask, max_items;
    TextItem* items;   // [frames][max_items]
    int* heads;        // [frames][4]: count, flags, first row, end row
};

__global__ __launch_bounds__(64) void overlay_text_layout_kernel(const TxLayout a) {
    __shared__ int cnt[64];
    __shared__ int s_flags, s_r0, s_r1;
    const long long q = blockIdx.x;
    const int lane = threadIdx.x;
    if (lane == 0) { s_flags = 0; s_r0 = 0x7fffffff; s_r1 = 0; }
    __syncthreads();
    TextItem* out = a.items + q * a.max_items;
    int base = 0, flags = 0, r0 = 0x7fffffff, r1 = 0;
    for (int kind = 1; kind <= TEXT_LINES; kind <<= 1) {
        if (!(a.mask & kind)) continue;
        const int n = text_candidates(a.s, a.t, kind, q);
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int c = c0 + lane;
            const int k = c < n ? text_candidate(a.s, a.t, a.st, kind, q, c, nullptr, 0, &flags) : 0;
            cnt[lane] = k;
            __syncthreads();
            int off = base, tot = 0;
            for (int j = 0; j < 64; ++j) {
                if (j < lane) off += cnt[j];
                tot += cnt[j];
            }
            __syncthreads();
            if (k > 0) {
                if (off + k > a.max_items) flags |= TEXT_FLAG_OVERFLOW;   // T6
                if (off < a.max_items) {
                    const int room = a.max_items - off;
                    text_candidate(a.s, a.t, a.st, kind, q, c, out + off, room, &flags);
                    for (int i = 0; i < k && i < room; ++i)
                        if (out[off + i].bx0 < out[off + i].bx1) {
                            r0 = out[off + i].by0 < r0 ? out[off + i].by0 : r0;
                            r1 = out[off + i].by1 > r1 ? out[off + i].by1 : r1;
                        }
                }
            }
            base += tot;
        }
    }
    if (flags) atomicOr(&s_flags, flags);
    if (r1 > r0) { atomicMin(&s_r0, r0); atomicMax(&s_r1, r1); }
    __syncthreads();
    if (lane == 0) {
        int* hd = a.heads + q * 4;
        hd[0] = base < a.max_items ? base : a.max_items;
        hd[1] = s_flags;
        hd[2] = s_r1 > s_r0 ? s_r0 : 0;
        hd[3] = s_r1 > s_r0 ? s_r1 : 0;
    }
}

struct TxDraw {
    const TextFont* fonts;
    const TextItem* items;
    const int* heads;
    uint8_t* dst;   // [frames][H][W][3], any alignment
    int W, H, max_items;
    int align;      // the buffer's address & 15
    int sources;    // the TEXT_* bits whose items this launch paints
};

__global__ __launch_bounds__(TX_THREADS) void overlay_text_draw_kernel(const TxDraw a) {
    __shared__ uint16_t bin[TEXT_MAX_ITEMS];
    __shared__ ushort4 box[TEXT_MAX_ITEMS];   // the binned items' boxes
    __shared__ uint8_t hit[TX_THREADS];
    __shared__ int s_c0, s_c1;
    const int f = blockIdx.y, t = threadIdx.x;
    const int r0 = blockIdx.x * TX_ROWS, r1 = r0 + TX_ROWS < a.H ? r0 + TX_ROWS : a.H;
    const int* hd = a.heads + (long long)f * 4;
    int n = hd[0];
    if (n <= 0 || r1 <= hd[2] || r0 >= hd[3]) return;   // the whole workgroup
    if (n > a.max_items) n = a.max_items;
    const TextItem* items = a.items + (long long)f * a.max_items;
    if (t == 0) { s_c0 = 0x7fffffff; s_c1 = 0; }
    __syncthreads();
    int nb = 0;
    for (int i0 = 0; i0 < n; i0 += TX_THREADS) {   // the items that meet the rows, in order
        const int i = i0 + t;
        int h = 0;
        ushort4 b = make_ushort4(0, 0, 0, 0);
        if (i < n) {
            const TextItem& it = items[i];
            h = (it.source & a.sources) && it.bx0 < it.bx1 && it.by0 < r1 && it.by1 > r0;
            b = make_ushort4((unsigned short)it.bx0, (unsigned short)it.by0, (unsigned short)it.bx1, (unsigned short)it.by1);
        }
        hit[t] = (uint8_t)h;
        const int tot = __syncthreads_count(h);
        if (h) {
            int pos = nb;
            for (int j = 0; j < t; ++j) pos += hit[j];
            bin[pos] = (uint16_t)i;
            box[pos] = b;
            atomicMin(&s_c0, (int)b.x);
            atomicMax(&s_c1, (int)b.z);
        }
        nb += tot;
        __syncthreads();
    }
    if (nb == 0) return;
    const int c0 = s_c0 * 3, c1 = s_c1 * 3;   // the bytes of a row the binned items span
    const int maxnp = (c1 - c0 + 15) / 16 + 1;
    const long long row_bytes = (long long)a.W * 3;
    for (int idx = t; idx < (r1 - r0) * maxnp; idx += TX_THREADS) {
        const int row = r0 + idx / maxnp;
        const long long rowstart = ((long long)f * a.H + row) * row_bytes;   // in the buffer
        const long long P0 = (rowstart + a.align + c0) >> 4, P1 = (rowstart + a.align + c1 - 1) >> 4;
        const long long P = P0 + idx % maxnp;
        if (P > P1) continue;
        const long long o0 = P * 16 - a.align;     // the piece's first byte in the buffer
        const int b0 = (int)(o0 - rowstart);       // and in the row
        const int lo = b0 > c0 ? b0 : c0, hi = b0 + 16 < c1 ? b0 + 16 : c1;   // the bytes of the piece this lane owns
        bool meets = false;
        for (int k = 0; k < nb && !meets; ++k) {
            const ushort4 b = box[k];
            meets = row >= b.y && row < b.w && (int)b.x * 3 < hi && (int)b.z * 3 > lo;
        }
        if (!meets) continue;
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
        bool any = false;
        for (int k = 0; k < nb; ++k) any |= text_fold_piece(a.fonts, items[bin[k]], row, b0, w);
        if (!any) continue;
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

struct adas::overlay_text {
    TextFont fonts[TEXT_FONTS];        // the device table's host copy (atlas: device pointers)
    TextFont* d_fonts = nullptr;
    TextStyle style;
    char* d_names[2] = {nullptr, nullptr};
    int n_names[2] = {0, 0};
    TextLine* d_lines = nullptr;       // [TEXT_MAX_LINES]
    TextLine lines[TEXT_MAX_LINES];
    int n_lines = 0;
    TextItem* items = nullptr;         // [max_batch][max_items]
    int* heads = nullptr;              // [max_batch][4]
    int max_batch = 0, max_items = 0, src_w = 0, src_h = 0;
    int n_fonts = 0;
    int run_frames = 0;
};

void adas::overlay_text_free(adas::overlay_text* s) {
    if (!s) return;
    for (int k = 0; k < TEXT_FONTS; ++k)
        if (s->fonts[k].atlas) (void)hipFree((void*)s->fonts[k].atlas);
    for (void* q : {(void*)s->d_fonts, (void*)s->d_names[0], (void*)s->d_names[1], (void*)s->d_lines, (void*)s->items, (void*)s->heads})
        if (q) (void)hipFree(q);
    delete s;
}

static void text_default_style(TextStyle* p) {
    memset(p, 0, sizeof(*p));
    p->show_ratio = 0.25;
    p->min_box_area = 10.0;
    p->max_text_items = 256;
    p->det_size_slot = 0; p->det_label_slot = 1;
    p->det_label_dx = 2; p->det_label_dy = -7; p->det_box_pad = 3;
    p->track_slot = 2; p->track_dy = -10;
    p->id_first = 3; p->id_count = 1; p->id_shadow_first = 4; p->id_shadow_count = 1;
    p->dist_size_first = 5; p->dist_size_count = 1; p->dist_first = 6; p->dist_count = 1; p->dist_shadow_first = 7; p->dist_shadow_count = 1;
    p->shadow_dx = 2; p->shadow_dy = 2;
    p->ldws_slot = 8; p->lkas_slot = 8; p->fcws_slot = 9;
    p->ldws_x = 10; p->ldws_y = 240; p->lkas_x = 10; p->lkas_y = 280; p->fcws_dx = 100; p->fcws_y = 240;
    p->id_shadow_sub = 30;
    const uint8_t white[3] = {255, 255, 255}, grey[3] = {150, 150, 150}, yellow[3] = {0, 255, 255}, red[3] = {0, 0, 255}, green[3] = {0, 255, 0},
                  orange[3] = {0, 102, 255};
    memcpy(p->label_color, white, 3); memcpy(p->dist_color, white, 3); memcpy(p->dist_shadow_color, grey, 3);
    const uint8_t* off[4] = {yellow, red, red, green};
    const uint8_t* cur[6] = {yellow, green, orange, red, orange, red};
    const uint8_t* col[4] = {yellow, green, orange, red};
    for (int k = 0; k < 4; ++k) memcpy(p->offset_colors[k], off[k], 3);
    for (int k = 0; k < 6; ++k) memcpy(p->curvature_colors[k], cur[k], 3);
    for (int k = 0; k < 4; ++k) memcpy(p->collision_colors[k], col[k], 3);
}

// the handle's text state, made on the first adas_overlay_set_* of the text
static int text_state(adas_overlay* h, adas::overlay_text** out) {
    adas::overlay_text** held = adas::overlay_text_slot(h);
    if (*held) { *out = *held; return ADAS_OK; }
    adas::overlay_text* s = new (std::nothrow) adas::overlay_text();
    ADAS_REQUIRE(s, ADAS_ERR_INVALID, "out of host memory");
    memset(s->fonts, 0, sizeof(s->fonts));
    memset(s->lines, 0, sizeof(s->lines));
    text_default_style(&s->style);
    int bh = 0, bw = 0;
    (void)adas::overlay_geometry(h, &s->src_h, &s->src_w, &bh, &bw, &s->max_batch);
    if (s->src_w > 65535 || s->src_h > 65535) {   // the draw kernel keeps the binned items' boxes as 16-bit values in LDS
        const int w = s->src_w, hh = s->src_h;
        delete s;
        ADAS_REQUIRE(false, ADAS_ERR_INVALID, "the overlay's text takes frames of at most 65535 x 65535 pixels (this handle: %d x %d)", w, hh);
    }
    s->max_items = s->style.max_text_items;
    hipError_t e = hipMalloc((void**)&s->d_fonts, sizeof(s->fonts));
    if (e == hipSuccess) e = hipMemset(s->d_fonts, 0, sizeof(s->fonts));
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_lines, sizeof(s->lines));
    if (e == hipSuccess) e = hipMemset(s->d_lines, 0, sizeof(s->lines));
    if (e == hipSuccess) e = hipMalloc((void**)&s->items, (size_t)s->max_batch * s->max_items * sizeof(TextItem));
    if (e == hipSuccess) e = hipMalloc((void**)&s->heads, (size_t)s->max_batch * 16);
    if (e == hipSuccess) e = hipMemset(s->heads, 0, (size_t)s->max_batch * 16);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        adas::overlay_text_free(s);
        return hip_fail(e, "hipMalloc(overlay text)", __FILE__, __LINE__);
    }
    *held = s;
    *out = s;
    return ADAS_OK;
}

static bool ladder_ok(const adas::overlay_text* s, int first, int count, int* bad) {
    for (int k = first; k < first + count; ++k)
        if (k < 0 || k >= TEXT_FONTS || !s->fonts[k].set) { *bad = k; return false; }
    return count >= 1;
}

// the draw launch over the item lists of the last layout: the items of the kinds `sources`
static int text_draw(adas::overlay_text* s, uint8_t* d_frames_bgr, int sources, int frames, hipStream_t strm) {
    if (!sources) return ADAS_OK;
    TxDraw d = {};
    d.fonts = s->d_fonts; d.items = s->items; d.heads = s->heads; d.dst = d_frames_bgr;
    d.W = s->src_w; d.H = s->src_h; d.max_items = s->max_items;
    d.align = (int)((uintptr_t)d_frames_bgr & 15);
    d.sources = sources;
    hipLaunchKernelGGL(overlay_text_draw_kernel, dim3((unsigned)((s->src_h + TX_ROWS - 1) / TX_ROWS), (unsigned)frames), dim3(TX_THREADS), 0, strm, d);
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

// one run, from wherever the sources live: the layout of `mask`, then the draw of its kinds in `draw_now` (the rest: text_draw, later)
static int text_launch(const char* who, adas_overlay* h, uint8_t* d_frames_bgr, const TextSrc& src, int mask, int draw_now, int n_streams, int n_frames,
                       void* stream) {
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "%s: null handle", who);
    ADAS_REQUIRE(mask >= 0 && !(mask & ~TEXT_ALL), ADAS_ERR_INVALID, "%s: unknown text bits 0x%x", who, mask);
    adas::overlay_text* s = *adas::overlay_text_slot(h);
    ADAS_REQUIRE(s && s->n_fonts > 0, ADAS_ERR_INVALID, "%s: no font set (call adas_overlay_set_font first)", who);
    ADAS_REQUIRE(n_streams > 0 && n_frames > 0, ADAS_ERR_INVALID, "%s: bad argument (%d streams x %d frames)", who, n_streams, n_frames);
    const long long frames = (long long)n_streams * n_frames;
    ADAS_REQUIRE(frames <= s->max_batch, ADAS_ERR_INVALID, "%s: %d streams x %d frames, the handle holds %d frames", who, n_streams, n_frames, s->max_batch);
    const TextStyle& st = s->style;
    int bad = -1;
#define TEXT_NEED_LADDER(bit, name, first, count) \
    ADAS_REQUIRE(!(mask & (bit)) || ladder_ok(s, (first), (count), &bad), ADAS_ERR_INVALID, "%s: the %s text needs font slot %d, which is empty", who, name, bad)
    TEXT_NEED_LADDER(TEXT_DETECTIONS, "detections", st.det_size_slot, 1);
    TEXT_NEED_LADDER(TEXT_DETECTIONS, "detections", st.det_label_slot, 1);
    TEXT_NEED_LADDER(TEXT_TRACKS, "tracks", st.track_slot, 1);
    TEXT_NEED_LADDER(TEXT_TRACK_IDS, "track_ids", st.id_first, st.id_count);
    TEXT_NEED_LADDER(TEXT_TRACK_IDS, "track_ids", st.id_shadow_first, st.id_shadow_count);
    TEXT_NEED_LADDER(TEXT_DISTANCE, "distance", st.dist_size_first, st.dist_size_count);
    TEXT_NEED_LADDER(TEXT_DISTANCE, "distance", st.dist_first, st.dist_count);
    TEXT_NEED_LADDER(TEXT_DISTANCE, "distance", st.dist_shadow_first, st.dist_shadow_count);
    TEXT_NEED_LADDER(TEXT_PANELS, "panels", st.ldws_slot, 1);
    TEXT_NEED_LADDER(TEXT_PANELS, "panels", st.lkas_slot, 1);
    TEXT_NEED_LADDER(TEXT_PANELS, "panels", st.fcws_slot, 1);
    for (int k = 0; k < s->n_lines; ++k) TEXT_NEED_LADDER(TEXT_LINES, "lines", s->lines[k].slot, 1);
#undef TEXT_NEED_LADDER
    ADAS_REQUIRE(!(mask & TEXT_DETECTIONS) || (src.det_xyxy && src.det_cls && src.det_cnt && src.det_cap > 0), ADAS_ERR_INVALID,
                 "%s: the detections text needs the detections (boxes, classes, counts)", who);
    ADAS_REQUIRE(!(mask & (TEXT_TRACKS | TEXT_TRACK_IDS)) || (src.trk_tlwh && src.trk_cls && src.trk_ids && src.trk_cnt && src.trk_cap > 0), ADAS_ERR_INVALID,
                 "%s: the tracks and track_ids text need the tracks (tlwh, classes, ids, counts)", who);
    ADAS_REQUIRE(!(mask & TEXT_TRACK_IDS) || (src.ring && src.len), ADAS_ERR_INVALID,
                 "%s: the track_ids text needs the trajectories' newest boxes and lengths", who);
    ADAS_REQUIRE(!(mask & TEXT_DISTANCE) || (src.dist_xy && src.dist_d && src.dist_cnt && src.dist_cap > 0), ADAS_ERR_INVALID,
                 "%s: the distance text needs the distance points (xy, d, counts)", who);
    ADAS_REQUIRE(!(mask & TEXT_PANELS) || (src.offset && src.curvature && src.collision), ADAS_ERR_INVALID,
                 "%s: the panels text needs the offset, curvature and collision types", who);
    if (!d_frames_bgr) {
        int written = 0;
        int rc = adas::overlay_own_frames(h, &d_frames_bgr, &written);
        if (rc) return rc;
        ADAS_REQUIRE(frames <= written, ADAS_ERR_INVALID, "%s: %d frames, but the handle's own buffer holds %d drawn frames (run the overlay into it first)", who,
                     (int)frames, written);
    }
    hipStream_t strm = (hipStream_t)stream;
    adas::overlay_note_stream(h, stream);
    s->run_frames = (int)frames;
    TxLayout a = {};
    a.s = src;
    a.s.src_w = s->src_w; a.s.src_h = s->src_h;
    a.t.fonts = s->d_fonts;
    a.t.det_names = s->d_names[0]; a.t.n_det_names = s->n_names[0];
    a.t.trk_names = s->d_names[1]; a.t.n_trk_names = s->n_names[1];
    adas::overlay_class_colors(h, 0, &a.t.det_colors, &a.t.n_det_colors);
    adas::overlay_class_colors(h, 1, &a.t.trk_colors, &a.t.n_trk_colors);
    a.t.lines = s->d_lines; a.t.n_lines = s->n_lines;
    a.st = st;
    a.mask = mask; a.max_items = s->max_items;
    a.items = s->items; a.heads = s->heads;
    hipLaunchKernelGGL(overlay_text_layout_kernel, dim3((unsigned)frames), dim3(64), 0, strm, a);
    ADAS_HIP_TRY(hipGetLastError());
    return text_draw(s, d_frames_bgr, mask & draw_now, (int)frames, strm);
}

void adas::overlay_text_font_tables(adas_overlay* h, const void** d_fonts, const void** h_fonts) {
    adas::overlay_text* s = h ? *adas::overlay_text_slot(h) : nullptr;
    *d_fonts = s ? s->d_fonts : nullptr;
    *h_fonts = s ? s->fonts : nullptr;
}

bool adas::overlay_text_ready(adas_overlay* h) { return h && *adas::overlay_text_slot(h) && (*adas::overlay_text_slot(h))->n_fonts > 0; }

// the run of adas_overlay_run_text under the caller's name: the sources where the handles keep them
int adas::overlay_run_text(const char* who, adas_overlay* h, uint8_t* d_frames_bgr, const adas_yolo_post* post, const adas_bytetrack* tracker,
                           const adas_analysis* analysis, int mask, int draw_now, int n_streams, int n_frames, void* stream) {
    const bool known = mask >= 0 && !(mask & ~TEXT_ALL);   // unknown bits are text_launch's refusal
    ADAS_REQUIRE(!known || !(mask & TEXT_DETECTIONS) || post, ADAS_ERR_INVALID, "%s: the detections text needs a post handle (the survivors)", who);
    ADAS_REQUIRE(!known || !(mask & (TEXT_TRACKS | TEXT_TRACK_IDS)) || tracker, ADAS_ERR_INVALID, "%s: the %s text needs a bytetrack handle", who,
                 (mask & TEXT_TRACKS) ? "tracks" : "track_ids");
    ADAS_REQUIRE(!known || !(mask & (TEXT_DISTANCE | TEXT_PANELS)) || analysis, ADAS_ERR_INVALID, "%s: the %s text needs an analysis handle", who,
                 (mask & TEXT_DISTANCE) ? "distance" : "panels");
    TextSrc s = {};
    if (post && known && (mask & TEXT_DETECTIONS)) {
        const int *xyxy, *cls, *counts;
        int cap = 0;
        adas::post_survivor_views(post, &xyxy, &cls, &counts, &cap);
        s.det_xyxy = xyxy; s.det_cls = cls; s.det_cnt = counts + 2; s.det_cnt_stride = 4; s.det_cap = cap;   // n_keep is word 2 of a frame's counts
    }
    if (tracker && known && (mask & (TEXT_TRACKS | TEXT_TRACK_IDS))) {
        ADAS_REQUIRE(n_frames == 1, ADAS_ERR_INVALID, "%s: the %s text reads the tracker's live table, which holds the last frame only: n_frames must be 1 (got %d)",
                     who, (mask & TEXT_TRACKS) ? "tracks" : "track_ids", n_frames);
        const unsigned char *hdr, *rows;
        size_t stream_bytes = 0, slot_bytes = 0;
        int ts = 0, cap = 0;
        adas::tracker_live_views(tracker, &hdr, &rows, &stream_bytes, &ts, &cap);
        ADAS_REQUIRE(n_streams <= ts, ADAS_ERR_INVALID, "%s: %d streams, the bytetrack handle holds %d", who, n_streams, ts);
        s.trk_tlwh = rows + offsetof(adas_track, tlwh); s.trk_act = rows + offsetof(adas_track, is_activated);
        s.trk_cls = rows + offsetof(adas_track, class_id); s.trk_ids = rows + offsetof(adas_track, track_id);
        s.trk_cnt = hdr + offsetof(adas_track_header, n_tracked);
        s.trk_frame_bytes = s.trk_cls_frame_bytes = s.trk_cnt_bytes = (long long)stream_bytes;
        s.trk_row_bytes = s.trk_cls_row_bytes = sizeof(adas_track);
        s.trk_cap = cap;
        adas::tracker_ring_views(tracker, &s.slot_ids, &s.len, &slot_bytes, &s.ring);
        s.len_row_bytes = (long long)slot_bytes;
        s.slot_frame_bytes = s.len_frame_bytes = s.ring_frame_bytes = (long long)stream_bytes;
    }
    if (analysis && known && (mask & (TEXT_DISTANCE | TEXT_PANELS))) {
        const int *fr, *pts;
        int stride = 0, maxp = 0, af = 0;
        ADAS_REQUIRE(adas::analysis_capacity(analysis, nullptr, &af) && (long long)n_streams * n_frames <= af, ADAS_ERR_INVALID,
                     "%s: %d streams x %d frames, the analysis handle holds %d frames", who, n_streams, n_frames, af);
        adas::analysis_frame_views(analysis, &fr, &stride, &pts, &maxp);
        s.dist_xy = pts; s.dist_d = adas::analysis_points_d(analysis); s.dist_cap = maxp;
        s.dist_cnt = fr + offsetof(adas_analysis_frame, n_points) / 4; s.dist_cnt_stride = stride;
        s.offset = fr + offsetof(adas_analysis_frame, offset_msg) / 4;
        s.curvature = fr + offsetof(adas_analysis_frame, curvature_msg) / 4;
        s.collision = fr + offsetof(adas_analysis_frame, collision_msg) / 4;
        s.msg_stride = stride;
    }
    return text_launch(who, h, d_frames_bgr, s, mask, draw_now, n_streams, n_frames, stream);
}

// the kinds `sources` of the last layout, painted now (the pipeline's step: the panel strings and the lines, behind the panels)
int adas::overlay_draw_text(const char* who, adas_overlay* h, int sources, int n_frames_total, void* stream) {
    adas::overlay_text* s = h ? *adas::overlay_text_slot(h) : nullptr;
    ADAS_REQUIRE(s && n_frames_total == s->run_frames, ADAS_ERR_INVALID, "%s: no text layout of %d frames to draw from", who, n_frames_total);
    uint8_t* frames = nullptr;
    int written = 0;
    int rc = adas::overlay_own_frames(h, &frames, &written);
    if (rc) return rc;
    ADAS_REQUIRE(n_frames_total <= written, ADAS_ERR_INVALID, "%s: %d frames, but the handle's own buffer holds %d drawn frames", who, n_frames_total, written);
    return text_draw(s, frames, sources & TEXT_ALL, n_frames_total, (hipStream_t)stream);
}

extern "C" {

int adas_overlay_default_text_style(adas_overlay_text_style* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_overlay_default_text_style: null argument");
    text_default_style((TextStyle*)p);
    return ADAS_OK;
}

int adas_overlay_set_text_style(adas_overlay* h, const adas_overlay_text_style* p) {
    const char* who = "adas_overlay_set_text_style";
    ADAS_REQUIRE(h && p, ADAS_ERR_INVALID, "%s: bad argument", who);
    TextStyle st;
    memcpy(&st, p, sizeof(st));
    ADAS_REQUIRE(st.max_text_items >= 1 && st.max_text_items <= TEXT_MAX_ITEMS, ADAS_ERR_INVALID, "%s: max_text_items %d (1 .. %d)", who, st.max_text_items,
                 TEXT_MAX_ITEMS);
    ADAS_REQUIRE(st.show_ratio > 0.0 && st.show_ratio <= 1.0, ADAS_ERR_INVALID, "%s: show_ratio %g", who, st.show_ratio);
    const int singles[] = {st.det_size_slot, st.det_label_slot, st.track_slot, st.ldws_slot, st.lkas_slot, st.fcws_slot};
    for (int v : singles) ADAS_REQUIRE(v >= 0 && v < TEXT_FONTS, ADAS_ERR_INVALID, "%s: font slot %d (0 .. %d)", who, v, TEXT_FONTS - 1);
    const int ladders[][2] = {{st.id_first, st.id_count},           {st.id_shadow_first, st.id_shadow_count}, {st.dist_size_first, st.dist_size_count},
                              {st.dist_first, st.dist_count},       {st.dist_shadow_first, st.dist_shadow_count}};
    for (const auto& l : ladders)
        ADAS_REQUIRE(l[0] >= 0 && l[1] >= 1 && l[0] + l[1] <= TEXT_FONTS, ADAS_ERR_INVALID, "%s: ladder of %d slots from %d (inside 0 .. %d)", who, l[1], l[0],
                     TEXT_FONTS - 1);
    adas::overlay_text* s = nullptr;
    int rc = text_state(h, &s);
    if (rc) return rc;
    ADAS_HIP_TRY(hipDeviceSynchronize());
    if (st.max_text_items != s->max_items) {
        TextItem* items = nullptr;
        ADAS_HIP_TRY(hipMalloc((void**)&items, (size_t)s->max_batch * st.max_text_items * sizeof(TextItem)));
        (void)hipFree(s->items);
        s->items = items;
        s->max_items = st.max_text_items;
        s->run_frames = 0;
    }
    s->style = st;
    adas::bump_config_generation();   // a captured step holds the style in its kernel arguments
    return ADAS_OK;
}

int adas_overlay_set_font(adas_overlay* h, int slot, const adas_overlay_font* font) {
    const char* who = "adas_overlay_set_font";
    ADAS_REQUIRE(h && font, ADAS_ERR_INVALID, "%s: bad argument", who);
    ADAS_REQUIRE(slot >= 0 && slot < TEXT_FONTS, ADAS_ERR_INVALID, "%s: slot %d (0 .. %d)", who, slot, TEXT_FONTS - 1);
    ADAS_REQUIRE(font->atlas, ADAS_ERR_INVALID, "%s: slot %d: atlas is null", who, slot);
    ADAS_REQUIRE(font->cell_h >= 1 && font->cell_h <= TEXT_MAX_CELL, ADAS_ERR_INVALID, "%s: slot %d: cell_h %d (1 .. %d)", who, slot, font->cell_h, TEXT_MAX_CELL);
    ADAS_REQUIRE(font->atlas_w >= 1 && font->atlas_w <= 65536, ADAS_ERR_INVALID, "%s: slot %d: atlas_w %d (1 .. 65536)", who, slot, font->atlas_w);
    ADAS_REQUIRE(font->baseline_row >= -4096 && font->baseline_row <= 4096, ADAS_ERR_INVALID, "%s: slot %d: baseline_row %d", who, slot, font->baseline_row);
    ADAS_REQUIRE(font->size_h >= 0 && font->size_h <= 4096, ADAS_ERR_INVALID, "%s: slot %d: size_h %d (0 .. 4096)", who, slot, font->size_h);
    ADAS_REQUIRE(font->size_w_extra >= -(4096 << 16) && font->size_w_extra <= (4096 << 16), ADAS_ERR_INVALID, "%s: slot %d: size_w_extra %d", who, slot,
                 font->size_w_extra);
    ADAS_REQUIRE(font->scale == font->scale && fabs(font->scale) <= 1e6, ADAS_ERR_INVALID, "%s: slot %d: scale %g", who, slot, font->scale);
    for (int g = 0; g < TEXT_GLYPHS; ++g) {
        ADAS_REQUIRE(font->glyph_w[g] >= 0 && font->glyph_w[g] <= TEXT_MAX_CELL, ADAS_ERR_INVALID, "%s: slot %d: glyph_w of character %d is %d (0 .. %d)", who, slot,
                     g + 32, font->glyph_w[g], TEXT_MAX_CELL);
        ADAS_REQUIRE(font->glyph_x[g] >= 0 && font->glyph_x[g] + font->glyph_w[g] <= font->atlas_w, ADAS_ERR_INVALID,
                     "%s: slot %d: glyph_x of character %d is %d: columns %d .. %d leave the atlas (%d columns)", who, slot, g + 32, font->glyph_x[g],
                     font->glyph_x[g], font->glyph_x[g] + font->glyph_w[g] - 1, font->atlas_w);
        ADAS_REQUIRE(font->bearing_x[g] >= -4096 && font->bearing_x[g] <= 4096, ADAS_ERR_INVALID, "%s: slot %d: bearing_x of character %d is %d", who, slot, g + 32,
                     font->bearing_x[g]);
        ADAS_REQUIRE(font->advance[g] >= 0 && font->advance[g] <= (4096 << 16), ADAS_ERR_INVALID, "%s: slot %d: advance of character %d is %d", who, slot, g + 32,
                     font->advance[g]);
    }
    adas::overlay_text* s = nullptr;
    int rc = text_state(h, &s);
    if (rc) return rc;
    const size_t bytes = (size_t)font->cell_h * font->atlas_w;
    uint8_t* atlas = nullptr;
    ADAS_HIP_TRY(hipMalloc((void**)&atlas, bytes));
    hipError_t e = hipMemcpy(atlas, font->atlas, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // a run in flight may still read the old atlas
    TextFont nf;
    memcpy(&nf, font, sizeof(nf));
    nf.atlas = atlas;
    nf.set = 1;
    if (e == hipSuccess) e = hipMemcpy(s->d_fonts + slot, &nf, sizeof(nf), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(atlas);
        return hip_fail(e, "hipMemcpy(overlay font)", __FILE__, __LINE__);
    }
    if (s->fonts[slot].atlas) (void)hipFree((void*)s->fonts[slot].atlas);
    else ++s->n_fonts;
    s->fonts[slot] = nf;
    return ADAS_OK;
}

int adas_overlay_set_text_labels(adas_overlay* h, int which, const char* const* names, int n) {
    const char* who = "adas_overlay_set_text_labels";
    ADAS_REQUIRE(h && (names || n == 0) && n >= 0 && n <= 65536, ADAS_ERR_INVALID, "%s: bad argument", who);
    ADAS_REQUIRE(which == ADAS_OVERLAY_DETECTIONS || which == ADAS_OVERLAY_TRACKS, ADAS_ERR_INVALID,
                 "%s: which is %d (ADAS_OVERLAY_DETECTIONS or ADAS_OVERLAY_TRACKS)", who, which);
    for (int k = 0; k < n; ++k)
        ADAS_REQUIRE(names[k] && strlen(names[k]) < (size_t)TEXT_LABEL_BYTES, ADAS_ERR_INVALID, "%s: name %d is null or longer than %d bytes", who, k,
                     TEXT_LABEL_BYTES - 1);
    adas::overlay_text* s = nullptr;
    int rc = text_state(h, &s);
    if (rc) return rc;
    const int t = which == ADAS_OVERLAY_TRACKS;
    char* table = nullptr;
    if (n > 0) {
        char* host = new (std::nothrow) char[(size_t)n * TEXT_LABEL_BYTES]();
        ADAS_REQUIRE(host, ADAS_ERR_INVALID, "out of host memory");
        for (int k = 0; k < n; ++k) memcpy(host + (size_t)k * TEXT_LABEL_BYTES, names[k], strlen(names[k]));
        hipError_t e = hipMalloc((void**)&table, (size_t)n * TEXT_LABEL_BYTES);
        if (e == hipSuccess) e = hipMemcpy(table, host, (size_t)n * TEXT_LABEL_BYTES, hipMemcpyHostToDevice);
        delete[] host;
        if (e != hipSuccess) {
            if (table) (void)hipFree(table);
            return hip_fail(e, "hipMalloc(overlay text labels)", __FILE__, __LINE__);
        }
    }
    ADAS_HIP_TRY(hipDeviceSynchronize());
    if (s->d_names[t]) (void)hipFree(s->d_names[t]);
    s->d_names[t] = table;
    s->n_names[t] = n;
    adas::bump_config_generation();   // a captured step holds the old table's address
    return ADAS_OK;
}

int adas_overlay_set_text_lines(adas_overlay* h, const adas_overlay_text_line* lines, int n) {
    const char* who = "adas_overlay_set_text_lines";
    ADAS_REQUIRE(h && (lines || n == 0) && n >= 0 && n <= TEXT_MAX_LINES, ADAS_ERR_INVALID, "%s: %d lines (0 .. %d)", who, n, TEXT_MAX_LINES);
    for (int k = 0; k < n; ++k) {
        ADAS_REQUIRE(lines[k].slot >= 0 && lines[k].slot < TEXT_FONTS, ADAS_ERR_INVALID, "%s: line %d: slot %d (0 .. %d)", who, k, lines[k].slot, TEXT_FONTS - 1);
        ADAS_REQUIRE(lines[k].len <= TEXT_MAX_CHARS, ADAS_ERR_INVALID, "%s: line %d: %d bytes (at most %d)", who, k, (int)lines[k].len, TEXT_MAX_CHARS);
        ADAS_REQUIRE(text_in_range_i(lines[k].x) && text_in_range_i(lines[k].y), ADAS_ERR_INVALID, "%s: line %d: origin (%d, %d)", who, k, lines[k].x, lines[k].y);
    }
    adas::overlay_text* s = nullptr;
    int rc = text_state(h, &s);
    if (rc) return rc;
    ADAS_HIP_TRY(hipDeviceSynchronize());
    memset(s->lines, 0, sizeof(s->lines));
    if (n) memcpy(s->lines, lines, (size_t)n * sizeof(TextLine));
    ADAS_HIP_TRY(hipMemcpy(s->d_lines, s->lines, sizeof(s->lines), hipMemcpyHostToDevice));
    s->n_lines = n;
    adas::bump_config_generation();   // the number of lines is a kernel argument
    return ADAS_OK;
}

int adas_overlay_run_text_arrays(adas_overlay* h, uint8_t* d_frames_bgr, const adas_overlay_text_arrays* a, int mask, int n_streams, int n_frames, void* stream) {
    const char* who = "adas_overlay_run_text_arrays";
    ADAS_REQUIRE(a, ADAS_ERR_INVALID, "%s: null argument", who);
    const TextSrc s = text_src_of_arrays(a->d_det_xyxy, a->d_det_cls, a->d_det_counts, a->det_cap, a->d_trk_tlwh, a->d_trk_cls, a->d_trk_ids, a->d_trk_counts,
                                         a->trk_cap, a->d_trk_last_tlbr, a->d_traj_len, a->d_dist_points, a->d_dist_d, a->d_dist_counts, a->dist_cap,
                                         a->d_offset_type, a->d_curvature_type, a->d_collision_type);
    return text_launch(who, h, d_frames_bgr, s, mask, TEXT_ALL, n_streams, n_frames, stream);
}

int adas_overlay_run_text(adas_overlay* h, uint8_t* d_frames_bgr, adas_yolo_post* post, struct adas_bytetrack* tracker, const adas_analysis* analysis, int mask,
                          int n_streams, int n_frames, void* stream) {
    return adas::overlay_run_text("adas_overlay_run_text", h, d_frames_bgr, post, tracker, analysis, mask, TEXT_ALL, n_streams, n_frames, stream);
}

int adas_overlay_fetch_text_items(adas_overlay* h, int frame, adas_overlay_text_item* items, int max_items, int32_t* n_items) {
    const char* who = "adas_overlay_fetch_text_items";
    adas::overlay_text* s = h ? *adas::overlay_text_slot(h) : nullptr;
    ADAS_REQUIRE(s && n_items && (items || max_items <= 0), ADAS_ERR_INVALID, "%s: no text set, or a null argument", who);
    ADAS_REQUIRE(frame >= 0 && frame < s->run_frames, ADAS_ERR_INVALID, "%s: frame %d was not part of the last text run (%d frames)", who, frame, s->run_frames);
    ADAS_HIP_TRY(hipDeviceSynchronize());
    int head[4];
    ADAS_HIP_TRY(hipMemcpy(head, s->heads + (size_t)frame * 4, sizeof(head), hipMemcpyDeviceToHost));
    *n_items = head[0];
    const int n = head[0] < max_items ? head[0] : max_items;
    if (n > 0) ADAS_HIP_TRY(hipMemcpy(items, s->items + (size_t)frame * s->max_items, (size_t)n * sizeof(TextItem), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_overlay_fetch_text_flags(adas_overlay* h, int frame, int32_t* flags) {
    const char* who = "adas_overlay_fetch_text_flags";
    adas::overlay_text* s = h ? *adas::overlay_text_slot(h) : nullptr;
    ADAS_REQUIRE(s && flags, ADAS_ERR_INVALID, "%s: no text set, or a null argument", who);
    ADAS_REQUIRE(frame >= 0 && frame < s->run_frames, ADAS_ERR_INVALID, "%s: frame %d was not part of the last text run (%d frames)", who, frame, s->run_frames);
    ADAS_HIP_TRY(hipDeviceSynchronize());
    ADAS_HIP_TRY(hipMemcpy(flags, s->heads + (size_t)frame * 4 + 1, 4, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

}  // extern "C"
