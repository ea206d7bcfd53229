// Host build of the YUV output's rules (csrc/yuvout_core.h; g++, one thread): the work items the device kernel runs -- yuvout_item over every
// frame and item index, through the same address functions (E7) -- with every load and store audited: a load must lie inside one row of one
// source frame, a store inside one plane row of one destination frame (an access that does not is counted and not made), both inside the
// arrays the caller handed over, and a 16- or 8-byte access must be aligned as the device needs it.  The CPU suite compares the frames with
// tests/yuvout_ref.py, the GPU suite the device's frames with these.  Test scaffolding only; never loaded by the product.
#include <stddef.h>
#define YUV_AUDIT 1
#include "yuvout_core.h"

using namespace adas;

namespace {
struct Audit {
    YuvGeom g;
    int batch = 0;
    const uint8_t *src = nullptr, *src_hi = nullptr;
    uint8_t *dst = nullptr, *dst_hi = nullptr;
    long long outside = 0, misaligned = 0, loads = 0, stores = 0, wide = 0, off_row = 0;
} A;

// [o, o + bytes) of the source lies in one row of one frame
bool in_source_row(long long o, int bytes) {
    const long long row = (long long)A.g.w * 3, fb = row * A.g.h;
    if (o < 0 || o + bytes > fb * A.batch) return false;
    return o / row == (o + bytes - 1) / row;
}
// [o, o + bytes) of the destination lies in one row of one plane of one frame
bool in_plane_row(long long o, int bytes) {
    if (o < 0) return false;
    const long long f = o / A.g.frame_stride, in = o - f * A.g.frame_stride;
    if (f >= A.batch) return false;
    for (int k = 0; k < yuv_planes(A.g.format); ++k) {
        long long off, pitch;
        yuv_plane(A.g, k, &off, &pitch);
        const long long rb = yuv_plane_row_bytes(A.g.format, A.g.w, k), rows = yuv_plane_rows(A.g.format, A.g.h, k);
        if (in < off) continue;
        const long long r = pitch ? (in - off) / pitch : 0;
        if (r >= rows) continue;
        const long long c = in - off - r * pitch;
        if (c + bytes <= rb) return true;
    }
    return false;
}
}  // namespace

namespace adas {
bool yuv_audit(const void* p, int bytes, int align, int store) {
    const uint8_t* q = (const uint8_t*)p;
    const uint8_t* lo = store ? A.dst : A.src;
    const uint8_t* hi = store ? A.dst_hi : A.src_hi;
    const bool inside = q >= lo && q + bytes <= hi;
    const bool row = inside && (store ? in_plane_row(q - lo, bytes) : in_source_row(q - lo, bytes));
    if (!inside) ++A.outside;
    if (inside && !row) ++A.off_row;
    if ((uintptr_t)q % (uintptr_t)align) ++A.misaligned;
    if (bytes > 1) ++A.wide;
    ++(store ? A.stores : A.loads);
    return inside && row;   // any other access is counted, not made
}
}  // namespace adas

namespace {
template <int FORMAT>
void run_items(const YuvGeom& g, int chroma, bool vec, const uint8_t* src, uint8_t* dst, int batch) {
    const uint32_t items = (uint32_t)yuvout_items_per_frame(g, vec);
    for (int f = 0; f < batch; ++f)
        for (uint32_t t = 0; t < items; ++t) {
            if (g.matrix == YUV_MATRIX_FULL)
                yuvout_item<FORMAT, YUV_MATRIX_FULL>(g, chroma, vec, src, dst, f, t);
            else
                yuvout_item<FORMAT, YUV_MATRIX_VIDEO>(g, chroma, vec, src, dst, f, t);
        }
}
}  // namespace

extern "C" {

// sizeof and the offsets of format, matrix, w, h, frame_stride, y_offset, y_pitch, u_offset, u_pitch, v_offset, v_pitch, chroma
void emu_yuvout_params_layout(int* out) {
    const int v[13] = {(int)sizeof(YuvOutParams),
                       (int)offsetof(YuvOutParams, g.format),
                       (int)offsetof(YuvOutParams, g.matrix),
                       (int)offsetof(YuvOutParams, g.w),
                       (int)offsetof(YuvOutParams, g.h),
                       (int)offsetof(YuvOutParams, g.frame_stride),
                       (int)offsetof(YuvOutParams, g.y_offset),
                       (int)offsetof(YuvOutParams, g.y_pitch),
                       (int)offsetof(YuvOutParams, g.u_offset),
                       (int)offsetof(YuvOutParams, g.u_pitch),
                       (int)offsetof(YuvOutParams, g.v_offset),
                       (int)offsetof(YuvOutParams, g.v_pitch),
                       (int)offsetof(YuvOutParams, chroma)};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
}

void emu_yuvout_default(YuvOutParams* p, int format, int w, int h) {
    yuv_default(&p->g, format, w, h);
    p->chroma = YUVOUT_CHROMA_MEAN;
}
int emu_yuvout_check(const YuvOutParams* p) { return yuvout_check(p->g, p->chroma); }
long long emu_yuvout_frame_bytes(const YuvOutParams* p) { return yuvout_check(p->g, p->chroma) == YUV_OK ? yuv_frame_extent(p->g) : 0; }

// E3 / E4 alone: n BGR triples -> yuv [n][3]
void emu_yuvout_colour(int matrix, const uint8_t* bgr, long long n, uint8_t* yuv) {
    for (long long i = 0; i < n; ++i) {
        int p[3];
        if (matrix == YUV_MATRIX_FULL)
            yuvout_colour<YUV_MATRIX_FULL>(bgr[i * 3], bgr[i * 3 + 1], bgr[i * 3 + 2], p);
        else
            yuvout_colour<YUV_MATRIX_VIDEO>(bgr[i * 3], bgr[i * 3 + 1], bgr[i * 3 + 2], p);
        for (int c = 0; c < 3; ++c) yuv[i * 3 + c] = (uint8_t)p[c];
    }
}

// the run's path for these two pointers, as yuvout_vector_ok decides
int emu_yuvout_vector_ok(const YuvOutParams* p, const void* src, const void* dst) { return yuvout_vector_ok(p->g, src, dst) ? 1 : 0; }

// A run as adas_yuvout_run makes it: `batch` frames from src into dst, walking every work item.  [src, src + src_bytes) and [dst, dst +
// dst_bytes) are what the items may touch.  path: -1 as yuvout_vector_ok decides, 0 generic cells.  info [7] = vector path taken, accesses
// outside the arrays, misaligned accesses, loads, stores, accesses wider than a byte, accesses inside the arrays but across or outside a
// row.  Returns yuvout_check's verdict (nothing runs unless it is 0).
int emu_yuvout_run(const YuvOutParams* pp, const uint8_t* src, long long src_bytes, uint8_t* dst, long long dst_bytes, int batch, int path,
                   long long* info) {
    const YuvGeom g = pp->g;
    const int why = yuvout_check(g, pp->chroma);
    if (why != YUV_OK) return why;
    const bool vec = path != 0 && yuvout_vector_ok(g, src, dst);
    A = Audit();
    A.g = g;
    A.batch = batch;
    A.src = src;
    A.src_hi = src + src_bytes;
    A.dst = dst;
    A.dst_hi = dst + dst_bytes;
    switch (g.format) {
        case YUV_NV12: run_items<YUV_NV12>(g, pp->chroma, vec, src, dst, batch); break;
        case YUV_NV21: run_items<YUV_NV21>(g, pp->chroma, vec, src, dst, batch); break;
        case YUV_I420: run_items<YUV_I420>(g, pp->chroma, vec, src, dst, batch); break;
        case YUV_YUYV: run_items<YUV_YUYV>(g, pp->chroma, vec, src, dst, batch); break;
        default: run_items<YUV_UYVY>(g, pp->chroma, vec, src, dst, batch); break;
    }
    if (info) {
        const long long v[7] = {vec ? 1 : 0, A.outside, A.misaligned, A.loads, A.stores, A.wide, A.off_row};
        for (int i = 0; i < 7; ++i) info[i] = v[i];
    }
    return YUV_OK;
}

}  // extern "C"
