// Host build of the YUV conversion's rules (csrc/yuv_core.h; g++, one thread): the work items the device kernel runs -- yuv_item over every
// frame and item index, through the same address functions (C7) -- with every load and store audited: its bytes must lie inside the source
// or destination array the caller handed over (an access outside is counted and not made), and a 16- or 8-byte access must be aligned as
// the device needs it.  The CPU suite compares the frames with tests/yuv_ref.py, the GPU suite the device's frames with these.  Test
// scaffolding only; never loaded by the product.
#include <stddef.h>
#define YUV_AUDIT 1
#include "yuv_core.h"

using namespace adas;

namespace {
struct Audit {
    const uint8_t *src_lo = nullptr, *src_hi = nullptr;
    uint8_t *dst_lo = nullptr, *dst_hi = nullptr;
    long long outside = 0, misaligned = 0, loads = 0, stores = 0, wide = 0;
} A;
}  // namespace

namespace adas {
bool yuv_audit(const void* p, int bytes, int align, int store) {
    const uint8_t* q = (const uint8_t*)p;
    const uint8_t* lo = store ? A.dst_lo : A.src_lo;
    const uint8_t* hi = store ? A.dst_hi : A.src_hi;
    const bool inside = q >= lo && q + bytes <= hi;
    if (!inside) ++A.outside;
    if ((uintptr_t)q % (uintptr_t)align) ++A.misaligned;
    if (bytes > 1) ++A.wide;
    ++(store ? A.stores : A.loads);
    return inside;   // an access outside is counted, not made
}
}  // namespace adas

namespace {
template <int FORMAT>
void run_items(const YuvGeom& g, bool vec, const uint8_t* src, uint8_t* dst, int batch) {
    const uint32_t items = (uint32_t)yuv_items_per_frame(g, vec);
    for (int f = 0; f < batch; ++f)
        for (uint32_t t = 0; t < items; ++t) {
            if (g.matrix == YUV_MATRIX_FULL)
                yuv_item<FORMAT, YUV_MATRIX_FULL>(g, vec, src, dst, f, t);
            else
                yuv_item<FORMAT, YUV_MATRIX_VIDEO>(g, vec, src, dst, f, t);
        }
}
}  // namespace

extern "C" {

// sizeof and the offsets of format, matrix, w, h, frame_stride, y_offset, y_pitch, u_offset, u_pitch, v_offset, v_pitch
void emu_yuv_params_layout(int* out) {
    const int v[12] = {(int)sizeof(YuvGeom),
                       (int)offsetof(YuvGeom, format),
                       (int)offsetof(YuvGeom, matrix),
                       (int)offsetof(YuvGeom, w),
                       (int)offsetof(YuvGeom, h),
                       (int)offsetof(YuvGeom, frame_stride),
                       (int)offsetof(YuvGeom, y_offset),
                       (int)offsetof(YuvGeom, y_pitch),
                       (int)offsetof(YuvGeom, u_offset),
                       (int)offsetof(YuvGeom, u_pitch),
                       (int)offsetof(YuvGeom, v_offset),
                       (int)offsetof(YuvGeom, v_pitch)};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

void emu_yuv_default(YuvGeom* g, int format, int w, int h) { yuv_default(g, format, w, h); }
int emu_yuv_check(const YuvGeom* g) { return yuv_check(*g); }
long long emu_yuv_frame_bytes(const YuvGeom* g) { return yuv_check(*g) == YUV_OK ? yuv_frame_extent(*g) : 0; }

// C4 / C5 alone: n triples -> bgr [n][3]
void emu_yuv_colour(int matrix, const uint8_t* Y, const uint8_t* U, const uint8_t* V, long long n, uint8_t* bgr) {
    for (long long i = 0; i < n; ++i) {
        int p[3];
        if (matrix == YUV_MATRIX_FULL)
            yuv_colour<YUV_MATRIX_FULL>(Y[i], U[i], V[i], p);
        else
            yuv_colour<YUV_MATRIX_VIDEO>(Y[i], U[i], V[i], p);
        for (int c = 0; c < 3; ++c) bgr[i * 3 + c] = (uint8_t)p[c];
    }
}

// A run as adas_yuv_run makes it: `batch` frames from src into dst, walking every work item.  [src, src + src_bytes) and [dst, dst + dst_bytes)
// are what the items may touch.  path: -1 as yuv_vector_ok decides, 0 generic cells.  info [6] = vector path taken, accesses outside,
// misaligned accesses, loads, stores, accesses wider than a byte.  Returns yuv_check's verdict (nothing runs unless it is 0).
int emu_yuv_run(const YuvGeom* gp, const uint8_t* src, long long src_bytes, uint8_t* dst, long long dst_bytes, int batch, int path, long long* info) {
    const YuvGeom g = *gp;
    const int why = yuv_check(g);
    if (why != YUV_OK) return why;
    const bool vec = path != 0 && yuv_vector_ok(g, src, dst);
    A = Audit();
    A.src_lo = src;
    A.src_hi = src + src_bytes;
    A.dst_lo = dst;
    A.dst_hi = dst + dst_bytes;
    switch (g.format) {
        case YUV_NV12: run_items<YUV_NV12>(g, vec, src, dst, batch); break;
        case YUV_NV21: run_items<YUV_NV21>(g, vec, src, dst, batch); break;
        case YUV_I420: run_items<YUV_I420>(g, vec, src, dst, batch); break;
        case YUV_YUYV: run_items<YUV_YUYV>(g, vec, src, dst, batch); break;
        default: run_items<YUV_UYVY>(g, vec, src, dst, batch); break;
    }
    if (info) {
        const long long v[6] = {vec ? 1 : 0, A.outside, A.misaligned, A.loads, A.stores, A.wide};
        for (int i = 0; i < 6; ++i) info[i] = v[i];
    }
    return YUV_OK;
}

}  // extern "C"
