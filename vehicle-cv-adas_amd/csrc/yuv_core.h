// yuv_core.h -- uncompressed camera formats into BGR: the rules of adas_yuv_* and the byte addresses of every load and store its work items
// make, shared by the HIP kernels (yuv_kernels.hip) and a host build (tests/hostemu/emu_yuv.cpp) so that an indexing mistake shows on the CPU.
// What a reference user's host code does with cv2.cvtColor(frame, COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YUY2 / _UYVY) before the loop sees a
// frame (the reference hides it in cv2.VideoCapture.read(), demo.py:220, videoDetection.py:14).  The rules below are the authority: parity
// with a real cv2 build is unpinned -- cv2 was not available where this was written, the constants of C4 are the ones OpenCV's colour
// conversion publishes for its 20-bit integer path, and tests/yuv_ref.py restates C1-C6 independently in NumPy.
//
//   C1 formats    width even for every format.  (x, y) is a pixel, the chroma sample it uses is the one at
//                   NV12   Y plane, then one plane of interleaved U,V pairs (4:2:0); height even; (x >> 1, y >> 1)
//                   NV21   as NV12 with V,U pairs;                                    height even; (x >> 1, y >> 1)
//                   I420   Y plane, U plane, V plane (4:2:0); YV12 is I420 with the two chroma offsets swapped by the caller;
//                                                                                     height even; (x >> 1, y >> 1)
//                   YUYV   packed 4:2:2, bytes Y0 U Y1 V;                             any height;  (x >> 1, y)
//                   UYVY   packed 4:2:2, bytes U Y0 V Y1;                             any height;  (x >> 1, y)
//   C2 layout     described by bytes, never assumed tight: frame f starts f * frame_stride bytes behind the source pointer; inside a frame a
//                 plane starts at its offset and its rows lie one pitch apart (y_offset / y_pitch, u_offset / u_pitch, v_offset / v_pitch).
//                 NV12 / NV21 use the u_* pair for the interleaved plane, the packed formats the y_* pair only; the unused pairs are
//                 ignored.  yuv_default fills the tight layout.  yuv_check refuses by name: odd width, odd height for 4:2:0, a pitch
//                 shorter than a row, a plane that starts in front of or ends behind the frame, planes that overlap.
//   C3 siting     replication only: every pixel of a chroma sample's 2x2 (4:2:0) or 2x1 (4:2:2) cell takes that sample, no interpolation.
//   C4 `video`    BT.601 limited range in 20-bit integers: u = U - 128, v = V - 128, y = max(0, Y - 16) * 1220542, half = 1 << 19,
//                   B = (y + half + 2116026 u) >> 20,  G = (y + half - 852492 v - 409993 u) >> 20,  R = (y + half + 1673527 v) >> 20,
//                 arithmetic shifts (floor), each clamped to 0..255.  int32 holds all of it: y <= 239 * 1220542 = 291709538, the chroma
//                 sums lie in [-2116026 * 128, 2116026 * 127] = [-270851328, 268735302] for B, within +-161598080 for G and +-214211456
//                 for R, so every sum in front of a shift lies inside [-271 * 10^6, 561 * 10^6], well inside +-2^31.
//   C5 `full`     JFIF full range: rule D8 of jpegdec_core.h, evaluated by calling jd_colour (Y, Cb = U, Cr = V) -- not restated here.
//   C6 output     BGR u8 [batch][h][w][3], tightly packed: what adas_pipeline_step_frames takes.  A frame's output depends on that frame's
//                 bytes and the handle's parameters alone.
//   C7 addressing the functions below give the byte offset of every access: yuv_y_at / yuv_u_at / yuv_v_at (a pixel's three source bytes
//                 inside its frame), yuv_dst_at (its three output bytes inside its frame), yuv_split (a row into 16-pixel vector groups and a
//                 tail of 2-pixel cells) and yuv_item_x (the first pixel of an item).  A work item is one cell column of one row unit (a row
//                 pair for 4:2:0, a row for 4:2:2):
//                   vector group   16 pixels x the unit's rows.  4:2:0: two 16-byte Y loads, one 16-byte chroma load (NV12 / NV21) or two
//                                  8-byte loads (I420), six 16-byte stores.  4:2:2: two 16-byte loads, three 16-byte stores.
//                   generic cell   one chroma sample's pixels (2x2 or 2x1), byte accesses, no alignment assumed, nothing read behind a row's
//                                  bytes or a plane's last row.
//                 yuv_vector_ok decides for a whole run: every address a group touches is a multiple of its access width exactly when w,
//                 the pitches and offsets in use, frame_stride and both base pointers are multiples of 16 (of 8 for I420's two chroma
//                 planes, which are read 8 bytes at a time).  (The destination is tight, so its rows start on multiples of
//                 16 only when w % 16 == 0: with any other width the whole frame goes through generic cells.  yuv_split is nevertheless
//                 written for any w, groups first and the tail behind them.)  Both paths produce the same bytes.
#pragma once
#include <stdint.h>
#include <string.h>
#include "jpegdec_core.h"

namespace adas {

#define YUV_NV12 0
#define YUV_NV21 1
#define YUV_I420 2
#define YUV_YUYV 3
#define YUV_UYVY 4
#define YUV_FORMATS 5
#define YUV_MATRIX_VIDEO 0
#define YUV_MATRIX_FULL 1

// yuv_check's verdicts
#define YUV_OK 0
#define YUV_BAD_FORMAT 1
#define YUV_BAD_MATRIX 2
#define YUV_BAD_SIZE 3
#define YUV_ODD_WIDTH 4
#define YUV_ODD_HEIGHT 5
#define YUV_SHORT_PITCH 6
#define YUV_OUTSIDE 7
#define YUV_OVERLAP 8

#define YUV_MAX_DIM 65534
#define YUV_GROUP 16   // pixels of a vector group

// adas_yuv_params, field for field (yuv_kernels.hip asserts it)
struct YuvGeom {
    int32_t format, matrix, w, h;
    int64_t frame_stride, y_offset, y_pitch, u_offset, u_pitch, v_offset, v_pitch;
};

ADAS_HDI bool yuv_is420(int format) { return format == YUV_NV12 || format == YUV_NV21 || format == YUV_I420; }
ADAS_HDI bool yuv_packed(int format) { return format == YUV_YUYV || format == YUV_UYVY; }
ADAS_HDI int yuv_planes(int format) { return format == YUV_I420 ? 3 : (yuv_packed(format) ? 1 : 2); }
// rows of plane k (0 the Y or packed plane, 1 U or UV, 2 V) and the bytes of one of its rows
ADAS_HDI long long yuv_plane_rows(int format, int h, int k) { return k == 0 ? h : h / 2; }
ADAS_HDI long long yuv_plane_row_bytes(int format, int w, int k) {
    if (k == 0) return yuv_packed(format) ? 2LL * w : w;
    return format == YUV_I420 ? w / 2 : w;
}
ADAS_HDI long long yuv_out_bytes(int w, int h) { return (long long)w * h * 3; }

// C2: the tight layout
ADAS_HDI void yuv_default(YuvGeom* g, int format, int w, int h) {
    g->format = format;
    g->matrix = YUV_MATRIX_VIDEO;
    g->w = w;
    g->h = h;
    const long long wy = yuv_plane_row_bytes(format, w, 0), wc = yuv_plane_row_bytes(format, w, 1);
    g->y_offset = 0;
    g->y_pitch = wy;
    g->u_offset = g->u_pitch = g->v_offset = g->v_pitch = 0;
    long long end = wy * h;
    if (yuv_planes(format) >= 2) {
        g->u_offset = end;
        g->u_pitch = wc;
        end += wc * (h / 2);
    }
    if (yuv_planes(format) == 3) {
        g->v_offset = end;
        g->v_pitch = wc;
        end += wc * (h / 2);
    }
    g->frame_stride = end;
}

ADAS_HDI void yuv_plane(const YuvGeom& g, int k, long long* off, long long* pitch) {
    *off = k == 0 ? g.y_offset : (k == 1 ? g.u_offset : g.v_offset);
    *pitch = k == 0 ? g.y_pitch : (k == 1 ? g.u_pitch : g.v_pitch);
}

// C1, C2: YUV_OK or why not
ADAS_HDI int yuv_check(const YuvGeom& g) {
    if (g.format < 0 || g.format >= YUV_FORMATS) return YUV_BAD_FORMAT;
    if (g.matrix != YUV_MATRIX_VIDEO && g.matrix != YUV_MATRIX_FULL) return YUV_BAD_MATRIX;
    if (g.w < 1 || g.h < 1 || g.w > YUV_MAX_DIM || g.h > YUV_MAX_DIM) return YUV_BAD_SIZE;
    if (g.w & 1) return YUV_ODD_WIDTH;
    if (yuv_is420(g.format) && (g.h & 1)) return YUV_ODD_HEIGHT;
    const int np = yuv_planes(g.format);
    long long lo[3], hi[3];
    for (int k = 0; k < np; ++k) {
        long long off, pitch;
        yuv_plane(g, k, &off, &pitch);
        const long long rb = yuv_plane_row_bytes(g.format, g.w, k), rows = yuv_plane_rows(g.format, g.h, k);
        if (pitch < rb) return YUV_SHORT_PITCH;
        if (pitch > ((long long)1 << 40) || off > ((long long)1 << 50)) return YUV_OUTSIDE;
        lo[k] = off;
        hi[k] = off + (rows - 1) * pitch + rb;
        if (off < 0 || g.frame_stride < 1 || hi[k] > g.frame_stride) return YUV_OUTSIDE;
    }
    for (int a = 0; a < np; ++a)
        for (int b = a + 1; b < np; ++b)
            if (lo[a] < hi[b] && lo[b] < hi[a]) return YUV_OVERLAP;
    return YUV_OK;
}

// the bytes of a frame that are read: up to the end of its last plane (the last frame of a batch needs no more than these)
ADAS_HDI long long yuv_frame_extent(const YuvGeom& g) {
    long long end = 0;
    for (int k = 0; k < yuv_planes(g.format); ++k) {
        long long off, pitch;
        yuv_plane(g, k, &off, &pitch);
        const long long e = off + (yuv_plane_rows(g.format, g.h, k) - 1) * pitch + yuv_plane_row_bytes(g.format, g.w, k);
        end = e > end ? e : end;
    }
    return end;
}

// ------------------------------------------------------------------------------------------------------------- C7: where the bytes are
// pixel (x, y)'s Y, U and V byte inside its frame
ADAS_HDI long long yuv_y_at(const YuvGeom& g, int x, int y) {
    if (g.format == YUV_YUYV) return g.y_offset + (long long)y * g.y_pitch + 2LL * x;
    if (g.format == YUV_UYVY) return g.y_offset + (long long)y * g.y_pitch + 2LL * x + 1;
    return g.y_offset + (long long)y * g.y_pitch + x;
}
ADAS_HDI long long yuv_u_at(const YuvGeom& g, int x, int y) {
    const int cx = x >> 1;
    switch (g.format) {
        case YUV_NV12: return g.u_offset + (long long)(y >> 1) * g.u_pitch + 2LL * cx;
        case YUV_NV21: return g.u_offset + (long long)(y >> 1) * g.u_pitch + 2LL * cx + 1;
        case YUV_I420: return g.u_offset + (long long)(y >> 1) * g.u_pitch + cx;
        case YUV_YUYV: return g.y_offset + (long long)y * g.y_pitch + 4LL * cx + 1;
        default: return g.y_offset + (long long)y * g.y_pitch + 4LL * cx;
    }
}
ADAS_HDI long long yuv_v_at(const YuvGeom& g, int x, int y) {
    const int cx = x >> 1;
    switch (g.format) {
        case YUV_NV12: return g.u_offset + (long long)(y >> 1) * g.u_pitch + 2LL * cx + 1;
        case YUV_NV21: return g.u_offset + (long long)(y >> 1) * g.u_pitch + 2LL * cx;
        case YUV_I420: return g.v_offset + (long long)(y >> 1) * g.v_pitch + cx;
        case YUV_YUYV: return g.y_offset + (long long)y * g.y_pitch + 4LL * cx + 3;
        default: return g.y_offset + (long long)y * g.y_pitch + 4LL * cx + 2;
    }
}
// pixel (x, y)'s B byte inside its (tight) destination frame
ADAS_HDI long long yuv_dst_at(const YuvGeom& g, int x, int y) { return ((long long)y * g.w + x) * 3; }

// a row into ngroups vector groups of 16 pixels from x = 0 and ntail generic cells of 2 pixels behind them
ADAS_HDI void yuv_split(int w, bool vec, int* ngroups, int* ntail) {
    *ngroups = vec ? w / YUV_GROUP : 0;
    *ntail = (w - *ngroups * YUV_GROUP) / 2;
}
ADAS_HDI int yuv_item_x(int i, int ngroups) { return i < ngroups ? i * YUV_GROUP : ngroups * YUV_GROUP + 2 * (i - ngroups); }
ADAS_HDI int yuv_unit_rows(int format) { return yuv_is420(format) ? 2 : 1; }
ADAS_HDI long long yuv_items_per_frame(const YuvGeom& g, bool vec) {
    int ng, nt;
    yuv_split(g.w, vec, &ng, &nt);
    return (long long)(ng + nt) * (g.h / yuv_unit_rows(g.format));
}

ADAS_HDI bool yuv_vector_ok(const YuvGeom& g, const void* src, const void* dst) {
    long long m = (long long)(uintptr_t)src | (long long)(uintptr_t)dst | g.w | g.frame_stride | g.y_offset | g.y_pitch;
    if (yuv_planes(g.format) == 2) m |= g.u_offset | g.u_pitch;
    if (yuv_planes(g.format) == 3) m |= (g.u_offset | g.u_pitch | g.v_offset | g.v_pitch) << 1;   // 8-byte loads: multiples of 8 will do
    return (m & 15) == 0;
}

// ------------------------------------------------------------------------------------------------------------------ memory accesses
// Every load and store of an item goes through these.  A host build that defines YUV_AUDIT sees each one's address, width and required
// alignment (yuv_audit) before it happens, and an access it answers with false does not happen (a load then gives zeros).
struct Yuv16 {
    uint32_t w[4];
};
#if defined(YUV_AUDIT) && !defined(__HIP_DEVICE_COMPILE__)
bool yuv_audit(const void* p, int bytes, int align, int store);
#define YUV_AUDIT_CALL(p, n, a, s) yuv_audit(p, n, a, s)
#else
#define YUV_AUDIT_CALL(p, n, a, s) true
#endif

ADAS_HDI Yuv16 yuv_ld16(const uint8_t* p) {
    Yuv16 v;
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    if (!YUV_AUDIT_CALL(p, 16, 16, 0)) return v;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 q = *(const uint4*)p;
    v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
#else
    memcpy(v.w, p, 16);
#endif
    return v;
}
// 8 bytes into words 0 and 1
ADAS_HDI Yuv16 yuv_ld8x8(const uint8_t* p) {
    Yuv16 v;
    v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    if (!YUV_AUDIT_CALL(p, 8, 8, 0)) return v;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint2 q = *(const uint2*)p;
    v.w[0] = q.x; v.w[1] = q.y;
#else
    memcpy(v.w, p, 8);
#endif
    return v;
}
ADAS_HDI void yuv_st16(uint8_t* p, const uint32_t* w) {
    if (!YUV_AUDIT_CALL(p, 16, 16, 1)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
#else
    memcpy(p, w, 16);
#endif
}
ADAS_HDI int yuv_ld1(const uint8_t* p) {
    if (!YUV_AUDIT_CALL(p, 1, 1, 0)) return 0;
    return *p;
}
ADAS_HDI void yuv_st1(uint8_t* p, int v) {
    if (!YUV_AUDIT_CALL(p, 1, 1, 1)) return;
    *p = (uint8_t)v;
}
// byte k (0..15) of a 16-byte piece, as it lies in memory (little endian words)
ADAS_HDI int yuv_byte(const Yuv16& v, int k) { return (int)((v.w[k >> 2] >> ((k & 3) * 8)) & 255u); }

// ------------------------------------------------------------------------------------------------------------------ C4, C5: a pixel
ADAS_HDI int yuv_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// clamp(s >> 20, 0, 255), evaluated as clamp(s, 0, 2^28 - 1) >> 20: the same number for every s, since s >> 20 is monotonic, is below 0
// exactly for s < 0 and above 255 exactly for s >= 2^28.  Written this way on purpose: from "shift, then clamp, then pack two bytes" hipcc
// (ROCm 7.2) forms gfx950's v_ashr_pk_u8_i32 and ORs its result with the word's other two bytes; built that way the device's vector groups
// carried stray bits in exactly those two bytes of a word while the host build of the same source was right ("YUV input").
ADAS_HDI int yuv_sat20(int s) {
    const int c = s < 0 ? 0 : (s > (1 << 28) - 1 ? (1 << 28) - 1 : s);
    return (int)((uint32_t)c >> 20);
}
ADAS_HDI void yuv_video(int Y, int U, int V, int* bgr) {
    const int u = U - 128, v = V - 128;
    const int y = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19);
    bgr[0] = yuv_sat20(y + 2116026 * u);
    bgr[1] = yuv_sat20(y - 852492 * v - 409993 * u);
    bgr[2] = yuv_sat20(y + 1673527 * v);
}
template <int MATRIX>
ADAS_HDI void yuv_colour(int Y, int U, int V, int* bgr) {
    if (MATRIX == YUV_MATRIX_FULL)
        jd_colour(Y, U, V, bgr);
    else
        yuv_video(Y, U, V, bgr);
}

// ------------------------------------------------------------------------------------------------------------------ the work items
// one generic cell: the pixels (x, y0) ... (x + 1, y0 + rows - 1) of frame `src` into frame `dst`
template <int MATRIX>
ADAS_HDI void yuv_cell(const YuvGeom& g, const uint8_t* src, uint8_t* dst, int x, int y0) {
    const int U = yuv_ld1(src + yuv_u_at(g, x, y0)), V = yuv_ld1(src + yuv_v_at(g, x, y0));
    const int rows = yuv_unit_rows(g.format);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < 2; ++k) {
            int bgr[3];
            yuv_colour<MATRIX>(yuv_ld1(src + yuv_y_at(g, x + k, y0 + r)), U, V, bgr);
            uint8_t* o = dst + yuv_dst_at(g, x + k, y0 + r);
            for (int c = 0; c < 3; ++c) yuv_st1(o + c, bgr[c]);
        }
}

// 16 pixels of one row from their Y bytes and the 8 chroma pairs: three 16-byte stores
template <int MATRIX>
ADAS_HDI void yuv_group_row(const int* Y, const int* U, const int* V, uint8_t* o) {
    uint32_t out[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int bgr[3];
        yuv_colour<MATRIX>(Y[k], U[k >> 1], V[k >> 1], bgr);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int b = k * 3 + c;
            out[b >> 2] |= (uint32_t)bgr[c] << ((b & 3) * 8);
        }
    }
    yuv_st16(o, out);
    yuv_st16(o + 16, out + 4);
    yuv_st16(o + 32, out + 8);
}

// one vector group: the pixels (x0, y0) ... (x0 + 15, y0 + rows - 1); FORMAT is g.format
template <int FORMAT, int MATRIX>
ADAS_HDI void yuv_group(const YuvGeom& g, const uint8_t* src, uint8_t* dst, int x0, int y0) {
    int Y[16], U[8], V[8];
    if (FORMAT == YUV_YUYV || FORMAT == YUV_UYVY) {
        const uint8_t* p = src + g.y_offset + (long long)y0 * g.y_pitch + 2LL * x0;   // = the lower of yuv_y_at and yuv_u_at of (x0, y0)
        const Yuv16 a = yuv_ld16(p), b = yuv_ld16(p + 16);
        const int yo = FORMAT == YUV_YUYV ? 0 : 1, uo = FORMAT == YUV_YUYV ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            Y[k] = yuv_byte(a, 2 * k + yo);
            Y[8 + k] = yuv_byte(b, 2 * k + yo);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            U[k] = yuv_byte(a, 4 * k + uo);
            V[k] = yuv_byte(a, 4 * k + uo + 2);
            U[4 + k] = yuv_byte(b, 4 * k + uo);
            V[4 + k] = yuv_byte(b, 4 * k + uo + 2);
        }
        yuv_group_row<MATRIX>(Y, U, V, dst + yuv_dst_at(g, x0, y0));
        return;
    }
    if (FORMAT == YUV_I420) {
        const Yuv16 u = yuv_ld8x8(src + yuv_u_at(g, x0, y0)), v = yuv_ld8x8(src + yuv_v_at(g, x0, y0));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            U[k] = yuv_byte(u, k);
            V[k] = yuv_byte(v, k);
        }
    } else {
        const Yuv16 c = yuv_ld16(src + g.u_offset + (long long)(y0 >> 1) * g.u_pitch + x0);   // = the lower of yuv_u_at and yuv_v_at of (x0, y0)
        const int uo = FORMAT == YUV_NV12 ? 0 : 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            U[k] = yuv_byte(c, 2 * k + uo);
            V[k] = yuv_byte(c, 2 * k + 1 - uo);
        }
    }
    const Yuv16 a = yuv_ld16(src + yuv_y_at(g, x0, y0)), b = yuv_ld16(src + yuv_y_at(g, x0, y0 + 1));
#pragma unroll
    for (int k = 0; k < 16; ++k) Y[k] = yuv_byte(a, k);
    yuv_group_row<MATRIX>(Y, U, V, dst + yuv_dst_at(g, x0, y0));
#pragma unroll
    for (int k = 0; k < 16; ++k) Y[k] = yuv_byte(b, k);
    yuv_group_row<MATRIX>(Y, U, V, dst + yuv_dst_at(g, x0, y0 + 1));
}

// item t (0 <= t < yuv_items_per_frame, which fits 31 bits: at most 32767 cells x 65534 rows) of frame f: src and dst are the run's base
// pointers; FORMAT is g0.format
template <int FORMAT, int MATRIX>
ADAS_HDI void yuv_item(const YuvGeom& g0, bool vec, const uint8_t* src, uint8_t* dst, int f, uint32_t t) {
    YuvGeom g = g0;
    g.format = FORMAT;   // the address functions fold their switch
    int ng, nt;
    yuv_split(g.w, vec, &ng, &nt);
    const uint32_t per_row = (uint32_t)(ng + nt);
    const int unit = (int)(t / per_row), i = (int)(t - (uint32_t)unit * per_row);
    const uint8_t* s = src + (long long)f * g.frame_stride;
    uint8_t* d = dst + (long long)f * yuv_out_bytes(g.w, g.h);
    const int x = yuv_item_x(i, ng), y0 = unit * yuv_unit_rows(FORMAT);
    if (i < ng)
        yuv_group<FORMAT, MATRIX>(g, s, d, x, y0);
    else
        yuv_cell<MATRIX>(g, s, d, x, y0);
}

}  // namespace adas
