// yuvout_core.h -- BGR frames into uncompressed video formats: the rules of adas_yuvout_* and the byte addresses of every load and store its
// work items make, shared by the HIP kernel (yuvout_kernels.hip) and a host build (tests/hostemu/emu_yuvout.cpp) so that an indexing mistake
// shows on the CPU.  The inverse of yuv_core.h: what cv2.VideoWriter.write(frame_show) (demo.py:314) does in front of its encoder, and what a
// caller's cv2.cvtColor(frame, COLOR_BGR2YUV_I420) or swscale does in front of any other one.  The rules below are the authority: parity with
// a real cv2 or swscale build is unpinned -- neither was available where this was written, the constants of E3 are the ones OpenCV's colour
// conversion publishes for its 20-bit integer path, and tests/yuvout_ref.py restates E1-E6 independently in NumPy.
//
//   E1 source      BGR u8 [batch][h][w][3], tightly packed: what the overlay, the step's camera frames, the JPEG decoder and the YUV converter
//                  hold.
//   E2 destination the five formats of yuv_core.h's rule C1 at the byte layout of its rule C2: YuvGeom now describes where the bytes go.
//                  frame_stride, y_/u_/v_offset and y_/u_/v_pitch as C2 has them, YV12 is I420 with the two chroma offsets exchanged, and
//                  yuv_check's refusals apply unchanged, by name.  A byte of the destination that belongs to no plane row (pitch padding, a
//                  gap between planes or frames) is never written.
//   E3 `video`     BT.601 limited range in 20-bit integers, half = 1 << 19:
//                    Y = ( 269484 R + 528482 G + 102760 B + half + (16 << 20)) >> 20
//                    U = (-155188 R - 305135 G + 460324 B + half + (128 << 20)) >> 20
//                    V = ( 460324 R - 385875 G -  74448 B + half + (128 << 20)) >> 20,   each clamped to 0..255.
//                  No input reaches the clamp: Y lies in 16..235, U and V in 16..240.  int32 holds all of it: the Y sum lies in
//                  [17301504, 246986634] (black, white), the U and the V sum in [(128 << 20) + half - 460323 * 255, (128 << 20) + half +
//                  460324 * 255] = [17359651, 252124636], so every sum in front of a shift lies inside [17301504, 252124636], well inside
//                  0 .. 2^28 - 1, which is also why the clamp never bites.
//   E4 `full`      JFIF full range: rule J2 of jpeg_core.h, evaluated by calling jpeg_luma / jpeg_cb / jpeg_cr -- not restated here.  There
//                  the clamp does bite: Cr of pure red is 256 in front of it.
//   E5 chroma      a cell is one chroma sample's pixels, 2x2 for 4:2:0 and 2x1 for 4:2:2.  Two modes:
//                    mean   (the default; what encoders' scalers do) U and V per pixel by E3 / E4, then (a + b + c + d + 2) >> 2 over the cell
//                           for 4:2:0, (a + b + 1) >> 1 for 4:2:2: jpeg_core.h's J3 form.
//                    first  U and V of the cell's first pixel (x even, and y even for 4:2:0) alone.
//   E6 determinism a frame's bytes depend on that frame's pixels and the handle's parameters alone.
//   E7 addressing  the functions below give the byte offset of every access: yuvout_src_at (a pixel's B byte inside its tight source frame),
//                  yuvout_y_at / yuvout_u_at / yuvout_v_at (its Y byte and its cell's U and V byte inside the destination frame: yuv_core.h's
//                  own), yuvout_split (a row into 16-pixel vector groups and a tail of 2-pixel cells) and yuvout_item_x (the first pixel of an
//                  item).  A work item is one cell column of one row unit (a row pair for 4:2:0, a row for 4:2:2):
//                    vector group   16 pixels x the unit's rows.  4:2:0: six 16-byte loads (two rows of 48 bytes), two 16-byte Y stores, one
//                                   16-byte interleaved chroma store (NV12 / NV21) or two 8-byte stores (I420).  4:2:2: three 16-byte loads,
//                                   two 16-byte stores.
//                    generic cell   one chroma sample's pixels (2x2 or 2x1), byte accesses, no alignment assumed, nothing read behind a row
//                                   and nothing written outside a plane row.
//                  yuvout_vector_ok decides for a whole run with yuv_vector_ok's conditions, source and destination exchanged: every address
//                  a group touches is a multiple of its access width exactly when w, the pitches and offsets in use, frame_stride and both
//                  base pointers are multiples of 16 (of 8 for I420's two chroma planes, which are written 8 bytes at a time).  (The source
//                  is tight, so its rows start on multiples of 16 only when w % 16 == 0: with any other width the whole frame goes through
//                  generic cells.  yuvout_split is nevertheless written for any w.)  Both paths write the same bytes.
#pragma once
#include <stdint.h>
#include <string.h>
#include "jpeg_core.h"
#include "yuv_core.h"

namespace adas {

#define YUVOUT_CHROMA_MEAN 0
#define YUVOUT_CHROMA_FIRST 1
#define YUVOUT_BAD_CHROMA 9   // behind yuv_check's verdicts

// adas_yuvout_params, field for field (yuvout_kernels.hip asserts it)
struct YuvOutParams {
    YuvGeom g;
    int32_t chroma;
};

ADAS_HDI int yuvout_check(const YuvGeom& g, int chroma) {
    const int why = yuv_check(g);
    if (why != YUV_OK) return why;
    return chroma == YUVOUT_CHROMA_MEAN || chroma == YUVOUT_CHROMA_FIRST ? YUV_OK : YUVOUT_BAD_CHROMA;
}

// ------------------------------------------------------------------------------------------------------------- E7: where the bytes are
// pixel (x, y)'s B byte inside its (tight) source frame
ADAS_HDI long long yuvout_src_at(const YuvGeom& g, int x, int y) { return ((long long)y * g.w + x) * 3; }
ADAS_HDI long long yuvout_src_bytes(int w, int h) { return (long long)w * h * 3; }
// pixel (x, y)'s Y byte and its cell's U and V byte inside the destination frame
ADAS_HDI long long yuvout_y_at(const YuvGeom& g, int x, int y) { return yuv_y_at(g, x, y); }
ADAS_HDI long long yuvout_u_at(const YuvGeom& g, int x, int y) { return yuv_u_at(g, x, y); }
ADAS_HDI long long yuvout_v_at(const YuvGeom& g, int x, int y) { return yuv_v_at(g, x, y); }

// a row into ngroups vector groups of 16 pixels from x = 0 and ntail generic cells of 2 pixels behind them
ADAS_HDI void yuvout_split(int w, bool vec, int* ngroups, int* ntail) { yuv_split(w, vec, ngroups, ntail); }
ADAS_HDI int yuvout_item_x(int i, int ngroups) { return yuv_item_x(i, ngroups); }
ADAS_HDI long long yuvout_items_per_frame(const YuvGeom& g, bool vec) { return yuv_items_per_frame(g, vec); }
// the same divisibility conditions with the two pointers exchanged: the tight BGR frames are now what is read
ADAS_HDI bool yuvout_vector_ok(const YuvGeom& g, const void* src, const void* dst) { return yuv_vector_ok(g, dst, src); }

// ------------------------------------------------------------------------------------------------------------------ memory accesses
// yuv_core.h's audited accesses (yuv_ld16, yuv_st16, yuv_ld1, yuv_st1) and an 8-byte store of words 0 and 1
ADAS_HDI void yuvout_st8(uint8_t* p, const uint32_t* w) {
    if (!YUV_AUDIT_CALL(p, 8, 8, 1)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint2*)p = make_uint2(w[0], w[1]);
#else
    memcpy(p, w, 8);
#endif
}

// ------------------------------------------------------------------------------------------------------------------ E3, E4: a pixel
// E3 through yuv_sat20, which clamps in front of its shift (yuv_core.h says why: shift, clamp, pack is the sequence hipcc got wrong)
ADAS_HDI void yuvout_video(int b, int g, int r, int* yuv) {
    const int half = 1 << 19;
    yuv[0] = yuv_sat20(269484 * r + 528482 * g + 102760 * b + half + (16 << 20));
    yuv[1] = yuv_sat20(-155188 * r - 305135 * g + 460324 * b + half + (128 << 20));
    yuv[2] = yuv_sat20(460324 * r - 385875 * g - 74448 * b + half + (128 << 20));
}
template <int MATRIX>
ADAS_HDI void yuvout_colour(int b, int g, int r, int* yuv) {
    if (MATRIX == YUV_MATRIX_FULL) {
        const JpegPx p{b, g, r};
        yuv[0] = jpeg_luma(p);
        yuv[1] = jpeg_cb(p);
        yuv[2] = jpeg_cr(p);
    } else {
        yuvout_video(b, g, r, yuv);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the work items
// one generic cell: the pixels (x, y0) ... (x + 1, y0 + rows - 1) of frame `src` into frame `dst`
template <int MATRIX>
ADAS_HDI void yuvout_cell(const YuvGeom& g, int chroma, const uint8_t* src, uint8_t* dst, int x, int y0) {
    const int rows = yuv_unit_rows(g.format);
    int su = 0, sv = 0, fu = 0, fv = 0;
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < 2; ++k) {
            const uint8_t* p = src + yuvout_src_at(g, x + k, y0 + r);
            const int b = yuv_ld1(p), gr = yuv_ld1(p + 1), rd = yuv_ld1(p + 2);
            int yuv[3];
            yuvout_colour<MATRIX>(b, gr, rd, yuv);
            yuv_st1(dst + yuvout_y_at(g, x + k, y0 + r), yuv[0]);
            su += yuv[1];
            sv += yuv[2];
            if (r == 0 && k == 0) {
                fu = yuv[1];
                fv = yuv[2];
            }
        }
    const int n = 2 * rows;   // E5: (sum + 2) >> 2 over four pixels, (sum + 1) >> 1 over two
    const int U = chroma == YUVOUT_CHROMA_FIRST ? fu : (su + n / 2) / n;
    const int V = chroma == YUVOUT_CHROMA_FIRST ? fv : (sv + n / 2) / n;
    yuv_st1(dst + yuvout_u_at(g, x, y0), U);
    yuv_st1(dst + yuvout_v_at(g, x, y0), V);
}

// 16 pixels of one row from their 48 bytes: Y[16] and the per-pixel U[16], V[16]
template <int MATRIX>
ADAS_HDI void yuvout_group_row(const uint8_t* p, int* Y, int* U, int* V) {
    const Yuv16 a = yuv_ld16(p), b = yuv_ld16(p + 16), c = yuv_ld16(p + 32);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int px[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int i = k * 3 + ch;
            px[ch] = i < 16 ? yuv_byte(a, i) : (i < 32 ? yuv_byte(b, i - 16) : yuv_byte(c, i - 32));
        }
        int yuv[3];
        yuvout_colour<MATRIX>(px[0], px[1], px[2], yuv);
        Y[k] = yuv[0];
        U[k] = yuv[1];
        V[k] = yuv[2];
    }
}

// n bytes (a multiple of 4, at most 32) into little-endian words
ADAS_HDI void yuvout_pack(const int* v, int n, uint32_t* w) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k)
        if (k < n) w[k >> 2] |= (uint32_t)v[k] << ((k & 3) * 8);
}

// one vector group: the pixels (x0, y0) ... (x0 + 15, y0 + rows - 1); FORMAT is g.format
template <int FORMAT, int MATRIX>
ADAS_HDI void yuvout_group(const YuvGeom& g, int chroma, const uint8_t* src, uint8_t* dst, int x0, int y0) {
    int Y[16], U[16], V[16], cu[8], cv[8];
    uint32_t w[8];
    const bool first = chroma == YUVOUT_CHROMA_FIRST;
    if (FORMAT == YUV_YUYV || FORMAT == YUV_UYVY) {
        yuvout_group_row<MATRIX>(src + yuvout_src_at(g, x0, y0), Y, U, V);
        int out[32];
        const int yo = FORMAT == YUV_YUYV ? 0 : 1, uo = FORMAT == YUV_YUYV ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            out[4 * k + yo] = Y[2 * k];
            out[4 * k + yo + 2] = Y[2 * k + 1];
            out[4 * k + uo] = first ? U[2 * k] : (U[2 * k] + U[2 * k + 1] + 1) >> 1;
            out[4 * k + uo + 2] = first ? V[2 * k] : (V[2 * k] + V[2 * k + 1] + 1) >> 1;
        }
        yuvout_pack(out, 32, w);
        uint8_t* o = dst + g.y_offset + (long long)y0 * g.y_pitch + 2LL * x0;   // = the lower of yuvout_y_at and yuvout_u_at of (x0, y0)
        yuv_st16(o, w);
        yuv_st16(o + 16, w + 4);
        return;
    }
    yuvout_group_row<MATRIX>(src + yuvout_src_at(g, x0, y0), Y, U, V);
    yuvout_pack(Y, 16, w);
    yuv_st16(dst + yuvout_y_at(g, x0, y0), w);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        cu[k] = first ? U[2 * k] : U[2 * k] + U[2 * k + 1];
        cv[k] = first ? V[2 * k] : V[2 * k] + V[2 * k + 1];
    }
    yuvout_group_row<MATRIX>(src + yuvout_src_at(g, x0, y0 + 1), Y, U, V);
    yuvout_pack(Y, 16, w);
    yuv_st16(dst + yuvout_y_at(g, x0, y0 + 1), w);
    if (!first) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cu[k] = (cu[k] + U[2 * k] + U[2 * k + 1] + 2) >> 2;
            cv[k] = (cv[k] + V[2 * k] + V[2 * k + 1] + 2) >> 2;
        }
    }
    if (FORMAT == YUV_I420) {
        yuvout_pack(cu, 8, w);
        yuvout_st8(dst + yuvout_u_at(g, x0, y0), w);
        yuvout_pack(cv, 8, w);
        yuvout_st8(dst + yuvout_v_at(g, x0, y0), w);
    } else {
        int out[16];
        const int uo = FORMAT == YUV_NV12 ? 0 : 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            out[2 * k + uo] = cu[k];
            out[2 * k + 1 - uo] = cv[k];
        }
        yuvout_pack(out, 16, w);
        yuv_st16(dst + g.u_offset + (long long)(y0 >> 1) * g.u_pitch + x0, w);   // = the lower of yuvout_u_at and yuvout_v_at of (x0, y0)
    }
}

// item t (0 <= t < yuvout_items_per_frame, which fits 31 bits: at most 32767 cells x 65534 rows) of frame f: src and dst are the run's base
// pointers; FORMAT is g0.format
template <int FORMAT, int MATRIX>
ADAS_HDI void yuvout_item(const YuvGeom& g0, int chroma, bool vec, const uint8_t* src, uint8_t* dst, int f, uint32_t t) {
    YuvGeom g = g0;
    g.format = FORMAT;   // the address functions fold their switch
    int ng, nt;
    yuvout_split(g.w, vec, &ng, &nt);
    const uint32_t per_row = (uint32_t)(ng + nt);
    const int unit = (int)(t / per_row), i = (int)(t - (uint32_t)unit * per_row);
    const uint8_t* s = src + (long long)f * yuvout_src_bytes(g.w, g.h);
    uint8_t* d = dst + (long long)f * g.frame_stride;
    const int x = yuvout_item_x(i, ng), y0 = unit * yuv_unit_rows(FORMAT);
    if (i < ng)
        yuvout_group<FORMAT, MATRIX>(g, chroma, s, d, x, y0);
    else
        yuvout_cell<MATRIX>(g, chroma, s, d, x, y0);
}

}  // namespace adas
