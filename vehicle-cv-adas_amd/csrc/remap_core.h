// remap_core.h -- camera frames rectified on the device: cv2.remap(frame, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0) of 8-bit BGR frames through
// a fixed-point map per stream, and the map of a lens model as cv2.initUndistortRectifyMap(K, D, R, new_K, size, CV_16SC2) writes it -- together
// what cv2.undistort does.  The stage in front of the fused step for cameras whose frames are not pinhole images.
//
// cv2 is third-party arithmetic and is not available here: this restates OpenCV 4.5's reference path (calib3d/imgproc undistort.cpp,
// initUndistortRectifyMap with m1type CV_16SC2; imgproc/src/imgwarp.cpp, remapBilinear<FixedPtCast<int, uchar, 15>>) and is checked against the
// same restatement in NumPy (tests/remap_ref.py) and against an independently associated float64 evaluation of the model.  Parity with a real
// cv2 build is UNPINNED.  OpenCV evaluates X, Y, W of rule U3 by running sums along a destination row (X += iR0 per column); a running sum
// cannot be parallelised bit for bit, so a coordinate here may differ from OpenCV's in its last ulps, which moves a map entry only when it
// sits on a 1/32-pixel tie.
//
//   U1  map format.  Per destination pixel (sx, sy) int16 and a fraction word ay * 32 + ax with ax, ay in 0..31: cv2's map1 (h, w, 2) int16 and
//       map2 (h, w) uint16.  The top 6 bits of the word are ignored on read.
//   U2  sampling.  warp_core.h's warp_sample, unchanged: weights (32-ax)(32-ay)*32 ... that sum to 2^15, a tap outside the source reads 0 in
//       every channel, no address outside the frame is ever formed.
//   U3  lens model.  K = (fx, fy, cx, cy), D = (k1, k2, p1, p2, k3, k4, k5, k6), new_K = (fx', fy', cx', cy'), R 3x3 row-major.
//       A = new_K * R with A[0][j] = fx'*R[0][j] + cx'*R[2][j], A[1][j] = fy'*R[1][j] + cy'*R[2][j], A[2][j] = R[2][j];
//       iR = warp_invert3x3(A).  For destination pixel (x, y), in IEEE fp64, contraction off, in exactly this association:
//         1. X = iR0*x + (iR1*y + iR2), Y = iR3*x + (iR4*y + iR5), W = iR6*x + (iR7*y + iR8)
//         2. w = 1/W, xn = X*w, yn = Y*w, x2 = xn*xn, y2 = yn*yn, r2 = x2 + y2, _2xy = 2*xn*yn
//         3. kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
//         4. xd = xn*kr + p1*_2xy + p2*(r2 + 2*x2), yd = yn*kr + p1*(r2 + 2*y2) + p2*_2xy      (sums left to right)
//         5. u = fx*xd + cx, v = fy*yd + cy
//         6. iu = (int)rint(warp_clamp_int(u * 32)), iv likewise
//         7. sx = warp_sat_s16(iu >> 5), ax = iu & 31, and the same for sy, ay
//       A non-finite coordinate goes through warp_clamp_int, saturates, and reads the border.
//   U4  refusals, by number and name (remap_why): 1 "non-finite parameter", 2 "zero focal length" (fx, fy, fx' or fy'),
//       3 "singular new_K * R", 4 "size outside 1..ADAS_WARP_MAX_ROWS x 1..ADAS_WARP_MAX_COLS", 5 "map index outside the handle's table".
//   U5  frame indexing.  Frame f of a batch belongs to stream f % n_streams (the pipeline's micro-batch order b * n_streams + s) and reads the
//       map map_of_stream[stream].  Several streams may share one map.
//   U6  write-once.  Every destination byte of frames [0, batch) is written exactly once, and no byte outside them.
//
// Addresses.  Map m's entries start at pixel m * map_stride of the two tables, map_stride = remap_map_stride(dst_h, dst_w) (the pixel count
// rounded up to 4, so every map starts on 16 bytes of (sx, sy) and 8 bytes of fractions).  A work item is a run of 4 consecutive pixels of one
// destination row of one frame (the row's last run has dst_w % 4 pixels when that is not 0).  Where the run's first map entry sits on a multiple of
// 4 entries the 4 (sx, sy) come as one 16-byte load and the 4 fractions as one 8-byte load, elsewhere entry by entry; where the run's first
// byte sits on a multiple of 4 bytes the 12 bytes leave as three dwords, elsewhere (and in a row's tail) byte by byte.  Same values either way.
// The taps come in one of two forms that give the same bytes: gathered from global memory by warp_sample (any pointer, any size), or -- where
// src_w * 3 and the source pointer are multiples of 16 -- from a workgroup's source box staged in LDS (the staged form, at the end of this file).
// Like warp_core.h the header also compiles for the host (tests/hostemu/emu_remap.cpp).
#pragma once
#include "warp_core.h"

#if !defined(ADAS_HDI)
#if defined(__HIPCC__)
#define ADAS_HDI __host__ __device__ __forceinline__
#else
#define ADAS_HDI inline
#endif
#endif

namespace adas {

enum { REMAP_OK = 0, REMAP_NONFINITE = 1, REMAP_ZERO_FOCAL = 2, REMAP_SINGULAR = 3, REMAP_BAD_SIZE = 4, REMAP_BAD_MAP = 5 };

static_assert(ADAS_WARP_MAX_ROWS == 4320 && ADAS_WARP_MAX_COLS == 16384, "remap_why's text for REMAP_BAD_SIZE names these two limits");
ADAS_HD const char* remap_why(int code) {
    switch (code) {
        case REMAP_NONFINITE: return "non-finite parameter";
        case REMAP_ZERO_FOCAL: return "zero focal length";
        case REMAP_SINGULAR: return "singular new_K * R";
        case REMAP_BAD_SIZE: return "size outside 1..4320 rows x 1..16384 columns";
        case REMAP_BAD_MAP: return "map index outside the handle's table";
    }
    return "";
}

struct RemapCamera {   // adas_remap_camera
    double K[4], D[8], new_K[4], R[9];
};

struct RemapModel {   // what the build kernel evaluates: U3's iR and the source camera
    double iR[9];
    double fx, fy, cx, cy;
    double k[8];   // k1, k2, p1, p2, k3, k4, k5, k6
};

struct RemapGeom {
    int sh, sw, dh, dw;
    int n_streams, n_maps;
    long long map_stride;   // entries between two maps of the tables
};

ADAS_HD bool remap_finite(double v) { return v - v == 0.0; }   // false for NaN and both infinities

ADAS_HD int remap_check_sizes(int src_h, int src_w, int dst_h, int dst_w) {
    const bool ok = src_h >= 1 && src_h <= ADAS_WARP_MAX_ROWS && dst_h >= 1 && dst_h <= ADAS_WARP_MAX_ROWS && src_w >= 1 &&
                    src_w <= ADAS_WARP_MAX_COLS && dst_w >= 1 && dst_w <= ADAS_WARP_MAX_COLS;
    return ok ? REMAP_OK : REMAP_BAD_SIZE;
}

ADAS_HD int remap_check_map(int map, int n_maps) { return map >= 0 && map < n_maps ? REMAP_OK : REMAP_BAD_MAP; }

ADAS_HD long long remap_map_stride(int dst_h, int dst_w) { return ((long long)dst_h * dst_w + 3) / 4 * 4; }
ADAS_HD int remap_runs(int dst_w) { return (dst_w + 3) / 4; }
// U5: the default table, stream s -> map min(s, n_maps - 1)
ADAS_HD int remap_default_map(int stream, int n_maps) { return stream < n_maps - 1 ? stream : n_maps - 1; }

// U4 on a camera, then U3's constants.  Returns REMAP_OK or the refusal.
ADAS_HD int remap_model_of(const RemapCamera& c, RemapModel* m) {
    for (int i = 0; i < 4; ++i)
        if (!remap_finite(c.K[i]) || !remap_finite(c.new_K[i])) return REMAP_NONFINITE;
    for (int i = 0; i < 8; ++i)
        if (!remap_finite(c.D[i])) return REMAP_NONFINITE;
    for (int i = 0; i < 9; ++i)
        if (!remap_finite(c.R[i])) return REMAP_NONFINITE;
    if (c.K[0] == 0.0 || c.K[1] == 0.0 || c.new_K[0] == 0.0 || c.new_K[1] == 0.0) return REMAP_ZERO_FOCAL;
    double A[9];
    for (int j = 0; j < 3; ++j) {
        A[j] = c.new_K[0] * c.R[j] + c.new_K[2] * c.R[6 + j];
        A[3 + j] = c.new_K[1] * c.R[3 + j] + c.new_K[3] * c.R[6 + j];
        A[6 + j] = c.R[6 + j];
    }
    if (!warp_invert3x3(A, m->iR)) return REMAP_SINGULAR;
    m->fx = c.K[0]; m->fy = c.K[1]; m->cx = c.K[2]; m->cy = c.K[3];
    for (int i = 0; i < 8; ++i) m->k[i] = c.D[i];
    return REMAP_OK;
}

// U3 steps 1-7 for destination pixel (x, y)
ADAS_HD WarpTap remap_model_tap(const RemapModel& m, int x, int y) {
    const double* iR = m.iR;
    const double k1 = m.k[0], k2 = m.k[1], p1 = m.k[2], p2 = m.k[3], k3 = m.k[4], k4 = m.k[5], k5 = m.k[6], k6 = m.k[7];
    const double X = iR[0] * x + (iR[1] * y + iR[2]);
    const double Y = iR[3] * x + (iR[4] * y + iR[5]);
    const double W = iR[6] * x + (iR[7] * y + iR[8]);
    const double w = 1.0 / W;
    const double xn = X * w, yn = Y * w;
    const double x2 = xn * xn, y2 = yn * yn;
    const double r2 = x2 + y2, _2xy = 2 * xn * yn;
    const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = xn * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
    const double yd = yn * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
    const double u = m.fx * xd + m.cx, v = m.fy * yd + m.cy;
    const int iu = (int)rint(warp_clamp_int(u * 32)), iv = (int)rint(warp_clamp_int(v * 32));
    WarpTap t;
    t.sx = warp_sat_s16(iu >> 5);
    t.sy = warp_sat_s16(iv >> 5);
    t.ax = iu & 31;
    t.ay = iv & 31;
    return t;
}

// Every load and store of an item goes through these.  A host build that defines REMAP_AUDIT sees each one's address, width and required
// alignment before it happens (remap_audit; kind 0 a (sx, sy) load, 1 a fraction load, 2 a frame store, 3 a table load, 4 a (sx, sy) store,
// 5 a fraction store, 6 a 16-byte source load of the staged form), and an access it answers with false does not happen (a load then gives zero).  The taps are warp_sample's.
#if defined(REMAP_AUDIT) && !defined(__HIP_DEVICE_COMPILE__)
bool remap_audit(const void* p, int bytes, int align, int kind);
#define REMAP_AUDIT_CALL(p, n, a, k) remap_audit(p, n, a, k)
#else
#define REMAP_AUDIT_CALL(p, n, a, k) true
#endif

ADAS_HDI int remap_ld_table(const int* table, int stream) {
    if (!REMAP_AUDIT_CALL(table + stream, 4, 4, 3)) return 0;
    return table[stream];
}
// one entry: (sx, sy) as a dword, sx in the low half
ADAS_HDI uint32_t remap_ld_xy1(const int16_t* p) {
    if (!REMAP_AUDIT_CALL(p, 4, 4, 0)) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint32_t*)p;
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}
ADAS_HDI uint32_t remap_ld_frac1(const uint16_t* p) {
    if (!REMAP_AUDIT_CALL(p, 2, 2, 1)) return 0;
    return *p;
}
ADAS_HDI void remap_ld_xy4(const int16_t* p, uint32_t v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0;
    if (!REMAP_AUDIT_CALL(p, 16, 16, 0)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 q = *(const uint4*)p;
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
#else
    memcpy(v, p, 16);
#endif
}
ADAS_HDI void remap_ld_frac4(const uint16_t* p, uint32_t v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0;
    if (!REMAP_AUDIT_CALL(p, 8, 8, 1)) return;
    uint32_t q[2];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint2 d = *(const uint2*)p;
    q[0] = d.x; q[1] = d.y;
#else
    memcpy(q, p, 8);
#endif
    v[0] = q[0] & 0xffff; v[1] = q[0] >> 16; v[2] = q[1] & 0xffff; v[3] = q[1] >> 16;
}
ADAS_HDI void remap_st1(uint8_t* p, uint32_t v) {
    if (!REMAP_AUDIT_CALL(p, 1, 1, 2)) return;
    *p = (uint8_t)v;
}
struct alignas(4) RemapRun12 {
    uint32_t a, b, c;
};
ADAS_HDI void remap_st12(uint8_t* p, uint32_t a, uint32_t b, uint32_t c) {
    if (!REMAP_AUDIT_CALL(p, 12, 4, 2)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    RemapRun12 o;
    o.a = a; o.b = b; o.c = c;
    *reinterpret_cast<RemapRun12*>(p) = o;
#else
    const uint32_t o[3] = {a, b, c};
    memcpy(p, o, 12);
#endif
}
ADAS_HDI void remap_st_entry(int16_t* xy, uint16_t* frac, const WarpTap t) {
    const uint32_t w = (uint32_t)(uint16_t)(int16_t)t.sx | ((uint32_t)(uint16_t)(int16_t)t.sy << 16);
    if (REMAP_AUDIT_CALL(xy, 4, 4, 4)) {
#if defined(__HIP_DEVICE_COMPILE__)
        *(uint32_t*)xy = w;
#else
        memcpy(xy, &w, 4);
#endif
    }
    if (REMAP_AUDIT_CALL(frac, 2, 2, 5)) *frac = (uint16_t)(t.ay * 32 + t.ax);
}

// U1: an entry as the sampler reads it
ADAS_HDI WarpTap remap_entry_tap(uint32_t xy, uint32_t frac) {
    WarpTap t;
    t.sx = (int)(int16_t)(uint16_t)(xy & 0xffff);
    t.sy = (int)(int16_t)(uint16_t)(xy >> 16);
    t.ax = (int)(frac & 31);
    t.ay = (int)((frac >> 5) & 31);
    return t;
}

// The build kernel's work item: entry `i` = y * dst_w + x of map `map` of the tables, i in [0, dst_h * dst_w)
ADAS_HDI void remap_build_item(const RemapGeom& g, const RemapModel& m, int16_t* xy, uint16_t* frac, int map, long long i) {
    const int y = (int)(i / g.dw), x = (int)(i - (long long)y * g.dw);
    const long long e = (long long)map * g.map_stride + i;
    remap_st_entry(xy + 2 * e, frac + e, remap_model_tap(m, x, y));
}

// ---- the remap kernel's work, in phases that both of its forms share.  A work item is run `run` in [0, remap_runs(dst_w)) of row y of frame f;
// `map` = the table's word of stream f % n_streams (U5).

// phase 1: the run's entries; returns the run's pixel count n (4, or dst_w % 4 in a row's tail)
ADAS_HDI int remap_run_entries(const RemapGeom& g, const int16_t* __restrict__ xy, const uint16_t* __restrict__ frac, int map, int y, int run,
                               uint32_t mx[4], uint32_t mf[4]) {
    const int x0 = run * 4;
    const int n = g.dw - x0 < 4 ? g.dw - x0 : 4;
    const long long e = (long long)map * g.map_stride + (long long)y * g.dw + x0;
    mx[0] = mx[1] = mx[2] = mx[3] = 0;
    mf[0] = mf[1] = mf[2] = mf[3] = 0;
    if (n == 4 && (e & 3) == 0) {
        remap_ld_xy4(xy + 2 * e, mx);
        remap_ld_frac4(frac + e, mf);
    } else {
        for (int i = 0; i < n; ++i) {
            mx[i] = remap_ld_xy1(xy + 2 * (e + i));
            mf[i] = remap_ld_frac1(frac + e + i);
        }
    }
    return n;
}

// last phase: the run's n pixels, (b, g, r) in the low 24 bits of px[i], into frame f
ADAS_HDI void remap_run_store(const RemapGeom& g, uint8_t* __restrict__ dst, int f, int y, int run, int n, const uint32_t px[4]) {
    uint8_t* p = dst + ((size_t)f * g.dh * g.dw + (size_t)y * g.dw + run * 4) * 3;
    if (n == 4 && ((uintptr_t)p & 3) == 0) {
        remap_st12(p, px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8));
    } else {
        for (int i = 0; i < n; ++i) {
            remap_st1(p + 3 * i + 0, px[i]);
            remap_st1(p + 3 * i + 1, px[i] >> 8);
            remap_st1(p + 3 * i + 2, px[i] >> 16);
        }
    }
}

// the direct form's middle phase: warp_sample's gathers from the frame in global memory
ADAS_HDI void remap_run_gather(const RemapGeom& g, const uint8_t* __restrict__ src, int f, int n, const uint32_t mx[4], const uint32_t mf[4],
                               uint32_t px[4]) {
    const uint8_t* __restrict__ frame = src + (size_t)f * g.sh * g.sw * 3;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        px[i] = 0;
        if (i < n) {
            int v[3];
            warp_sample(frame, g.sh, g.sw, remap_entry_tap(mx[i], mf[i]), v);
            px[i] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
        }
    }
}

// The direct form's work item: entries, gathers, store
ADAS_HDI void remap_item(const RemapGeom& g, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int16_t* __restrict__ xy,
                         const uint16_t* __restrict__ frac, int map, int f, int y, int run) {
    uint32_t mx[4], mf[4], px[4];
    const int n = remap_run_entries(g, xy, frac, map, y, run, mx, mf);
    remap_run_gather(g, src, f, n, mx, mf, px);
    remap_run_store(g, dst, f, y, run, n, px);
}

// ---- the staged form.  A workgroup is a destination tile of REMAP_TILE_ROWS rows by REMAP_TILE_RUNS runs of one frame.  Its lanes load their
// entries, the tile's source box -- the bounding box of every tap that lies inside the source -- comes into LDS in aligned 16-byte pieces,
// neighbouring lanes on neighbouring pieces, and the taps are read from LDS: each source byte crosses the memory pipeline once per tile
// in place of once per tap.  It needs src_w * 3 and the source pointer to be multiples of 16 (remap_tile_ok: decided per run, on the host);
// a tile whose box is larger than REMAP_TILE_LDS bytes takes the direct form's gathers (decided per workgroup).  The sampler restates
// warp_sample on the box's addresses -- the same weights, warp_blend, zeros outside -- and gives the same bytes.
#define REMAP_TILE_ROWS 4
#define REMAP_TILE_RUNS 64
#define REMAP_TILE_LDS 16384   // the most bytes of a staged box
#define REMAP_TILE_PAD 16      // behind the box: remap_lds8 reads three aligned dwords from a tap's first byte on

struct RemapTile {
    int x_lo;    // first byte of the box within a source row, a multiple of 16
    int pitch;   // bytes of a box row, a multiple of 16; 0: no tap of the tile lies inside the source
    int y_lo;    // first source row of the box
    int rows;
};

ADAS_HD bool remap_tile_ok(const RemapGeom& g, const void* src) { return (g.sw * 3) % 16 == 0 && ((uintptr_t)src & 15) == 0; }

// ext = {min x, max x, min y, max y} over the source pixels the run's taps read; start it at {INT_MAX, -1, INT_MAX, -1}
ADAS_HDI void remap_run_extent(const RemapGeom& g, int n, const uint32_t mx[4], int ext[4]) {
    for (int i = 0; i < n; ++i) {
        const WarpTap t = remap_entry_tap(mx[i], 0);
        const int x0 = t.sx < 0 ? 0 : t.sx, x1 = t.sx + 1 > g.sw - 1 ? g.sw - 1 : t.sx + 1;
        const int y0 = t.sy < 0 ? 0 : t.sy, y1 = t.sy + 1 > g.sh - 1 ? g.sh - 1 : t.sy + 1;
        if (x0 > x1 || y0 > y1) continue;   // every tap of this pixel is outside
        ext[0] = x0 < ext[0] ? x0 : ext[0];
        ext[1] = x1 > ext[1] ? x1 : ext[1];
        ext[2] = y0 < ext[2] ? y0 : ext[2];
        ext[3] = y1 > ext[3] ? y1 : ext[3];
    }
}

ADAS_HDI RemapTile remap_tile_of(const int ext[4]) {
    RemapTile T;
    T.x_lo = T.pitch = T.y_lo = T.rows = 0;
    if (ext[1] < ext[0]) return T;
    T.x_lo = (ext[0] * 3) & ~15;
    T.pitch = ((ext[1] * 3 + 3 + 15) & ~15) - T.x_lo;   // <= src_w * 3 - x_lo, as src_w * 3 is a multiple of 16
    T.y_lo = ext[2];
    T.rows = ext[3] - ext[2] + 1;
    return T;
}
ADAS_HDI bool remap_tile_fits(const RemapTile& T) { return (long long)T.pitch * T.rows <= REMAP_TILE_LDS; }
ADAS_HDI int remap_tile_pieces(const RemapTile& T) { return T.rows * (T.pitch / 16); }

// piece p in [0, remap_tile_pieces): 16 source bytes into the box
ADAS_HDI void remap_tile_load(const RemapGeom& g, const RemapTile& T, const uint8_t* __restrict__ src, int f, uint8_t* lds, int p) {
    const int per_row = T.pitch / 16, r = p / per_row, c = p - r * per_row;
    const uint8_t* q = src + (size_t)f * g.sh * g.sw * 3 + (size_t)(T.y_lo + r) * g.sw * 3 + T.x_lo + 16 * c;
    uint8_t* o = lds + r * T.pitch + 16 * c;
    if (!REMAP_AUDIT_CALL(q, 16, 16, 6)) {
        memset(o, 0, 16);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint4*)o = *(const uint4*)q;
#else
    memcpy(o, q, 16);
#endif
}

// 8 bytes of the box from byte offset o on, from three aligned dwords
ADAS_HDI unsigned long long remap_lds8(const uint8_t* lds, int o) {
    const int q = o & ~3, s = (o & 3) * 8;
    uint32_t d[3];
#if defined(__HIP_DEVICE_COMPILE__)
    d[0] = *(const uint32_t*)(lds + q);
    d[1] = *(const uint32_t*)(lds + q + 4);
    d[2] = *(const uint32_t*)(lds + q + 8);
#else
    memcpy(d, lds + q, 12);
#endif
    unsigned long long r = ((unsigned long long)d[0] | ((unsigned long long)d[1] << 32)) >> s;
    if (s) r |= (unsigned long long)d[2] << (64 - s);
    return r;
}

// warp_sample on the box
ADAS_HDI void remap_tile_sample(const RemapGeom& g, const RemapTile& T, const uint8_t* lds, const WarpTap t, int out[3]) {
    const int w00 = (32 - t.ax) * (32 - t.ay) * 32, w01 = t.ax * (32 - t.ay) * 32;
    const int w10 = (32 - t.ax) * t.ay * 32, w11 = t.ax * t.ay * 32;
    const int sx = t.sx, sy = t.sy;
    if (sx >= 0 && sy >= 0 && sy + 1 < g.sh && sx + 1 < g.sw) {   // all four taps inside: 6 consecutive bytes per row
        const int o = (sy - T.y_lo) * T.pitch + sx * 3 - T.x_lo;
        const unsigned long long a = remap_lds8(lds, o), b = remap_lds8(lds, o + T.pitch);
        for (int c = 0; c < 3; ++c)
            out[c] = warp_blend((int)((a >> (8 * c)) & 0xff), (int)((a >> (8 * (3 + c))) & 0xff), (int)((b >> (8 * c)) & 0xff),
                                (int)((b >> (8 * (3 + c))) & 0xff), w00, w01, w10, w11);
        return;
    }
    const bool x0 = sx >= 0 && sx < g.sw, x1 = sx + 1 >= 0 && sx + 1 < g.sw;
    const bool y0 = sy >= 0 && sy < g.sh, y1 = sy + 1 >= 0 && sy + 1 < g.sh;
    if (!((x0 || x1) && (y0 || y1))) {
        out[0] = out[1] = out[2] = 0;
        return;
    }
    // an index that is outside is replaced by one inside the box; its tap reads 0
    const uint8_t* r0 = lds + ((y0 ? sy : T.y_lo) - T.y_lo) * T.pitch;
    const uint8_t* r1 = lds + ((y1 ? sy + 1 : T.y_lo) - T.y_lo) * T.pitch;
    const int c0 = (x0 ? sx * 3 : T.x_lo) - T.x_lo, c1 = (x1 ? (sx + 1) * 3 : T.x_lo) - T.x_lo;
    for (int c = 0; c < 3; ++c) {
        const int p00 = (y0 && x0) ? r0[c0 + c] : 0, p01 = (y0 && x1) ? r0[c1 + c] : 0;
        const int p10 = (y1 && x0) ? r1[c0 + c] : 0, p11 = (y1 && x1) ? r1[c1 + c] : 0;
        out[c] = warp_blend(p00, p01, p10, p11, w00, w01, w10, w11);
    }
}

ADAS_HDI void remap_run_sample_tile(const RemapGeom& g, const RemapTile& T, const uint8_t* lds, int n, const uint32_t mx[4], const uint32_t mf[4],
                                    uint32_t px[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        px[i] = 0;
        if (i < n) {
            int v[3];
            remap_tile_sample(g, T, lds, remap_entry_tap(mx[i], mf[i]), v);
            px[i] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
        }
    }
}

}  // namespace adas
