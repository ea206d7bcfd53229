// jpeg_core.h -- the rules of the baseline JPEG encoder behind adas_jpeg_* (the line the demo ends its loop with, vout.write(frame_show),
// demo.py:314, as one compressed stream per frame).  Written from ITU-T T.81 (the standard and its Annex K tables), not from a library.
// THE DEFINITIONS HERE ARE THE AUTHORITY; every rule is integer arithmetic, so host and device cannot disagree.
//   J1 geometry  baseline sequential DCT (SOF0), 8 bit, three components; Y sampled 2x2, Cb and Cr 1x1: an MCU is 16x16 pixels and six blocks
//                in the order Y00 Y01 Y10 Y11 Cb Cr.  Any width and height >= 1; pixels beyond the right or bottom edge repeat the last
//                column or row.
//   J2 colour    input BGR u8, interleaved.  Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
//                                           Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32768) >> 16
//                                           Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32768) >> 16,   each clamped to 0..255.
//   J3 chroma    (a + b + c + d + 2) >> 2 over each 2x2 cell of the padded image's clamped Cb / Cr.
//   J4 transform level shift by 128, then two passes of the 8-point DCT matrix M[u][x] = c(u) sqrt(2) cos((2x + 1) u pi / 16), c(0) = 1 / sqrt(2),
//                held as K = round(8192 M) (row 0 and row 4 are exact) and evaluated on the sums and differences of mirrored inputs:
//                rows: T = (sum K f + 256) >> 9  (16 times the exact pass), columns: F' = (sum K T + 65536) >> 17.  F' approximates 8 F, F the
//                orthonormal DCT.  Bound: |K - 8192 M| <= 0.5, |f| <= 128, so T is off 16 x the exact pass by at most 8 * 0.5 * 128 / 512 + 0.5
//                = 1.5, which the second pass (sum |M| <= 8) carries to 8 * 1.5 / 16 = 0.75; its own constants add at most
//                8 * 0.5 * (16 * 1024 + 1.5) / 2^17 = 0.5 and its rounding 0.5:  |F' - 8 F| <= JPEG_FDCT_ERR = 1.75.  Largest seen over the
//                CPU suite's 6270 random and extreme blocks: 0.88 (tests/test_jpeg_cpu.py).  Every intermediate fits 32 bits: |T| <= 16384,
//                |sum K T| <= 65536 * 16384 = 2^30.  The DC term is exact: F'(0, 0) = sum f.
//   J5 quantise  tables: Annex K luminance / chrominance scaled by a quality q of 1..100: s = 5000 / q for q < 50, else 200 - 2 q;
//                d = clamp((base * s + 50) / 100, 1, 255).  level = sign(F') * ((|F'| + 4 d) / (8 d)) in integer division (half away from zero,
//                the 8 of J4 folded in).  AC levels are clamped to +-1023; the DC difference fits category 11 by construction
//                (|sum f| <= 8192, so |DC level| <= 1024 and |difference| <= 2040).
//   J6 entropy   zigzag order, the four Annex K Huffman tables, one DC predictor per component.  The restart interval is one MCU row
//                (DRI = ceil(w / 16)): every segment starts with its predictors at 0 and is padded with 1-bits to a byte; RSTm with
//                m = row mod 8 goes between segments, none after the last; inside a segment every 0xFF byte is followed by 0x00.
//   J7 stream    SOI, DQT x 2, SOF0, DHT x 4 (DC0, AC0, DC1, AC1), DRI, SOS, segments, EOI; no APP0.  The JPEG_HEADER_BYTES header bytes are a
//                function of (w, h, quality) only (jpeg_build_header).
//   J8 capacity  jpeg_bound(w, h) = header + blocks * 416 + markers: a block is at most 20 + 63 * 26 = 1658 bits, doubled for stuffing.  A frame
//                whose stream would not fit its capacity gets length 0 and JPEG_OVERFLOW; no byte at or beyond the capacity is written.
//   J9           the bytes of a frame depend on its pixels and (w, h, quality) alone.
// The header compiles for the host as well (tests/hostemu/emu_jpeg.cpp).
#pragma once
#include <stdint.h>

#if !defined(ADAS_HD)
#if defined(__HIPCC__)
#define ADAS_DEV __device__ __forceinline__
#define ADAS_HD __host__ __device__ inline
#pragma clang fp contract(off)
#else
#define ADAS_DEV inline
#define ADAS_HD inline
#endif
#endif

#if !defined(ADAS_HDI)
#if defined(__HIPCC__)
#define ADAS_HDI __host__ __device__ __forceinline__
#else
#define ADAS_HDI inline
#endif
#endif

namespace adas {

#define JPEG_HEADER_BYTES 611
#define JPEG_BLOCK_MAX_BITS 1658
#define JPEG_BLOCK_MAX_BYTES 416
#define JPEG_OVERFLOW 1          /* ADAS_JPEG_OVERFLOW */
#define JPEG_FDCT_ERR 1.75       /* |F' - 8 F|, J4 */
#define JPEG_MAX_DIM 65535       /* SOF0 holds 16-bit sizes */

struct JpegGeom {
    int w, h;
    int mcu_w, mcu_h;     // MCUs per row (= DRI), MCU rows (= segments)
    int seg_blocks;       // 6 * mcu_w
    long long blocks;     // of a frame
};

ADAS_HDI JpegGeom jpeg_geometry(int w, int h) {
    JpegGeom g;
    g.w = w; g.h = h;
    g.mcu_w = (w + 15) / 16; g.mcu_h = (h + 15) / 16;
    g.seg_blocks = 6 * g.mcu_w;
    g.blocks = (long long)g.seg_blocks * g.mcu_h;
    return g;
}

ADAS_HDI long long jpeg_bound(int w, int h) {
    const JpegGeom g = jpeg_geometry(w, h);
    return (long long)JPEG_HEADER_BYTES + g.blocks * JPEG_BLOCK_MAX_BYTES + 2LL * (g.mcu_h - 1) + 2;
}

// zigzag position k -> natural index (row * 8 + column)
ADAS_HDI int jpeg_zigzag(int k) {
    constexpr uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return ZZ[k];
}

// natural index -> zigzag position
ADAS_HDI int jpeg_zigzag_position(int natural) {
    constexpr uint8_t INV[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return INV[natural];
}

// what the kernels read: the divisors in zigzag order, the Huffman codes as (code << 8) | size, by DC category and by AC symbol (run << 4 | size)
struct JpegTables {
    uint16_t q[2][64];
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

// J5: divisor `natural` (row * 8 + column) of table `cls` (0 luminance, 1 chrominance) at `quality`
inline int jpeg_quant_divisor(int cls, int natural, int quality) {
    static const uint8_t BASE[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int d = (BASE[cls][natural] * s + 50) / 100;
    return d < 1 ? 1 : (d > 255 ? 255 : d);
}

// Annex K.3: BITS (codes of each length 1..16) and HUFFVAL of table t = 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance
inline const uint8_t* jpeg_huff_spec(int t, const uint8_t** vals, int* n_vals) {
    static const uint8_t BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                        {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                        {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    static const uint8_t DCV[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ACL[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
        0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
        0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
        0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
        0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
        0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
        0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    static const uint8_t ACC[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
        0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
        0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
        0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
        0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
        0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
        0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    *vals = t == 1 ? ACL : (t == 3 ? ACC : DCV);
    *n_vals = (t & 1) ? 162 : 12;
    return BITS[t];
}

// Annex C: the codes of a table in order of length, then of value
inline void jpeg_build_tables(int quality, JpegTables* T) {
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) T->q[c][k] = (uint16_t)jpeg_quant_divisor(c, jpeg_zigzag(k), quality);
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < 12; ++i) T->dc[c][i] = 0;
        for (int i = 0; i < 256; ++i) T->ac[c][i] = 0;
    }
    for (int t = 0; t < 4; ++t) {
        const uint8_t* vals;
        int n;
        const uint8_t* bits = jpeg_huff_spec(t, &vals, &n);
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < bits[len - 1]; ++i, ++k) {
                const uint32_t e = (code++ << 8) | (uint32_t)len;
                if (t & 1) T->ac[t >> 1][vals[k]] = e;
                else T->dc[t >> 1][vals[k]] = e;
            }
            code <<= 1;
        }
    }
}

// J7: the JPEG_HEADER_BYTES bytes in front of the first segment
inline int jpeg_build_header(int w, int h, int quality, uint8_t* out) {
    uint8_t* p = out;
    auto put = [&](int v) { *p++ = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 255); };
    put16(0xFFD8);
    for (int c = 0; c < 2; ++c) {
        put16(0xFFDB); put16(67); put(c);
        for (int k = 0; k < 64; ++k) put(jpeg_quant_divisor(c, jpeg_zigzag(k), quality));
    }
    put16(0xFFC0); put16(17); put(8); put16(h); put16(w); put(3);
    put(1); put(0x22); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    for (int t = 0; t < 4; ++t) {
        const uint8_t* vals;
        int n;
        const uint8_t* bits = jpeg_huff_spec(t, &vals, &n);
        put16(0xFFC4); put16(2 + 1 + 16 + n); put(((t & 1) << 4) | (t >> 1));
        for (int i = 0; i < 16; ++i) put(bits[i]);
        for (int i = 0; i < n; ++i) put(vals[i]);
    }
    put16(0xFFDD); put16(4); put16((w + 15) / 16);
    put16(0xFFDA); put16(12); put(3);
    put(1); put(0x00);
    put(2); put(0x11);
    put(3); put(0x11);
    put(0); put(63); put(0);
    return (int)(p - out);
}

// J2 on one pixel
struct JpegPx {
    int b, g, r;
};
ADAS_HDI JpegPx jpeg_px(const uint8_t* p) { return JpegPx{p[0], p[1], p[2]}; }
ADAS_HDI int jpeg_luma(JpegPx p) {
    const int v = (19595 * p.r + 38470 * p.g + 7471 * p.b + 32768) >> 16;
    return v > 255 ? 255 : v;
}
ADAS_HDI int jpeg_cb(JpegPx p) {
    const int v = (-11059 * p.r - 21709 * p.g + 32768 * p.b + 8388608 + 32768) >> 16;
    return v > 255 ? 255 : (v < 0 ? 0 : v);
}
ADAS_HDI int jpeg_cr(JpegPx p) {
    const int v = (32768 * p.r - 27439 * p.g - 5329 * p.b + 8388608 + 32768) >> 16;
    return v > 255 ? 255 : (v < 0 ? 0 : v);
}

// J2, J3 on one row of a block, level-shifted, from wherever its pixels come: a luminance row from the 8 pixels px(0..7), a chrominance row
// (k6 = 4: Cb, 5: Cr) from the 16 pixels pa(0..15) of the upper and pb(0..15) of the lower source row
template <class Px>
ADAS_HDI void jpeg_row_luma(Px px, int* f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = jpeg_luma(px(i)) - 128;
}
template <class PxA, class PxB>
ADAS_HDI void jpeg_row_chroma(int k6, PxA pa, PxB pb, int* f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const JpegPx p0 = pa(2 * i), p1 = pa(2 * i + 1), p2 = pb(2 * i), p3 = pb(2 * i + 1);
        const int s = k6 == 4 ? jpeg_cb(p0) + jpeg_cb(p1) + jpeg_cb(p2) + jpeg_cb(p3) : jpeg_cr(p0) + jpeg_cr(p1) + jpeg_cr(p2) + jpeg_cr(p3);
        f[i] = ((s + 2) >> 2) - 128;
    }
}

// J1: where row j of block k6 (Y00 Y01 Y10 Y11 Cb Cr) of MCU (my, mx) lies: the source rows ya (and yb for chrominance), clamped to the frame,
// its first column x0 and its width in pixels (8 or 16); columns at and beyond w repeat column w - 1
ADAS_HDI void jpeg_row_place(int h, int my, int mx, int k6, int j, int* ya, int* yb, int* x0, int* n) {
    if (k6 < 4) {
        const int y = my * 16 + (k6 >> 1) * 8 + j;
        *ya = *yb = y < h ? y : h - 1;
        *x0 = mx * 16 + (k6 & 1) * 8;
        *n = 8;
    } else {
        const int y = my * 16 + 2 * j;
        *ya = y < h ? y : h - 1;
        *yb = y + 1 < h ? y + 1 : h - 1;
        *x0 = mx * 16;
        *n = 16;
    }
}

// J1-J3: the level-shifted samples f [8] of row j of block k6 of MCU (my, mx) of a frame [h][w][3] that may start on any byte
ADAS_HDI void jpeg_load_row(const uint8_t* frame, int w, int h, int my, int mx, int k6, int j, int* f) {
    int ya, yb, x0, n;
    jpeg_row_place(h, my, mx, k6, j, &ya, &yb, &x0, &n);
    const uint8_t *ra = frame + (size_t)ya * w * 3, *rb = frame + (size_t)yb * w * 3;
    auto pa = [&](int i) { return jpeg_px(ra + (size_t)(x0 + i < w ? x0 + i : w - 1) * 3); };
    auto pb = [&](int i) { return jpeg_px(rb + (size_t)(x0 + i < w ? x0 + i : w - 1) * 3); };
    if (k6 < 4) jpeg_row_luma(pa, f);
    else jpeg_row_chroma(k6, pa, pb, f);
}
ADAS_HDI void jpeg_load_block(const uint8_t* frame, int w, int h, int my, int mx, int k6, int* f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) jpeg_load_row(frame, w, h, my, mx, k6, j, f + j * 8);
}

// J4: one 8-point pass over a[0], a[stride], ...: out = (sum K a + round) >> shift, on the sums (even u) and differences (odd u) of mirrored inputs
ADAS_HDI void jpeg_fdct_pass(int* a, int stride, int round, int shift) {
    constexpr int K[8][4] = {{8192, 8192, 8192, 8192},   {11363, 9633, 6436, 2260},   {10703, 4433, -4433, -10703}, {9633, -2260, -11363, -6436},
                             {8192, -8192, -8192, 8192}, {6436, -11363, 2260, 9633}, {4433, -10703, 10703, -4433}, {2260, -6436, 9633, -11363}};
    int s[4], d[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        s[x] = a[x * stride] + a[(7 - x) * stride];
        d[x] = a[x * stride] - a[(7 - x) * stride];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int* v = (u & 1) ? d : s;
        const int acc = K[u][0] * v[0] + K[u][1] * v[1] + K[u][2] * v[2] + K[u][3] * v[3];
        a[u * stride] = (acc + round) >> shift;
    }
}

// f [64] level-shifted samples -> F' [64] (natural order), in place
ADAS_HDI void jpeg_fdct(int* f) {
#pragma unroll
    for (int y = 0; y < 8; ++y) jpeg_fdct_pass(f + y * 8, 1, 256, 9);
#pragma unroll
    for (int x = 0; x < 8; ++x) jpeg_fdct_pass(f + x, 8, 65536, 17);
}

// J5 on one coefficient; ac: clamp to +-1023
ADAS_HDI int jpeg_quantise(int F, int d, bool ac) {
    const int a = F < 0 ? -F : F;
    int l = (a + 4 * d) / (8 * d);
    if (ac && l > 1023) l = 1023;
    return F < 0 ? -l : l;
}

// category of a value: the bits of |v|
ADAS_HDI int jpeg_category(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// J6 on one block: the codes of a DC difference and of the 63 AC levels go to put(bits, count), count <= 27.  The levels come eight at a time:
// group(g, l) fills l[0..7] with the levels at zigzag positions 8 g .. 8 g + 7 (l[0] of group 0, the DC level, is not looked at); a group of
// zeros is a run of eight without a look at its members.
template <class Group, class Put>
ADAS_HDI void jpeg_code_block8(const uint32_t* dc_tab, const uint32_t* ac_tab, int dc_diff, Group group, Put put) {
    {
        const int s = jpeg_category(dc_diff);
        const uint32_t e = dc_tab[s];
        const uint32_t v = (uint32_t)(dc_diff < 0 ? dc_diff + (1 << s) - 1 : dc_diff) & ((1u << s) - 1u);
        put(((e >> 8) << s) | v, (int)(e & 255) + s);
    }
    int run = 0;
    for (int g = 0; g < 8; ++g) {
        int l[8];
        group(g, l);
        if (g == 0) l[0] = 0;
        if ((l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) == 0) {
            run += g ? 8 : 7;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (g == 0 && j == 0) continue;
            const int lv = l[j];
            if (lv == 0) {
                ++run;
                continue;
            }
            while (run >= 16) {
                const uint32_t z = ac_tab[0xF0];
                put(z >> 8, (int)(z & 255));
                run -= 16;
            }
            const int s = jpeg_category(lv);
            const uint32_t e = ac_tab[(run << 4) | s];
            const uint32_t v = (uint32_t)(lv < 0 ? lv + (1 << s) - 1 : lv) & ((1u << s) - 1u);
            put(((e >> 8) << s) | v, (int)(e & 255) + s);
            run = 0;
        }
    }
    if (run) {
        const uint32_t z = ac_tab[0x00];
        put(z >> 8, (int)(z & 255));
    }
}
// the same from lev(k), the level at zigzag position k
template <class Lev, class Put>
ADAS_HDI void jpeg_code_block(const uint32_t* dc_tab, const uint32_t* ac_tab, int dc_diff, Lev lev, Put put) {
    jpeg_code_block8(dc_tab, ac_tab, dc_diff, [&](int g, int* l) {
        for (int j = 0; j < 8; ++j) l[j] = lev(8 * g + j);
    }, put);
}

// A segment's bits are gathered in 32-bit words, most significant bit first.  `count` bits (1..27) at bit `pos`: *hi belongs into word
// pos >> 5, *lo (often 0) into the word behind it; OR them in.  jpeg_word_byte: byte j (0..3) of such a word in stream order.
ADAS_HDI void jpeg_split_bits(int pos, uint32_t bits, int count, uint32_t* hi, uint32_t* lo) {
    const unsigned long long v = (unsigned long long)bits << (64 - count - (pos & 31));
    *hi = (uint32_t)(v >> 32);
    *lo = (uint32_t)v;
}
ADAS_HDI uint32_t jpeg_word_byte(uint32_t w, int j) { return (w >> (24 - 8 * j)) & 255u; }
// the bits of the partial byte behind `nbytes` whole bytes, `n` of them (1..7), as a value: what the next round of blocks starts with
ADAS_HDI uint32_t jpeg_carry_bits(const uint32_t* buf, int nbytes, int n) { return jpeg_word_byte(buf[nbytes >> 2], nbytes & 3) >> (8 - n); }

// the block in a segment whose DC level block b (0 .. seg_blocks - 1, six per MCU) is predicted from; -1: the predictor is 0
ADAS_HDI int jpeg_dc_predecessor(int b) {
    const int k6 = b % 6;
    if (k6 >= 1 && k6 <= 3) return b - 1;
    if (b < 6) return -1;
    return k6 == 0 ? b - 3 : b - 6;
}

}  // namespace adas
