// jpegdec_core.h -- the rules of the baseline JPEG decoder behind adas_jpegdec_* (the line the demo starts its loop with, cap.read(), for a
// camera or file that delivers MJPEG): the counterpart of jpeg_core.h.  Written from ITU-T T.81, not from a library; the upsampling rule D7 is
// the triangle filter libjpeg documents, so that a frame decoded here and one decoded there differ by DCT rounding only.
// THE DEFINITIONS HERE ARE THE AUTHORITY; every rule is integer arithmetic, so host and device cannot disagree.
//   D1 streams   SOI; APPn, COM and stand-alone markers (TEM, a stray RSTm) are skipped; DQT with 8-bit entries, ids 0..3, several tables per
//                segment; SOF0 with 8-bit samples; DHT of class 0 / 1 and id 0 / 1, several tables per segment; DRI (0 included); one SOS over all
//                components with Ss = 0, Se = 63, Ah = Al = 0; entropy data; EOI (a missing one is tolerated, bytes behind it are ignored).  0xFF
//                fill bytes in front of a marker are accepted.  Components: one (grey, its sampling factors are ignored), or three with the first
//                sampled 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4) and the other two 1x1.  Component ids are not interpreted; the scan's components
//                are taken in the frame's order.  Three components are YCbCr unless an Adobe APP14 segment with transform 0 is present.
//   D2 flags     one word per frame, never an error code.  The header is walked once in stream order and the first violation met decides:
//                UNSUPPORTED  a valid JPEG outside D1: another SOFn, DAC, DNL, DHP, EXP, JPGn or reserved marker segment, a sample precision
//                             other than 8, a component count other than 1 or 3, other sampling factors, a 16-bit DQT, a DHT or scan table id of
//                             2..3, an SOS that does not cover all components (what a second SOS usually goes with) or has other Ss / Se / Ah / Al, the
//                             Adobe transform 0 with three components (checked at SOS); a second SOS among the marker segments that
//                             follow the scan's end (jd_second_scan, run by the segment search: the flag word is then UNSUPPORTED alone).
//                             Inside SOF0 the order is precision, count, sampling.
//                FORMAT       no SOI; a byte that is not 0xFF where a marker is due; SOI, EOI or 0xFF 0x00 in the header; a header or a segment
//                             that ends early or has a wrong length; a second SOF0; an SOS without SOF0; table ids above 3; a DQT precision
//                             above 1; a DHT class above 1, more than 256 values or counts that over-subscribe the code space (for some length l
//                             more than 2^l code words are used up); a table the scan refers to that is missing; a stream length of 0 or less
//                             or above the handle's capacity (nothing of such a stream is read).
//                SIZE         SOF0's width or height differ from the handle's (checked behind SOF0's UNSUPPORTED cases).
//                CORRUPT      an error in the entropy data (D3, D4).  A frame with one of the first three flags has every pixel 0; a CORRUPT
//                             frame is decoded as D4 says.  Frames do not influence each other.
//   D3 segments  an MCU is (8 hs) x (8 vs) pixels, hs, vs the first component's sampling (1, 1 for grey); mcux = ceil(w / 8 hs), mcuy =
//                ceil(h / 8 vs).  The scan starts behind the SOS segment and ends at the first position i with byte[i] = 0xFF, i + 1 < length and
//                byte[i + 1] none of 0x00, 0xFF, 0xD0..0xD7, or at the stream's length.  Every position i of the scan with byte[i] = 0xFF
//                and byte[i + 1] = 0xD0 + m is a restart marker; the r-th of them (from 0) ends segment r and segment r + 1 starts behind it.
//                Segment k holds the MCUs [k DRI, min((k + 1) DRI, mcux mcuy)); with DRI = 0 the scan is one segment.  The frame is CORRUPT
//                if some m != r mod 8 or if the segments found are not ceil(mcux mcuy / DRI) (1 for DRI = 0); min(found, expected) segments
//                are decoded all the same, each from its own bytes.
//   D4 entropy   Annex F.2.2 with the stream's tables; one DC predictor per component, 0 at a segment's start; inside a segment 0xFF 0x00 is
//                the byte 0xFF, and a 0xFF followed by anything else (fill, or the segment's last byte) ends the segment's data.  An error is:
//                16 bits that start no code word; a DC category above 11; an AC symbol with size above 10, or size 0 and a run other than 0
//                (EOB) or 15 (ZRL); a run that passes index 63 (ZRL from k > 48, or k + run > 63); the segment's data ending inside a block.
//                On an error the block it happens in and every later block of that segment have all-zero coefficients and the frame is CORRUPT.
//                Bits behind a segment's last block are ignored.
//                SAFETY, for any byte string of any content: the decoder reads only the aligned 32-bit words that hold bytes
//                [start, start + length) of a stream (a byte goes through jd_get, which refuses an index outside 0 .. length - 1 by
//                returning 0 without a read, or through jd_refill's four-byte path and the segment search's piece loads, which name only
//                words that hold a byte of the stream); it writes only into the frame record, the segment table, the coefficient and plane arenas (all
//                sized from the handle's width and height alone: jpegdec_cap_blocks, jpegdec_cap_segments; every index into them is derived
//                from mcux, mcuy, hs, vs, which SIZE pins to the handle's) and the destination frame; every loop consumes at least one byte of
//                the header, one bit of a segment (every code word is at least one bit long) or finishes a block, so a frame takes at most
//                c1 * length + c2 * blocks steps.
//   D5 dequant   level x q, clamped to -2048..2047; the DC level (predictor + difference) is clamped to -32768..32767 after every addition.  An
//                orthonormal 8x8 DCT of 8-bit samples cannot exceed +-1024: the clamps only bite on nonsense streams, and make int16 storage and
//                32-bit arithmetic safe.
//   D6 transform f = (1 / 8) M^T F M with the M of J4, held as K = round(8192 M): along the rows T[v][x] = (sum_u K[u][x] F[v][u] + 2048) >> 12
//                (twice the exact pass G), along the columns s[y][x] = (sum_v K[v][y] T[v][x] + 65536) >> 17, pixel = clamp(s + 128, 0, 255).
//                32 bits: sum_u |K[u][x]| = 61212 for every x, so |sum K F| <= 61212 * 2048 = 125362176 < 2^27, |T| <= 30606, and
//                |sum K T| <= 61212 * 30606 = 1873454472 < 2^31.  (One bit more in T would not fit; the constants are J4's by decision.)
//                Error of p = sum K T / 2^17, the value in front of the last rounding, against the exact f, with e = K - 8192 M (|e| <= 0.5,
//                0 in rows 0 and 4: six entries per column) and ||.|| the Euclidean norm of the block:
//                  rounding of T         (1 / 16) sum_v |M[v][y]| * 0.5 = 7.4722 / 32                                  <= 0.2336
//                  e in the first pass   (1 / 65536) ||M column|| sqrt(sum_v (0.5 sqrt 6 ||F row v||)^2) = sqrt 8 * 0.5 sqrt 6 ||F|| / 65536
//                                                                                                                        <= 5.29e-5 ||F||
//                  e in the second pass  0.5 sqrt 6 ||T column|| / 2^17, ||T column|| <= 2 sqrt 8 ||F|| + sqrt 8 (0.5 + 0.5 sqrt 6 ||F|| / 4096)
//                                                                                                                        <= 5.30e-5 ||F|| + 1.4e-5
//                |p - f| <= JPEGDEC_IDCT_ERR_BASE + JPEGDEC_IDCT_ERR_SLOPE ||F|| = 0.2337 + 1.06e-4 ||F||.  A block of 8-bit samples has
//                ||F|| <= 1024 (Parseval); for every block with ||F|| <= 2048 -- twice that, which covers what quantisation adds --
//                |p - f| <= JPEGDEC_IDCT_ERR = 0.451 < 0.5, so the pixel differs from round(f) by at most 1.  For the nonsense blocks the
//                D5 clamp still lets through (||F|| <= 8 * 2048) the bound grows to 1.97: with 13-bit constants no choice of shifts keeps
//                those below 0.5, and no decoder agrees with another on them.  Largest seen over the CPU suite: tests/test_jpegdec_cpu.py.
//   D7 chroma    the triangle filter, with edges at the true component size cw x ch = ceil(w / 2) x ceil(h / 2) (4:2:2: ceil(w / 2) x h), not at
//                the MCU-padded size.  4:2:0: s[i] = 3 near[i] + far[i], near the chroma row y >> 1, far the row above it for even y and below
//                it for odd y, clamped to 0 .. ch - 1; out[2i] = (3 s[i] + s[i - 1] + 8) >> 4, out[2i + 1] = (3 s[i] + s[i + 1] + 7) >> 4, and
//                (4 s[0] + 8) >> 4 at x = 0, (4 s[cw - 1] + 7) >> 4 at x = 2 cw - 1.  4:2:2: out[2i] = (3 c[i] + c[i - 1] + 1) >> 2,
//                out[2i + 1] = (3 c[i] + c[i + 1] + 2) >> 2, c[0] at x = 0 and c[cw - 1] at x = 2 cw - 1.  (For an odd w the column 2 cw - 1
//                lies outside the frame.)  Both rules were compared with libjpeg-turbo on the CPU: tests/test_jpegdec_cpu.py.
//   D8 colour    Cb' = Cb - 128, Cr' = Cr - 128: R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16),
//                G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), arithmetic shifts, each clamped to 0..255.  Grey: B = G = R = Y.  Output is
//                BGR u8 [batch][h][w][3], tightly packed: what adas_pipeline_step_frames takes.
//   D9           a frame's pixels and flags depend on its stream's bytes and the handle's (w, h, capacity) alone.
// The header compiles for the host as well (tests/hostemu/emu_jpegdec.cpp, tests/hostemu/jpegdec_fuzz_main.cpp).
#pragma once
#include <stdint.h>
#include "jpeg_core.h"

namespace adas {

#define JPEGDEC_UNSUPPORTED 1   /* ADAS_JPEGDEC_* */
#define JPEGDEC_FORMAT 2
#define JPEGDEC_SIZE 4
#define JPEGDEC_CORRUPT 8
#define JPEGDEC_REJECT (JPEGDEC_UNSUPPORTED | JPEGDEC_FORMAT | JPEGDEC_SIZE)   /* every pixel 0 */
#define JPEGDEC_IDCT_ERR_BASE 0.2337
#define JPEGDEC_IDCT_ERR_SLOPE 1.06e-4
#define JPEGDEC_IDCT_ERR 0.451       /* BASE + SLOPE * 2048, D6 */
#define JPEGDEC_MAX_CAPACITY 0x7fffffffLL   /* segment offsets are 32 bits */

// ---------------------------------------------------------------------------------------------------------------- the bytes of a stream
// A stream may start on any byte.  It is read through the aligned words that hold its bytes: word wi covers bytes 4 wi - a .. 4 wi - a + 3.
struct JdSrc {
    const uint32_t* q;   // the aligned word that holds byte 0
    int a;               // where byte 0 sits in it
    long long n;         // bytes
    long long wi;        // the word held in w; -1: none
    uint32_t w;
};
ADAS_HDI JdSrc jd_src(const uint8_t* p, long long n) {
    JdSrc s;
    const uintptr_t addr = (uintptr_t)p;
    s.q = (const uint32_t*)(addr & ~(uintptr_t)3);
    s.a = (int)(addr & 3);
    s.n = n > 0 ? n : 0;
    s.wi = -1;
    s.w = 0;
    return s;
}
// word wi, which holds at least one byte of the stream.  The device reads it whole; the host build, which runs under a sanitizer at the very
// end of a heap block, gathers the bytes that belong to the stream.
ADAS_HDI uint32_t jd_word(const JdSrc& s, long long wi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return s.q[wi];
#else
    const uint8_t* b = (const uint8_t*)s.q;
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j) {
        const long long i = wi * 4 + j - s.a;
        if (i >= 0 && i < s.n) w |= (uint32_t)b[wi * 4 + j] << (8 * j);
    }
    return w;
#endif
}
// byte i; an index outside the stream reads nothing and gives 0
ADAS_HDI int jd_get(JdSrc& s, long long i) {
    if (i < 0 || i >= s.n) return 0;
    const long long j = i + s.a;
    if ((j >> 2) != s.wi) {
        s.wi = j >> 2;
        s.w = jd_word(s, s.wi);
    }
    return (int)((s.w >> ((int)(j & 3) * 8)) & 255u);
}

// ---------------------------------------------------------------------------------------------------------------- what the header leaves
// A Huffman table in decode form (Annex F.2.2.3: maxcode, valptr - mincode) with a look-up of the first 8 bits in front
struct JdHuff {
    int32_t maxcode[18];   // [l], l = 1..16: the largest code of length l, -1: none
    int32_t valoff[18];    // [l]: index of the first value of length l minus its code
    int32_t nvals;
    int32_t defined;
    uint16_t look[256];    // the next 8 bits -> (length << 8) | value for a code of at most 8 bits, else 0
    uint8_t vals[256];
};
struct JdFrame {
    int32_t flags;
    int32_t ncomp;          // 1 or 3
    int32_t hs, vs;         // sampling of the first component (1, 1 for grey)
    int32_t dri;
    int32_t mcux, mcuy;
    int32_t nseg;           // segments D3 expects
    int32_t found;          // segments the scan holds (the segment search)
    int32_t scan_start, scan_end;
    int32_t adobe;          // transform byte of an Adobe APP14 segment + 1; 0: none
    int32_t have_sof;
    int32_t qdef;           // bit t: quantisation table t is defined
    uint8_t tq[4], td[4], ta[4];
    uint16_t q[4][64];      // zigzag order
    JdHuff huff[4];         // class * 2 + id
};

// the arenas of a frame are sized from the handle's width and height alone: blocks over all components in the largest geometry D1 allows
// (three planes of MCU-padded 4:2:0 luminance size), and segments (one MCU each in the smallest MCU)
ADAS_HDI long long jpegdec_cap_blocks(int w, int h) { return 3LL * (2 * ((w + 15) / 16)) * (2 * ((h + 15) / 16)); }
ADAS_HDI long long jpegdec_cap_segments(int w, int h) { return (long long)((w + 7) / 8) * ((h + 7) / 8); }

// where component c's blocks lie in a frame's coefficient arena ([block][64]) and its samples in the plane arena (64 bytes per block, rows of
// bw * 8 samples): bw x bh blocks from block `off`
struct JdComp {
    int hc, vc, bw, bh;
    long long off;
};
ADAS_HDI JdComp jd_comp(const JdFrame* F, int c) {
    JdComp k;
    k.hc = c == 0 ? F->hs : 1;
    k.vc = c == 0 ? F->vs : 1;
    k.bw = F->mcux * k.hc;
    k.bh = F->mcuy * k.vc;
    const long long n0 = (long long)F->mcux * F->hs * F->mcuy * F->vs, n1 = (long long)F->mcux * F->mcuy;
    k.off = c == 0 ? 0 : (c == 1 ? n0 : n0 + n1);
    return k;
}
ADAS_HDI long long jd_frame_blocks(const JdFrame* F) {
    const long long n0 = (long long)F->mcux * F->hs * F->mcuy * F->vs, n1 = (long long)F->mcux * F->mcuy;
    return F->ncomp == 3 ? n0 + 2 * n1 : n0;
}

// ---------------------------------------------------------------------------------------------------------------- D1, D2: the header
// Annex C and F.2.2.3 from BITS (16 counts at byte `at`) and the values behind them; false: over-subscribed
ADAS_HDI bool jd_build_huff(JdSrc& s, long long at, int nvals, JdHuff* H) {
    for (int i = 0; i < 256; ++i) H->look[i] = 0;
    for (int i = 0; i < 256; ++i) H->vals[i] = (uint8_t)(i < nvals ? jd_get(s, at + 16 + i) : 0);
    H->nvals = nvals;
    H->maxcode[0] = H->maxcode[17] = -1;
    H->valoff[0] = H->valoff[17] = 0;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = jd_get(s, at + l - 1);
        if (code + cnt > (1 << l)) return false;
        H->valoff[l] = k - code;
        H->maxcode[l] = cnt ? code + cnt - 1 : -1;
        if (l <= 8)
            for (int i = 0; i < cnt; ++i) {
                const int first = (code + i) << (8 - l), e = (l << 8) | H->vals[k + i];
                for (int j = 0; j < (1 << (8 - l)); ++j) H->look[first + j] = (uint16_t)e;
            }
        code = (code + cnt) << 1;
        k += cnt;
    }
    H->defined = 1;
    return true;
}

// Walks the markers of stream s up to the scan and fills *F (zeroed here first).  length: what the caller was given for the stream, s.n = 0 when
// it is outside 1..capacity.  Returns F->flags.
ADAS_HDI int jd_parse_header(JdSrc& s, long long length, long long capacity, int w, int h, JdFrame* F) {
    {
        uint32_t* z = (uint32_t*)F;
        for (unsigned i = 0; i < sizeof(JdFrame) / 4; ++i) z[i] = 0;
    }
    const long long n = s.n;
#define JD_FAIL(f) return F->flags = (f)
    if (length <= 0 || length > capacity || n != length) JD_FAIL(JPEGDEC_FORMAT);
    if (n < 2 || jd_get(s, 0) != 0xFF || jd_get(s, 1) != 0xD8) JD_FAIL(JPEGDEC_FORMAT);
    long long pos = 2;
    for (;;) {
        if (pos >= n || jd_get(s, pos) != 0xFF) JD_FAIL(JPEGDEC_FORMAT);
        while (pos < n && jd_get(s, pos) == 0xFF) ++pos;      // fill bytes and the marker's own 0xFF
        if (pos >= n) JD_FAIL(JPEGDEC_FORMAT);
        const int m = jd_get(s, pos++);
        if (m == 0x00 || m == 0xD8 || m == 0xD9) JD_FAIL(JPEGDEC_FORMAT);
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone
        if (pos + 2 > n) JD_FAIL(JPEGDEC_FORMAT);
        const int L = (jd_get(s, pos) << 8) | jd_get(s, pos + 1);
        if (L < 2 || pos + L > n) JD_FAIL(JPEGDEC_FORMAT);
        const long long b = pos + 2, e = pos + L;             // the segment's body
        if (m == 0xC0) {
            if (F->have_sof || L < 8) JD_FAIL(JPEGDEC_FORMAT);
            const int nf = jd_get(s, b + 5);
            if (L != 8 + 3 * nf) JD_FAIL(JPEGDEC_FORMAT);
            if (jd_get(s, b) != 8) JD_FAIL(JPEGDEC_UNSUPPORTED);
            if (nf != 1 && nf != 3) JD_FAIL(JPEGDEC_UNSUPPORTED);
            for (int c = 0; c < nf; ++c) {
                const int hv = jd_get(s, b + 6 + 3 * c + 1), t = jd_get(s, b + 6 + 3 * c + 2);
                if (t > 3) JD_FAIL(JPEGDEC_FORMAT);
                F->tq[c] = (uint8_t)t;
                if (nf == 3 && c == 0 && hv != 0x22 && hv != 0x21 && hv != 0x11) JD_FAIL(JPEGDEC_UNSUPPORTED);
                if (nf == 3 && c > 0 && hv != 0x11) JD_FAIL(JPEGDEC_UNSUPPORTED);
                if (c == 0) {
                    F->hs = nf == 3 ? hv >> 4 : 1;
                    F->vs = nf == 3 ? hv & 15 : 1;
                }
            }
            const int sh = (jd_get(s, b + 1) << 8) | jd_get(s, b + 2), sw = (jd_get(s, b + 3) << 8) | jd_get(s, b + 4);
            if (sw != w || sh != h) JD_FAIL(JPEGDEC_SIZE);
            F->ncomp = nf;
            F->mcux = (w + 8 * F->hs - 1) / (8 * F->hs);
            F->mcuy = (h + 8 * F->vs - 1) / (8 * F->vs);
            F->have_sof = 1;
        } else if (m == 0xDB) {
            long long p = b;
            while (p < e) {
                const int pt = jd_get(s, p);
                if ((pt >> 4) > 1 || (pt & 15) > 3) JD_FAIL(JPEGDEC_FORMAT);
                if ((pt >> 4) == 1) JD_FAIL(JPEGDEC_UNSUPPORTED);
                if (p + 65 > e) JD_FAIL(JPEGDEC_FORMAT);
                for (int k = 0; k < 64; ++k) F->q[pt & 15][k] = (uint16_t)jd_get(s, p + 1 + k);
                F->qdef |= 1 << (pt & 15);
                p += 65;
            }
        } else if (m == 0xC4) {
            long long p = b;
            while (p < e) {
                const int ct = jd_get(s, p);
                if ((ct >> 4) > 1 || (ct & 15) > 3) JD_FAIL(JPEGDEC_FORMAT);
                if ((ct & 15) > 1) JD_FAIL(JPEGDEC_UNSUPPORTED);
                if (p + 17 > e) JD_FAIL(JPEGDEC_FORMAT);
                int nv = 0;
                for (int l = 0; l < 16; ++l) nv += jd_get(s, p + 1 + l);
                if (nv > 256 || p + 17 + nv > e) JD_FAIL(JPEGDEC_FORMAT);
                if (!jd_build_huff(s, p + 1, nv, &F->huff[(ct >> 4) * 2 + (ct & 15)])) JD_FAIL(JPEGDEC_FORMAT);
                p += 17 + nv;
            }
        } else if (m == 0xDD) {
            if (L != 4) JD_FAIL(JPEGDEC_FORMAT);
            F->dri = (jd_get(s, b) << 8) | jd_get(s, b + 1);
        } else if (m == 0xDA) {
            if (!F->have_sof || L < 3) JD_FAIL(JPEGDEC_FORMAT);
            const int ns = jd_get(s, b);
            if (L != 6 + 2 * ns) JD_FAIL(JPEGDEC_FORMAT);
            if (ns != F->ncomp) JD_FAIL(JPEGDEC_UNSUPPORTED);
            for (int c = 0; c < ns; ++c) {
                const int t = jd_get(s, b + 1 + 2 * c + 1);
                if ((t >> 4) > 3 || (t & 15) > 3) JD_FAIL(JPEGDEC_FORMAT);
                if ((t >> 4) > 1 || (t & 15) > 1) JD_FAIL(JPEGDEC_UNSUPPORTED);
                F->td[c] = (uint8_t)(t >> 4);
                F->ta[c] = (uint8_t)(t & 15);
            }
            if (jd_get(s, b + 1 + 2 * ns) != 0 || jd_get(s, b + 2 + 2 * ns) != 63 || jd_get(s, b + 3 + 2 * ns) != 0) JD_FAIL(JPEGDEC_UNSUPPORTED);
            if (F->ncomp == 3 && F->adobe == 1) JD_FAIL(JPEGDEC_UNSUPPORTED);
            for (int c = 0; c < ns; ++c)
                if (!((F->qdef >> F->tq[c]) & 1) || !F->huff[F->td[c]].defined || !F->huff[2 + F->ta[c]].defined) JD_FAIL(JPEGDEC_FORMAT);
            const long long mcus = (long long)F->mcux * F->mcuy;
            F->nseg = F->dri ? (int32_t)((mcus + F->dri - 1) / F->dri) : 1;
            F->scan_start = F->scan_end = (int32_t)e;
            return F->flags;
        } else if (m >= 0xE0 && m <= 0xEF) {
            if (m == 0xEE && L >= 14 && jd_get(s, b) == 'A' && jd_get(s, b + 1) == 'd' && jd_get(s, b + 2) == 'o' && jd_get(s, b + 3) == 'b' &&
                jd_get(s, b + 4) == 'e')
                F->adobe = jd_get(s, b + 11) + 1;
        } else if (m != 0xFE) {
            JD_FAIL(JPEGDEC_UNSUPPORTED);
        }
        pos = e;
    }
#undef JD_FAIL
}

// ---------------------------------------------------------------------------------------------------------------- D3: the segments
// What a position of the scan is: 0 nothing, 1 + m a restart marker RSTm, -1 the scan's end
ADAS_HDI int jd_marker_at(JdSrc& s, long long i) {
    if (jd_get(s, i) != 0xFF || i + 1 >= s.n) return 0;
    const int m = jd_get(s, i + 1);
    if (m == 0x00 || m == 0xFF) return 0;
    return m >= 0xD0 && m <= 0xD7 ? 1 + (m & 7) : -1;
}
// D2's second SOS: the marker segments from the scan's end on are stepped over by their lengths, up to EOI, the stream's end or the first
// thing that is no marker segment; true when one of them is an SOS.  Every step consumes at least one byte.
ADAS_HDI bool jd_second_scan(JdSrc& s, long long pos) {
    const long long n = s.n;
    for (;;) {
        if (pos >= n || jd_get(s, pos) != 0xFF) return false;
        while (pos < n && jd_get(s, pos) == 0xFF) ++pos;
        if (pos >= n) return false;
        const int m = jd_get(s, pos++);
        if (m == 0xDA) return true;
        if (m == 0x00 || m == 0xD8 || m == 0xD9) return false;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (pos + 2 > n) return false;
        const int L = (jd_get(s, pos) << 8) | jd_get(s, pos + 1);
        if (L < 2 || pos + L > n) return false;
        pos += L;
    }
}
// what the segment search leaves in the record: a second SOS makes the frame UNSUPPORTED (and black), else D3's CORRUPT cases
ADAS_HDI void jd_finish_segments(JdSrc& s, JdFrame* F, long long end, int found, int bad) {
    F->scan_end = (int32_t)end;
    F->found = found;
    if (jd_second_scan(s, end)) F->flags = JPEGDEC_UNSUPPORTED;
    else if (bad || found != F->nseg) F->flags |= JPEGDEC_CORRUPT;
}
// One thread's version of the segment search: seg[k][2] = first byte and end of segment k, k < cap; fills F->found, F->scan_end and the D3 part
// of F->flags.  (The device finds the markers in parallel, jpegdec_kernels.hip, and must give the same table.)
ADAS_HDI void jd_find_segments(JdSrc& s, JdFrame* F, int32_t* seg, long long cap) {
    long long i = F->scan_start;
    int r = 0, bad = 0;
    seg[0] = F->scan_start;
    for (; i < s.n; ++i) {
        const int k = jd_marker_at(s, i);
        if (k < 0) break;
        if (k > 0) {
            if (k - 1 != (r & 7)) bad = 1;
            if (r < cap) seg[2 * r + 1] = (int32_t)i;
            ++r;
            if (r < cap) seg[2 * r] = (int32_t)(i + 2);
        }
    }
    if (r < cap) seg[2 * r + 1] = (int32_t)i;
    jd_finish_segments(s, F, i, r + 1, bad);
}

// ---------------------------------------------------------------------------------------------------------------- D4, D5: a segment
struct JdBits {
    unsigned long long acc;   // the next n bits, from bit 63 down
    int n;
    long long pos, end;
    bool dry;                 // the segment's data has ended
};
ADAS_HDI void jd_refill(JdSrc& s, JdBits& B) {
    if (B.n <= 32 && !B.dry && B.pos + 4 <= B.end) {      // four bytes at once when none of them is 0xFF; what the loop below would do with them
        const long long j = B.pos + s.a, wi = j >> 2;
        const int sh = (int)(j & 3) * 8;
        const uint32_t lo = wi == s.wi ? s.w : jd_word(s, wi);
        uint32_t v = lo;
        s.wi = wi;
        s.w = lo;
        if (sh) {                                          // the stream's byte pos + 3 lies in the next word
            const uint32_t hi = jd_word(s, wi + 1);
            v = (lo >> sh) | (hi << (32 - sh));
            s.wi = wi + 1;
            s.w = hi;
        }
        if (!((~v - 0x01010101u) & v & 0x80808080u)) {
            B.acc |= (unsigned long long)__builtin_bswap32(v) << (32 - B.n);
            B.n += 32;
            B.pos += 4;
            return;
        }
    }
    while (B.n <= 56 && !B.dry) {
        if (B.pos >= B.end) {
            B.dry = true;
            break;
        }
        const int b = jd_get(s, B.pos);
        if (b == 0xFF) {
            if (B.pos + 1 < B.end && jd_get(s, B.pos + 1) == 0) {
                B.pos += 2;
            } else {
                B.dry = true;
                break;
            }
        } else {
            ++B.pos;
        }
        B.acc |= (unsigned long long)b << (56 - B.n);
        B.n += 8;
    }
}
// the next symbol of table H; -1: an error
ADAS_HDI int jd_symbol(JdSrc& s, JdBits& B, const JdHuff* H) {
    if (B.n < 16) jd_refill(s, B);
    const int p = (int)(B.acc >> 48);
    int l, v = -1;
    const int e = H->look[p >> 8];
    if (e) {
        l = e >> 8;
        v = e & 255;
    } else {
        for (l = 9; l <= 16; ++l) {
            const int c = p >> (16 - l);
            if (c <= H->maxcode[l]) {
                const int idx = H->valoff[l] + c;
                if (idx >= 0 && idx < H->nvals) v = H->vals[idx];
                break;
            }
        }
        if (v < 0) return -1;
    }
    if (l > B.n) return -1;
    B.acc <<= l;
    B.n -= l;
    return v;
}
// Annex F.2.2.1 RECEIVE and EXTEND of `size` bits (1..11); false: the data ended
ADAS_HDI bool jd_receive(JdSrc& s, JdBits& B, int size, int* v) {
    if (B.n < size) jd_refill(s, B);
    if (size > B.n) return false;
    const int x = (int)(B.acc >> (64 - size));
    B.acc <<= size;
    B.n -= size;
    *v = x >> (size - 1) ? x : x - (1 << size) + 1;
    return true;
}
ADAS_HDI int jd_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One block into o[64] (natural order, all zero on entry): false on an error, with o zero again
ADAS_HDI void jd_fill_zigzag(uint8_t* zz) {
    for (int k = 0; k < 64; ++k) zz[k] = (uint8_t)jpeg_zigzag(k);
}
// zz: jd_fill_zigzag's table, wherever the caller keeps it
ADAS_HDI bool jd_decode_block(JdSrc& s, JdBits& B, const JdHuff* dc, const JdHuff* ac, const uint16_t* q, const uint8_t* zz, int* pred, int16_t* o) {
    bool ok = true;
    const int t = jd_symbol(s, B, dc);
    int d = 0;
    if (t < 0 || t > 11) ok = false;
    else if (t > 0) ok = jd_receive(s, B, t, &d);
    if (ok) {
        *pred = jd_clamp(*pred + d, -32768, 32767);
        o[0] = (int16_t)jd_clamp(*pred * (int)q[0], -2048, 2047);
        int k = 1;
        while (k < 64) {
            const int rs = jd_symbol(s, B, ac);
            if (rs < 0) {
                ok = false;
                break;
            }
            const int run = rs >> 4, size = rs & 15;
            if (size == 0) {
                if (run == 0) break;
                if (run != 15 || k > 48) {
                    ok = false;
                    break;
                }
                k += 16;
                continue;
            }
            k += run;
            int v;
            if (size > 10 || k > 63 || !jd_receive(s, B, size, &v)) {
                ok = false;
                break;
            }
            o[zz[k]] = (int16_t)jd_clamp(v * (int)q[k], -2048, 2047);
            ++k;
        }
    }
    if (!ok)
        for (int i = 0; i < 64; ++i) o[i] = 0;
    return ok;
}

// Segment k of a frame whose table is seg: its MCUs' coefficients into coef (the frame's arena, zero on entry).  false: CORRUPT
ADAS_HDI bool jd_decode_segment(JdSrc& s, const JdFrame* F, const uint8_t* zz, const int32_t* seg, int k, int16_t* coef) {
    JdBits B;
    B.acc = 0;
    B.n = 0;
    B.pos = seg[2 * k];
    B.end = seg[2 * k + 1];
    B.dry = false;
    if (B.end > s.n) B.end = s.n;
    const long long mcus = (long long)F->mcux * F->mcuy;      // at most jpegdec_cap_segments: fits an int
    const long long m0 = F->dri ? (long long)k * F->dri : 0;
    const long long m1 = F->dri ? (m0 + F->dri < mcus ? m0 + F->dri : mcus) : mcus;
    const JdComp C0 = jd_comp(F, 0), C1 = jd_comp(F, 1), C2 = jd_comp(F, 2);
    int pred[3] = {0, 0, 0};
    int mx = (int)(m0 % F->mcux), my = (int)(m0 / F->mcux);
    for (long long m = m0; m < m1; ++m) {
        for (int c = 0; c < F->ncomp; ++c) {
            const JdComp& C = c == 0 ? C0 : (c == 1 ? C1 : C2);
            const JdHuff *dc = &F->huff[F->td[c]], *ac = &F->huff[2 + F->ta[c]];
            const uint16_t* q = F->q[F->tq[c]];
            for (int v = 0; v < C.vc; ++v)
                for (int hh = 0; hh < C.hc; ++hh) {
                    const long long blk = C.off + (long long)(my * C.vc + v) * C.bw + mx * C.hc + hh;
                    if (!jd_decode_block(s, B, dc, ac, q, zz, &pred[c], coef + blk * 64)) return false;
                }
        }
        if (++mx == F->mcux) {
            mx = 0;
            ++my;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- D6: the inverse transform
// out[x] = (sum_u K[u][x] a[u] + round) >> shift over a[0], a[stride], ..., in place: the even u give the mirrored sums, the odd u the differences
ADAS_HDI void jd_idct_pass(int* a, int stride, int round, int shift) {
    constexpr int K[8][4] = {{8192, 8192, 8192, 8192},   {11363, 9633, 6436, 2260},   {10703, 4433, -4433, -10703}, {9633, -2260, -11363, -6436},
                             {8192, -8192, -8192, 8192}, {6436, -11363, 2260, 9633}, {4433, -10703, 10703, -4433}, {2260, -6436, 9633, -11363}};
    int in[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) in[u] = a[u * stride];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int ev = K[0][x] * in[0] + K[2][x] * in[2] + K[4][x] * in[4] + K[6][x] * in[6];
        const int od = K[1][x] * in[1] + K[3][x] * in[3] + K[5][x] * in[5] + K[7][x] * in[7];
        a[x * stride] = (ev + od + round) >> shift;
        a[(7 - x) * stride] = (ev - od + round) >> shift;
    }
}
#define JPEGDEC_PASS1_ROUND 2048
#define JPEGDEC_PASS1_SHIFT 12
#define JPEGDEC_PASS2_ROUND 65536
#define JPEGDEC_PASS2_SHIFT 17
ADAS_HDI int jd_sample(int s) { return jd_clamp(s + 128, 0, 255); }
// F [64] coefficients (natural order) -> s [64], the samples in front of the level shift, in place
ADAS_HDI void jd_idct(int* f) {
#pragma unroll
    for (int v = 0; v < 8; ++v) jd_idct_pass(f + v * 8, 1, JPEGDEC_PASS1_ROUND, JPEGDEC_PASS1_SHIFT);
#pragma unroll
    for (int x = 0; x < 8; ++x) jd_idct_pass(f + x, 8, JPEGDEC_PASS2_ROUND, JPEGDEC_PASS2_SHIFT);
}

// ---------------------------------------------------------------------------------------------------------------- D7, D8: a pixel
// chroma sample of component c at pixel (x, y) from the frame's planes
ADAS_HDI int jd_chroma(const JdFrame* F, const uint8_t* planes, int w, int h, int c, int x, int y) {
    const JdComp C = jd_comp(F, c);
    const uint8_t* p = planes + C.off * 64;
    const int pw = C.bw * 8;
    if (F->hs == 1) return p[(size_t)y * pw + x];
    const int cw = (w + 1) / 2, j = x >> 1;
    if (F->vs == 1) {
        const uint8_t* r = p + (size_t)y * pw;
        if (x & 1) return j == cw - 1 ? r[j] : (3 * r[j] + r[j + 1] + 2) >> 2;
        return j == 0 ? r[0] : (3 * r[j] + r[j - 1] + 1) >> 2;
    }
    const int ch = (h + 1) / 2, i = y >> 1;
    const int fi = (y & 1) ? (i + 1 < ch ? i + 1 : ch - 1) : (i > 0 ? i - 1 : 0);
    const uint8_t *near = p + (size_t)i * pw, *far = p + (size_t)fi * pw;
    const int s = 3 * near[j] + far[j];
    if (x & 1) return j == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[j + 1] + far[j + 1] + 7) >> 4;
    return j == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[j - 1] + far[j - 1] + 8) >> 4;
}
ADAS_HDI void jd_colour(int Y, int cb, int cr, int* bgr) {
    cb -= 128;
    cr -= 128;
    bgr[2] = jd_clamp(Y + ((91881 * cr + 32768) >> 16), 0, 255);
    bgr[0] = jd_clamp(Y + ((116130 * cb + 32768) >> 16), 0, 255);
    bgr[1] = jd_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
}
// pixel (x, y) of a frame that carries none of the JPEGDEC_REJECT flags
ADAS_HDI void jd_pixel(const JdFrame* F, const uint8_t* planes, int w, int h, int x, int y, int* bgr) {
    const int Y = planes[(size_t)y * (F->mcux * F->hs * 8) + x];
    if (F->ncomp == 1) {
        bgr[0] = bgr[1] = bgr[2] = Y;
        return;
    }
    jd_colour(Y, jd_chroma(F, planes, w, h, 1, x, y), jd_chroma(F, planes, w, h, 2, x, y), bgr);
}

}  // namespace adas
