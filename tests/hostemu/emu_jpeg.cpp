// Host build of the JPEG encoder's rules (csrc/jpeg_core.h; g++, one thread): the block functions the device kernels evaluate -- sampling,
// transform, quantiser, the block coder -- composed segment by segment into a whole stream, so that the CPU suite can compare them byte for
// byte with tests/jpeg_ref.py and the GPU suite the device's streams with these.  Test scaffolding only; never loaded by the product.
#include <string.h>
#include <vector>
#include "jpeg_core.h"

using namespace adas;

namespace {

struct BitWriter {   // J6: most significant bit first, 0x00 behind every 0xFF
    std::vector<uint8_t>* out;
    uint32_t acc = 0;
    int n = 0;
    void put(uint32_t bits, int count) {
        for (int i = count - 1; i >= 0; --i) {
            acc = (acc << 1) | ((bits >> i) & 1u);
            if (++n == 8) flush();
        }
    }
    void flush() {
        out->push_back((uint8_t)acc);
        if ((uint8_t)acc == 0xFF) out->push_back(0);
        acc = 0;
        n = 0;
    }
    void pad() {
        while (n) put(1, 1);
    }
};

void frame_levels(const uint8_t* frame, const JpegGeom& g, const JpegTables& T, int16_t* levels) {
    for (int seg = 0; seg < g.mcu_h; ++seg)
        for (int b = 0; b < g.seg_blocks; ++b) {
            int v[64];
            const int k6 = b % 6;
            jpeg_load_block(frame, g.w, g.h, seg, b / 6, k6, v);
            jpeg_fdct(v);
            int16_t* dst = levels + ((size_t)seg * g.seg_blocks + b) * 64;
            for (int k = 0; k < 64; ++k) dst[k] = (int16_t)jpeg_quantise(v[jpeg_zigzag(k)], T.q[k6 >= 4][k], k > 0);
        }
}

// One segment the way jpeg_entropy_kernel composes it: `round` blocks at a time, each block's bits ORed into a word buffer at the prefix sum of
// the bit counts, whole bytes stuffed out of the words, the bits of the last partial byte carried into the next round.
bool segment_in_rounds(const int16_t* lv, int nblk, const JpegTables& T, int round, std::vector<uint8_t>* s) {
    std::vector<uint32_t> buf;
    int carry_n = 0;
    uint32_t carry_v = 0;
    auto or_bits = [&](int pos, uint32_t bits, int count) {
        uint32_t hi, lo;
        jpeg_split_bits(pos, bits, count, &hi, &lo);
        buf[pos >> 5] |= hi;
        if (lo) buf[(pos >> 5) + 1] |= lo;
    };
    auto code = [&](int b, auto put) {
        const int cls = (b % 6) >= 4, pb = jpeg_dc_predecessor(b);
        const int16_t* blk = lv + (size_t)b * 64;
        jpeg_code_block(T.dc[cls], T.ac[cls], blk[0] - (pb >= 0 ? lv[(size_t)pb * 64] : 0), [&](int k) { return (int)blk[k]; }, put);
    };
    for (int c0 = 0; c0 < nblk; c0 += round) {
        const int c1 = c0 + round < nblk ? c0 + round : nblk;
        std::vector<int> at(c1 - c0);
        int total = carry_n;
        for (int b = c0; b < c1; ++b) {
            at[b - c0] = total;
            code(b, [&](uint32_t, int n) { total += n; });
        }
        if (total - carry_n > (c1 - c0) * JPEG_BLOCK_MAX_BITS) return false;
        buf.assign((size_t)(total + 31) / 32 + 2, 0u);
        if (carry_n) or_bits(0, carry_v, carry_n);
        for (int b = c0; b < c1; ++b) {
            int pos = at[b - c0];
            code(b, [&](uint32_t bits, int n) {
                or_bits(pos, bits, n);
                pos += n;
            });
        }
        const bool last = c1 == nblk;
        const int rem = total & 7;
        int nbytes = total >> 3;
        if (last && rem) {
            or_bits(total, (1u << (8 - rem)) - 1u, 8 - rem);
            ++nbytes;
        }
        carry_n = last ? 0 : rem;
        carry_v = carry_n ? jpeg_carry_bits(buf.data(), nbytes, carry_n) : 0u;
        for (int i = 0; i < nbytes; ++i) {
            const uint32_t v = jpeg_word_byte(buf[i >> 2], i & 3);
            s->push_back((uint8_t)v);
            if (v == 255u) s->push_back(0);
        }
    }
    return true;
}

}  // namespace

extern "C" {

int emu_jpeg_header_bytes() { return JPEG_HEADER_BYTES; }
int emu_jpeg_zigzag(int k) { return jpeg_zigzag(k); }
int emu_jpeg_zigzag_position(int natural) { return jpeg_zigzag_position(natural); }
double emu_jpeg_fdct_err() { return JPEG_FDCT_ERR; }
long long emu_jpeg_bound(int w, int h) { return jpeg_bound(w, h); }

// q [2][64]: the divisors in zigzag order
void emu_jpeg_tables(int quality, uint16_t* q) {
    JpegTables T;
    jpeg_build_tables(quality, &T);
    memcpy(q, T.q, sizeof(T.q));
}

int emu_jpeg_header(int w, int h, int quality, uint8_t* out) { return jpeg_build_header(w, h, quality, out); }

// f [n][64] level-shifted samples -> F' [n][64], natural order
void emu_jpeg_fdct(const int* f, int* F, int n) {
    for (int i = 0; i < n; ++i) {
        memcpy(F + (size_t)i * 64, f + (size_t)i * 64, 64 * sizeof(int));
        jpeg_fdct(F + (size_t)i * 64);
    }
}

void emu_jpeg_quantise(const int* F, const int* d, const int* ac, int* level, int n) {
    for (int i = 0; i < n; ++i) level[i] = jpeg_quantise(F[i], d[i], ac[i] != 0);
}

// the samples of one block (level-shifted), J1-J3
void emu_jpeg_load_block(const uint8_t* frame, int w, int h, int my, int mx, int k6, int* f) { jpeg_load_block(frame, w, h, my, mx, k6, f); }

// levels [mcu_h][seg_blocks][64] of one frame, zigzag order
void emu_jpeg_levels(const uint8_t* frame, int w, int h, int quality, int16_t* levels) {
    JpegTables T;
    jpeg_build_tables(quality, &T);
    frame_levels(frame, jpeg_geometry(w, h), T, levels);
}

// frames [n][h][w][3] -> out [n][capacity] (the caller's bytes stay where nothing is written), lengths [n], flags [n]
// round: 0 -- one bit writer per segment; > 0 -- the kernel's composition, `round` blocks at a time (256 on the device)
int emu_jpeg_encode(const uint8_t* frames, int n, int w, int h, int quality, long long capacity, int round, uint8_t* out, long long* lengths,
                    int32_t* flags) {
    if (w < 1 || h < 1 || w > JPEG_MAX_DIM || h > JPEG_MAX_DIM || quality < 1 || quality > 100 || capacity < JPEG_HEADER_BYTES) return -1;
    const JpegGeom g = jpeg_geometry(w, h);
    JpegTables T;
    jpeg_build_tables(quality, &T);
    uint8_t hdr[JPEG_HEADER_BYTES];
    if (jpeg_build_header(w, h, quality, hdr) != JPEG_HEADER_BYTES) return -2;
    std::vector<int16_t> levels((size_t)g.blocks * 64);
    for (int f = 0; f < n; ++f) {
        frame_levels(frames + (size_t)f * h * w * 3, g, T, levels.data());
        std::vector<uint8_t> s(hdr, hdr + JPEG_HEADER_BYTES);
        for (int seg = 0; seg < g.mcu_h; ++seg) {
            const int16_t* lv = levels.data() + (size_t)seg * g.seg_blocks * 64;
            const size_t start = s.size();
            BitWriter bw{&s};
            if (round > 0 && !segment_in_rounds(lv, g.seg_blocks, T, round, &s)) return -3;
            for (int b = 0; b < g.seg_blocks && round <= 0; ++b) {
                const int cls = (b % 6) >= 4, pb = jpeg_dc_predecessor(b);
                const int diff = lv[(size_t)b * 64] - (pb >= 0 ? lv[(size_t)pb * 64] : 0);
                const int16_t* blk = lv + (size_t)b * 64;
                int bits = 0;
                jpeg_code_block(T.dc[cls], T.ac[cls], diff, [&](int k) { return (int)blk[k]; }, [&](uint32_t v, int c) {
                    bw.put(v, c);
                    bits += c;
                });
                if (bits > JPEG_BLOCK_MAX_BITS) return -3;
            }
            bw.pad();
            if ((long long)(s.size() - start) > (long long)g.seg_blocks * JPEG_BLOCK_MAX_BYTES) return -4;   // the device's segment slot
            if (seg + 1 < g.mcu_h) {
                s.push_back(0xFF);
                s.push_back((uint8_t)(0xD0 + (seg & 7)));
            }
        }
        s.push_back(0xFF);
        s.push_back(0xD9);
        if ((long long)s.size() > jpeg_bound(w, h)) return -5;
        if ((long long)s.size() > capacity) {
            lengths[f] = 0;
            flags[f] = JPEG_OVERFLOW;
        } else {
            memcpy(out + (size_t)f * capacity, s.data(), s.size());
            lengths[f] = (long long)s.size();
            flags[f] = 0;
        }
    }
    return 0;
}

}  // extern "C"
