// Host build of the JPEG decoder's rules (csrc/jpegdec_core.h; g++, one thread): the functions the device kernels evaluate -- header walk,
// segment search, segment decoder, inverse transform, upsampling and colour -- composed frame by frame, with every stage's arrays handed out,
// so that the CPU suite can compare them with tests/jpegdec_ref.py and the GPU suite the device's frames with these.  Test scaffolding
// only; never loaded by the product.
#include <string.h>
#include <vector>
#include "jpegdec_core.h"

using namespace adas;

extern "C" {

double emu_jpegdec_idct_err(double norm) { return JPEGDEC_IDCT_ERR_BASE + JPEGDEC_IDCT_ERR_SLOPE * norm; }
double emu_jpegdec_idct_err_2048() { return JPEGDEC_IDCT_ERR; }
long long emu_jpegdec_cap_blocks(int w, int h) { return jpegdec_cap_blocks(w, h); }
long long emu_jpegdec_cap_segments(int w, int h) { return jpegdec_cap_segments(w, h); }

// coefficient blocks [n][64] (natural order) -> acc [n][64], the sums in front of the last rounding shift (p = acc / 2^17), and px [n][64]
void emu_jpegdec_idct(const int16_t* F, int n, int* acc, uint8_t* px) {
    for (int i = 0; i < n; ++i) {
        int f[64];
        for (int k = 0; k < 64; ++k) f[k] = F[(size_t)i * 64 + k];
        for (int v = 0; v < 8; ++v) jd_idct_pass(f + v * 8, 1, JPEGDEC_PASS1_ROUND, JPEGDEC_PASS1_SHIFT);
        for (int x = 0; x < 8; ++x) jd_idct_pass(f + x, 8, 0, 0);
        for (int k = 0; k < 64; ++k) {
            acc[(size_t)i * 64 + k] = f[k];
            px[(size_t)i * 64 + k] = (uint8_t)jd_sample((f[k] + JPEGDEC_PASS2_ROUND) >> JPEGDEC_PASS2_SHIFT);
        }
    }
}

// One stream -> flags; info [8] = ncomp, hs, vs, dri, mcux, mcuy, expected segments, found segments; coef [cap_blocks][64] and planes
// [cap_blocks * 64] as the device's arenas hold them (either may be null); bgr [h][w][3] (zeros for a rejected frame).
int emu_jpegdec_decode(const uint8_t* stream, long long length, long long capacity, int w, int h, int32_t* info, int16_t* coef, uint8_t* planes,
                       uint8_t* bgr) {
    const bool ok = length > 0 && length <= capacity;
    JdSrc s = jd_src(stream, ok ? length : 0);
    std::vector<JdFrame> rec(1);
    JdFrame* F = rec.data();
    jd_parse_header(s, length, capacity, w, h, F);
    const long long cap_blocks = jpegdec_cap_blocks(w, h), cap_segs = jpegdec_cap_segments(w, h);
    std::vector<int16_t> cf((size_t)cap_blocks * 64, 0);
    std::vector<uint8_t> pl((size_t)cap_blocks * 64, 0);
    std::vector<int32_t> seg((size_t)cap_segs * 2, 0);
    if (!(F->flags & JPEGDEC_REJECT)) {
        jd_find_segments(s, F, seg.data(), cap_segs);
    }
    if (!(F->flags & JPEGDEC_REJECT)) {      // the segment search may have met a second SOS
        uint8_t zz[64];
        jd_fill_zigzag(zz);
        long long ndec = F->found < F->nseg ? F->found : F->nseg;
        if (ndec > cap_segs) ndec = cap_segs;
        for (long long k = 0; k < ndec; ++k)
            if (!jd_decode_segment(s, F, zz, seg.data(), (int)k, cf.data())) F->flags |= JPEGDEC_CORRUPT;
        const long long nblk = jd_frame_blocks(F);
        for (int c = 0; c < F->ncomp; ++c) {
            const JdComp C = jd_comp(F, c);
            for (int by = 0; by < C.bh; ++by)
                for (int bx = 0; bx < C.bw; ++bx) {
                    const long long blk = C.off + (long long)by * C.bw + bx;
                    if (blk >= nblk) return -1;
                    int f[64];
                    for (int k = 0; k < 64; ++k) f[k] = cf[(size_t)blk * 64 + k];
                    jd_idct(f);
                    for (int y = 0; y < 8; ++y)
                        for (int x = 0; x < 8; ++x) pl[(size_t)C.off * 64 + ((size_t)by * 8 + y) * ((size_t)C.bw * 8) + (size_t)bx * 8 + x] = (uint8_t)jd_sample(f[y * 8 + x]);
                }
        }
    }
    if (info) {
        const int32_t v[8] = {F->ncomp, F->hs, F->vs, F->dri, F->mcux, F->mcuy, F->nseg, F->found};
        memcpy(info, v, sizeof(v));
    }
    if (coef) memcpy(coef, cf.data(), cf.size() * sizeof(int16_t));
    if (planes) memcpy(planes, pl.data(), pl.size());
    if (bgr) {
        if (F->flags & JPEGDEC_REJECT) {
            memset(bgr, 0, (size_t)w * h * 3);
        } else {
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    int p[3];
                    jd_pixel(F, pl.data(), w, h, x, y, p);
                    for (int c = 0; c < 3; ++c) bgr[((size_t)y * w + x) * 3 + c] = (uint8_t)p[c];
                }
        }
    }
    return F->flags;
}

// D7, D8 alone: planes as emu_jpegdec_decode hands them out, with the geometry (ncomp, hs, vs) -> bgr
void emu_jpegdec_colour(const uint8_t* planes, int w, int h, int ncomp, int hs, int vs, uint8_t* bgr) {
    std::vector<JdFrame> rec(1);
    JdFrame* F = rec.data();
    memset(F, 0, sizeof(*F));
    F->ncomp = ncomp;
    F->hs = hs;
    F->vs = vs;
    F->mcux = (w + 8 * hs - 1) / (8 * hs);
    F->mcuy = (h + 8 * vs - 1) / (8 * vs);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int p[3];
            jd_pixel(F, planes, w, h, x, y, p);
            for (int c = 0; c < 3; ++c) bgr[((size_t)y * w + x) * 3 + c] = (uint8_t)p[c];
        }
}

}  // extern "C"
