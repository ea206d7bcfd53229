// Stand-alone bounds check of the JPEG decoder's rules (csrc/jpegdec_core.h, D4's safety property):
//     jpegdec_fuzz [-n mutations_per_seed] W:H:file ...
// decodes each seed stream (a handle of W x H) and a deterministic set of mutations of it -- byte flips, truncations, edited header fields,
// planted markers, wrong declared lengths -- the way the device composes a run: header, segment search, segments, transform, pixels.  Every
// stream is copied to the very end of an exact-size heap block and every arena is an exact-size heap block, so a build with
// -fsanitize=address,undefined reports any read or write outside them; a plain build checks that every decode returns with documented
// flags only.  Exit status 0: all of them did.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "jpegdec_core.h"

using namespace adas;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// flags, or -1 for an undocumented outcome
static int decode(const uint8_t* data, long long n, long long told, long long capacity, int w, int h, unsigned* checksum) {
    uint8_t* block = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);      // the stream ends where the block ends
    if (n > 0) memcpy(block, data, (size_t)n);
    const bool ok = told > 0 && told <= capacity && told <= n;     // the caller's length never exceeds what it owns
    JdSrc s = jd_src(block, ok ? told : 0);
    JdFrame* F = (JdFrame*)malloc(sizeof(JdFrame));
    const long long cap_blocks = jpegdec_cap_blocks(w, h), cap_segs = jpegdec_cap_segments(w, h);
    int16_t* coef = (int16_t*)calloc((size_t)cap_blocks * 64, sizeof(int16_t));
    uint8_t* planes = (uint8_t*)calloc((size_t)cap_blocks * 64, 1);
    int32_t* seg = (int32_t*)calloc((size_t)cap_segs * 2, sizeof(int32_t));
    uint8_t* bgr = (uint8_t*)calloc((size_t)w * h * 3, 1);
    jd_parse_header(s, ok ? told : 0, capacity, w, h, F);
    int rc = F->flags;
    if (!(F->flags & JPEGDEC_REJECT)) {
        jd_find_segments(s, F, seg, cap_segs);
    }
    if (!(F->flags & JPEGDEC_REJECT)) {      // the segment search may have met a second SOS
        uint8_t zz[64];
        jd_fill_zigzag(zz);
        long long ndec = F->found < F->nseg ? F->found : F->nseg;
        if (ndec > cap_segs) ndec = cap_segs;
        for (long long k = 0; k < ndec; ++k)
            if (!jd_decode_segment(s, F, zz, seg, (int)k, coef)) F->flags |= JPEGDEC_CORRUPT;
        for (int c = 0; c < F->ncomp; ++c) {
            const JdComp C = jd_comp(F, c);
            for (int by = 0; by < C.bh; ++by)
                for (int bx = 0; bx < C.bw; ++bx) {
                    int f[64];
                    const long long blk = C.off + (long long)by * C.bw + bx;
                    for (int k = 0; k < 64; ++k) f[k] = coef[(size_t)blk * 64 + k];
                    jd_idct(f);
                    for (int y = 0; y < 8; ++y)
                        for (int x = 0; x < 8; ++x) planes[(size_t)C.off * 64 + ((size_t)by * 8 + y) * ((size_t)C.bw * 8) + (size_t)bx * 8 + x] = (uint8_t)jd_sample(f[y * 8 + x]);
                }
        }
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                int p[3];
                jd_pixel(F, planes, w, h, x, y, p);
                for (int c = 0; c < 3; ++c) bgr[((size_t)y * w + x) * 3 + c] = (uint8_t)p[c];
            }
        rc = F->flags;
        if (rc & ~JPEGDEC_CORRUPT) rc = -1;
    } else {
        rc = F->flags;
        if (rc != JPEGDEC_UNSUPPORTED && rc != JPEGDEC_FORMAT && rc != JPEGDEC_SIZE) rc = -1;
    }
    for (size_t i = 0; i < (size_t)w * h * 3; ++i) *checksum = *checksum * 31u + bgr[i];
    free(block); free(F); free(coef); free(planes); free(seg); free(bgr);
    return rc;
}

int main(int argc, char** argv) {
    int per_seed = 400, first = 1;
    if (argc > 2 && !strcmp(argv[1], "-n")) {
        per_seed = atoi(argv[2]);
        first = 3;
    }
    long long total = 0, by_flag[16] = {0};
    unsigned checksum = 0;
    for (int a = first; a < argc; ++a) {
        int w = 0, h = 0, at = 0;
        if (sscanf(argv[a], "%d:%d:%n", &w, &h, &at) < 2 || at == 0 || w < 1 || h < 1 || w > 4096 || h > 4096) {
            fprintf(stderr, "bad argument %s (W:H:file)\n", argv[a]);
            return 2;
        }
        FILE* fp = fopen(argv[a] + at, "rb");
        if (!fp) {
            fprintf(stderr, "cannot read %s\n", argv[a] + at);
            return 2;
        }
        std::vector<uint8_t> seed;
        uint8_t tmp[4096];
        size_t got;
        while ((got = fread(tmp, 1, sizeof(tmp), fp)) > 0) seed.insert(seed.end(), tmp, tmp + got);
        fclose(fp);
        const long long n = (long long)seed.size(), capacity = n + 64;
        size_t header = 0;      // the bytes in front of the scan: where header fields live
        for (size_t i = 0; i + 1 < seed.size(); ++i)
            if (seed[i] == 0xFF && seed[i + 1] == 0xDA) {
                header = i + 14;
                break;
            }
        if (header > seed.size()) header = seed.size();
        for (int m = 0; m <= per_seed; ++m) {
            std::vector<uint8_t> s = seed;
            long long told = -1;
            if (m > 0 && !s.empty()) {
                switch (m % 8) {
                case 0:       // a few byte flips anywhere
                    for (int k = 1 + (int)(rnd() % 4); k > 0; --k) s[rnd() % s.size()] ^= (uint8_t)(1u << (rnd() % 8));
                    break;
                case 1:       // truncated anywhere
                    s.resize(rnd() % s.size());
                    break;
                case 2:       // a header byte replaced
                    if (header) s[rnd() % header] = (uint8_t)rnd();
                    break;
                case 3:       // a header byte made an extreme
                    if (header) s[rnd() % header] = (rnd() & 1) ? 0xFF : 0x00;
                    break;
                case 4: {     // a marker planted anywhere
                    const size_t i = rnd() % s.size();
                    s[i] = 0xFF;
                    if (i + 1 < s.size()) s[i + 1] = (uint8_t)(0xC0 + rnd() % 64);
                    break;
                }
                case 5:       // scan bytes replaced by random ones
                    for (int k = 1 + (int)(rnd() % 16); k > 0; --k) s[header < s.size() ? header + rnd() % (s.size() - header) : s.size() - 1] = (uint8_t)rnd();
                    break;
                case 6:       // truncated inside the header
                    s.resize(header ? rnd() % header : 0);
                    break;
                default:      // a declared length that is not the stream's: shorter, zero, negative, above the capacity
                    told = (long long)(rnd() % (2 * s.size() + 200)) - 50;
                    break;
                }
            }
            const long long len = (long long)s.size();
            const int rc = decode(s.data(), len, told == -1 ? len : told, capacity, w, h, &checksum);
            if (rc < 0) {
                fprintf(stderr, "%s mutation %d: undocumented flags\n", argv[a], m);
                return 1;
            }
            if (m == 0 && rc != 0 && rc != JPEGDEC_UNSUPPORTED) {
                fprintf(stderr, "%s: the seed itself decodes with flags %d\n", argv[a], rc);
                return 1;
            }
            ++by_flag[rc & 15];
            ++total;
        }
    }
    printf("jpegdec_fuzz: %lld decodes, flags 0: %lld, UNSUPPORTED %lld, FORMAT %lld, SIZE %lld, CORRUPT %lld, checksum %08x\n", total, by_flag[0],
           by_flag[1], by_flag[2], by_flag[4], by_flag[8], checksum);
    return 0;
}
