// Host build of csrc/overlay_core.h (g++, one thread): the pixel rules the device kernels run, composed the way the kernels compose them
// (coverage bit planes first, then one pass over the pixels), so that the CPU suite can compare them byte for byte with tests/overlay_ref.py.
// Test scaffolding only; never loaded by the product.
#include <string.h>
#include <algorithm>
#include <vector>
#include "overlay_core.h"

using namespace adas;

namespace {

struct RowOps {   // overlay_poly_edge_row on one row's bit arrays
    uint32_t *fillw, *togw;
    void fill(int xl, int xr) {
        for (int w = xl >> 5; w <= (xr >> 5); ++w) fillw[w] |= overlay_word_mask(xl, xr, w);
    }
    void set(int q) { fillw[q >> 5] |= 1u << (q & 31); }
    void toggle(int t) { togw[t >> 5] ^= 1u << (t & 31); }
};

// ORs `bit` into cov [H][W] on the polygon's coverage; returns ADAS_OVERLAY_POLY_RANGE's condition
int poly_cover(const int* pts, int n, int H, int W, uint8_t* cov, uint8_t bit) {
    if (n <= 0) return 0;
    if (!overlay_poly_in_range(pts, n)) return 1;
    const int rw = (W + 31) / 32;
    std::vector<uint32_t> fillw(rw), togw(rw);
    for (int y = 0; y < H; ++y) {
        std::fill(fillw.begin(), fillw.end(), 0u);
        std::fill(togw.begin(), togw.end(), 0u);
        RowOps ops{fillw.data(), togw.data()};
        for (int e = 0; e < n; ++e) overlay_poly_edge_row(pts, n, e, y, W, ops);
        uint32_t carry = 0u;
        for (int w = 0; w < rw; ++w) {
            const uint32_t m = overlay_prefix_xor(togw[w], carry) | fillw[w];
            carry ^= (uint32_t)__builtin_popcount(togw[w]) & 1u;
            for (int b = 0; b < 32 && w * 32 + b < W; ++b)
                if ((m >> b) & 1u) cov[(size_t)y * W + w * 32 + b] |= bit;
        }
    }
    return 0;
}

void disc_cover(int cx, int cy, int r, int H, int W, uint8_t* cov, uint8_t bit) {
    int hw[ADAS_OVERLAY_MAX_RADIUS + 1];
    overlay_disc_halfwidths(r, hw);
    for (int j = -r; j <= r; ++j) {
        int y, xl, xr;
        if (!overlay_disc_row(cx, cy, j, hw[j < 0 ? -j : j], W, H, &y, &xl, &xr)) continue;
        for (int x = xl; x <= xr; ++x) cov[(size_t)y * W + x] |= bit;
    }
}

}  // namespace

extern "C" {

int emu_overlay_blend(int a, double alpha, int b) { return overlay_blend(a, b, overlay_alpha(alpha)); }

void emu_overlay_disc_halfwidths(int r, int* hw) { overlay_disc_halfwidths(r, hw); }

// mask [H][W] |= 1 on the disc
void emu_overlay_disc(int cx, int cy, int r, int H, int W, uint8_t* mask) { disc_cover(cx, cy, r, H, W, mask, 1); }

// mask [H][W] |= 1 on the pixels of the line inside the image, row by row from the closed form
void emu_overlay_line(int ax, int ay, int bx, int by, int H, int W, uint8_t* mask) {
    for (int y = 0; y < H; ++y) {
        long long xl, xr;
        if (!overlay_line_row(ax, ay, bx, by, y, &xl, &xr)) continue;
        if (xl < 0) xl = 0;
        if (xr > W - 1) xr = W - 1;
        for (long long x = xl; x <= xr; ++x) mask[(size_t)y * W + x] |= 1;
    }
}

// mask [H][W] |= 1 on the polygon; returns the frame's flags
int emu_overlay_poly(const int* pts, int n, int H, int W, uint8_t* mask) { return poly_cover(pts, n, H, W, mask, 1); }

// D5 on one frame.  img [H][W][3] in place; lane_pts [4][128][2], lane_cnt [4]; poly [n_poly][2]; dist [n_dist][2]; lane_bgr [4][3] is the
// table AFTER the offset rule; stages: 1 lanes, 2 area, 4 distance; direct != 0: the lane discs are written (the bird view).  Returns flags.
int emu_overlay_compose(uint8_t* img, int H, int W, const int* lane_pts, const int* lane_cnt, int r_lane, const uint8_t* lane_bgr, double lane_alpha,
                        const int* poly, int n_poly, int area_on, const uint8_t* area_bgr, double area_alpha, const int* dist, int n_dist, int r_dist,
                        const uint8_t* dist_bgr, int stages, int direct) {
    std::vector<uint8_t> cov((size_t)H * W, 0);
    int flags = 0;
    if (stages & 1)
        for (int l = 0; l < 4; ++l)
            for (int i = 0; i < lane_cnt[l] && i < 128; ++i)
                disc_cover(lane_pts[(l * 128 + i) * 2], lane_pts[(l * 128 + i) * 2 + 1], r_lane, H, W, cov.data(), (uint8_t)(1u << l));
    if ((stages & 2) && area_on) flags |= poly_cover(poly, n_poly, H, W, cov.data(), OV_BIT_AREA);
    if (stages & 4)
        for (int i = 0; i < n_dist; ++i) disc_cover(dist[2 * i], dist[2 * i + 1], r_dist, H, W, cov.data(), OV_BIT_DIST);
    OverlayStyle st;
    for (int l = 0; l < 4; ++l) st.lane[l] = overlay_pack_bgr(lane_bgr + 3 * l);
    st.area = overlay_pack_bgr(area_bgr);
    st.dist = overlay_pack_bgr(dist_bgr);
    st.lane_w = overlay_alpha(lane_alpha);
    st.area_w = overlay_alpha(area_alpha);
    st.lane_direct = direct;
    for (size_t p = 0; p < (size_t)H * W; ++p)
        for (int c = 0; c < 3; ++c) img[p * 3 + c] = (uint8_t)overlay_pixel(img[p * 3 + c], cov[p], c, st);
    return flags;
}

}  // extern "C"
