// Host build of csrc/warp_core.h (g++, one thread): the per-pixel text the device kernel runs, so that the CPU suite can compare it
// byte for byte with tests/warp_ref.py.  Test scaffolding only; never loaded by the product.
#include "warp_core.h"

using namespace adas;

extern "C" {

// src [sh][sw][3] -> dst [dh][dw][3]; M9 and inverse_map as adas_warp_set_matrix.  Returns -1 for a singular matrix.
int emu_warp_perspective(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, const double* M9, int inverse_map) {
    double m[9];
    if (inverse_map) memcpy(m, M9, sizeof(m));
    else if (!warp_invert3x3(M9, m)) return -1;
    const int bw = warp_block_width(dh, dw);
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            int v[3];
            warp_sample(src, sh, sw, warp_coord(m, bw, x, y), v);
            uint8_t* p = dst + ((size_t)y * dw + x) * 3;
            for (int c = 0; c < 3; ++c) p[c] = (uint8_t)v[c];
        }
    return 0;
}

int emu_warp_invert(const double* M9, double* out9) { return warp_invert3x3(M9, out9) ? 0 : -1; }

int emu_warp_block_width(int dh, int dw) { return warp_block_width(dh, dw); }

}  // extern "C"
