// Host build of csrc/birdview_core.h (g++, one thread): the text the device kernel runs per stream, so that the CPU suite can compare it
// with analysis.PerspectiveTransformation / the golden trace, and the GPU suite can compare the kernel with it bit for bit.
// Test scaffolding only; never loaded by the product.
#include "birdview_core.h"

using namespace adas;

static_assert(sizeof(BirdState) == 256, "BirdState layout");

extern "C" {

int emu_birdview_state_bytes() { return (int)sizeof(BirdState); }

// PerspectiveTransformation(img_size=(w, h)); dst8 (optional) receives the destination corners.  -1: degenerate img_size
int emu_birdview_init(int w, int h, BirdState* st, float* dst8) {
    double A[72];
    if (dst8) birdview_dst(w, h, dst8);
    return birdview_init(w, h, *st, A) ? 0 : -1;
}

// One frame of the kernel's per-stream walk: the request `mode` meets a frame with lane points pts [4][128][2], counts cnt[4] and
// detection flags det[4].  Returns what the kernel stores in `applied`: 1 applied, 0 not, -1 rejected.
int emu_birdview_frame(BirdState* st, int w, int h, int mode, const int* pts, const int* cnt, const int* det) {
    if (mode == BIRD_MODE_NONE || !(det[1] && det[2])) return 0;
    BirdLaneStats s[2];
    int n[2];
    for (int l = 0; l < 2; ++l) {
        s[l] = bird_stats_empty();
        n[l] = cnt[1 + l] < 0 ? 0 : (cnt[1 + l] > 128 ? 128 : cnt[1 + l]);
        const int* p = pts + (size_t)(1 + l) * 128 * 2;
        for (int i = 0; i < n[l]; ++i) bird_stats_add(s[l], p[2 * i], p[2 * i + 1]);
    }
    BirdState next;
    double A[72];
    return birdview_apply(*st, w, h, mode, n[0], s[0], n[1], s[1], next, A);
}

// cv2.getPerspectiveTransform on float32 corners.  -1: singular / non-finite
int emu_birdview_perspective(const float* src8, const float* dst8, double* H9) {
    double A[72];
    return birdview_perspective(src8, dst8, H9, A) ? 0 : -1;
}

}  // extern "C"
