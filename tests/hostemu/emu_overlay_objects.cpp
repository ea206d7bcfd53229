// Host build of the object layer of csrc/overlay_core.h (rules D6-D9; g++, one thread): the closed forms the device kernels evaluate, composed
// the way the kernels compose them (one record per box, then every pixel walks the records in order), so that the CPU suite can compare
// them byte for byte with tests/overlay_objects_ref.py.  Test scaffolding only; never loaded by the product.
#include <string.h>
#include <vector>
#include "overlay_core.h"

using namespace adas;

namespace {

struct Style {
    int hw[3][ADAS_OVERLAY_MAX_RADIUS + 1];
    OverlayObjStyle s;
    Style(int rect_t, int arm_t, int track_t) {
        s.radii = overlay_obj_radii(rect_t, arm_t, track_t);
        s.hw = hw[0];
        s.hw_stride = ADAS_OVERLAY_MAX_RADIUS + 1;
        for (int w = 0; w < 3; ++w) overlay_disc_halfwidths(overlay_obj_radius(s, w), hw[w]);
    }
};

// mask |= 1 on the segment's pixels inside the image, row by row from the closed form
void seg_cover(long long ax, long long ay, long long bx, long long by, int R, const int* hw, int H, int W, uint8_t* mask) {
    for (int y = 0; y < H; ++y) {
        long long xl, xr;
        if (!overlay_seg_row(ax, ay, bx, by, R, hw, y, &xl, &xr)) continue;
        if (xl < 0) xl = 0;
        if (xr > W - 1) xr = W - 1;
        for (long long x = xl; x <= xr; ++x) mask[(size_t)y * W + x] |= 1;
    }
}

}  // namespace

extern "C" {

int emu_overlay_tint(int a, int b) { return overlay_tint(a, b); }

void emu_overlay_segment(int ax, int ay, int bx, int by, int t, int H, int W, uint8_t* mask) {
    int hw[ADAS_OVERLAY_MAX_RADIUS + 1];
    const int R = overlay_seg_radius(t);
    overlay_disc_halfwidths(R, hw);
    seg_cover(ax, ay, bx, by, R, hw, H, W, mask);
}

void emu_overlay_rect(int x1, int y1, int x2, int y2, int t, int H, int W, uint8_t* mask) {
    int hw[ADAS_OVERLAY_MAX_RADIUS + 1];
    const int R = overlay_seg_radius(t);
    overlay_disc_halfwidths(R, hw);
    for (int k = 0; k < 4; ++k) {
        long long ax, ay, bx, by;
        overlay_rect_edge(x1, y1, x2, y2, k, &ax, &ay, &bx, &by);
        seg_cover(ax, ay, bx, by, R, hw, H, W, mask);
    }
}

// mask [H][W] = 1 where a detection's record writes: per pixel, as the streaming pass asks
void emu_overlay_corner_rect(const int* xyxy, int arm_t, int rect_t, int H, int W, uint8_t* mask) {
    Style st(rect_t, arm_t, 2);
    const OverlayObject o = overlay_make_detection(xyxy, 0u, st.s, W, H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) mask[(size_t)y * W + x] = (uint8_t)(overlay_object_ops(o, x, y, st.s) & 1);
}

// D9 on one frame, in place: img [H][W][3] is the frame after AREA.  det_xyxy [n_det][4] + det_cls; trk_tlwh [n_trk][4] fp64 + trk_cls, rows
// of activated tracked tracks; the colour tables are [n][3] BGR (n = 0: every object is unknown, black); stages: 16 detections, 32 tracks.
void emu_overlay_objects(uint8_t* img, int H, int W, const int* det_xyxy, const int* det_cls, int n_det, const uint8_t* det_bgr, int n_det_bgr,
                         const double* trk_tlwh, const int* trk_cls, int n_trk, const uint8_t* trk_bgr, int n_trk_bgr, double min_box_area,
                         int rect_t, int arm_t, int track_t, int stages) {
    Style st(rect_t, arm_t, track_t);
    std::vector<uint32_t> dt(n_det_bgr), tt(n_trk_bgr);
    for (int i = 0; i < n_det_bgr; ++i) dt[i] = overlay_pack_bgr(det_bgr + 3 * i);
    for (int i = 0; i < n_trk_bgr; ++i) tt[i] = overlay_pack_bgr(trk_bgr + 3 * i);
    std::vector<OverlayObject> recs;
    if (stages & 16)
        for (int i = 0; i < n_det; ++i)
            recs.push_back(overlay_make_detection(det_xyxy + 4 * i, overlay_class_colour(det_cls[i], dt.data(), n_det_bgr), st.s, W, H));
    if (stages & 32)
        for (int k = 0; k < n_trk; ++k)
            recs.push_back(overlay_make_track(trk_tlwh + 4 * k, 1, min_box_area, overlay_class_colour(trk_cls[k], tt.data(), n_trk_bgr), st.s, W, H));
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (const OverlayObject& o : recs) {
                const int ops = overlay_object_ops(o, x, y, st.s);
                if (!ops) continue;
                uint8_t* p = img + ((size_t)y * W + x) * 3;
                for (int c = 0; c < 3; ++c) p[c] = (uint8_t)overlay_object_channel(p[c], ops, o.colour, c);
            }
}

}  // extern "C"
