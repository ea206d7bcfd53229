// Host build of the trajectories stage of the overlay (csrc/overlay_track_core.h; g++, one thread): the per-track arithmetic and the closed
// forms of rules D10-D12 the device kernels evaluate, composed the way the kernels compose them -- one list of primitives per track, every
// (primitive, row) pair ORs its runs into a plane, every marked pixel takes the fold -- so that the CPU suite can compare them record for
// record and byte for byte with tests/overlay_tracks_ref.py.  Test scaffolding only; never loaded by the product.
#include <string.h>
#include <vector>
#include "adas_hip.h"
#include "overlay_track_core.h"

using namespace adas;

namespace {

struct TrackHw {
    int hw[(ADAS_OVERLAY_TRACK_MAX_R + 1) * ADAS_OVERLAY_TRACK_HW];
    OverlayTrackStyle s;
    TrackHw() {
        for (int R = 0; R <= ADAS_OVERLAY_TRACK_MAX_R; ++R) overlay_track_halfwidths(R, hw);
        s.hw = hw;
    }
};

struct MaskFill {   // overlay_prim_row's runs on one row of a byte mask
    uint8_t* row;
    void fill(int xl, int xr) {
        for (int x = xl; x <= xr; ++x) row[x] = 1;
    }
};

// mode 0: the rows' runs (what the mark kernel ORs); mode 1: the per-pixel test (what the sparse pass asks)
void prim_mask(const OverlayPrim& p, const TrackHw& t, int H, int W, uint8_t* mask, int mode) {
    for (int y = 0; y < H; ++y) {
        if (mode == 0) {
            MaskFill ops{mask + (size_t)y * W};
            overlay_prim_row(p, t.s, y, W, ops);
        } else {
            for (int x = 0; x < W; ++x)
                if (overlay_prim_hit(p, t.s, x, y)) mask[(size_t)y * W + x] = 1;
        }
    }
}

}  // namespace

extern "C" {

void emu_track_table(int* r, int* t) { overlay_mark_table(r, t); }

long long emu_isqrt(long long v) { return overlay_isqrt(v); }

// Tq of a segment, -1 when it is skipped for its range
long long emu_segment_tq(long long ax, long long ay, long long bx, long long by, int t) {
    const OverlayPrim p = overlay_make_segment(OV_PRIM_SHAFT, ax, ay, bx, by, t, 0u, 16, 16);
    return p.skip ? -1 : p.tq;
}

void emu_arrow_tips(long long p1x, long long p1y, long long p2x, long long p2y, double tip, long long* q) { overlay_arrow_tips(p1x, p1y, p2x, p2y, tip, q); }

void emu_circle_mask(int cx, int cy, int r, int t, int H, int W, uint8_t* mask, int mode) {
    TrackHw hw;
    prim_mask(overlay_make_circle(cx, cy, r, t, 0u, W, H), hw, H, W, mask, mode);
}

// returns 1 when the segment is skipped for its range
int emu_segment_mask(long long ax, long long ay, long long bx, long long by, int t, int H, int W, uint8_t* mask, int mode) {
    TrackHw hw;
    const OverlayPrim p = overlay_make_segment(OV_PRIM_SHAFT, ax, ay, bx, by, t, 0u, W, H);
    prim_mask(p, hw, H, W, mask, mode);
    return p.skip;
}

double emu_median(const double* v, int n) {
    double w[ADAS_OVERLAY_TRACK_RING];
    for (int i = 0; i < n; ++i) w[i] = v[i];
    overlay_sort_small(w, n, 1);
    return overlay_median_sorted(w, n, 1);
}

// One frame, in place: img [H][W][3] is the frame after AREA and the detections.  trk_tlwh [n_trk][4] fp64 + trk_cls, rows of activated
// tracked tracks; traj [n_trk][30][4] oldest first + traj_len; stages: 32 tracks, 128 trajectories.  marks: up to max_marks records, *n_marks
// their total; returns the frame's flags.
int emu_overlay_tracks(uint8_t* img, int H, int W, const double* trk_tlwh, const int* trk_cls, int n_trk, const uint8_t* trk_bgr, int n_trk_bgr,
                       const double* traj, const int* traj_len, double min_box_area, int track_t, int stages, adas_overlay_track_mark* marks, int max_marks,
                       int* n_marks) {
    int ohw[3][ADAS_OVERLAY_MAX_RADIUS + 1];
    OverlayObjStyle os;
    os.radii = overlay_obj_radii(1, 5, track_t);
    os.hw = ohw[0];
    os.hw_stride = ADAS_OVERLAY_MAX_RADIUS + 1;
    for (int w = 0; w < 3; ++w) overlay_disc_halfwidths(overlay_obj_radius(os, w), ohw[w]);
    TrackHw hw;
    std::vector<uint32_t> tt(n_trk_bgr);
    for (int i = 0; i < n_trk_bgr; ++i) tt[i] = overlay_pack_bgr(trk_bgr + 3 * i);
    std::vector<OverlayObject> objs;
    if (stages & 32) {   // the streaming pass's part: D9 over the tracks' boxes
        for (int k = 0; k < n_trk; ++k)
            objs.push_back(overlay_make_track(trk_tlwh + 4 * k, 1, min_box_area, overlay_class_colour(trk_cls[k], tt.data(), n_trk_bgr), os, W, H));
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (const OverlayObject& o : objs) {
                    const int ops = overlay_object_ops(o, x, y, os);
                    if (!ops) continue;
                    uint8_t* p = img + ((size_t)y * W + x) * 3;
                    for (int c = 0; c < 3; ++c) p[c] = (uint8_t)overlay_object_channel(p[c], ops, o.colour, c);
                }
    }
    *n_marks = 0;
    if (!(stages & 128)) return 0;
    int tab_r[ADAS_OVERLAY_TRACK_RING], tab_t[ADAS_OVERLAY_TRACK_RING];
    overlay_mark_table(tab_r, tab_t);
    std::vector<OverlayPrim> prims((size_t)(n_trk > 0 ? n_trk : 1) * ADAS_OVERLAY_TRACK_PRIMS);
    std::vector<OverlayTrackHead> heads(n_trk > 0 ? n_trk : 1);
    int flags = 0, n = 0;
    for (int k = 0; k < n_trk; ++k) {
        double work[2 * (ADAS_OVERLAY_TRACK_RING - 1)];
        OverlayPrim* out = prims.data() + (size_t)k * ADAS_OVERLAY_TRACK_PRIMS;
        int range = 0;
        const int np = overlay_track_prims(trk_tlwh + 4 * k, 1, min_box_area, overlay_class_colour(trk_cls[k], tt.data(), n_trk_bgr),
                                           traj + (size_t)k * ADAS_OVERLAY_TRACK_RING * 4, 0, traj_len[k], tab_r, tab_t, W, H, work, 1, out, &range);
        heads[k] = overlay_track_head(out, np, range);
        if (range) flags |= ADAS_OVERLAY_TRACK_RANGE;
        n = overlay_track_marks(out, np, k, marks, max_marks, n);
    }
    *n_marks = n;
    std::vector<uint8_t> plane((size_t)H * W, 0);
    for (int k = 0; k < n_trk; ++k)
        for (int i = 0; i < heads[k].n; ++i) prim_mask(prims[(size_t)k * ADAS_OVERLAY_TRACK_PRIMS + i], hw, H, W, plane.data(), 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int bgr[3];
            const bool hit = overlay_track_pixel(heads.data(), prims.data(), n_trk, hw.s, (stages & 32) ? objs.data() : nullptr, os, x, y, bgr);
            if (hit != (plane[(size_t)y * W + x] != 0)) flags |= 1 << 30;   // the runs and the per-pixel test disagree: reported, never expected
            if (!hit || !plane[(size_t)y * W + x]) continue;
            uint8_t* p = img + ((size_t)y * W + x) * 3;
            for (int c = 0; c < 3; ++c) p[c] = (uint8_t)bgr[c];
        }
    return flags;
}

}  // extern "C"
