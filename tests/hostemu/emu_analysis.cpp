// Host build of csrc/analysis_core.h (g++, one thread): the text the device kernel runs per stream and frame, so that the CPU suite can
// compare it with analysis.SingleCamDistanceMeasure / point_in_polygon / TaskConditions and the golden traces, and the GPU suite can
// compare the kernel with it field for field.  Test scaffolding only; never loaded by the product.
#include "analysis_core.h"

using namespace adas;

static_assert(sizeof(AnalysisState) == 256, "AnalysisState layout");
static_assert(sizeof(AnalysisInput) == 48, "AnalysisInput layout");
static_assert(sizeof(AnalysisFrame) == 80, "AnalysisFrame layout");
static_assert(sizeof(AnalysisCfg) == 56, "AnalysisCfg layout");

extern "C" {

void emu_analysis_sizes(int* out4) {
    out4[0] = (int)sizeof(AnalysisCfg); out4[1] = (int)sizeof(AnalysisState); out4[2] = (int)sizeof(AnalysisInput); out4[3] = (int)sizeof(AnalysisFrame);
}

void emu_analysis_state_init(AnalysisState* st) { analysis_state_init(*st); }

// the state machine alone: one frame of inputs; returns the request word
int emu_analysis_step(AnalysisState* st, const AnalysisCfg* cfg, const AnalysisInput* in, AnalysisFrame* out) {
    out->n_points = 0; out->has_collision = 0; out->collision_x = 0; out->collision_y = 0; out->collision_d = 0.0; out->collision_index = -1;
    out->flags = 0;
    return analysis_step(*st, *cfg, *in, *out);
}

int emu_analysis_point_in_polygon(const int* poly, int n, double x, double y) {
    int any_on = 0, parity = 0;
    for (int i = 0; i < n; ++i) {
        int on = 0;
        parity ^= analysis_poly_edge(poly, n, i, x, y, &on);
        any_on |= on;
    }
    return analysis_poly_decide(n, any_on, parity);
}

// One frame as the kernel walks it: n survivors (xyxy [n][4] doubles, cls [n]; at most max_points are read), the detector's flags word, the
// polygon (npoly points), the geometry's (area_status, direction, curvature, offset).  pts_xy [max_points][2] / pts_d [max_points]
// receive the distance points.  Returns the request word.
int emu_analysis_frame(AnalysisState* st, const AnalysisCfg* cfg, const double* ref_height, const double* xyxy, const int* cls, int n, int det_flags,
                       int max_points, const int* poly, int npoly, int area_status, int direction, double curvature, double offset, int* pts_xy,
                       double* pts_d, AnalysisFrame* out) {
    out->flags = (det_flags & 1) ? ANA_FLAG_OVERFLOW : 0;
    if (n < 0) n = 0;
    if (n > max_points) { n = max_points; out->flags |= ANA_FLAG_TRUNCATED; }
    int np = 0;
    for (int i = 0; i < n; ++i) {
        int x, y;
        double d;
        if (analysis_measure(*cfg, ref_height, xyxy + 4 * (size_t)i, cls[i], &x, &y, &d)) {
            pts_xy[2 * np] = x; pts_xy[2 * np + 1] = y; pts_d[np] = d;
            ++np;
        }
    }
    int best = -1;
    double bd = 0.0;
    if (np > 0 && npoly > 0)
        for (int j = 0; j < np; ++j) {
            if (emu_analysis_point_in_polygon(poly, npoly, (double)pts_xy[2 * j], (double)pts_xy[2 * j + 1]) < 0) continue;
            if (best < 0 || analysis_nearer(pts_d[j], j, bd, best)) { best = j; bd = pts_d[j]; }
        }
    out->n_points = np;
    out->has_collision = best >= 0;
    out->collision_index = best;
    out->collision_x = best >= 0 ? pts_xy[2 * best] : 0;
    out->collision_y = best >= 0 ? pts_xy[2 * best + 1] : 0;
    out->collision_d = best >= 0 ? bd : 0.0;
    AnalysisInput in;
    in.has_point = best >= 0; in.area = area_status; in.has_offset = direction != ANA_DIR_NONE; in.has_curvature = direction != ANA_DIR_NONE;
    in.direction = direction; in.reserved = 0; in.distance = out->collision_d; in.offset = offset; in.curvature = curvature;
    return analysis_step(*st, *cfg, in, *out);
}

}  // extern "C"
