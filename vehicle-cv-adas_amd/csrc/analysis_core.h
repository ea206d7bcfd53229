// analysis_core.h -- what demo.py:284-296 computes per frame behind the two detectors, per video stream:
//   distanceMeasure.py:50-74    SingleCamDistanceMeasure.updateDistance: a foot point and a distance per known object
//   distanceMeasure.py:76-93    .calcCollisionPoint: the nearest measured object whose foot point lies in (or on) the ego-lane polygon
//   taskConditions.py:88-312    TaskConditions: the median-window FCWS / LDWS / LKAS state machine and the bird view's re-anchoring toggle
// (analysis.SingleCamDistanceMeasure / point_in_polygon / TaskConditions are the project's host restatement of the same text.)
//
// Everything is IEEE fp64 in the association the reference writes, contraction off; no dynamic memory, every loop bounded by a
// window length (5, 5, 10) or by the caller's element count.  The per-element pieces (one survivor, one polygon edge) are what the
// kernel's lanes stride; the state machine is one lane's work.
//
// Where this text DEFINES behaviour the reference leaves to chance:
//   * a window that mixes directions picks R before L before F: `max(set(strings), key=record.count)` (taskConditions.py:262) looks a
//     string up in a list of pairs, every key is 0, so it returns the first element of the set's iteration order; under
//     PYTHONHASHSEED=0 -- the seed every golden is made under -- that order is R, L, F for every subset and insertion order;
//   * a frame whose curvature is not finite, where the reference's int(float(...)) raises, is a frame without a curve estimate
//     (UpdateRouteStatus(None, None)) and n_nonfinite counts it.
//
// Per frame: UpdateCollisionStatus, UpdateOffsetStatus, UpdateRouteStatus, then CheckStatus() FOR THE NEXT FRAME -- the reference calls
// it at the start of frame t+1 (demo.py:287) and nothing in between touches what it reads.  Its result is the stream's request word.
//
// Like birdview_core.h / lane_core.h this header compiles for the host with one thread (tests/hostemu/emu_analysis.cpp).
#pragma once
#include "warp_core.h"   // ADAS_HD

namespace adas {

enum { ANA_COLLISION_UNKNOWN = 0, ANA_COLLISION_NORMAL = 1, ANA_COLLISION_PROMPT = 2, ANA_COLLISION_WARNING = 3 };
enum { ANA_OFFSET_UNKNOWN = 0, ANA_OFFSET_RIGHT = 1, ANA_OFFSET_LEFT = 2, ANA_OFFSET_CENTER = 3 };
enum { ANA_CURVE_UNKNOWN = 0, ANA_CURVE_STRAIGHT = 1, ANA_CURVE_EASY_LEFT = 2, ANA_CURVE_HARD_LEFT = 3, ANA_CURVE_EASY_RIGHT = 4, ANA_CURVE_HARD_RIGHT = 5 };
enum { ANA_MODE_NONE = 0, ANA_MODE_DEFAULT = 1, ANA_MODE_TOP = 2, ANA_MODE_BOTTOM = 3 };   // = BIRD_MODE_* / ADAS_BIRDVIEW_*
enum { ANA_DIR_NONE = 0, ANA_DIR_L = 1, ANA_DIR_R = 2, ANA_DIR_F = 3 };                     // = adas_lane_geometry_result.direction
enum { ANA_FLAG_OVERFLOW = 1, ANA_FLAG_NONFINITE = 2, ANA_FLAG_TRUNCATED = 4 };

// The constants of the reference's calls.  The layout is the head of the C ABI's adas_analysis_params.
struct AnalysisCfg {
    double focal;              // SingleCamDistanceMeasure.f (distanceMeasure.py:21)
    double y_limit;            // boxes whose bottom lies below this row are not measured (:62)
    double distance_thres;     // UpdateCollisionStatus(distance_thres=1.5)
    double offset_thres;       // UpdateOffsetStatus(offset_thres=0.65)
    double curvae_thres;       // UpdateRouteStatus(curvae_thres=500)
    double calib_curvae_thres; // _calibration_curve(curvae_thres=15000)
    int calib_frequency;       // _calibration_curve(frequency=3)
    int n_classes;             // entries of the ref_height table
};

// One stream's TaskConditions.  The layout is the C ABI's adas_analysis_state.
struct AnalysisState {
    int collision_msg, offset_msg, curvature_msg;
    int toggle_status, transform_status;   // ANA_MODE_*
    int osc[2];                            // toggle_oscillator_status
    int cnt_offset, cnt_curvae, cnt_bird;  // toggle_status_counter: Offset, Curvae, BirdViewAngle
    int n_collision, n_offset, n_curvature;   // window lengths
    int n_nonfinite;
    double collision_rec[5];               // vehicle_collision_record, oldest first
    double offset_rec[5];                  // vehicle_offset_record
    double curvature_rec[10];              // vehicle_curvature_record: the curvature ...
    int direction_rec[10];                 // ... and the direction (ANA_DIR_*) of each entry
};

// What one frame hands the state machine.  The layout is the C ABI's adas_analysis_input.
struct AnalysisInput {
    int has_point;       // calcCollisionPoint returned a point
    int area;            // lane_info.area_status
    int has_offset;      // vehicle_offset is not None
    int has_curvature;   // vehicle_curvature is not None
    int direction;       // ANA_DIR_*; ANA_DIR_NONE: vehicle_direction is None
    int reserved;
    double distance;     // the point's metres
    double offset;
    double curvature;
};

// One frame's record.  The layout is the C ABI's adas_analysis_frame.
struct AnalysisFrame {
    int n_points;
    int has_collision;
    int collision_x, collision_y;
    double collision_d;
    int collision_index;                   // into the frame's distance points, -1: none
    int collision_msg, offset_msg, curvature_msg;   // after the frame's three updates
    int toggle_status, transform_status;   // after the updates, BEFORE the next frame's CheckStatus
    int osc[2];
    int counters[3];                       // Offset, Curvae, BirdViewAngle
    int check;                             // CheckStatus() for the next frame
    int request;                           // the word written for the next frame: the new transform_status if check, else none
    int flags;                             // ANA_FLAG_*
};

// ------------------------------------------------------------------------------------------------ distance
// Python's // on two integers held exactly in doubles: floor, not truncation (corners can be negative)
ADAS_HD double ana_floor_half(double s) { return floor(s / 2.0); }

// updateDistance for one survivor: xyxy = RectInfo.tolist() as doubles, cls its class.  false: not measured.
ADAS_HD bool analysis_measure(const AnalysisCfg& c, const double* ref_height, const double* xyxy, int cls, int* px, int* py, double* pd) {
    const double xmin = xyxy[0], ymin = xyxy[1], xmax = xyxy[2], ymax = xyxy[3];
    const double ref = (cls >= 0 && cls < c.n_classes) ? ref_height[cls] : 0.0;
    if (ref == 0.0 || ymax > c.y_limit || ymax == ymin) return false;
    const double inches = ref * c.focal / (ymax - ymin);
    *px = (int)ana_floor_half(xmax + xmin);
    *py = (int)ymax;
    *pd = inches / 12 * 0.3048;
    return true;
}

// ------------------------------------------------------------------------------------------------ polygon
// Edge i of analysis.point_in_polygon: from vertex i - 1 (the last one for i = 0) to vertex i.  Returns the crossing bit; *on is set
// when the point lies on the edge.  The caller ORs `on` and XORs the crossings over all edges, in any order.
ADAS_HD int analysis_poly_edge(const int* poly, int n, int i, double x, double y, int* on) {
    const int j = i == 0 ? n - 1 : i - 1;
    const double x0 = (double)poly[2 * j], y0 = (double)poly[2 * j + 1];
    const double x1 = (double)poly[2 * i], y1 = (double)poly[2 * i + 1];
    const double cross = (x1 - x0) * (y - y0) - (y1 - y0) * (x - x0);
    const double lox = x0 < x1 ? x0 : x1, hix = x0 < x1 ? x1 : x0;
    const double loy = y0 < y1 ? y0 : y1, hiy = y0 < y1 ? y1 : y0;
    *on = (cross == 0.0 && lox <= x && x <= hix && loy <= y && y <= hiy) ? 1 : 0;
    if ((y0 <= y && y < y1) || (y1 <= y && y < y0)) {
        const double t = (y - y0) / (y1 - y0);
        if (x0 + t * (x1 - x0) > x) return 1;
    }
    return 0;
}
// +1 inside, 0 on the boundary, -1 outside
ADAS_HD int analysis_poly_decide(int n, int any_on, int parity) { return n <= 0 ? -1 : (any_on ? 0 : (parity ? 1 : -1)); }

// sorted(points, key=d) is stable: (d, i) < (bd, bi)
ADAS_HD bool analysis_nearer(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// ------------------------------------------------------------------------------------------------ state machine
ADAS_HD bool ana_finite(double v) { return v - v == 0.0; }

// TaskConditions() after the first CheckStatus(): the reference's first call returns True with "Default", which the owner of the bird
// view queues when it resets a stream
ADAS_HD void analysis_state_init(AnalysisState& s) {
    s.collision_msg = ANA_COLLISION_UNKNOWN; s.offset_msg = ANA_OFFSET_UNKNOWN; s.curvature_msg = ANA_CURVE_UNKNOWN;
    s.toggle_status = ANA_MODE_NONE; s.transform_status = ANA_MODE_DEFAULT;
    s.osc[0] = 0; s.osc[1] = 0;
    s.cnt_offset = 0; s.cnt_curvae = 0; s.cnt_bird = 0;
    s.n_collision = 0; s.n_offset = 0; s.n_curvature = 0; s.n_nonfinite = 0;
    for (int k = 0; k < 5; ++k) { s.collision_rec[k] = 0.0; s.offset_rec[k] = 0.0; }
    for (int k = 0; k < 10; ++k) { s.curvature_rec[k] = 0.0; s.direction_rec[k] = ANA_DIR_NONE; }
}

// LimitedList.append (taskConditions.py:14-37)
ADAS_HD void ana_push(double* rec, int& n, int cap, double v) {
    if (n == cap) {
        for (int k = 1; k < cap; ++k) rec[k - 1] = rec[k];
        n = cap - 1;
    }
    rec[n] = v;
    n = n + 1;
}
// np.median of a full window of 5: the middle of a sorted copy
ADAS_HD double ana_median5(const double* rec) {
    double t[5];
    for (int k = 0; k < 5; ++k) t[k] = rec[k];
    for (int i = 1; i < 5; ++i)
        for (int j = i; j > 0 && t[j] < t[j - 1]; --j) {
            const double v = t[j]; t[j] = t[j - 1]; t[j - 1] = v;
        }
    return t[2];
}
// np.median([int(float(c)) for c in window of 10]): the mean of the two middle truncated values
ADAS_HD double ana_median10_trunc(const double* rec) {
    double t[10];
    for (int k = 0; k < 10; ++k) t[k] = trunc(rec[k]);
    for (int i = 1; i < 10; ++i)
        for (int j = i; j > 0 && t[j] < t[j - 1]; --j) {
            const double v = t[j]; t[j] = t[j - 1]; t[j - 1] = v;
        }
    return (t[4] + t[5]) / 2;
}

// UpdateCollisionStatus (:283-312)
ADAS_HD void analysis_update_collision(AnalysisState& s, const AnalysisCfg& c, int has_point, double distance, int area) {
    if (!has_point) {
        s.collision_msg = area ? ANA_COLLISION_NORMAL : ANA_COLLISION_UNKNOWN;
        s.n_collision = 0;
        return;
    }
    ana_push(s.collision_rec, s.n_collision, 5, distance);
    if (s.n_collision >= 5) {
        const double d = ana_median5(s.collision_rec);
        if (d <= c.distance_thres) s.collision_msg = ANA_COLLISION_WARNING;
        else if (d <= 2 * c.distance_thres) s.collision_msg = ANA_COLLISION_PROMPT;
        else s.collision_msg = ANA_COLLISION_NORMAL;
    }
}

// UpdateOffsetStatus (:200-239) with _calc_deviation (:126-148)
ADAS_HD void analysis_update_offset(AnalysisState& s, const AnalysisCfg& c, int has_offset, double offset) {
    if (!has_offset) {
        s.offset_msg = ANA_OFFSET_UNKNOWN;
        s.n_offset = 0;
        return;
    }
    ana_push(s.offset_rec, s.n_offset, 5, offset);
    if (s.n_offset < 5) {
        s.offset_msg = ANA_OFFSET_UNKNOWN;
        return;
    }
    const double m = ana_median5(s.offset_rec);
    const int cm = s.curvature_msg;
    if (fabs(m) <= c.offset_thres) s.offset_msg = ANA_OFFSET_CENTER;
    else if (m > 0 && cm != ANA_CURVE_HARD_LEFT && cm != ANA_CURVE_EASY_LEFT) s.offset_msg = ANA_OFFSET_RIGHT;
    else if (m < 0 && cm != ANA_CURVE_HARD_RIGHT && cm != ANA_CURVE_EASY_RIGHT) s.offset_msg = ANA_OFFSET_LEFT;
    else s.offset_msg = ANA_OFFSET_UNKNOWN;
    if (s.cnt_offset < 10) {
        s.cnt_offset = s.cnt_offset + 1;
        return;
    }
    bool all_pos = true, all_neg = true;
    for (int k = 0; k < 5; ++k) {
        all_pos = all_pos && s.offset_rec[k] > 0.2;
        all_neg = all_neg && s.offset_rec[k] < -0.2;
    }
    if (all_pos) { s.osc[0] = 1; s.cnt_offset = 0; }
    if (all_neg) { s.osc[1] = 1; s.cnt_offset = 0; }
    if (s.osc[0] && s.osc[1]) {
        s.toggle_status = ANA_MODE_TOP;
        s.osc[0] = 0; s.osc[1] = 0;
    } else {
        s.cnt_offset = 0;
    }
}

// UpdateRouteStatus (:241-281) with _calc_direction (:150-177) and _calibration_curve (:103-124)
ADAS_HD void analysis_update_route(AnalysisState& s, const AnalysisCfg& c, int direction, int has_curvature, double curvature) {
    if (!has_curvature) {
        s.n_curvature = 0;
        s.curvature_msg = ANA_CURVE_UNKNOWN;
        return;
    }
    if (direction != ANA_DIR_NONE && s.offset_msg == ANA_OFFSET_CENTER) {
        if (s.n_curvature == 10) {
            for (int k = 1; k < 10; ++k) {
                s.curvature_rec[k - 1] = s.curvature_rec[k];
                s.direction_rec[k - 1] = s.direction_rec[k];
            }
            s.n_curvature = 9;
        }
        s.curvature_rec[s.n_curvature] = curvature;
        s.direction_rec[s.n_curvature] = direction;
        s.n_curvature = s.n_curvature + 1;
        if (s.n_curvature >= 10) {
            bool any_r = false, any_l = false;
            for (int k = 0; k < 10; ++k) {
                any_r = any_r || s.direction_rec[k] == ANA_DIR_R;
                any_l = any_l || s.direction_rec[k] == ANA_DIR_L;
            }
            const int avg_dir = any_r ? ANA_DIR_R : (any_l ? ANA_DIR_L : ANA_DIR_F);
            const double avg = ana_median10_trunc(s.curvature_rec);
            const int cm = s.curvature_msg;
            int msg;
            if (avg <= c.curvae_thres) {
                if (avg_dir == ANA_DIR_L && cm != ANA_CURVE_EASY_RIGHT) msg = ANA_CURVE_HARD_LEFT;
                else if (avg_dir == ANA_DIR_R && cm != ANA_CURVE_EASY_LEFT) msg = ANA_CURVE_HARD_RIGHT;
                else msg = ANA_CURVE_UNKNOWN;
            } else {
                msg = avg_dir == ANA_DIR_L ? ANA_CURVE_EASY_LEFT : (avg_dir == ANA_DIR_R ? ANA_CURVE_EASY_RIGHT : ANA_CURVE_STRAIGHT);
            }
            s.curvature_msg = msg;
            if (s.cnt_curvae >= 10) {
                // offset_msg == CENTER implies a full offset window: [-1] is entry 4
                if (msg != ANA_CURVE_STRAIGHT && fabs(s.offset_rec[4]) < 0.2 && !(s.osc[0] || s.osc[1])) s.toggle_status = ANA_MODE_BOTTOM;
                else s.cnt_curvae = 0;
            } else {
                s.cnt_curvae = s.cnt_curvae + 1;
            }
        } else {
            s.curvature_msg = ANA_CURVE_UNKNOWN;
        }
    } else {
        s.n_curvature = 0;
        s.curvature_msg = ANA_CURVE_UNKNOWN;
    }
    if (s.cnt_bird > c.calib_frequency) {
        s.cnt_bird = 0;
        s.toggle_status = ANA_MODE_DEFAULT;
    } else {
        s.cnt_bird = curvature >= c.calib_curvae_thres ? s.cnt_bird + 1 : 0;
    }
}

// CheckStatus (:179-198)
ADAS_HD int analysis_check_status(AnalysisState& s) {
    if (s.curvature_msg == ANA_CURVE_UNKNOWN && s.offset_msg == ANA_OFFSET_UNKNOWN) { s.osc[0] = 0; s.osc[1] = 0; }
    if (s.toggle_status != s.transform_status) {
        s.transform_status = s.toggle_status;
        s.toggle_status = ANA_MODE_NONE;
        return 1;
    }
    return 0;
}

// One frame of one stream.  Fills the state-machine part of `out` (the caller fills n_points and the collision point; flags are ORed
// into) and returns the request word for the stream's next frame.
ADAS_HD int analysis_step(AnalysisState& s, const AnalysisCfg& c, const AnalysisInput& in, AnalysisFrame& out) {
    int has_curv = in.has_curvature, dir = in.direction;
    if (has_curv && !ana_finite(in.curvature)) {
        has_curv = 0;
        dir = ANA_DIR_NONE;
        s.n_nonfinite = s.n_nonfinite + 1;
        out.flags = out.flags | ANA_FLAG_NONFINITE;
    }
    analysis_update_collision(s, c, in.has_point, in.distance, in.area);
    analysis_update_offset(s, c, in.has_offset, in.offset);
    analysis_update_route(s, c, dir, has_curv, in.curvature);
    out.collision_msg = s.collision_msg; out.offset_msg = s.offset_msg; out.curvature_msg = s.curvature_msg;
    out.toggle_status = s.toggle_status; out.transform_status = s.transform_status;
    out.osc[0] = s.osc[0]; out.osc[1] = s.osc[1];
    out.counters[0] = s.cnt_offset; out.counters[1] = s.cnt_curvae; out.counters[2] = s.cnt_bird;
    out.check = analysis_check_status(s);
    out.request = out.check ? s.transform_status : ANA_MODE_NONE;
    return out.request;
}

}  // namespace adas
