// birdview_core.h -- the per-video bird-view trapezoid and its homographies, per stream:
//   perspectiveTransformation.py:21-37   __init__: src / dst corners from img_size, M, M_inv
//   perspectiveTransformation.py:39-86   updateTransformParams(left_lanes, right_lanes, type): re-anchor the frontal-view trapezoid on
//                                        the two ego lanes, then cv2.getPerspectiveTransform both ways
// (analysis.PerspectiveTransformation is the project's host restatement of the same text.)
//
// The corners are float32 as in the reference (np.float32([...])): a value taken from the lane points is an integer +- a constant
// evaluated in float64 and then rounded to float32; a value derived from the previous trapezoid ("Top": bl[0] - 10, br[0] + 10) is a
// float32 operation, because self.src[1][0] - 10 is one in NumPy.  "Top" therefore accumulates: the state has to persist per stream.
//
// cv2.getPerspectiveTransform solves the 8x8 system below with cv::solve(DECOMP_LU); analysis.perspective_matrix stands in for it
// with np.linalg.solve (LAPACK LU).  Here: Gaussian elimination with partial pivoting in IEEE fp64, contraction off, from the float32
// corners widened to double (their pairwise products are exact in double), H[8] = 1.  Same error class as the two LU solvers, another
// elimination order: the matrices agree with the exact rational solution to ~1e-11 relative to the row (condition ~1e8), not bit for bit.
//
// REJECTION.  Where the corners are degenerate (e.g. a collapsed top edge: max(Lx) - 20 == min(Rx) + 20) the reference raises inside
// cv2 / LAPACK or goes on with garbage (inf / nan matrices).  Here such an update is REJECTED: the state stays bit for bit what it was
// and n_rejected counts it.  An update is rejected when either system has a zero pivot, when a solution is not finite, or when
// det M == 0 (the warp could not invert it).
//
// Like warp_core.h / lane_core.h this header compiles for the host with one thread (tests/hostemu/emu_birdview.cpp).
#pragma once
#include "warp_core.h"   // ADAS_HD, warp_invert3x3

namespace adas {

enum { BIRD_MODE_NONE = 0, BIRD_MODE_DEFAULT = 1, BIRD_MODE_TOP = 2, BIRD_MODE_BOTTOM = 3 };

// One stream's live state.  The layout is the C ABI's adas_birdview_state (include/adas_hip.h).
struct BirdState {
    float src[8];       // frontal-view trapezoid: tl, bl, br, tr as (x, y)
    double M[9];        // frontal -> bird view           getPerspectiveTransform(src, dst)
    double M_inv[9];    // bird view -> frontal           getPerspectiveTransform(dst, src)   (transformToFrontalView)
    double M_warp[9];   // warp_invert3x3(M): the destination -> source matrix cv2.warpPerspective(img, M, ...) forms
    int n_updates;      // updates applied
    int n_rejected;     // updates rejected (state unchanged)
};

// min / max over one ego lane's integer points
struct BirdLaneStats {
    int min_y, min_x, max_x;
};
ADAS_HD BirdLaneStats bird_stats_empty() {
    BirdLaneStats s;
    s.min_y = 2147483647; s.min_x = 2147483647; s.max_x = -2147483647 - 1;
    return s;
}
ADAS_HD void bird_stats_add(BirdLaneStats& s, int x, int y) {
    s.min_y = y < s.min_y ? y : s.min_y;
    s.min_x = x < s.min_x ? x : s.min_x;
    s.max_x = x > s.max_x ? x : s.max_x;
}

// PerspectiveTransformation.__init__ (:24-34): tl, bl, br, tr
ADAS_HD void birdview_initial_src(int w, int h, float src[8]) {
    src[0] = (float)((double)w * 0.3);  src[1] = (float)((double)h * 0.7);
    src[2] = (float)((double)w * 0.2);  src[3] = (float)(double)h;
    src[4] = (float)((double)w * 0.95); src[5] = (float)(double)h;
    src[6] = (float)((double)w * 0.8);  src[7] = (float)((double)h * 0.7);
}
ADAS_HD void birdview_dst(int w, int h, float dst[8]) {
    const double ox = (double)w / 4;
    dst[0] = (float)ox;               dst[1] = 0.0f;
    dst[2] = (float)ox;               dst[3] = (float)(double)h;
    dst[4] = (float)((double)w - ox); dst[5] = (float)(double)h;
    dst[6] = (float)((double)w - ox); dst[7] = 0.0f;
}

// updateTransformParams (:56-86) on the corners alone.  L / R: stats of lanes_points[1] / [2] (both non-empty).
// false: an unknown mode, nothing written (the reference's silent return).
ADAS_HD bool birdview_update(float src[8], int mode, const BirdLaneStats& L, const BirdLaneStats& R) {
    if (mode != BIRD_MODE_DEFAULT && mode != BIRD_MODE_TOP && mode != BIRD_MODE_BOTTOM) return false;
    const double top_y = (double)(L.min_y < R.min_y ? L.min_y : R.min_y);
    if (mode == BIRD_MODE_TOP || mode == BIRD_MODE_DEFAULT) {
        src[0] = (float)((double)L.max_x - 20); src[1] = (float)top_y;   // tl
        src[6] = (float)((double)R.min_x + 20); src[7] = (float)top_y;   // tr
    }
    if (mode == BIRD_MODE_TOP) {            // float32 arithmetic on the previous corners
        src[2] = src[2] - 10.0f;
        src[4] = src[4] + 10.0f;
    } else if (mode == BIRD_MODE_BOTTOM) {
        src[2] = (float)((double)L.min_x - 20);
        src[4] = (float)((double)R.max_x + 20);
    } else {
        src[2] = (float)((double)L.min_x - 5);
        src[4] = (float)((double)R.max_x + 5);
    }
    return true;
}

ADAS_HD bool bird_finite(double v) { return v - v == 0.0; }   // false for inf and nan

// cv2.getPerspectiveTransform(src, dst): H with dst ~ H @ src, H[8] = 1.  A: 72 doubles of work space (the augmented 8x9 system).
// false: a zero pivot or a non-finite entry; H is then not written.
ADAS_HD bool birdview_perspective(const float* src, const float* dst, double* H, double* A) {
    for (int i = 0; i < 4; ++i) {
        const double x = (double)src[2 * i], y = (double)src[2 * i + 1];
        const double u = (double)dst[2 * i], v = (double)dst[2 * i + 1];
        double* r0 = A + 9 * i;
        double* r1 = A + 9 * (i + 4);
        r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -x * u; r0[7] = -y * u; r0[8] = u;
        r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x; r1[4] = y; r1[5] = 1.0; r1[6] = -x * v; r1[7] = -y * v; r1[8] = v;
    }
    for (int k = 0; k < 8; ++k) {
        int p = k;
        double best = fabs(A[9 * k + k]);
        for (int i = k + 1; i < 8; ++i) {   // the first row holding the largest magnitude
            const double a = fabs(A[9 * i + k]);
            if (a > best) { best = a; p = i; }
        }
        if (!(best > 0.0)) return false;    // zero (or nan) pivot column
        if (p != k)
            for (int j = k; j < 9; ++j) {
                const double t = A[9 * k + j];
                A[9 * k + j] = A[9 * p + j];
                A[9 * p + j] = t;
            }
        const double piv = A[9 * k + k];
        for (int i = k + 1; i < 8; ++i) {
            const double f = A[9 * i + k] / piv;
            if (f != 0.0)
                for (int j = k + 1; j < 9; ++j) A[9 * i + j] = A[9 * i + j] - f * A[9 * k + j];
            A[9 * i + k] = 0.0;
        }
    }
    double h[8];
    for (int k = 7; k >= 0; --k) {
        double s = A[9 * k + 8];
        for (int j = k + 1; j < 8; ++j) s = s - A[9 * k + j] * h[j];
        h[k] = s / A[9 * k + k];
        if (!bird_finite(h[k])) return false;
    }
    for (int k = 0; k < 8; ++k) H[k] = h[k];
    H[8] = 1.0;
    return true;
}

// the three matrices of a trapezoid into `out` (src is copied too); false: rejected, `out` is then partly written and must be dropped
ADAS_HD bool birdview_matrices(const float src[8], const float dst[8], BirdState& out, double* A) {
    for (int k = 0; k < 8; ++k) out.src[k] = src[k];
    if (!birdview_perspective(src, dst, out.M, A)) return false;
    if (!birdview_perspective(dst, src, out.M_inv, A)) return false;
    if (!warp_invert3x3(out.M, out.M_warp)) return false;   // det M == 0
    for (int k = 0; k < 9; ++k)
        if (!bird_finite(out.M_warp[k])) return false;
    return true;
}

// PerspectiveTransformation(img_size): false when img_size itself is degenerate
ADAS_HD bool birdview_init(int w, int h, BirdState& st, double* A) {
    float src[8], dst[8];
    birdview_initial_src(w, h, src);
    birdview_dst(w, h, dst);
    st.n_updates = 0;
    st.n_rejected = 0;
    return birdview_matrices(src, dst, st, A);
}

// One request on one stream: updateTransformParams(lanes_points[1], lanes_points[2], mode).  `next` is scratch for the candidate state.
// Returns 1: applied, 0: nothing to do (unknown mode / an empty lane: the reference returns silently), -1: rejected.
ADAS_HD int birdview_apply(BirdState& st, int w, int h, int mode, int nL, const BirdLaneStats& L, int nR, const BirdLaneStats& R, BirdState& next,
                           double* A) {
    if (nL <= 0 || nR <= 0) return 0;
    float src[8], dst[8];
    for (int k = 0; k < 8; ++k) src[k] = st.src[k];
    if (!birdview_update(src, mode, L, R)) return 0;
    birdview_dst(w, h, dst);
    if (!birdview_matrices(src, dst, next, A)) {
        st.n_rejected = st.n_rejected + 1;
        return -1;
    }
    for (int k = 0; k < 8; ++k) st.src[k] = next.src[k];
    for (int k = 0; k < 9; ++k) {
        st.M[k] = next.M[k];
        st.M_inv[k] = next.M_inv[k];
        st.M_warp[k] = next.M_warp[k];
    }
    st.n_updates = st.n_updates + 1;
    return 1;
}

}  // namespace adas
