// analysis_kernels.hip -- the last block of the reference's per-frame loop (demo.py:284-296) kept on the device per video stream:
// SingleCamDistanceMeasure.updateDistance / calcCollisionPoint and TaskConditions' FCWS / LDWS / LKAS state machine, whose CheckStatus()
// is what tells the bird view which re-anchoring rule a stream applies next.  The arithmetic is analysis_core.h; this file is the kernel
// around it and the C ABI (adas_analysis_*).
//
// One workgroup of four waves per stream, frames of the stream walked in temporal order inside the launch (as adas_birdview_run and the
// micro-batched tracker do); no communication between workgroups.  Per frame:
//   wave 0      strides the survivors, measures them and compacts the measured points IN SURVIVOR ORDER into LDS (ballot + prefix count);
//   all waves   stage the frame's ego-lane polygon in LDS once (at most 2 x img_h int32 pairs);
//   every wave  takes points round-robin; its lanes stride the polygon's edges, one ballot ORs "on an edge", another XORs the crossings;
//   wave 0      arg-mins (distance, index) over the points inside or on the polygon;
//   thread 0    advances the state machine (analysis_step) and stores the stream's request word for its next frame.
// A frame without survivors, without measured points or without a polygon skips the polygon pass.  The state machine is latency-bound by
// design: a few hundred dependent operations per frame on windows of 5, 5 and 10 entries, kept in LDS (dynamic indices: out of scratch).
#include "common.h"
#include <string.h>
#include <new>
#include <vector>
#include "analysis_core.h"

using namespace adas;

static_assert(sizeof(AnalysisState) == sizeof(adas_analysis_state), "adas_analysis_state layout");
static_assert(sizeof(AnalysisInput) == sizeof(adas_analysis_input), "adas_analysis_input layout");
static_assert(sizeof(AnalysisFrame) == sizeof(adas_analysis_frame), "adas_analysis_frame layout");
static_assert(offsetof(adas_analysis_params, n_classes) == offsetof(AnalysisCfg, n_classes) && sizeof(AnalysisCfg) == 56, "adas_analysis_params head");
static_assert(sizeof(adas_lane_geometry_result) == 48 && offsetof(adas_lane_geometry_result, curvature) == 32, "adas_lane_geometry_result layout");
static_assert(ANA_MODE_DEFAULT == ADAS_BIRDVIEW_DEFAULT && ANA_MODE_TOP == ADAS_BIRDVIEW_TOP && ANA_MODE_BOTTOM == ADAS_BIRDVIEW_BOTTOM, "request words");

namespace {

constexpr int ANA_THREADS = 256, ANA_WAVES = ANA_THREADS / 64;

struct AnaDev {
    AnalysisCfg cfg;
    const double* ref_height;   // [cfg.n_classes] inches, 0: class not measured
    AnalysisState* state;       // [n_streams] live state
    AnalysisFrame* frames;      // [max_frames] records of the last run
    int* pts_xy;                // [max_frames][max_points][2] distance points of the last run ...
    double* pts_d;              // [max_frames][max_points]    ... and their metres
    int max_points, max_poly;
    // what this run reads
    const AnalysisInput* inputs;   // non-null: the state machine alone, one record per frame
    const double* xyxy;            // [frames][det_stride][4] fp64 of the int-truncated corners
    const int* cls;                // [frames][det_stride]
    const int* counts;             // [frames][4]: n_found, n_candidates, n_keep, flags
    int det_stride;
    const int* poly;               // frame q's polygon at poly + q * poly_stride, (x, y) int32 pairs
    size_t poly_stride;
    const int *poly_n0, *poly_n1;  // its point count: poly_n0[q * poly_n_stride] (+ poly_n1[...] when non-null)
    int poly_n_stride;
    const int* geo_i;              // frame q's area_status / direction at geo_i[q * geo_i_stride + 0 / 3]
    const double* geo_d;           // its curvature / offset at geo_d[q * geo_d_stride + 0 / 1]
    int geo_i_stride, geo_d_stride;
    int* request;                  // [n_streams] or null: the stream's request word for its next frame
    int n_streams, n_frames;
};

__global__ __launch_bounds__(ANA_THREADS) void analysis_kernel(AnaDev d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ AnalysisState st;   // thread 0's alone
    __shared__ int sh_points;
    double* p_d = (double*)smem;                 // [max_points]
    int* p_xy = (int*)(p_d + d.max_points);      // [max_points][2]
    int* p_in = p_xy + 2 * d.max_points;         // [max_points] point_in_polygon of each point
    int* poly = p_in + d.max_points;             // [max_poly][2]
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) st = d.state[s];
    for (int f = 0; f < d.n_frames; ++f) {       // frame f of stream s sits at f * n_streams + s; temporal order
        const size_t q = (size_t)f * d.n_streams + s;
        AnalysisFrame fr;
        fr.n_points = 0; fr.has_collision = 0; fr.collision_x = 0; fr.collision_y = 0; fr.collision_d = 0.0; fr.collision_index = -1;
        fr.flags = 0;
        if (d.inputs) {
            if (tid == 0) {
                const AnalysisInput in = d.inputs[q];
                const int req = analysis_step(st, d.cfg, in, fr);
                d.frames[q] = fr;
                if (d.request) d.request[s] = req;
            }
            continue;
        }
        int n = d.counts[q * 4 + 2];
        if (d.counts[q * 4 + 3] & 1) fr.flags |= ANA_FLAG_OVERFLOW;
        const int cap = d.det_stride < d.max_points ? d.det_stride : d.max_points;
        if (n < 0) n = 0;
        if (n > cap) { n = cap; fr.flags |= ANA_FLAG_TRUNCATED; }
        int np = d.poly_n0[q * d.poly_n_stride] + (d.poly_n1 ? d.poly_n1[q * d.poly_n_stride] : 0);
        np = np < 0 ? 0 : (np > d.max_poly ? d.max_poly : np);
        __syncthreads();   // the previous frame's readers are done with the LDS arrays
        if (wave == 0) {
            int base = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {   // wave-uniform trip count: every lane reaches the ballot
                const int i = i0 + lane;
                int x = 0, y = 0;
                double m = 0.0;
                bool ok = false;
                if (i < n) {
                    const size_t r = q * d.det_stride + i;
                    ok = analysis_measure(d.cfg, d.ref_height, d.xyxy + r * 4, d.cls[r], &x, &y, &m);
                }
                const unsigned long long mask = __ballot(ok);
                if (ok) {
                    const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));   // < n <= max_points
                    p_xy[2 * pos] = x; p_xy[2 * pos + 1] = y; p_d[pos] = m;
                    const size_t g = q * d.max_points + pos;
                    d.pts_xy[2 * g] = x; d.pts_xy[2 * g + 1] = y; d.pts_d[g] = m;
                }
                base += __popcll(mask);
            }
            if (lane == 0) sh_points = base;
        }
        const int* gp = d.poly + q * d.poly_stride;
        for (int i = tid; i < 2 * np; i += ANA_THREADS) poly[i] = gp[i];
        __syncthreads();
        const int m = sh_points;
        int best = 2147483647;
        double best_d = 0.0;
        if (m > 0 && np > 0) {   // block-uniform
            for (int j = wave; j < m; j += ANA_WAVES) {
                const double x = (double)p_xy[2 * j], y = (double)p_xy[2 * j + 1];
                int any_on = 0, parity = 0;
                for (int e0 = 0; e0 < np; e0 += 64) {
                    const int e = e0 + lane;
                    int on = 0, cross = 0;
                    if (e < np) cross = analysis_poly_edge(poly, np, e, x, y, &on);
                    any_on |= __ballot(on) != 0ull;
                    parity ^= __popcll(__ballot(cross)) & 1;
                }
                if (lane == 0) p_in[j] = analysis_poly_decide(np, any_on, parity);
            }
            __syncthreads();
            if (wave == 0) {
                for (int j = lane; j < m; j += 64)
                    if (p_in[j] >= 0 && (best == 2147483647 || analysis_nearer(p_d[j], j, best_d, best))) { best = j; best_d = p_d[j]; }
                for (int o = 32; o > 0; o >>= 1) {
                    const double od = __shfl_xor(best_d, o, 64);
                    const int oj = __shfl_xor(best, o, 64);
                    if (oj != 2147483647 && (best == 2147483647 || analysis_nearer(od, oj, best_d, best))) { best = oj; best_d = od; }
                }
            }
        }
        if (tid == 0) {
            fr.n_points = m;
            AnalysisInput in;
            const int dir = d.geo_i[q * d.geo_i_stride + 3];
            in.has_point = best != 2147483647;
            in.area = d.geo_i[q * d.geo_i_stride] != 0;
            in.has_offset = dir != ANA_DIR_NONE; in.has_curvature = dir != ANA_DIR_NONE;   // no curve estimate: offset and curvature are None
            in.direction = dir; in.reserved = 0;
            in.curvature = d.geo_d[q * d.geo_d_stride]; in.offset = d.geo_d[q * d.geo_d_stride + 1];
            in.distance = 0.0;
            if (in.has_point) {
                fr.has_collision = 1; fr.collision_index = best;
                fr.collision_x = p_xy[2 * best]; fr.collision_y = p_xy[2 * best + 1]; fr.collision_d = best_d;
                in.distance = best_d;
            }
            const int req = analysis_step(st, d.cfg, in, fr);
            d.frames[q] = fr;
            if (d.request) d.request[s] = req;
        }
    }
    if (tid == 0) d.state[s] = st;
}

size_t analysis_lds_bytes(int max_points, int max_poly) { return (size_t)max_points * 20 + (size_t)max_poly * 8; }

}  // namespace

struct adas_analysis {
    adas_analysis_params p;
    int n_streams = 0, max_frames = 0;
    AnaDev dev;
    AnalysisInput* d_inputs = nullptr;   // [max_frames] staging of adas_analysis_run_inputs
    void* arena = nullptr;
    int run_frames = 0;                  // frames the last run wrote
    int run_points = 0;                  // 1: the last run measured distance points
    hipStream_t last = 0;
    adas_birdview* bird = nullptr;       // bound by the pipeline: reset queues the initial "Default" there ...
    hipStream_t bird_stream = 0;         // ... on the stream the next step is ordered behind
};

namespace adas {
int analysis_capacity(const ::adas_analysis* h, int* n_streams, int* max_frames) {
    if (!h) return 0;
    if (n_streams) *n_streams = h->n_streams;
    if (max_frames) *max_frames = h->max_frames;
    return 1;
}
void analysis_frame_views(const ::adas_analysis* h, const int** frames, int* stride, const int** pts_xy, int* max_points) {
    *frames = (const int*)h->dev.frames;
    *stride = (int)(sizeof(AnalysisFrame) / 4);
    *pts_xy = h->dev.pts_xy;
    *max_points = h->dev.max_points;
}
const double* analysis_points_d(const ::adas_analysis* h) { return h->dev.pts_d; }
int analysis_bind_birdview(::adas_analysis* h, ::adas_birdview* bird, int n_streams, void* hip_stream) {
    h->bird = bird;
    h->bird_stream = (hipStream_t)hip_stream;
    if (!bird) return ADAS_OK;
    for (int s = 0; s < n_streams; ++s) {   // the reference's first CheckStatus() returns True with "Default"
        int rc = adas_birdview_request(bird, s, ADAS_BIRDVIEW_DEFAULT, hip_stream);
        if (rc) return rc;
    }
    return ADAS_OK;
}
}  // namespace adas

static int analysis_reset_streams(adas_analysis* h, int first, int count) {
    AnalysisState init;
    analysis_state_init(init);
    for (int s = first; s < first + count; ++s) ADAS_HIP_TRY(hipMemcpy(h->dev.state + s, &init, sizeof(init), hipMemcpyHostToDevice));
    return ADAS_OK;
}

static int analysis_launch(adas_analysis* h, AnaDev& d, int n_streams, int n_frames, hipStream_t st, int with_points) {
    d.n_streams = n_streams;
    d.n_frames = n_frames;
    hipLaunchKernelGGL(analysis_kernel, dim3((unsigned)n_streams), dim3(ANA_THREADS), analysis_lds_bytes(d.max_points, d.max_poly), st, d);
    ADAS_HIP_TRY(hipGetLastError());
    h->last = st;
    h->run_frames = n_streams * n_frames;
    h->run_points = with_points;
    return ADAS_OK;
}

#define ANA_RUN_REQUIRE(name)                                                                                                                    \
    ADAS_REQUIRE(h && n_streams > 0 && n_streams <= h->n_streams && n_frames > 0 && (long long)n_streams * n_frames <= h->max_frames, ADAS_ERR_INVALID, \
                 name ": bad argument (%d streams x %d frames; the handle holds %d streams, %d frames)", n_streams, n_frames, h ? h->n_streams : 0,    \
                 h ? h->max_frames : 0)

extern "C" {

int adas_analysis_default_params(adas_analysis_params* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_analysis_default_params: null argument");
    memset(p, 0, sizeof(*p));
    p->focal = 100.0; p->y_limit = 650.0;
    p->distance_thres = 1.5; p->offset_thres = 0.65; p->curvae_thres = 500.0;
    p->calib_frequency = 3; p->calib_curvae_thres = 15000.0;
    p->max_points = 512; p->max_poly = 1440;
    return ADAS_OK;
}

int adas_analysis_create(const adas_analysis_params* p, int n_streams, int max_frames, adas_analysis** out) {
    ADAS_REQUIRE(p && out && n_streams > 0 && n_streams <= 65535 && max_frames >= n_streams, ADAS_ERR_INVALID,
                 "adas_analysis_create: bad argument (n_streams %d, max_frames %d: the tables hold one run = n_streams x frames per stream)", n_streams,
                 max_frames);
    ADAS_REQUIRE(p->n_classes >= 0 && p->n_classes <= 65536 && (p->n_classes == 0 || p->h_ref_height), ADAS_ERR_INVALID,
                 "adas_analysis_create: n_classes %d needs a ref_height table", p->n_classes);
    ADAS_REQUIRE(p->max_points >= 1 && p->max_points <= 2048 && p->max_poly >= 1 && p->max_poly <= 8640, ADAS_ERR_INVALID,
                 "adas_analysis_create: max_points must be in [1, 2048], max_poly in [1, 8640] (got %d, %d)", p->max_points, p->max_poly);
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    adas_analysis* h = new (std::nothrow) adas_analysis();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->p = *p;
    h->p.h_ref_height = nullptr;   // the caller's table is copied, not kept
    h->n_streams = n_streams;
    h->max_frames = max_frames;
    const size_t S = n_streams, F = max_frames, P = p->max_points, NC = p->n_classes > 0 ? p->n_classes : 1;
    const size_t bytes = S * sizeof(AnalysisState) + F * sizeof(AnalysisFrame) + F * sizeof(AnalysisInput) + F * P * 16 + NC * 8 + 256;
    if (hipMalloc(&h->arena, bytes) != hipSuccess) {
        delete h;
        return hip_fail(hipGetLastError(), "hipMalloc(analysis arena)", __FILE__, __LINE__);
    }
    (void)hipMemset(h->arena, 0, bytes);
    unsigned char* q = (unsigned char*)h->arena;   // 8-byte members first: every table stays aligned
    AnaDev& d = h->dev;
    memset(&d, 0, sizeof(d));
    memcpy(&d.cfg, p, sizeof(AnalysisCfg));
    d.state = (AnalysisState*)q; q += S * sizeof(AnalysisState);
    d.frames = (AnalysisFrame*)q; q += F * sizeof(AnalysisFrame);
    h->d_inputs = (AnalysisInput*)q; q += F * sizeof(AnalysisInput);
    d.pts_d = (double*)q; q += F * P * 8;
    double* ref = (double*)q; q += NC * 8;
    d.pts_xy = (int*)q;
    d.ref_height = ref;
    d.max_points = p->max_points;
    d.max_poly = p->max_poly;
    int rc = ADAS_OK;
    if (p->n_classes > 0 && hipMemcpy(ref, p->h_ref_height, (size_t)p->n_classes * 8, hipMemcpyHostToDevice) != hipSuccess)
        rc = hip_fail(hipGetLastError(), "hipMemcpy(ref_height)", __FILE__, __LINE__);
    const size_t lds = analysis_lds_bytes(p->max_points, p->max_poly);
    if (rc == ADAS_OK && lds > 48 * 1024 &&
        hipFuncSetAttribute((const void*)analysis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024) != hipSuccess)
        rc = hip_fail(hipGetLastError(), "hipFuncSetAttribute(analysis_kernel)", __FILE__, __LINE__);
    if (rc == ADAS_OK) rc = analysis_reset_streams(h, 0, n_streams);
    if (rc != ADAS_OK) {
        (void)hipFree(h->arena);
        delete h;
        return rc;
    }
    *out = h;
    return ADAS_OK;
}

int adas_analysis_destroy(adas_analysis* h) {
    if (!h) return ADAS_OK;
    if (h->arena) (void)hipFree(h->arena);
    delete h;
    return ADAS_OK;
}

int adas_analysis_reset(adas_analysis* h, int stream) {
    ADAS_REQUIRE(h && stream >= -1 && stream < h->n_streams, ADAS_ERR_INVALID, "adas_analysis_reset: bad argument");
    ADAS_HIP_TRY(hipDeviceSynchronize());   // runs may sit on any stream
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? h->n_streams : 1;
    int rc = analysis_reset_streams(h, first, count);
    if (rc) return rc;
    if (h->bird)   // TaskConditions() starts with toggle_status "Default": its first CheckStatus() asks for it
        for (int s = first; s < first + count; ++s) {
            rc = adas_birdview_request(h->bird, s, ADAS_BIRDVIEW_DEFAULT, h->bird_stream);
            if (rc) return rc;
        }
    return ADAS_OK;
}

int adas_analysis_run_arrays(adas_analysis* h, const double* d_xyxy, const int32_t* d_cls, const int32_t* d_counts, int det_stride, const int32_t* d_poly,
                             int poly_cap, const int32_t* d_poly_counts, const adas_lane_geometry_result* d_geometry, int32_t* d_request, int n_streams,
                             int n_frames, void* stream) {
    ANA_RUN_REQUIRE("adas_analysis_run_arrays");
    ADAS_REQUIRE(d_xyxy && d_cls && d_counts && det_stride > 0 && d_poly && poly_cap > 0 && d_poly_counts && d_geometry, ADAS_ERR_INVALID,
                 "adas_analysis_run_arrays: null array or empty capacity");
    AnaDev d = h->dev;
    d.xyxy = d_xyxy; d.cls = d_cls; d.counts = d_counts; d.det_stride = det_stride;
    d.poly = d_poly; d.poly_stride = (size_t)poly_cap * 2;
    if (poly_cap < d.max_poly) d.max_poly = poly_cap;   // never read past a frame's slab
    d.poly_n0 = d_poly_counts; d.poly_n1 = nullptr; d.poly_n_stride = 1;
    d.geo_i = (const int*)d_geometry; d.geo_i_stride = (int)(sizeof(adas_lane_geometry_result) / 4);
    d.geo_d = (const double*)((const unsigned char*)d_geometry + offsetof(adas_lane_geometry_result, curvature));
    d.geo_d_stride = (int)(sizeof(adas_lane_geometry_result) / 8);
    d.request = d_request;
    return analysis_launch(h, d, n_streams, n_frames, (hipStream_t)stream, 1);
}

int adas_analysis_run(adas_analysis* h, adas_yolo_post* post, adas_lane_geometry* geometry, adas_birdview* bird, int n_streams, int n_frames, void* stream) {
    ANA_RUN_REQUIRE("adas_analysis_run");
    ADAS_REQUIRE(post && geometry, ADAS_ERR_INVALID, "adas_analysis_run: needs a yolo_post and a lane_geometry handle");
    const int frames = n_streams * n_frames;
    ADAS_REQUIRE(frames <= adas::handle_max_batch(post) && frames <= adas::handle_max_batch(geometry), ADAS_ERR_INVALID,
                 "adas_analysis_run: %d frames, the post handle holds %d, the geometry handle %d", frames, adas::handle_max_batch(post),
                 adas::handle_max_batch(geometry));
    int bs = 0;
    ADAS_REQUIRE(!bird || (adas::birdview_capacity(bird, &bs, nullptr) && bs >= n_streams), ADAS_ERR_INVALID,
                 "adas_analysis_run: the bird-view handle holds %d streams, the run has %d", bs, n_streams);
    AnaDev d = h->dev;
    const int32_t* cn = nullptr;
    const double* sc = nullptr;
    int rc = adas_yolo_post_device_views(post, &d.xyxy, &sc, &d.cls, &cn);
    if (rc) return rc;
    d.counts = cn;
    rc = adas_yolo_post_capacity(post, &d.det_stride);
    if (rc) return rc;
    const int32_t *hdr = nullptr, *area = nullptr;
    const double* vals = nullptr;
    int32_t area_stride = 0;
    rc = adas_lane_geometry_device_views(geometry, &hdr, &vals, &area, &area_stride);
    if (rc) return rc;
    d.poly = area; d.poly_stride = (size_t)area_stride;
    if (area_stride / 2 < d.max_poly) d.max_poly = area_stride / 2;
    d.poly_n0 = hdr + 1; d.poly_n1 = hdr + 2; d.poly_n_stride = 8;   // area_points = the left points, then the reversed right points
    d.geo_i = hdr; d.geo_i_stride = 8;
    d.geo_d = vals; d.geo_d_stride = 2;
    d.request = bird ? adas::birdview_request_table(bird) : nullptr;
    return analysis_launch(h, d, n_streams, n_frames, (hipStream_t)stream, 1);
}

int adas_analysis_run_inputs(adas_analysis* h, const adas_analysis_input* h_inputs, int n_streams, int n_frames, void* stream) {
    ANA_RUN_REQUIRE("adas_analysis_run_inputs");
    ADAS_REQUIRE(h_inputs, ADAS_ERR_INVALID, "adas_analysis_run_inputs: null table");
    hipStream_t st = (hipStream_t)stream;
    // from pageable host memory: the call may block until the copy is staged, and is not capturable
    ADAS_HIP_TRY(hipMemcpyAsync(h->d_inputs, h_inputs, (size_t)n_streams * n_frames * sizeof(AnalysisInput), hipMemcpyHostToDevice, st));
    AnaDev d = h->dev;
    d.inputs = h->d_inputs;
    return analysis_launch(h, d, n_streams, n_frames, st, 0);
}

int adas_analysis_fetch_stream(adas_analysis* h, int stream, adas_analysis_state* state) {
    ADAS_REQUIRE(h && state && stream >= 0 && stream < h->n_streams, ADAS_ERR_INVALID, "adas_analysis_fetch_stream: bad argument");
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(state, h->dev.state + stream, sizeof(AnalysisState), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_analysis_fetch_frame(adas_analysis* h, int frame, adas_analysis_frame* out) {
    ADAS_REQUIRE(h && out && frame >= 0 && frame < h->max_frames, ADAS_ERR_INVALID, "adas_analysis_fetch_frame: bad argument");
    ADAS_REQUIRE(frame < h->run_frames, ADAS_ERR_INVALID, "adas_analysis_fetch_frame: frame %d was not part of the last run (%d frames)", frame,
                 h->run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(out, h->dev.frames + frame, sizeof(AnalysisFrame), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_analysis_fetch_points(adas_analysis* h, int frame, int32_t* xy, double* d, int n) {
    ADAS_REQUIRE(h && frame >= 0 && frame < h->max_frames && n >= 0 && n <= h->dev.max_points, ADAS_ERR_INVALID, "adas_analysis_fetch_points: bad argument");
    ADAS_REQUIRE(frame < h->run_frames && h->run_points, ADAS_ERR_INVALID,
                 "adas_analysis_fetch_points: frame %d has no distance points from the last run (%d frames%s)", frame, h->run_frames,
                 h->run_points ? "" : ", the state machine alone");
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    const size_t g = (size_t)frame * h->dev.max_points;
    if (xy && n) ADAS_HIP_TRY(hipMemcpy(xy, h->dev.pts_xy + 2 * g, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (d && n) ADAS_HIP_TRY(hipMemcpy(d, h->dev.pts_d + g, (size_t)n * 8, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

}  // extern "C"
