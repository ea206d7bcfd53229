// birdview_kernels.hip -- the bird-view trapezoid of every video stream kept on the device: PerspectiveTransformation's src corners,
// M, M_inv and the warp's destination -> source matrix, re-anchored on the ego lanes by updateTransformParams' rules
// (perspectiveTransformation.py:39-86) without a round trip to the host.  The arithmetic is birdview_core.h; this file is the kernel
// around it and the C ABI (adas_birdview_*).
//
// The host only says WHICH rule a stream should apply next (adas_birdview_request: a one-word store into a device table, stream-ordered
// ahead of the step, so a captured step replays unchanged).  The kernel decides WHETHER to apply it -- only on a frame whose two ego
// lanes are detected (area_status, core.py:143-148) -- consumes the request either way (CheckStatus() consumes the toggle regardless),
// and leaves every frame's M / M_warp in per-frame tables for the geometry kernel and the image warp behind it.
//
// One wave per stream: the min / max over the <= 128 points of each ego lane are wave reductions, the two 8x8 eliminations are lane 0's
// work (latency-bound by design: ~1.5k dependent fp64 operations, once per request; a step without a request only copies 18 doubles
// per frame).  One launch per step.
#include "common.h"
#include <string.h>
#include <new>
#include <vector>
#include "birdview_core.h"

using namespace adas;

static_assert(sizeof(BirdState) == sizeof(adas_birdview_state), "adas_birdview_state layout");
static_assert(ADAS_UFLD_MAX_POINTS == 128, "lane point capacity");

namespace {

struct BirdDev {
    int img_w, img_h;
    BirdState* state;   // [n_streams] live state
    int* request;       // [n_streams] mode queued for the stream's next run, 0 = none
    double* M;          // [max_frames][9] frontal -> bird view, per frame of the last run
    double* M_warp;     // [max_frames][9] its inverse (destination -> source of the image warp)
    int* applied;       // [max_frames] 1: the request was applied on this frame, -1: rejected there, 0: neither
    const int *lane_cnt, *lane_det, *lane_pts;   // the decoder's arrays
    int n_streams, n_frames;
};

__device__ __forceinline__ int wave_min_i32(int v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void birdview_kernel(BirdDev d) {
    __shared__ double A[72];   // the augmented 8x9 system (dynamic row indices: kept out of scratch)
    const int s = blockIdx.x, lane = threadIdx.x;
    BirdState st = d.state[s];             // wave-uniform
    const int mode = d.request[s];
    bool changed = false;
    for (int f = 0; f < d.n_frames; ++f) {   // frame f of stream s sits at f * n_streams + s; temporal order
        const size_t q = (size_t)f * d.n_streams + s;
        int applied = 0;
        if (f == 0 && mode != BIRD_MODE_NONE) {   // a request lands on the first frame of the run only
            const int* det = d.lane_det + q * 4;
            if (det[1] && det[2]) {
                BirdLaneStats ls[2];
                int n[2];
                for (int l = 0; l < 2; ++l) {
                    const int c = d.lane_cnt[q * 4 + 1 + l];
                    n[l] = c < 0 ? 0 : (c > ADAS_UFLD_MAX_POINTS ? ADAS_UFLD_MAX_POINTS : c);
                    const int* p = d.lane_pts + (q * 4 + 1 + l) * ADAS_UFLD_MAX_POINTS * 2;
                    BirdLaneStats t = bird_stats_empty();
                    for (int i = lane; i < n[l]; i += 64) bird_stats_add(t, p[2 * i], p[2 * i + 1]);
                    ls[l].min_y = wave_min_i32(t.min_y);
                    ls[l].min_x = wave_min_i32(t.min_x);
                    ls[l].max_x = wave_max_i32(t.max_x);
                }
                if (lane == 0) {
                    BirdState next;
                    applied = birdview_apply(st, d.img_w, d.img_h, mode, n[0], ls[0], n[1], ls[1], next, A);
                    changed = applied != 0;
                }
            }
        }
        if (lane == 0) {   // later frames of the step see the updated state
            for (int k = 0; k < 9; ++k) {
                d.M[q * 9 + k] = st.M[k];
                d.M_warp[q * 9 + k] = st.M_warp[k];
            }
            d.applied[q] = applied;
        }
    }
    if (lane == 0) {
        if (changed) d.state[s] = st;
        if (mode != BIRD_MODE_NONE) d.request[s] = BIRD_MODE_NONE;   // consumed whether or not it was applied
    }
}

__global__ void birdview_request_kernel(int* request, int stream, int mode) { request[stream] = mode; }

}  // namespace

struct adas_birdview {
    adas_birdview_params p;
    int n_streams = 0, max_frames = 0;
    BirdState init;          // PerspectiveTransformation(img_size): what create and reset upload
    BirdDev dev;
    void* arena = nullptr;
    int run_frames = 0;      // frames the last run wrote into the per-frame tables
    hipStream_t last = 0;
};

namespace adas {
int birdview_capacity(const ::adas_birdview* h, int* n_streams, int* max_frames) {
    if (!h) return 0;
    if (n_streams) *n_streams = h->n_streams;
    if (max_frames) *max_frames = h->max_frames;
    return 1;
}
int* birdview_request_table(::adas_birdview* h) { return h ? h->dev.request : nullptr; }
}  // namespace adas

static int birdview_reset_streams(adas_birdview* h, int first, int count) {
    for (int s = first; s < first + count; ++s) ADAS_HIP_TRY(hipMemcpy(h->dev.state + s, &h->init, sizeof(BirdState), hipMemcpyHostToDevice));
    ADAS_HIP_TRY(hipMemset(h->dev.request + first, 0, (size_t)count * sizeof(int)));
    return ADAS_OK;
}

extern "C" {

int adas_birdview_create(const adas_birdview_params* p, int n_streams, int max_frames, adas_birdview** out) {
    ADAS_REQUIRE(p && out && n_streams > 0 && n_streams <= 65535 && max_frames >= n_streams, ADAS_ERR_INVALID,
                 "adas_birdview_create: bad argument (n_streams %d, max_frames %d: the tables hold one run = n_streams x frames per stream)", n_streams,
                 max_frames);
    ADAS_REQUIRE(p->img_w > 0 && p->img_w <= ADAS_WARP_MAX_COLS && p->img_h > 0 && p->img_h <= ADAS_WARP_MAX_ROWS, ADAS_ERR_INVALID,
                 "adas_birdview_create: img_size must be 1..%d by 1..%d, got %dx%d", ADAS_WARP_MAX_COLS, ADAS_WARP_MAX_ROWS, p->img_w, p->img_h);
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    adas_birdview* h = new (std::nothrow) adas_birdview();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    double A[72];
    if (!birdview_init(p->img_w, p->img_h, h->init, A)) {
        delete h;
        ADAS_REQUIRE(false, ADAS_ERR_INVALID, "adas_birdview_create: img_size %dx%d gives a degenerate trapezoid", p->img_w, p->img_h);
    }
    h->p = *p;
    h->n_streams = n_streams;
    h->max_frames = max_frames;
    const size_t S = n_streams, F = max_frames;
    const size_t bytes = S * sizeof(BirdState) + F * 18 * sizeof(double) + (S + F) * sizeof(int) + 256;
    if (hipMalloc(&h->arena, bytes) != hipSuccess) {
        delete h;
        return hip_fail(hipGetLastError(), "hipMalloc(birdview arena)", __FILE__, __LINE__);
    }
    (void)hipMemset(h->arena, 0, bytes);
    unsigned char* q = (unsigned char*)h->arena;
    BirdDev& d = h->dev;
    d.img_w = p->img_w; d.img_h = p->img_h;
    d.state = (BirdState*)q; q += S * sizeof(BirdState);
    d.M = (double*)q; q += F * 9 * sizeof(double);
    d.M_warp = (double*)q; q += F * 9 * sizeof(double);
    d.request = (int*)q; q += S * sizeof(int);
    d.applied = (int*)q;
    d.lane_cnt = d.lane_det = d.lane_pts = nullptr;
    d.n_streams = d.n_frames = 0;
    int rc = birdview_reset_streams(h, 0, n_streams);
    if (rc == ADAS_OK) {   // device_views are meaningful before the first run: every row starts as the initial matrices
        std::vector<double> tab(F * 18);
        for (size_t f = 0; f < F; ++f) {
            memcpy(&tab[9 * f], h->init.M, 72);
            memcpy(&tab[9 * (F + f)], h->init.M_warp, 72);
        }
        if (hipMemcpy(d.M, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)   // M_warp follows M in the arena
            rc = hip_fail(hipGetLastError(), "hipMemcpy(birdview tables)", __FILE__, __LINE__);
    }
    if (rc != ADAS_OK) {
        (void)hipFree(h->arena);
        delete h;
        return rc;
    }
    *out = h;
    return ADAS_OK;
}

int adas_birdview_destroy(adas_birdview* h) {
    if (!h) return ADAS_OK;
    if (h->arena) (void)hipFree(h->arena);
    delete h;
    return ADAS_OK;
}

int adas_birdview_reset(adas_birdview* h, int stream) {
    ADAS_REQUIRE(h && stream >= -1 && stream < h->n_streams, ADAS_ERR_INVALID, "adas_birdview_reset: bad argument");
    ADAS_HIP_TRY(hipDeviceSynchronize());   // runs and requests may sit on different streams
    return stream < 0 ? birdview_reset_streams(h, 0, h->n_streams) : birdview_reset_streams(h, stream, 1);
}

int adas_birdview_request(adas_birdview* h, int stream, int mode, void* hip_stream) {
    ADAS_REQUIRE(h && stream >= 0 && stream < h->n_streams, ADAS_ERR_INVALID, "adas_birdview_request: stream %d of %d", stream, h ? h->n_streams : 0);
    hipLaunchKernelGGL(birdview_request_kernel, dim3(1), dim3(1), 0, (hipStream_t)hip_stream, h->dev.request, stream, mode);
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

int adas_birdview_run(adas_birdview* h, const adas_ufld_decode* decode, int n_streams, int n_frames, void* hip_stream) {
    ADAS_REQUIRE(h && decode && n_streams > 0 && n_streams <= h->n_streams && n_frames > 0 && (long long)n_streams * n_frames <= h->max_frames &&
                     n_streams * n_frames <= adas::handle_max_batch(decode),
                 ADAS_ERR_INVALID, "adas_birdview_run: bad argument (%d streams x %d frames; the handle holds %d streams, %d frames; the decoder %d)",
                 n_streams, n_frames, h ? h->n_streams : 0, h ? h->max_frames : 0, adas::handle_max_batch(decode));
    hipStream_t st = (hipStream_t)hip_stream;
    BirdDev d = h->dev;
    adas::decode_lane_views(decode, &d.lane_cnt, &d.lane_det, &d.lane_pts);
    d.n_streams = n_streams;
    d.n_frames = n_frames;
    hipLaunchKernelGGL(birdview_kernel, dim3((unsigned)n_streams), dim3(64), 0, st, d);
    ADAS_HIP_TRY(hipGetLastError());
    h->last = st;
    h->run_frames = n_streams * n_frames;
    return ADAS_OK;
}

int adas_birdview_fetch_stream(adas_birdview* h, int stream, adas_birdview_state* state) {
    ADAS_REQUIRE(h && state && stream >= 0 && stream < h->n_streams, ADAS_ERR_INVALID, "adas_birdview_fetch_stream: bad argument");
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(state, h->dev.state + stream, sizeof(BirdState), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_birdview_fetch_frame(adas_birdview* h, int frame, double* M9, double* M_warp9, int32_t* applied) {
    ADAS_REQUIRE(h && frame >= 0 && frame < h->max_frames, ADAS_ERR_INVALID, "adas_birdview_fetch_frame: bad argument");
    ADAS_REQUIRE(frame < h->run_frames, ADAS_ERR_INVALID, "adas_birdview_fetch_frame: frame %d was not part of the last run (%d frames)", frame,
                 h->run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    if (M9) ADAS_HIP_TRY(hipMemcpy(M9, h->dev.M + 9 * (size_t)frame, 72, hipMemcpyDeviceToHost));
    if (M_warp9) ADAS_HIP_TRY(hipMemcpy(M_warp9, h->dev.M_warp + 9 * (size_t)frame, 72, hipMemcpyDeviceToHost));
    if (applied) ADAS_HIP_TRY(hipMemcpy(applied, h->dev.applied + frame, 4, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_birdview_pending(adas_birdview* h, int stream, int32_t* mode) {
    ADAS_REQUIRE(h && mode && stream >= 0 && stream < h->n_streams, ADAS_ERR_INVALID, "adas_birdview_pending: bad argument");
    ADAS_HIP_TRY(hipDeviceSynchronize());   // a request may sit on any stream
    ADAS_HIP_TRY(hipMemcpy(mode, h->dev.request + stream, 4, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_birdview_device_views(adas_birdview* h, const double** d_M, const double** d_M_warp) {
    ADAS_REQUIRE(h && d_M && d_M_warp, ADAS_ERR_INVALID, "adas_birdview_device_views: bad argument");
    *d_M = h->dev.M;
    *d_M_warp = h->dev.M_warp;
    return ADAS_OK;
}

}  // extern "C"
