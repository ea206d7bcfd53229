// warp_kernels.hip -- the bird-view image on the device: cv2.warpPerspective(frame, M, img_size, INTER_LINEAR) of BGR u8
// frames that already sit in HBM (PerspectiveTransformation.transformToBirdView / transformToFrontalView,
// perspectiveTransformation.py:89-117; demo.py:289 warps every 1280x720 frame).  The per-pixel arithmetic is warp_core.h
// (a restatement of OpenCV 4.5's reference path, parity with a real cv2 build UNPINNED); this file is the kernel around it and the
// C ABI (adas_warp_*).
//
// Memory-bound: 2.76 MB read + 2.76 MB written per 720p frame.  A thread produces a run of 4 consecutive destination pixels
// (12 bytes) and, where the run starts on a 4-byte boundary (every run when dst_w % 4 == 0), stores it as three dwords; consecutive
// lanes take consecutive runs of a row, so a wave writes 768 contiguous bytes.  The gathers go through L2 as they are: a homography
// maps a destination row to a nearly straight source line.  No LDS.
#include "common.h"
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "warp_core.h"

using namespace adas;

namespace {

struct WarpDev {
    const uint8_t* src;   // [batch][sh][sw][3]
    uint8_t* dst;         // [batch][dh][dw][3]
    const double* M;      // [batch][9] destination -> source
    int sh, sw, dh, dw;
    int bw;               // warp_block_width(dh, dw)
    int rows;             // destination rows per workgroup
    int runs;             // 4-pixel runs per row = ceil(dw / 4)
};

struct alignas(4) Run12 {
    uint32_t a, b, c;
};

__global__ __launch_bounds__(256) void warp_perspective_kernel(WarpDev d) {
    const int f = blockIdx.y;
    double M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = d.M[9 * f + k];   // workgroup-uniform
    const uint8_t* __restrict__ src = d.src + (size_t)f * d.sh * d.sw * 3;
    uint8_t* __restrict__ dst = d.dst + (size_t)f * d.dh * d.dw * 3;
    const int y0 = blockIdx.x * d.rows;
    const int nrows = d.dh - y0 < d.rows ? d.dh - y0 : d.rows;
    const int total = nrows * d.runs;
    for (int t = threadIdx.x; t < total; t += blockDim.x) {
        const int r = t / d.runs, run = t - r * d.runs;
        const int y = y0 + r, x0 = run * 4;
        const int n = d.dw - x0 < 4 ? d.dw - x0 : 4;   // the row tail: dw % 4 pixels
        uint32_t px[4] = {0, 0, 0, 0};                 // (b, g, r) of each pixel of the run in the low 24 bits
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {   // bx is per pixel: a run may straddle two of OpenCV's blocks when bw % 4 != 0
                int v[3];
                warp_sample(src, d.sh, d.sw, warp_coord(M, d.bw, x0 + i, y), v);
                px[i] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
            }
        }
        uint8_t* p = dst + ((size_t)y * d.dw + x0) * 3;
        if (n == 4 && ((uintptr_t)p & 3) == 0) {
            Run12 o;
            o.a = px[0] | (px[1] << 24);
            o.b = (px[1] >> 8) | (px[2] << 16);
            o.c = (px[2] >> 16) | (px[3] << 8);
            *reinterpret_cast<Run12*>(p) = o;
        } else {
            for (int i = 0; i < n; ++i) {
                p[3 * i + 0] = (uint8_t)px[i];
                p[3 * i + 1] = (uint8_t)(px[i] >> 8);
                p[3 * i + 2] = (uint8_t)(px[i] >> 16);
            }
        }
    }
}

// destination rows per workgroup; ADAS_WARP_ROWS overrides (A/B measurements, tools/bench_warp.py)
int warp_rows() {
    static int v = -2;
    if (v == -2) {
        const char* e = getenv("ADAS_WARP_ROWS");
        v = e ? atoi(e) : -1;
        if (v < 1 || v > 1024) v = -1;
    }
    return v > 0 ? v : 4;
}

}  // namespace

struct adas_warp {
    adas_warp_params p;
    int max_batch = 0;
    std::vector<double> M;             // [max_batch][9] destination -> source (already inverted), the host copy
    std::vector<unsigned char> dirty;  // rows of M the device table does not hold yet
    double* d_M = nullptr;             // device table, allocated by the first run
    uint8_t* d_dst = nullptr;          // the handle's own [max_batch][dst_h][dst_w][3], allocated when first asked for
    int dst_frames = 0;                // frames [0, dst_frames) of d_dst have been written by some run
    hipStream_t last = 0;
    size_t frame_bytes() const { return (size_t)p.dst_h * p.dst_w * 3; }
};

static int warp_own_buffer(adas_warp* h) {
    if (!h->d_dst) ADAS_HIP_TRY(hipMalloc((void**)&h->d_dst, h->frame_bytes() * h->max_batch));
    return ADAS_OK;
}

namespace adas {
int warp_geometry(const ::adas_warp* h, int* src_h, int* src_w, int* max_batch) {
    if (!h) return 0;
    *src_h = h->p.src_h;
    *src_w = h->p.src_w;
    *max_batch = h->max_batch;
    return 1;
}
void warp_dst_geometry(const ::adas_warp* h, int* dst_h, int* dst_w) {
    *dst_h = h->p.dst_h;
    *dst_w = h->p.dst_w;
}
}  // namespace adas

// frames [0, batch) of src through matrices M [batch][9] (device, destination -> source) into dst, or the handle's own buffer
static int warp_launch(adas_warp* h, const uint8_t* src, uint8_t* dst, const double* M, int batch, hipStream_t st) {
    WarpDev d;
    d.src = src;
    d.dst = dst ? dst : h->d_dst;
    d.M = M;
    d.sh = h->p.src_h; d.sw = h->p.src_w; d.dh = h->p.dst_h; d.dw = h->p.dst_w;
    d.bw = warp_block_width(d.dh, d.dw);
    d.rows = warp_rows();
    d.runs = (d.dw + 3) / 4;
    hipLaunchKernelGGL(warp_perspective_kernel, dim3((unsigned)((d.dh + d.rows - 1) / d.rows), (unsigned)batch), dim3(256), 0, st, d);
    ADAS_HIP_TRY(hipGetLastError());
    h->last = st;
    if (!dst && batch > h->dst_frames) h->dst_frames = batch;
    return ADAS_OK;
}

extern "C" {

int adas_warp_create(const adas_warp_params* p, int max_batch, adas_warp** out) {
    ADAS_REQUIRE(p && out && max_batch > 0 && max_batch <= 65535, ADAS_ERR_INVALID, "adas_warp_create: bad argument");
    ADAS_REQUIRE(p->src_h > 0 && p->src_h <= ADAS_WARP_MAX_ROWS && p->dst_h > 0 && p->dst_h <= ADAS_WARP_MAX_ROWS && p->src_w > 0 &&
                     p->src_w <= ADAS_WARP_MAX_COLS && p->dst_w > 0 && p->dst_w <= ADAS_WARP_MAX_COLS,
                 ADAS_ERR_INVALID, "adas_warp_create: images must be 1..%d rows by 1..%d columns (source %dx%d, destination %dx%d)",
                 ADAS_WARP_MAX_ROWS, ADAS_WARP_MAX_COLS, p->src_h, p->src_w, p->dst_h, p->dst_w);
    adas_warp* h = new (std::nothrow) adas_warp();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->p = *p;
    h->max_batch = max_batch;
    h->M.assign((size_t)max_batch * 9, 0.0);
    for (int f = 0; f < max_batch; ++f) h->M[9 * f] = h->M[9 * f + 4] = h->M[9 * f + 8] = 1.0;   // identity until set_matrix
    h->dirty.assign(max_batch, 1);
    *out = h;   // device memory comes with the first run: the handle and its matrices are host state
    return ADAS_OK;
}

int adas_warp_destroy(adas_warp* h) {
    if (!h) return ADAS_OK;
    if (h->d_M) (void)hipFree(h->d_M);
    if (h->d_dst) (void)hipFree(h->d_dst);
    delete h;
    return ADAS_OK;
}

int adas_warp_set_matrix(adas_warp* h, int frame, const double* M9, int inverse_map) {
    ADAS_REQUIRE(h && M9 && frame >= -1 && frame < h->max_batch, ADAS_ERR_INVALID, "adas_warp_set_matrix: bad argument");
    double m[9];
    if (inverse_map) memcpy(m, M9, sizeof(m));
    else ADAS_REQUIRE(warp_invert3x3(M9, m), ADAS_ERR_INVALID, "adas_warp_set_matrix: the matrix is singular (determinant 0)");
    for (int f = frame < 0 ? 0 : frame; f < (frame < 0 ? h->max_batch : frame + 1); ++f) {
        memcpy(&h->M[9 * (size_t)f], m, sizeof(m));
        h->dirty[f] = 1;
    }
    return ADAS_OK;
}

int adas_warp_run(adas_warp* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, int batch, void* stream) {
    ADAS_REQUIRE(h && d_src_bgr && batch > 0 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_warp_run: bad argument (batch %d, handle holds %d)",
                 batch, h ? h->max_batch : 0);
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    hipStream_t st = (hipStream_t)stream;
    if (!h->d_M) ADAS_HIP_TRY(hipMalloc((void**)&h->d_M, h->M.size() * sizeof(double)));
    if (!d_dst_bgr) {
        int rc = warp_own_buffer(h);
        if (rc) return rc;
    }
    // changed rows go ahead of the launch on its stream; the source is pageable memory, which the runtime has read (staged) by the time
    // the call returns, so a later set_matrix cannot reach an earlier run.  The price: a run that follows a set_matrix may block the host
    // for that copy, and cannot be captured into a graph (include/adas_hip.h says so)
    for (int f = 0; f < h->max_batch;) {
        if (!h->dirty[f]) { ++f; continue; }
        int e = f;
        while (e < h->max_batch && h->dirty[e]) h->dirty[e++] = 0;
        ADAS_HIP_TRY(hipMemcpyAsync(h->d_M + 9 * (size_t)f, &h->M[9 * (size_t)f], (size_t)(e - f) * 9 * sizeof(double), hipMemcpyHostToDevice, st));
        f = e;
    }
    return warp_launch(h, d_src_bgr, d_dst_bgr, h->d_M, batch, st);
}

int adas_warp_run_device_matrices(adas_warp* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const double* d_M_warp, int batch, void* stream) {
    ADAS_REQUIRE(h && d_src_bgr && d_M_warp && batch > 0 && batch <= h->max_batch, ADAS_ERR_INVALID,
                 "adas_warp_run_device_matrices: bad argument (batch %d, handle holds %d)", batch, h ? h->max_batch : 0);
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    // the handle's own buffer is allocated here only outside a capture: adas_warp_device_view beforehand makes the run a plain launch
    if (!d_dst_bgr) {
        int rc = warp_own_buffer(h);
        if (rc) return rc;
    }
    return warp_launch(h, d_src_bgr, d_dst_bgr, d_M_warp, batch, (hipStream_t)stream);
}

int adas_warp_fetch(adas_warp* h, int frame, uint8_t* h_dst_bgr) {
    ADAS_REQUIRE(h && h_dst_bgr && frame >= 0 && frame < h->max_batch, ADAS_ERR_INVALID, "adas_warp_fetch: bad argument");
    ADAS_REQUIRE(h->dst_frames > 0, ADAS_ERR_INVALID, "adas_warp_fetch: no run has written the handle's own buffer (run with d_dst = NULL)");
    ADAS_REQUIRE(frame < h->dst_frames, ADAS_ERR_INVALID, "adas_warp_fetch: frame %d of the handle's own buffer was never written (largest batch run into it: %d)",
                 frame, h->dst_frames);
    ADAS_HIP_TRY(hipMemcpyAsync(h_dst_bgr, h->d_dst + (size_t)frame * h->frame_bytes(), h->frame_bytes(), hipMemcpyDeviceToHost, h->last));
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    return ADAS_OK;
}

int adas_warp_device_view(adas_warp* h, const uint8_t** d_dst_bgr) {
    ADAS_REQUIRE(h && d_dst_bgr, ADAS_ERR_INVALID, "adas_warp_device_view: bad argument");
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    int rc = warp_own_buffer(h);
    if (rc) return rc;
    *d_dst_bgr = h->d_dst;
    return ADAS_OK;
}

}  // extern "C"
