// scale_kernels.hip -- finished BGR u8 frames on the device reduced to previews and a stream mosaic: every frame of a step becomes a tile, the
// tiles share canvases, and a tile can carry its stream's collision state as a coloured border.  What a video wall, a low-rate preview
// recording or a thumbnail strip takes, without the full frames crossing the bus.  The rules and every byte address are scale_core.h (S1-S8);
// this file is the two kernels around its phases and items, and the C ABI (adas_scale_*).
//   scale_area_kernel    `area` with scale_vector_ok (the tile's row bytes and both pointers multiples of 16: 640x360, 320x180 and 160x90
//                        tiles): a workgroup per segment of a tile row, canvases along grid.y.  Each source row of the segment's span comes
//                        into LDS in 16-byte pieces, neighbouring lanes on neighbouring pieces, the next row's loads in flight under the
//                        current row's sums (two LDS rows, one barrier per source row); a lane sums its own pixel; the segment leaves in
//                        16-byte stores.
//   scale_kernel<MODE>   a lane per work item, canvases along grid.y.  `linear` with scale_vector_ok: an item is 16 consecutive bytes of a
//                        canvas row, byte loads of the taps and one 16-byte store.  Otherwise an item is one canvas pixel with byte
//                        accesses: any pointer, any size.
// Integer arithmetic in `area`, P5's fp32 / fp64 coefficient rule in `linear`, one plain launch without allocation or host synchronisation:
// adas_scale_run is capturable.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "scale_core.h"

using namespace adas;

static_assert(SCALE_MODE_AREA == ADAS_SCALE_AREA && SCALE_MODE_LINEAR == ADAS_SCALE_LINEAR, "scale_core.h restates ADAS_SCALE_*");
static_assert(sizeof(adas_scale_params) == 52 && sizeof(ScaleParams) == 52 && offsetof(adas_scale_params, mode) == 16 &&
                  offsetof(adas_scale_params, border) == 28 && offsetof(adas_scale_params, background) == 32 &&
                  offsetof(adas_scale_params, border_bgr) == 36 && offsetof(ScaleParams, border_bgr) == 36 && offsetof(ScaleParams, rows) == 24 &&
                  offsetof(adas_scale_params, rows) == 24,
              "adas_scale_params is ScaleParams and _lib.ScaleParams");

namespace {

constexpr int SCALE_THREADS = 256;

template <int MODE>
__global__ __launch_bounds__(SCALE_THREADS) void scale_kernel(ScaleParams p, int vec, int batch, uint32_t items, const uint8_t* __restrict__ src,
                                                             const uint8_t* __restrict__ state, long long state_stride, uint8_t* __restrict__ dst) {
    const uint32_t t = blockIdx.x * (uint32_t)SCALE_THREADS + threadIdx.x;
    if (t >= items) return;
    scale_item<MODE>(p, vec != 0, batch, src, state, state_stride, dst, (int)blockIdx.y, t);
}

// PIECES: the 16-byte pieces of a source row a lane loads at most, 1 (a row of up to 4 KB: the camera sizes) or SCALE_STAGE_PIECES
template <int PIECES>
__global__ __launch_bounds__(SCALE_BLOCK) void scale_area_kernel(ScaleParams p, ScaleStaged sg, int batch, const uint8_t* __restrict__ src,
                                                                 const uint8_t* __restrict__ state, long long state_stride, uint8_t* __restrict__ dst) {
    extern __shared__ uint4 scale_lds[];
    uint8_t* lds = (uint8_t*)scale_lds;
    uint8_t* lds_out = lds + 2 * sg.lds_row;
    const int tid = (int)threadIdx.x;
    const ScaleBlock B = scale_block(p, sg, batch, state, state_stride, (int)blockIdx.y, blockIdx.x);
    uint32_t acc[3] = {0, 0, 0};
    ScalePiece v[PIECES];
    if (B.y_lo < B.y_hi) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) v[i] = scale_stage_load(p, B, src, B.y_lo, tid, i);
#pragma unroll
        for (int i = 0; i < PIECES; ++i) scale_stage_write(sg, lds, tid, i, v[i]);
        __syncthreads();
    }
    for (int sy = B.y_lo; sy < B.y_hi; ++sy) {   // block-uniform bounds
        const int cur = (sy - B.y_lo) & 1;
        if (sy + 1 < B.y_hi) {
#pragma unroll
            for (int i = 0; i < PIECES; ++i) v[i] = scale_stage_load(p, B, src, sy + 1, tid, i);
        }
        scale_block_accumulate(p, B, lds + cur * sg.lds_row, sy, tid, acc);
        if (sy + 1 < B.y_hi) {
#pragma unroll
            for (int i = 0; i < PIECES; ++i) scale_stage_write(sg, lds + (cur ^ 1) * sg.lds_row, tid, i, v[i]);
        }
        __syncthreads();
    }
    scale_block_finish(p, B, lds_out, tid, acc);
    __syncthreads();
    scale_block_store(B, lds_out, dst, tid);
}

const char* scale_why(int code) {
    switch (code) {
        case SCALE_BAD_MODE: return "unknown mode";
        case SCALE_BAD_SIZE: return "source and tile sides must be in 1..16383";
        case SCALE_BAD_MOSAIC: return "mosaic columns and rows must be in 1..16383";
        case SCALE_ENLARGE: return "area does not enlarge";
        case SCALE_BIG_D: return "area needs src_w * src_h <= 8388608";
        case SCALE_BAD_BORDER: return "border must be >= 0 and 2 * border < min(dst_w, dst_h)";
        case SCALE_BIG_CANVAS: return "a canvas must stay below 2^31 bytes";
    }
    return "";
}

ScaleParams params_of(const adas_scale_params& p) {
    ScaleParams q;
    static_assert(sizeof(q) == sizeof(p), "");
    memcpy(&q, &p, sizeof(q));
    return q;
}

}  // namespace

struct adas_scale {
    ScaleParams p;
    int max_batch = 0;
    long long canvas_bytes = 0;
    size_t own_bytes = 0;         // of d_canvases: canvases(max_batch) * canvas_bytes
    uint8_t* d_canvases = nullptr;
    hipStream_t last = nullptr;   // the stream of the last run: what the fetches drain
    int run_canvases = 0;         // canvases the last run wrote ...
    bool run_own = false;         // ... into the handle's own buffer
};

void adas::scale_geometry_of(const adas_scale* h, int* src_w, int* src_h, int* canvas_w, int* canvas_h, int* tiles, int* max_batch, int* border) {
    *src_w = h ? h->p.src_w : 0;
    *src_h = h ? h->p.src_h : 0;
    *canvas_w = h ? h->p.cols * h->p.dst_w : 0;
    *canvas_h = h ? h->p.rows * h->p.dst_h : 0;
    *tiles = h ? h->p.cols * h->p.rows : 0;
    *max_batch = h ? h->max_batch : 0;
    *border = h ? h->p.border : 0;
}

extern "C" {

int adas_scale_default_params(adas_scale_params* p, int src_w, int src_h, int dst_w, int dst_h) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_scale_default_params: null argument");
    ScaleParams q;
    memset(&q, 0, sizeof(q));
    q.src_w = src_w; q.src_h = src_h; q.dst_w = dst_w; q.dst_h = dst_h;
    q.mode = SCALE_MODE_AREA;
    q.cols = q.rows = 1;
    // demo.py's ControlPanel.CollisionDict as BGR: UNKNOWN, NORMAL, PROMPT, WARNING
    const uint8_t col[4][3] = {{0, 255, 255}, {0, 255, 0}, {0, 102, 255}, {0, 0, 255}};
    for (int k = 0; k < 4; ++k) memcpy(q.border_bgr[k], col[k], 3);
    ADAS_REQUIRE(scale_check(q) != SCALE_BAD_SIZE, ADAS_ERR_INVALID, "adas_scale_default_params: %dx%d -> %dx%d (%s)", src_w, src_h, dst_w, dst_h,
                 scale_why(SCALE_BAD_SIZE));
    memcpy(p, &q, sizeof(q));
    return ADAS_OK;
}

int64_t adas_scale_canvas_bytes(const adas_scale_params* p) {
    if (!p) return 0;
    const ScaleParams q = params_of(*p);
    return scale_check(q) == SCALE_OK ? (int64_t)scale_canvas_bytes(q) : 0;
}

int adas_scale_canvases(const adas_scale_params* p, int batch) {
    if (!p || batch < 1) return 0;
    const ScaleParams q = params_of(*p);
    return scale_check(q) == SCALE_OK ? scale_canvases(q, batch) : 0;
}

int adas_scale_destroy(adas_scale* h) {
    if (!h) return ADAS_OK;
    if (h->d_canvases) (void)hipFree(h->d_canvases);
    delete h;
    return ADAS_OK;
}

int adas_scale_create(const adas_scale_params* p, int max_batch, adas_scale** out) {
    const char* who = "adas_scale_create";
    ADAS_REQUIRE(p && out, ADAS_ERR_INVALID, "%s: null argument", who);
    const ScaleParams q = params_of(*p);
    const int why = scale_check(q);
    ADAS_REQUIRE(why == SCALE_OK, ADAS_ERR_INVALID, "%s: %s (mode %d, %dx%d -> %dx%d, mosaic %dx%d, border %d)", who, scale_why(why), q.mode, q.src_w,
                 q.src_h, q.dst_w, q.dst_h, q.cols, q.rows, q.border);
    ADAS_REQUIRE(max_batch >= 1 && max_batch <= 65535, ADAS_ERR_INVALID, "%s: max_batch %d (1..65535)", who, max_batch);
    adas_scale* h = new (std::nothrow) adas_scale();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->p = q;
    h->max_batch = max_batch;
    h->canvas_bytes = scale_canvas_bytes(q);
    h->own_bytes = (size_t)scale_canvases(q, max_batch) * (size_t)h->canvas_bytes;
    hipError_t e = hipMalloc((void**)&h->d_canvases, h->own_bytes);
    if (e == hipSuccess) e = hipMemset(h->d_canvases, 0, h->own_bytes);
    if (e != hipSuccess) {
        adas_scale_destroy(h);
        return hip_fail(e, "hipMalloc(scale)", __FILE__, __LINE__);
    }
    *out = h;
    return ADAS_OK;
}

int adas_scale_run(adas_scale* h, const uint8_t* d_bgr, int batch, const void* d_state, int64_t state_stride, uint8_t* d_dst, void* stream) {
    ADAS_REQUIRE(h && d_bgr, ADAS_ERR_INVALID, "adas_scale_run: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_scale_run: batch %d, the handle holds %d frames", batch, h->max_batch);
    ADAS_REQUIRE(!d_state || h->p.border == 0 || ((uintptr_t)d_state % 4 == 0 && state_stride % 4 == 0), ADAS_ERR_INVALID,
                 "adas_scale_run: the states are int32: d_state and state_stride (%lld) must be multiples of 4", (long long)state_stride);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* dst = d_dst ? d_dst : h->d_canvases;
    ScaleStaged sg;
    const int path = scale_path(h->p, d_bgr, dst, &sg);
    const bool vec = path == SCALE_PATH_PIECES;
    const uint32_t items = scale_items_per_canvas(h->p, vec);
    const int canvases = scale_canvases(h->p, batch);
    h->last = st;
    h->run_canvases = canvases;
    h->run_own = d_dst == nullptr;
    const dim3 grid((items + SCALE_THREADS - 1) / SCALE_THREADS, (unsigned)canvases), block(SCALE_THREADS);
    const uint8_t* state = (const uint8_t*)d_state;
    if (path == SCALE_PATH_STAGED && sg.lds_row / 16 <= SCALE_BLOCK)
        hipLaunchKernelGGL(scale_area_kernel<1>, dim3(scale_staged_blocks_per_canvas(h->p, sg), (unsigned)canvases), dim3(SCALE_BLOCK),
                           (size_t)scale_staged_lds_bytes(sg), st, h->p, sg, batch, d_bgr, state, (long long)state_stride, dst);
    else if (path == SCALE_PATH_STAGED)
        hipLaunchKernelGGL(scale_area_kernel<SCALE_STAGE_PIECES>, dim3(scale_staged_blocks_per_canvas(h->p, sg), (unsigned)canvases), dim3(SCALE_BLOCK),
                           (size_t)scale_staged_lds_bytes(sg), st, h->p, sg, batch, d_bgr, state, (long long)state_stride, dst);
    else if (h->p.mode == SCALE_MODE_LINEAR)
        hipLaunchKernelGGL((scale_kernel<SCALE_MODE_LINEAR>), grid, block, 0, st, h->p, (int)vec, batch, items, d_bgr, state, (long long)state_stride, dst);
    else
        hipLaunchKernelGGL((scale_kernel<SCALE_MODE_AREA>), grid, block, 0, st, h->p, (int)vec, batch, items, d_bgr, state, (long long)state_stride, dst);
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

int adas_scale_fetch(adas_scale* h, int canvas, uint8_t* h_dst) {
    ADAS_REQUIRE(h && h_dst, ADAS_ERR_INVALID, "adas_scale_fetch: null argument");
    ADAS_REQUIRE(h->run_own && canvas >= 0 && canvas < h->run_canvases, ADAS_ERR_INVALID,
                 "adas_scale_fetch: canvas %d was not written into the handle's buffer by the last run (%d canvases)", canvas,
                 h->run_own ? h->run_canvases : 0);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_dst, h->d_canvases + (size_t)canvas * (size_t)h->canvas_bytes, (size_t)h->canvas_bytes, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_scale_fetch_all(adas_scale* h, int canvases, uint8_t* h_dst) {
    ADAS_REQUIRE(h && h_dst, ADAS_ERR_INVALID, "adas_scale_fetch_all: null argument");
    ADAS_REQUIRE(h->run_own && canvases >= 1 && canvases <= h->run_canvases, ADAS_ERR_INVALID,
                 "adas_scale_fetch_all: %d canvases were not written into the handle's buffer by the last run (%d canvases)", canvases,
                 h->run_own ? h->run_canvases : 0);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_dst, h->d_canvases, (size_t)canvases * (size_t)h->canvas_bytes, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_scale_device_view(adas_scale* h, const uint8_t** d_canvases) {
    ADAS_REQUIRE(h && d_canvases, ADAS_ERR_INVALID, "adas_scale_device_view: null argument");
    *d_canvases = h->d_canvases;
    return ADAS_OK;
}

}  // extern "C"
