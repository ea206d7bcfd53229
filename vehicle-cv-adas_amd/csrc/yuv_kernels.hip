// yuv_kernels.hip -- uncompressed camera formats (NV12, NV21, I420 / YV12, YUYV, UYVY) into BGR u8 frames on the device, where
// adas_pipeline_step_frames reads them: what a UVC camera, an ISP, a hardware video decoder or `ffmpeg -pix_fmt nv12` delivers crosses the bus
// as 1.5 or 2 bytes per pixel instead of 3 and is converted in front of the step.  The rules and every byte address are yuv_core.h (C1-C7);
// this file is one kernel around yuv_item and the C ABI (adas_yuv_*).
//   yuv_kernel<FORMAT, MATRIX>   a lane per work item, frames along grid.y.  With yuv_vector_ok (w, pitches, offsets, frame_stride and both
//                                pointers multiples of 16: 1280x720 tight, every decoder surface) an item is a 16-pixel group of a row unit:
//                                16-byte loads and stores only, neighbouring lanes on neighbouring 16 source bytes.  Otherwise an item is one
//                                chroma sample's pixels with byte accesses: any pointer, any pitch, nothing read behind a row or a plane.
// Integer arithmetic only, no LDS, one plain launch without allocation or host synchronisation: adas_yuv_run is capturable.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "yuv_core.h"

using namespace adas;

static_assert(YUV_NV12 == ADAS_YUV_NV12 && YUV_NV21 == ADAS_YUV_NV21 && YUV_I420 == ADAS_YUV_I420 && YUV_YUYV == ADAS_YUV_YUYV &&
                  YUV_UYVY == ADAS_YUV_UYVY && YUV_MATRIX_VIDEO == ADAS_YUV_MATRIX_VIDEO && YUV_MATRIX_FULL == ADAS_YUV_MATRIX_FULL,
              "yuv_core.h restates ADAS_YUV_*");
static_assert(sizeof(adas_yuv_params) == 72 && sizeof(YuvGeom) == 72 && offsetof(adas_yuv_params, frame_stride) == 16 &&
                  offsetof(YuvGeom, frame_stride) == 16 && offsetof(adas_yuv_params, v_pitch) == 64 && offsetof(YuvGeom, v_pitch) == 64 &&
                  offsetof(adas_yuv_params, height) == offsetof(YuvGeom, h),
              "adas_yuv_params is YuvGeom and _lib.YuvParams");

namespace {

constexpr int YUV_THREADS = 256;

template <int FORMAT, int MATRIX>
__global__ __launch_bounds__(YUV_THREADS) void yuv_kernel(YuvGeom g, int vec, uint32_t items, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
    const uint32_t t = blockIdx.x * (uint32_t)YUV_THREADS + threadIdx.x;
    if (t >= items) return;
    yuv_item<FORMAT, MATRIX>(g, vec != 0, src, dst, (int)blockIdx.y, t);
}

template <int FORMAT>
void yuv_launch_m(const YuvGeom& g, bool vec, uint32_t items, const uint8_t* src, uint8_t* dst, int batch, hipStream_t st) {
    const dim3 grid((items + YUV_THREADS - 1) / YUV_THREADS, (unsigned)batch), block(YUV_THREADS);
    if (g.matrix == YUV_MATRIX_FULL)
        hipLaunchKernelGGL((yuv_kernel<FORMAT, YUV_MATRIX_FULL>), grid, block, 0, st, g, (int)vec, items, src, dst);
    else
        hipLaunchKernelGGL((yuv_kernel<FORMAT, YUV_MATRIX_VIDEO>), grid, block, 0, st, g, (int)vec, items, src, dst);
}

const char* yuv_why(int code) {
    switch (code) {
        case YUV_BAD_FORMAT: return "unknown format";
        case YUV_BAD_MATRIX: return "unknown matrix";
        case YUV_BAD_SIZE: return "width and height must be in 1..65534";
        case YUV_ODD_WIDTH: return "odd width";
        case YUV_ODD_HEIGHT: return "odd height for a 4:2:0 format";
        case YUV_SHORT_PITCH: return "pitch shorter than a row";
        case YUV_OUTSIDE: return "plane outside the frame";
        case YUV_OVERLAP: return "planes overlap";
    }
    return "";
}

YuvGeom geom_of(const adas_yuv_params& p) {
    YuvGeom g;
    static_assert(sizeof(g) == sizeof(p), "");
    memcpy(&g, &p, sizeof(g));
    return g;
}

}  // namespace

struct adas_yuv {
    YuvGeom g;
    int max_batch = 0;
    long long out_bytes = 0;     // of one BGR frame
    long long extent = 0;        // bytes of a source frame that are read
    uint8_t* d_frames = nullptr;
    // adas_yuv_run_host: two device buffers for the raw frames; ev_ran[k]: the conversion that last read buffer k is done
    uint8_t* d_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_ran[2] = {nullptr, nullptr};
    bool ran[2] = {false, false};
    unsigned long long stage_next = 0;
    hipStream_t last = nullptr;   // the stream of the last run: what the fetches drain
    int run_frames = 0;           // frames the last run converted ...
    bool run_own = false;         // ... into the handle's own buffer
};

void adas::yuv_geometry_of(const adas_yuv* h, int* width, int* height, int* max_batch, long long* src_bytes) {
    *width = h ? h->g.w : 0;
    *height = h ? h->g.h : 0;
    *max_batch = h ? h->max_batch : 0;
    *src_bytes = h ? h->g.frame_stride : 0;
}

uint8_t* adas::yuv_frames(adas_yuv* h) { return h ? h->d_frames : nullptr; }

long long adas::yuv_extent_of(const adas_yuv* h) { return h ? h->extent : 0; }

static int yuv_launch(adas_yuv* h, const uint8_t* d_src, int batch, uint8_t* d_dst, hipStream_t st) {
    uint8_t* dst = d_dst ? d_dst : h->d_frames;
    const bool vec = yuv_vector_ok(h->g, d_src, dst);
    const uint32_t items = (uint32_t)yuv_items_per_frame(h->g, vec);
    h->last = st;
    h->run_frames = batch;
    h->run_own = d_dst == nullptr;
    switch (h->g.format) {
        case YUV_NV12: yuv_launch_m<YUV_NV12>(h->g, vec, items, d_src, dst, batch, st); break;
        case YUV_NV21: yuv_launch_m<YUV_NV21>(h->g, vec, items, d_src, dst, batch, st); break;
        case YUV_I420: yuv_launch_m<YUV_I420>(h->g, vec, items, d_src, dst, batch, st); break;
        case YUV_YUYV: yuv_launch_m<YUV_YUYV>(h->g, vec, items, d_src, dst, batch, st); break;
        default: yuv_launch_m<YUV_UYVY>(h->g, vec, items, d_src, dst, batch, st); break;
    }
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

extern "C" {

int adas_yuv_default_params(adas_yuv_params* p, int format, int width, int height) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_yuv_default_params: null argument");
    ADAS_REQUIRE(format >= 0 && format < YUV_FORMATS, ADAS_ERR_INVALID, "adas_yuv_default_params: unknown format %d", format);
    ADAS_REQUIRE(width >= 1 && height >= 1 && width <= YUV_MAX_DIM && height <= YUV_MAX_DIM, ADAS_ERR_INVALID,
                 "adas_yuv_default_params: a %dx%d frame (%s)", width, height, yuv_why(YUV_BAD_SIZE));
    YuvGeom g;
    yuv_default(&g, format, width, height);
    memcpy(p, &g, sizeof(g));
    return ADAS_OK;
}

int64_t adas_yuv_frame_bytes(const adas_yuv_params* p) {
    if (!p) return 0;
    const YuvGeom g = geom_of(*p);
    return yuv_check(g) == YUV_OK ? (int64_t)yuv_frame_extent(g) : 0;
}

int adas_yuv_destroy(adas_yuv* h) {
    if (!h) return ADAS_OK;
    for (void* q : {(void*)h->d_frames, (void*)h->d_stage[0], (void*)h->d_stage[1]})
        if (q) (void)hipFree(q);
    for (int k = 0; k < 2; ++k)
        if (h->ev_ran[k]) (void)hipEventDestroy(h->ev_ran[k]);
    delete h;
    return ADAS_OK;
}

int adas_yuv_create(const adas_yuv_params* p, int max_batch, adas_yuv** out) {
    const char* who = "adas_yuv_create";
    ADAS_REQUIRE(p && out, ADAS_ERR_INVALID, "%s: null argument", who);
    const YuvGeom g = geom_of(*p);
    const int why = yuv_check(g);
    ADAS_REQUIRE(why == YUV_OK, ADAS_ERR_INVALID,
                 "%s: %s (format %d, %dx%d, frame_stride %lld, y %lld/%lld, u %lld/%lld, v %lld/%lld as offset/pitch)", who, yuv_why(why), g.format, g.w,
                 g.h, (long long)g.frame_stride, (long long)g.y_offset, (long long)g.y_pitch, (long long)g.u_offset, (long long)g.u_pitch,
                 (long long)g.v_offset, (long long)g.v_pitch);
    ADAS_REQUIRE(max_batch >= 1 && max_batch <= 65535, ADAS_ERR_INVALID, "%s: max_batch %d (1..65535)", who, max_batch);
    adas_yuv* h = new (std::nothrow) adas_yuv();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->g = g;
    h->max_batch = max_batch;
    h->out_bytes = yuv_out_bytes(g.w, g.h);
    h->extent = yuv_frame_extent(g);
    hipError_t e = hipMalloc((void**)&h->d_frames, (size_t)max_batch * (size_t)h->out_bytes);
    if (e == hipSuccess) e = hipMemset(h->d_frames, 0, (size_t)max_batch * (size_t)h->out_bytes);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&h->ev_ran[k], hipEventDisableTiming);
    if (e != hipSuccess) {
        adas_yuv_destroy(h);
        return hip_fail(e, "hipMalloc(yuv)", __FILE__, __LINE__);
    }
    *out = h;
    return ADAS_OK;
}

int adas_yuv_run(adas_yuv* h, const uint8_t* d_src, int batch, uint8_t* d_dst_bgr, void* stream) {
    ADAS_REQUIRE(h && d_src, ADAS_ERR_INVALID, "adas_yuv_run: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_yuv_run: batch %d, the handle holds %d frames", batch, h->max_batch);
    return yuv_launch(h, d_src, batch, d_dst_bgr, (hipStream_t)stream);
}

int adas_yuv_run_host(adas_yuv* h, const uint8_t* h_src, int batch, uint8_t* d_dst_bgr, void* stream) {
    ADAS_REQUIRE(h && h_src, ADAS_ERR_INVALID, "adas_yuv_run_host: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_yuv_run_host: batch %d, the handle holds %d frames", batch, h->max_batch);
    const int k = (int)(h->stage_next & 1);
    if (!h->d_stage[k]) ADAS_HIP_TRY(hipMalloc((void**)&h->d_stage[k], (size_t)h->max_batch * (size_t)h->g.frame_stride));
    // the conversion that last read this buffer may have been queued on another stream: the copy waits for it
    if (h->ran[k]) ADAS_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, h->ev_ran[k], 0));
    const size_t bytes = (size_t)(batch - 1) * (size_t)h->g.frame_stride + (size_t)h->extent;
    ADAS_HIP_TRY(hipMemcpyAsync(h->d_stage[k], h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    ++h->stage_next;
    int rc = yuv_launch(h, h->d_stage[k], batch, d_dst_bgr, (hipStream_t)stream);
    if (rc) return rc;
    ADAS_HIP_TRY(hipEventRecord(h->ev_ran[k], (hipStream_t)stream));
    h->ran[k] = true;
    return ADAS_OK;
}

int adas_yuv_fetch(adas_yuv* h, int frame, uint8_t* h_bgr) {
    ADAS_REQUIRE(h && h_bgr, ADAS_ERR_INVALID, "adas_yuv_fetch: null argument");
    ADAS_REQUIRE(h->run_own && frame >= 0 && frame < h->run_frames, ADAS_ERR_INVALID,
                 "adas_yuv_fetch: frame %d was not written into the handle's buffer by the last run (%d frames)", frame, h->run_own ? h->run_frames : 0);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_bgr, h->d_frames + (size_t)frame * h->out_bytes, (size_t)h->out_bytes, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_yuv_device_view(adas_yuv* h, const uint8_t** d_frames_bgr) {
    ADAS_REQUIRE(h && d_frames_bgr, ADAS_ERR_INVALID, "adas_yuv_device_view: null argument");
    *d_frames_bgr = h->d_frames;
    return ADAS_OK;
}

}  // extern "C"
