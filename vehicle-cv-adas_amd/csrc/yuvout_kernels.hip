// yuvout_kernels.hip -- BGR u8 frames on the device into uncompressed video formats (NV12, NV21, I420 / YV12, YUYV, UYVY): what an encoder
// other than MJPEG, `ffmpeg -f rawvideo -pix_fmt yuv420p`, a V4L2 loopback or a hardware encoder on another box takes.  The drawn frame leaves
// the device as 1.5 or 2 bytes per pixel instead of 3, a whole step's frames in one copy.  The rules and every byte address are
// yuvout_core.h (E1-E7); this file is one kernel around yuvout_item and the C ABI (adas_yuvout_*).
//   yuvout_kernel<FORMAT, MATRIX>   a lane per work item, frames along grid.y.  With yuvout_vector_ok (w, pitches, offsets, frame_stride and
//                                   both pointers multiples of 16: 1280x720 tight) an item is a 16-pixel group of a row unit: 16-byte loads,
//                                   16- and 8-byte stores only, neighbouring lanes on neighbouring 48 source bytes.  Otherwise an item is one
//                                   chroma sample's pixels with byte accesses: any pointer, any pitch, nothing written outside a plane row.
// Integer arithmetic only, no LDS, one plain launch without allocation or host synchronisation: adas_yuvout_run is capturable.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "yuvout_core.h"

using namespace adas;

static_assert(YUVOUT_CHROMA_MEAN == ADAS_YUVOUT_CHROMA_MEAN && YUVOUT_CHROMA_FIRST == ADAS_YUVOUT_CHROMA_FIRST, "yuvout_core.h restates ADAS_YUVOUT_*");
static_assert(sizeof(adas_yuvout_params) == 80 && sizeof(YuvOutParams) == 80 && offsetof(adas_yuvout_params, frame_stride) == 16 &&
                  offsetof(adas_yuvout_params, v_pitch) == 64 && offsetof(adas_yuvout_params, chroma) == 72 && offsetof(YuvOutParams, chroma) == 72 &&
                  offsetof(adas_yuvout_params, height) == offsetof(YuvGeom, h),
              "adas_yuvout_params is YuvOutParams and _lib.YuvOutParams");

namespace {

constexpr int YUVOUT_THREADS = 256;

template <int FORMAT, int MATRIX>
__global__ __launch_bounds__(YUVOUT_THREADS) void yuvout_kernel(YuvGeom g, int chroma, int vec, uint32_t items, const uint8_t* __restrict__ src,
                                                               uint8_t* __restrict__ dst) {
    const uint32_t t = blockIdx.x * (uint32_t)YUVOUT_THREADS + threadIdx.x;
    if (t >= items) return;
    yuvout_item<FORMAT, MATRIX>(g, chroma, vec != 0, src, dst, (int)blockIdx.y, t);
}

template <int FORMAT>
void yuvout_launch_m(const YuvGeom& g, int chroma, bool vec, uint32_t items, const uint8_t* src, uint8_t* dst, int batch, hipStream_t st) {
    const dim3 grid((items + YUVOUT_THREADS - 1) / YUVOUT_THREADS, (unsigned)batch), block(YUVOUT_THREADS);
    if (g.matrix == YUV_MATRIX_FULL)
        hipLaunchKernelGGL((yuvout_kernel<FORMAT, YUV_MATRIX_FULL>), grid, block, 0, st, g, chroma, (int)vec, items, src, dst);
    else
        hipLaunchKernelGGL((yuvout_kernel<FORMAT, YUV_MATRIX_VIDEO>), grid, block, 0, st, g, chroma, (int)vec, items, src, dst);
}

const char* yuvout_why(int code) {
    switch (code) {
        case YUV_BAD_FORMAT: return "unknown format";
        case YUV_BAD_MATRIX: return "unknown matrix";
        case YUV_BAD_SIZE: return "width and height must be in 1..65534";
        case YUV_ODD_WIDTH: return "odd width";
        case YUV_ODD_HEIGHT: return "odd height for a 4:2:0 format";
        case YUV_SHORT_PITCH: return "pitch shorter than a row";
        case YUV_OUTSIDE: return "plane outside the frame";
        case YUV_OVERLAP: return "planes overlap";
        case YUVOUT_BAD_CHROMA: return "unknown chroma mode";
    }
    return "";
}

YuvOutParams params_of(const adas_yuvout_params& p) {
    YuvOutParams q;
    static_assert(sizeof(q) == sizeof(p), "");
    memcpy(&q, &p, sizeof(q));
    return q;
}

}  // namespace

struct adas_yuvout {
    YuvGeom g;
    int chroma = 0;
    int max_batch = 0;
    long long src_bytes = 0;     // of one BGR frame
    long long extent = 0;        // bytes of a destination frame up to the end of its last plane
    size_t own_bytes = 0;        // of d_frames: (max_batch - 1) * frame_stride + extent
    uint8_t* d_frames = nullptr;
    hipStream_t last = nullptr;   // the stream of the last run: what the fetches drain
    int run_frames = 0;           // frames the last run converted ...
    bool run_own = false;         // ... into the handle's own buffer
};

void adas::yuvout_geometry_of(const adas_yuvout* h, int* width, int* height, int* max_batch) {
    *width = h ? h->g.w : 0;
    *height = h ? h->g.h : 0;
    *max_batch = h ? h->max_batch : 0;
}

extern "C" {

int adas_yuvout_default_params(adas_yuvout_params* p, int format, int width, int height) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_yuvout_default_params: null argument");
    ADAS_REQUIRE(format >= 0 && format < YUV_FORMATS, ADAS_ERR_INVALID, "adas_yuvout_default_params: unknown format %d", format);
    ADAS_REQUIRE(width >= 1 && height >= 1 && width <= YUV_MAX_DIM && height <= YUV_MAX_DIM, ADAS_ERR_INVALID,
                 "adas_yuvout_default_params: a %dx%d frame (%s)", width, height, yuvout_why(YUV_BAD_SIZE));
    YuvOutParams q;
    memset(&q, 0, sizeof(q));
    yuv_default(&q.g, format, width, height);
    q.chroma = YUVOUT_CHROMA_MEAN;
    memcpy(p, &q, sizeof(q));
    return ADAS_OK;
}

int64_t adas_yuvout_frame_bytes(const adas_yuvout_params* p) {
    if (!p) return 0;
    const YuvOutParams q = params_of(*p);
    return yuvout_check(q.g, q.chroma) == YUV_OK ? (int64_t)yuv_frame_extent(q.g) : 0;
}

int adas_yuvout_destroy(adas_yuvout* h) {
    if (!h) return ADAS_OK;
    if (h->d_frames) (void)hipFree(h->d_frames);
    delete h;
    return ADAS_OK;
}

int adas_yuvout_create(const adas_yuvout_params* p, int max_batch, adas_yuvout** out) {
    const char* who = "adas_yuvout_create";
    ADAS_REQUIRE(p && out, ADAS_ERR_INVALID, "%s: null argument", who);
    const YuvOutParams q = params_of(*p);
    const YuvGeom& g = q.g;
    const int why = yuvout_check(g, q.chroma);
    ADAS_REQUIRE(why == YUV_OK, ADAS_ERR_INVALID,
                 "%s: %s (format %d, %dx%d, chroma %d, frame_stride %lld, y %lld/%lld, u %lld/%lld, v %lld/%lld as offset/pitch)", who, yuvout_why(why),
                 g.format, g.w, g.h, q.chroma, (long long)g.frame_stride, (long long)g.y_offset, (long long)g.y_pitch, (long long)g.u_offset,
                 (long long)g.u_pitch, (long long)g.v_offset, (long long)g.v_pitch);
    ADAS_REQUIRE(max_batch >= 1 && max_batch <= 65535, ADAS_ERR_INVALID, "%s: max_batch %d (1..65535)", who, max_batch);
    adas_yuvout* h = new (std::nothrow) adas_yuvout();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->g = g;
    h->chroma = q.chroma;
    h->max_batch = max_batch;
    h->src_bytes = yuvout_src_bytes(g.w, g.h);
    h->extent = yuv_frame_extent(g);
    h->own_bytes = (size_t)(max_batch - 1) * (size_t)g.frame_stride + (size_t)h->extent;
    // the bytes no plane row owns are never written by a run: they stay the zeros of this memset
    hipError_t e = hipMalloc((void**)&h->d_frames, h->own_bytes);
    if (e == hipSuccess) e = hipMemset(h->d_frames, 0, h->own_bytes);
    if (e != hipSuccess) {
        adas_yuvout_destroy(h);
        return hip_fail(e, "hipMalloc(yuvout)", __FILE__, __LINE__);
    }
    *out = h;
    return ADAS_OK;
}

int adas_yuvout_run(adas_yuvout* h, const uint8_t* d_bgr, int batch, uint8_t* d_dst, void* stream) {
    ADAS_REQUIRE(h && d_bgr, ADAS_ERR_INVALID, "adas_yuvout_run: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_yuvout_run: batch %d, the handle holds %d frames", batch, h->max_batch);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* dst = d_dst ? d_dst : h->d_frames;
    const bool vec = yuvout_vector_ok(h->g, d_bgr, dst);
    const uint32_t items = (uint32_t)yuvout_items_per_frame(h->g, vec);
    h->last = st;
    h->run_frames = batch;
    h->run_own = d_dst == nullptr;
    switch (h->g.format) {
        case YUV_NV12: yuvout_launch_m<YUV_NV12>(h->g, h->chroma, vec, items, d_bgr, dst, batch, st); break;
        case YUV_NV21: yuvout_launch_m<YUV_NV21>(h->g, h->chroma, vec, items, d_bgr, dst, batch, st); break;
        case YUV_I420: yuvout_launch_m<YUV_I420>(h->g, h->chroma, vec, items, d_bgr, dst, batch, st); break;
        case YUV_YUYV: yuvout_launch_m<YUV_YUYV>(h->g, h->chroma, vec, items, d_bgr, dst, batch, st); break;
        default: yuvout_launch_m<YUV_UYVY>(h->g, h->chroma, vec, items, d_bgr, dst, batch, st); break;
    }
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

int adas_yuvout_fetch(adas_yuvout* h, int frame, uint8_t* h_dst) {
    ADAS_REQUIRE(h && h_dst, ADAS_ERR_INVALID, "adas_yuvout_fetch: null argument");
    ADAS_REQUIRE(h->run_own && frame >= 0 && frame < h->run_frames, ADAS_ERR_INVALID,
                 "adas_yuvout_fetch: frame %d was not written into the handle's buffer by the last run (%d frames)", frame, h->run_own ? h->run_frames : 0);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_dst, h->d_frames + (size_t)frame * (size_t)h->g.frame_stride, (size_t)h->extent, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_yuvout_fetch_all(adas_yuvout* h, int batch, uint8_t* h_dst) {
    ADAS_REQUIRE(h && h_dst, ADAS_ERR_INVALID, "adas_yuvout_fetch_all: null argument");
    ADAS_REQUIRE(h->run_own && batch >= 1 && batch <= h->run_frames, ADAS_ERR_INVALID,
                 "adas_yuvout_fetch_all: %d frames were not written into the handle's buffer by the last run (%d frames)", batch,
                 h->run_own ? h->run_frames : 0);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_dst, h->d_frames, (size_t)(batch - 1) * (size_t)h->g.frame_stride + (size_t)h->extent, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_yuvout_device_view(adas_yuvout* h, const uint8_t** d_frames) {
    ADAS_REQUIRE(h && d_frames, ADAS_ERR_INVALID, "adas_yuvout_device_view: null argument");
    *d_frames = h->d_frames;
    return ADAS_OK;
}

}  // extern "C"
