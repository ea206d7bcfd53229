// jpegdec_kernels.hip -- baseline JPEG decoding on the device: compressed camera frames in (a few hundred KB each instead of width x height x 3
// bytes over the bus), BGR u8 frames out where adas_pipeline_step_frames reads them.  The rules are jpegdec_core.h (D1-D9); this file is the
// five kernels around them and the C ABI (adas_jpegdec_*).  A restart segment is the unit of independence.  A run is a memset of the
// coefficient arena and
//   jpegdec_header_kernel     one wave per frame, its first lane walks the markers (jd_parse_header) and writes the frame's record: flags,
//                             sampling, DRI, the scan's start, the quantisation tables and the four Huffman tables in decode form (about 4 KB
//                             per frame).
//   jpegdec_segment_kernel    one workgroup per frame walks the scan once and finds its end and its restart markers: every lane tests 16-byte
//                             pieces (and looks one byte past a piece's end), a workgroup scan puts the hits in order into the table of
//                             segment starts and ends, D3's marker order and count are checked, and the first lane steps over the marker
//                             segments behind the scan's end looking for a second SOS (D2).
//   jpegdec_entropy_kernel    one wave per segment, the frame's record in LDS, its first lane decodes: jd_decode_segment with a 64-bit bit
//                             buffer fed through aligned words, dequantised int16 coefficients [block][64] into the arena.  The walk is serial
//                             and data-dependent; the kernel is latency-bound and takes 95 % of a run.  Without restart markers a frame is
//                             one lane.
//   jpegdec_transform_kernel  eight lanes per block: lane r transforms row r, the rows meet in LDS, lane r transforms column r, the samples meet
//                             in LDS and lane r stores row r (8 bytes) into the component's plane, at component resolution.
//   jpegdec_colour_kernel     a lane per 16 destination bytes: chroma upsampling and colour conversion (jd_pixel) into BGR, one 16-byte store;
//                             the destination may start on any byte, the pieces in front of the first and behind the last 16-byte boundary
//                             go byte by byte.  Rejected frames get zeros.  Lane 0 of a frame publishes its flags.
// Plain launches without allocation or host synchronisation: adas_jpegdec_run is capturable.  The streams may start on any byte and lie at any
// stride; they are read through aligned words that each hold at least one of their bytes (jd_get).
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "jpegdec_core.h"

using namespace adas;

static_assert(JPEGDEC_UNSUPPORTED == ADAS_JPEGDEC_UNSUPPORTED && JPEGDEC_FORMAT == ADAS_JPEGDEC_FORMAT && JPEGDEC_SIZE == ADAS_JPEGDEC_SIZE &&
                  JPEGDEC_CORRUPT == ADAS_JPEGDEC_CORRUPT,
              "jpegdec_core.h restates ADAS_JPEGDEC_*");
static_assert(sizeof(adas_jpegdec_params) == 24 && offsetof(adas_jpegdec_params, capacity) == 16, "adas_jpegdec_params is _lib.JpegDecParams");
static_assert(sizeof(JdFrame) % 4 == 0, "the record is copied as words");

namespace {

constexpr int JD_THREADS = 256;
constexpr int JD_BLOCKS = JD_THREADS / 8;   // blocks of a transform workgroup
constexpr int JD_PIECE = 16;                // bytes a lane of the segment search tests at a time
constexpr int JD_WAVE = 64;
constexpr int JD_SEG_THREADS = 1024;         // lanes of the segment search
constexpr int JD_SEG_WAVES = 128;             // entropy workgroups (one wave each) per frame

struct JdArgs {
    int w, h, batch;
    long long capacity, cap_blocks, cap_segs;
    const uint8_t* streams;
    const int64_t* lengths;     // [batch]
    const int64_t* offsets;     // [batch] from streams, or null: frame f at f * stride
    long long stride;
    JdFrame* rec;               // [batch]
    int32_t* seg;               // [batch][cap_segs][2]
    int16_t* coef;              // [batch][cap_blocks][64]
    uint8_t* planes;            // [batch][cap_blocks * 64]
    uint8_t* dst;               // [batch][h][w][3], any alignment
    int32_t* flags;             // [batch]
};

__device__ __forceinline__ JdSrc jd_stream(const JdArgs& a, int f, long long* length) {
    const long long len = a.lengths[f];
    *length = len;
    const bool ok = len > 0 && len <= a.capacity;
    return jd_src(a.streams + (a.offsets ? a.offsets[f] : (long long)f * a.stride), ok ? len : 0);
}

// one wave per frame, its first lane walks the header: 64 frames in the lanes of one wave would each wait for the other 63's branches
__global__ __launch_bounds__(JD_WAVE) void jpegdec_header_kernel(const JdArgs a) {
    const int f = blockIdx.x;
    if (threadIdx.x != 0) return;
    long long len;
    JdSrc s = jd_stream(a, f, &len);
    jd_parse_header(s, len, a.capacity, a.w, a.h, &a.rec[f]);
}

// exclusive scan of v over the segment search's JD_SEG_THREADS lanes; *total: the sum.  sh: one word of LDS per wave, free again on return
__device__ __forceinline__ int jd_scan(int v, int* sh, int t, int* total) {
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if ((t & 63) >= d) x += y;
    }
    if ((t & 63) == 63) sh[t >> 6] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < JD_SEG_THREADS / 64; ++w) {
        const int s = sh[w];
        if (w < (t >> 6)) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// The scan is walked once, JD_SEG_THREADS pieces of 16 bytes at a time: a lane loads its piece and the byte behind it as five aligned words
// (each holds a byte of the stream, or is not read), notes the restart markers that start in the piece and the first other marker; the
// workgroup takes the smallest of the latter (the scan's end, then the walk stops), drops the restart markers behind it and puts the rest in
// order with a scan of their counts.  Gives jd_find_segments' table, count, end and flag.
__global__ __launch_bounds__(JD_SEG_THREADS) void jpegdec_segment_kernel(const JdArgs a) {
    __shared__ int s_end, s_bad;
    __shared__ int sh[JD_SEG_THREADS / 64];
    const int t = threadIdx.x, f = blockIdx.x;
    JdFrame* F = &a.rec[f];
    if (F->flags & JPEGDEC_REJECT) return;
    long long len;
    const JdSrc s = jd_stream(a, f, &len);
    const int start = F->scan_start, n = (int)s.n;
    const long long last_word = ((long long)n - 1 + s.a) >> 2;
    if (t == 0) {
        s_end = 0x7fffffff;
        s_bad = 0;
    }
    __syncthreads();
    int32_t* seg = a.seg + (size_t)f * a.cap_segs * 2;
    int r0 = 0, bad = 0, end = n;
    for (long long chunk = start; chunk < n; chunk += JD_SEG_THREADS * JD_PIECE) {
        const long long base = chunk + (long long)t * JD_PIECE;
        int cnt = 0, at[JD_PIECE / 2], code[JD_PIECE / 2];
        if (base < n) {
            const long long j0 = base + s.a, w0 = j0 >> 2;
            const int sh8 = (int)(j0 & 3) * 8;
            uint32_t w[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) w[i] = w0 + i <= last_word ? s.q[w0 + i] : 0u;
            uint32_t v[5];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = sh8 ? (w[i] >> sh8) | (w[i + 1] << (32 - sh8)) : w[i];
            v[4] = w[4] >> sh8;
            int other = 0x7fffffff;
#pragma unroll
            for (int k = JD_PIECE - 1; k >= 0; --k) {
                const long long i = base + k;
                const uint32_t b0 = (v[k >> 2] >> ((k & 3) * 8)) & 255u, b1 = (v[(k + 1) >> 2] >> (((k + 1) & 3) * 8)) & 255u;
                if (b0 == 0xFFu && i + 1 < n && b1 != 0u && b1 != 0xFFu && !(b1 >= 0xD0u && b1 <= 0xD7u)) other = (int)i;
            }
            if (other != 0x7fffffff) atomicMin(&s_end, other);
#pragma unroll
            for (int k = 0; k < JD_PIECE; ++k) {
                const long long i = base + k;
                const uint32_t b0 = (v[k >> 2] >> ((k & 3) * 8)) & 255u, b1 = (v[(k + 1) >> 2] >> (((k + 1) & 3) * 8)) & 255u;
                if (b0 == 0xFFu && i + 1 < n && b1 >= 0xD0u && b1 <= 0xD7u && i < other && cnt < JD_PIECE / 2) {
                    at[cnt] = (int)i;
                    code[cnt++] = (int)(b1 & 7u);
                }
            }
        }
        __syncthreads();
        const int e = s_end;
        int keep = 0;
        for (int j = 0; j < cnt; ++j) keep += at[j] < e;      // in order: the kept ones come first
        int total = 0;
        const int first = r0 + jd_scan(keep, sh, t, &total);
        for (int j = 0; j < keep; ++j) {
            const int r = first + j;
            if (code[j] != (r & 7)) bad = 1;
            if (r < a.cap_segs) seg[2 * r + 1] = at[j];
            if (r + 1 < a.cap_segs) seg[2 * (r + 1)] = at[j] + 2;
        }
        r0 += total;
        if (e != 0x7fffffff) {
            end = e;
            break;
        }
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (t == 0) {
        seg[0] = start;
        if (r0 < a.cap_segs) seg[2 * r0 + 1] = end;
        JdSrc tail = s;
        jd_finish_segments(tail, F, end, r0 + 1, s_bad);
    }
}

// One wave per segment and only its first lane decodes: the walk is serial and data-dependent, so segments that share a wave would each wait
// for the others' branches, while a wave of its own costs a segment nothing.  The wave's lanes bring the frame's record into LDS together.  A
// frame has JD_SEG_WAVES workgroups; one with more segments than that gives each several.
__global__ __launch_bounds__(JD_WAVE) void jpegdec_entropy_kernel(const JdArgs a) {
    __shared__ JdFrame F;
    __shared__ uint8_t zz[64];
    const int t = threadIdx.x, f = blockIdx.y;
    const JdFrame* G = &a.rec[f];
    if (G->flags & JPEGDEC_REJECT) return;
    long long ndec = G->found < G->nseg ? G->found : G->nseg;
    if (ndec > a.cap_segs) ndec = a.cap_segs;
    if ((long long)blockIdx.x >= ndec) return;
    for (unsigned i = t; i < sizeof(JdFrame) / 4; i += JD_WAVE) ((uint32_t*)&F)[i] = ((const uint32_t*)G)[i];
    zz[t] = (uint8_t)jpeg_zigzag(t);
    __syncthreads();
    if (t != 0) return;
    long long len;
    JdSrc s = jd_stream(a, f, &len);
    bool ok = true;
    for (long long k = blockIdx.x; k < ndec; k += gridDim.x)
        ok &= jd_decode_segment(s, &F, zz, a.seg + (size_t)f * a.cap_segs * 2, (int)k, a.coef + (size_t)f * a.cap_blocks * 64);
    if (!ok) atomicOr(&a.rec[f].flags, JPEGDEC_CORRUPT);
}

__global__ __launch_bounds__(JD_THREADS) void jpegdec_transform_kernel(const JdArgs a) {
    __shared__ int T[JD_BLOCKS][8][9];
    __shared__ alignas(8) uint8_t px[JD_BLOCKS][8][8];
    const int t = threadIdx.x, f = blockIdx.y;
    const JdFrame* F = &a.rec[f];
    if (F->flags & JPEGDEC_REJECT) return;
    const long long nblk = jd_frame_blocks(F);
    if ((long long)blockIdx.x * JD_BLOCKS >= nblk) return;
    const int lb = t >> 3, r = t & 7;
    const long long blk = (long long)blockIdx.x * JD_BLOCKS + lb;
    const bool live = blk < nblk;
    int v[8];
    if (live) {
        const uint4 q = *(const uint4*)(a.coef + ((size_t)f * a.cap_blocks + blk) * 64 + r * 8);
        v[0] = (int16_t)(q.x & 0xffffu); v[1] = (int16_t)(q.x >> 16);
        v[2] = (int16_t)(q.y & 0xffffu); v[3] = (int16_t)(q.y >> 16);
        v[4] = (int16_t)(q.z & 0xffffu); v[5] = (int16_t)(q.z >> 16);
        v[6] = (int16_t)(q.w & 0xffffu); v[7] = (int16_t)(q.w >> 16);
        jd_idct_pass(v, 1, JPEGDEC_PASS1_ROUND, JPEGDEC_PASS1_SHIFT);
#pragma unroll
        for (int x = 0; x < 8; ++x) T[lb][r][x] = v[x];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int y = 0; y < 8; ++y) v[y] = T[lb][y][r];
        jd_idct_pass(v, 1, JPEGDEC_PASS2_ROUND, JPEGDEC_PASS2_SHIFT);
#pragma unroll
        for (int y = 0; y < 8; ++y) px[lb][y][r] = (uint8_t)jd_sample(v[y]);
    }
    __syncthreads();
    if (!live) return;
    const JdComp C1 = jd_comp(F, 1), C2 = jd_comp(F, 2);
    const JdComp C = F->ncomp == 1 || blk < C1.off ? jd_comp(F, 0) : (blk < C2.off ? C1 : C2);
    const long long local = blk - C.off;
    const int by = (int)(local / C.bw), bx = (int)(local % C.bw);
    uint8_t* dst = a.planes + (size_t)f * a.cap_blocks * 64 + (size_t)C.off * 64 + ((size_t)by * 8 + r) * ((size_t)C.bw * 8) + (size_t)bx * 8;
    *(uint2*)dst = *(const uint2*)&px[lb][r][0];
}

__global__ __launch_bounds__(JD_THREADS) void jpegdec_colour_kernel(const JdArgs a) {
    const int f = blockIdx.y;
    const long long p = (long long)blockIdx.x * JD_THREADS + threadIdx.x;
    const JdFrame* F = &a.rec[f];
    const int flags = F->flags;
    if (p == 0) a.flags[f] = flags;
    const long long fsz = (long long)a.w * a.h * 3;
    uint8_t* dst = a.dst + (size_t)f * fsz;
    long long head = (long long)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > fsz) head = fsz;
    const long long lo = p == 0 ? 0 : head + 16 * (p - 1);
    long long hi = p == 0 ? head : lo + 16;
    if (hi > fsz) hi = fsz;
    if (lo >= hi) return;
    alignas(16) uint8_t out[16];
    const int cnt = (int)(hi - lo);
    if (flags & JPEGDEC_REJECT) {
        for (int j = 0; j < 16; ++j) out[j] = 0;
    } else {
        const uint8_t* planes = a.planes + (size_t)f * a.cap_blocks * 64;
        const long long pix = lo / 3;
        int ch = (int)(lo % 3), x = (int)(pix % a.w), y = (int)(pix / a.w);
        int bgr[3];
        jd_pixel(F, planes, a.w, a.h, x, y, bgr);
        for (int j = 0; j < cnt; ++j) {
            out[j] = (uint8_t)bgr[ch];
            if (++ch == 3 && j + 1 < cnt) {
                ch = 0;
                if (++x == a.w) {
                    x = 0;
                    ++y;
                }
                jd_pixel(F, planes, a.w, a.h, x, y, bgr);
            }
        }
    }
    if (cnt == 16 && p > 0) {
        *(uint4*)(dst + lo) = *(const uint4*)out;
    } else {
        for (int j = 0; j < cnt; ++j) dst[lo + j] = out[j];
    }
}

}  // namespace

struct adas_jpegdec {
    adas_jpegdec_params p;
    int max_batch = 0;
    long long cap_blocks = 0, cap_segs = 0, frame_bytes = 0;
    JdFrame* d_rec = nullptr;
    int32_t* d_seg = nullptr;
    int16_t* d_coef = nullptr;
    uint8_t* d_planes = nullptr;
    uint8_t* d_frames = nullptr;
    int32_t* d_flags = nullptr;
    // streams from the host: two slots of [lengths int64 [max_batch]][offsets int64 [max_batch]][the streams, each from a multiple of 4], pinned
    // on the host and mirrored on the device; ev_staged[k]: the copy out of the pinned slot k is done
    uint8_t* h_stage[2] = {nullptr, nullptr};
    uint8_t* d_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_staged[2] = {nullptr, nullptr};
    bool staged[2] = {false, false};
    hipEvent_t ev_ran[2] = {nullptr, nullptr};      // adas_jpegdec_run_host: the run that read device slot k is done
    bool ran[2] = {false, false};
    unsigned long long stage_next = 0;
    size_t stage_bytes = 0;
    hipStream_t last = nullptr;   // the stream of the last run: what the fetches drain
    int run_frames = 0;           // frames the last run decoded ...
    bool run_own = false;         // ... into the handle's own buffer
};

void adas::jpegdec_geometry_of(const adas_jpegdec* h, int* width, int* height, int* max_batch) {
    *width = h ? h->p.width : 0;
    *height = h ? h->p.height : 0;
    *max_batch = h ? h->max_batch : 0;
}

uint8_t* adas::jpegdec_frames(adas_jpegdec* h) { return h ? h->d_frames : nullptr; }

int adas::jpegdec_next_slot(const adas_jpegdec* h) { return h ? (int)(h->stage_next & 1) : 0; }

static int jpegdec_launch(adas_jpegdec* h, const uint8_t* d_streams, const int64_t* d_lengths, const int64_t* d_offsets, long long stride, int batch,
                          uint8_t* d_dst, hipStream_t st) {
    JdArgs a = {};
    a.w = h->p.width; a.h = h->p.height; a.batch = batch;
    a.capacity = h->p.capacity; a.cap_blocks = h->cap_blocks; a.cap_segs = h->cap_segs;
    a.streams = d_streams; a.lengths = d_lengths; a.offsets = d_offsets; a.stride = stride;
    a.rec = h->d_rec; a.seg = h->d_seg; a.coef = h->d_coef; a.planes = h->d_planes;
    a.dst = d_dst ? d_dst : h->d_frames;
    a.flags = h->d_flags;
    h->last = st;
    h->run_frames = batch;
    h->run_own = d_dst == nullptr;
    ADAS_HIP_TRY(hipMemsetAsync(h->d_coef, 0, (size_t)batch * h->cap_blocks * 64 * sizeof(int16_t), st));   // D4: what no code reaches is zero
    hipLaunchKernelGGL(jpegdec_header_kernel, dim3((unsigned)batch), dim3(JD_WAVE), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_segment_kernel, dim3((unsigned)batch), dim3(JD_SEG_THREADS), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3((unsigned)(h->cap_segs < JD_SEG_WAVES ? h->cap_segs : JD_SEG_WAVES), (unsigned)batch), dim3(JD_WAVE), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_transform_kernel, dim3((unsigned)((h->cap_blocks + JD_BLOCKS - 1) / JD_BLOCKS), (unsigned)batch), dim3(JD_THREADS), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    const long long pieces = h->frame_bytes / 16 + 2;
    hipLaunchKernelGGL(jpegdec_colour_kernel, dim3((unsigned)((pieces + JD_THREADS - 1) / JD_THREADS), (unsigned)batch), dim3(JD_THREADS), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

// Packs `batch` host streams into the next staging slot and queues its copy on copy_stream; *slot: which.  A length above the capacity (or
// below 1) travels as a length alone: nothing of that stream is copied, the header kernel flags it.
int adas::jpegdec_stage_host(adas_jpegdec* h, const uint8_t* const* h_streams, const int64_t* h_lengths, int batch, void* copy_stream, int* slot) {
    const char* who = "adas_jpegdec_run_host";
    ADAS_REQUIRE(h && h_streams && h_lengths && slot, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "%s: batch %d, the handle holds %d frames", who, batch, h->max_batch);
    for (int f = 0; f < batch; ++f)
        ADAS_REQUIRE(h_streams[f] || h_lengths[f] <= 0 || h_lengths[f] > h->p.capacity, ADAS_ERR_INVALID, "%s: stream %d is null", who, f);
    const size_t table = (size_t)h->max_batch * 16;
    const int k = (int)(h->stage_next & 1);
    if (h->staged[k]) ADAS_HIP_TRY(hipEventSynchronize(h->ev_staged[k]));   // the copy two calls back has left the pinned slot
    int64_t* len = (int64_t*)h->h_stage[k];
    int64_t* off = len + h->max_batch;
    size_t at = 0;
    for (int f = 0; f < batch; ++f) {
        const bool ok = h_lengths[f] > 0 && h_lengths[f] <= h->p.capacity;
        len[f] = h_lengths[f];
        off[f] = (int64_t)at;
        if (ok) {
            memcpy(h->h_stage[k] + table + at, h_streams[f], (size_t)h_lengths[f]);
            at += ((size_t)h_lengths[f] + 3) & ~(size_t)3;
        }
    }
    ADAS_HIP_TRY(hipMemcpyAsync(h->d_stage[k], h->h_stage[k], table + at, hipMemcpyHostToDevice, (hipStream_t)copy_stream));
    ADAS_HIP_TRY(hipEventRecord(h->ev_staged[k], (hipStream_t)copy_stream));
    h->staged[k] = true;
    ++h->stage_next;
    *slot = k;
    return ADAS_OK;
}

int adas::jpegdec_run_slot(adas_jpegdec* h, int slot, int batch, uint8_t* d_dst_bgr, void* stream) {
    const int64_t* len = (const int64_t*)h->d_stage[slot];
    return jpegdec_launch(h, h->d_stage[slot] + (size_t)h->max_batch * 16, len, len + h->max_batch, 0, batch, d_dst_bgr, (hipStream_t)stream);
}

extern "C" {

int adas_jpegdec_default_params(adas_jpegdec_params* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_jpegdec_default_params: null argument");
    memset(p, 0, sizeof(*p));
    p->width = 1280;
    p->height = 720;
    p->capacity = 0;
    return ADAS_OK;
}

int adas_jpegdec_destroy(adas_jpegdec* h) {
    if (!h) return ADAS_OK;
    for (void* q : {(void*)h->d_rec, (void*)h->d_seg, (void*)h->d_coef, (void*)h->d_planes, (void*)h->d_frames, (void*)h->d_flags, (void*)h->d_stage[0],
                    (void*)h->d_stage[1]})
        if (q) (void)hipFree(q);
    for (int k = 0; k < 2; ++k) {
        if (h->h_stage[k]) (void)hipHostFree(h->h_stage[k]);
        if (h->ev_staged[k]) (void)hipEventDestroy(h->ev_staged[k]);
        if (h->ev_ran[k]) (void)hipEventDestroy(h->ev_ran[k]);
    }
    delete h;
    return ADAS_OK;
}

int adas_jpegdec_create(const adas_jpegdec_params* p, int max_batch, adas_jpegdec** out) {
    const char* who = "adas_jpegdec_create";
    ADAS_REQUIRE(p && out, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(p->width >= 1 && p->height >= 1 && p->width <= JPEG_MAX_DIM && p->height <= JPEG_MAX_DIM, ADAS_ERR_INVALID,
                 "%s: a %dx%d frame (width and height must be in 1..%d)", who, p->width, p->height, JPEG_MAX_DIM);
    ADAS_REQUIRE(max_batch >= 1, ADAS_ERR_INVALID, "%s: max_batch %d", who, max_batch);
    const long long cap = p->capacity ? (long long)p->capacity : jpeg_bound(p->width, p->height);
    ADAS_REQUIRE(cap >= 1 && cap <= JPEGDEC_MAX_CAPACITY, ADAS_ERR_INVALID, "%s: a capacity of %lld bytes per stream is outside 1..%lld", who, cap,
                 (long long)JPEGDEC_MAX_CAPACITY);
    adas_jpegdec* h = new (std::nothrow) adas_jpegdec();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->p = *p;
    h->p.capacity = cap;
    h->max_batch = max_batch;
    h->cap_blocks = jpegdec_cap_blocks(p->width, p->height);
    h->cap_segs = jpegdec_cap_segments(p->width, p->height);
    h->frame_bytes = (long long)p->width * p->height * 3;
    const size_t B = (size_t)max_batch;
    hipError_t e = hipMalloc((void**)&h->d_rec, B * sizeof(JdFrame));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_seg, B * (size_t)h->cap_segs * 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_coef, B * (size_t)h->cap_blocks * 64 * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_planes, B * (size_t)h->cap_blocks * 64);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_frames, B * (size_t)h->frame_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_flags, B * sizeof(int32_t));
    h->stage_bytes = B * 16 + B * ((size_t)cap + 4);
    for (int k = 0; k < 2; ++k) {
        if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_stage[k], h->stage_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void**)&h->d_stage[k], h->stage_bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_staged[k], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_ran[k], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMemset(h->d_flags, 0, B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(h->d_frames, 0, B * (size_t)h->frame_bytes);
    if (e != hipSuccess) {
        adas_jpegdec_destroy(h);
        return hip_fail(e, "hipMalloc(jpegdec)", __FILE__, __LINE__);
    }
    *out = h;
    return ADAS_OK;
}

int adas_jpegdec_run(adas_jpegdec* h, const uint8_t* d_streams, const int64_t* d_lengths, int64_t stride, int batch, uint8_t* d_dst_bgr, void* stream) {
    ADAS_REQUIRE(h && d_streams && d_lengths, ADAS_ERR_INVALID, "adas_jpegdec_run: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_jpegdec_run: batch %d, the handle holds %d frames", batch, h->max_batch);
    ADAS_REQUIRE(stride >= 0, ADAS_ERR_INVALID, "adas_jpegdec_run: a stride of %lld bytes", (long long)stride);
    return jpegdec_launch(h, d_streams, d_lengths, nullptr, stride, batch, d_dst_bgr, (hipStream_t)stream);
}

int adas_jpegdec_run_host(adas_jpegdec* h, const uint8_t* const* h_streams, const int64_t* h_lengths, int batch, uint8_t* d_dst_bgr, void* stream) {
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "adas_jpegdec_run_host: null argument");
    int slot = (int)(h->stage_next & 1);
    // the run that last read this device slot may have been queued on another stream: the copy waits for it
    if (h->ran[slot]) ADAS_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, h->ev_ran[slot], 0));
    int rc = adas::jpegdec_stage_host(h, h_streams, h_lengths, batch, stream, &slot);
    if (rc) return rc;
    rc = adas::jpegdec_run_slot(h, slot, batch, d_dst_bgr, stream);
    if (rc) return rc;
    ADAS_HIP_TRY(hipEventRecord(h->ev_ran[slot], (hipStream_t)stream));
    h->ran[slot] = true;
    return ADAS_OK;
}

int adas_jpegdec_fetch(adas_jpegdec* h, int frame, uint8_t* h_bgr) {
    ADAS_REQUIRE(h && h_bgr, ADAS_ERR_INVALID, "adas_jpegdec_fetch: null argument");
    ADAS_REQUIRE(h->run_own && frame >= 0 && frame < h->run_frames, ADAS_ERR_INVALID,
                 "adas_jpegdec_fetch: frame %d was not written into the handle's buffer by the last run (%d frames)", frame, h->run_own ? h->run_frames : 0);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_bgr, h->d_frames + (size_t)frame * h->frame_bytes, (size_t)h->frame_bytes, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_jpegdec_fetch_flags(adas_jpegdec* h, int batch, int32_t* flags) {
    ADAS_REQUIRE(h && flags, ADAS_ERR_INVALID, "adas_jpegdec_fetch_flags: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->run_frames, ADAS_ERR_INVALID, "adas_jpegdec_fetch_flags: %d frames, the last run decoded %d", batch, h->run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(flags, h->d_flags, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_jpegdec_device_view(adas_jpegdec* h, const uint8_t** d_frames_bgr, const int32_t** d_flags) {
    ADAS_REQUIRE(h && d_frames_bgr && d_flags, ADAS_ERR_INVALID, "adas_jpegdec_device_view: null argument");
    *d_frames_bgr = h->d_frames;
    *d_flags = h->d_flags;
    return ADAS_OK;
}

}  // extern "C"
