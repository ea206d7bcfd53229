// jpeg_kernels.hip -- baseline JPEG on the device: one compressed stream per frame from BGR u8 frames that sit in HBM (the overlay's drawn
// frames, or a caller's), so a drawn frame leaves the device as a few hundred KB instead of width x height x 3 bytes.  The rules are
// jpeg_core.h (J1-J9); this file is the three kernels around them and the C ABI (adas_jpeg_*).  A restart segment (one MCU row) is the unit of
// independence.  A run is
//   jpeg_transform_kernel  eight lanes per 8x8 block, a row and then a column each: colour conversion, chroma averaging, edge
//                          replication (aligned 4-byte loads shifted into place: the source may start on any byte; a row that reaches beyond
//                          the right edge goes byte by byte), the integer DCT (the rows meet in LDS) and the quantiser, into an int16 level
//                          arena [frame][segment][8][blocks of the segment][8] in zigzag order: eight levels of a block are 16 bytes, and
//                          consecutive blocks lie side by side, so this kernel's stores and the next kernel's loads are 16 bytes per lane
//                          along the lanes.
//   jpeg_entropy_kernel    one workgroup per (frame, segment), one lane per block, 256 blocks at a time: the lanes count their blocks' bits
//                          (eight levels per load, a group of zeros is a run of eight), a workgroup scan (wave shuffles, one LDS word per
//                          wave) places them, every lane gathers its codes in a register and ORs them a word at a time into an LDS bit
//                          buffer sized for the worst case of 256 blocks; the buffer's whole bytes are then stuffed (a second scan over the
//                          0xFF counts) into the segment's slot of a scratch arena and the bits of the last partial byte are carried into
//                          the next 256 blocks.  The segment's byte length is recorded.
//   jpeg_assemble_kernel   one workgroup per (frame, segment): sums the segment lengths in front of its own and all of them, and copies its
//                          segment behind the header, RST markers and segments before it; segment 0 adds the header, the last one EOI, and
//                          segment 0 writes the frame's length and flags.  A frame that would not fit its capacity gets length 0 and
//                          ADAS_JPEG_OVERFLOW and none of its workgroups writes a byte.
// Plain launches without allocation or synchronisation: capturable.  Every byte below a frame's length is written exactly once per run, bytes
// from the length up to the capacity are left alone.  The yardstick is a device-to-device copy of the same frames (tools/bench_jpeg.py).
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include "jpeg_core.h"

using namespace adas;

static_assert(JPEG_OVERFLOW == ADAS_JPEG_OVERFLOW, "jpeg_core.h restates ADAS_JPEG_OVERFLOW");
static_assert(sizeof(adas_jpeg_params) == 24 && offsetof(adas_jpeg_params, quality) == 8 && offsetof(adas_jpeg_params, capacity) == 16,
              "adas_jpeg_params is _lib.JpegParams");

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_BLOCKS = JP_THREADS / 8;   // blocks of a transform workgroup
constexpr int JP_BUF_WORDS = (JP_THREADS * JPEG_BLOCK_MAX_BITS + 31) / 32 + 8;   // 256 worst-case blocks and a carried partial byte

struct JpArgs {
    JpegGeom g;
    int frames;
    long long capacity;         // bytes between two frames' streams
    long long seg_slot;         // bytes between two segments' slots in the scratch arena
    const uint8_t* src;         // [frames][h][w][3], any alignment
    const JpegTables* tab;
    const uint8_t* header;      // [JPEG_HEADER_BYTES]
    int16_t* levels;            // [frames][mcu_h][8][seg_blocks][8]: zigzag position 8 g + j of block b at [g][b][j]
    uint8_t* segs;              // [frames][mcu_h][seg_slot]
    int* seg_len;               // [frames][mcu_h]
    uint8_t* out;               // [frames][capacity]
    long long* lengths;         // [frames]
    int32_t* flags;             // [frames]
    long long* meta;            // [frames][2]: length and flags side by side, what a fetch reads in one copy
};

// NB bytes (a multiple of 4) from any address p as NB / 4 little-endian words, read as aligned 4-byte words: every word read holds at least one
// of the NB bytes, so it lies in a page they lie in (the word behind the last is read only when p is not aligned and then holds the last byte)
template <int NB>
__device__ __forceinline__ void jp_load_bytes(const uint8_t* p, uint32_t* out) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
    const int sh = (int)(a & 3) * 8;
    uint32_t w[NB / 4 + 1];
#pragma unroll
    for (int i = 0; i < NB / 4; ++i) w[i] = q[i];
    w[NB / 4] = sh ? q[NB / 4] : 0u;
#pragma unroll
    for (int i = 0; i < NB / 4; ++i) out[i] = (uint32_t)((((unsigned long long)w[i + 1] << 32) | w[i]) >> sh);
}
// pixel i of a row held as such words
__device__ __forceinline__ JpegPx jp_px(const uint32_t* w, int i) {
    auto byte = [&](int j) { return (int)((w[j >> 2] >> ((j & 3) * 8)) & 255u); };
    return JpegPx{byte(3 * i), byte(3 * i + 1), byte(3 * i + 2)};
}

// jpeg_load_row for a row that lies inside the frame's width: its 24 (luminance) or 2 x 48 (chrominance) bytes as aligned words, not byte by byte;
// a row that reaches beyond the right edge goes through jpeg_load_row itself
__device__ __forceinline__ void jp_load_row(const uint8_t* frame, int w, int h, int my, int mx, int k6, int j, int* f) {
    int ya, yb, x0, n;
    jpeg_row_place(h, my, mx, k6, j, &ya, &yb, &x0, &n);
    if (x0 + n > w) {
        jpeg_load_row(frame, w, h, my, mx, k6, j, f);
    } else if (k6 < 4) {
        uint32_t a[6];
        jp_load_bytes<24>(frame + ((size_t)ya * w + x0) * 3, a);
        jpeg_row_luma([&](int i) { return jp_px(a, i); }, f);
    } else {
        uint32_t a[12], b[12];
        jp_load_bytes<48>(frame + ((size_t)ya * w + x0) * 3, a);
        jp_load_bytes<48>(frame + ((size_t)yb * w + x0) * 3, b);
        jpeg_row_chroma(k6, [&](int i) { return jp_px(a, i); }, [&](int i) { return jp_px(b, i); }, f);
    }
}

// Eight lanes per block, 32 blocks per workgroup: lane r loads and transforms row r, the rows meet in LDS, lane r transforms and quantises
// column r (the same two jpeg_fdct_pass calls per value as jpeg_fdct), the levels meet in LDS in zigzag order, and the workgroup stores them
// with consecutive lanes on consecutive blocks.
__global__ __launch_bounds__(JP_THREADS) void jpeg_transform_kernel(const JpArgs a) {
    __shared__ int rows[JP_BLOCKS][8][9];
    __shared__ alignas(16) int16_t lev[JP_BLOCKS][66];
    const int t = threadIdx.x;
    {
        const int lb = t >> 3, r = t & 7;
        const long long gid = (long long)blockIdx.x * JP_BLOCKS + lb;
        const bool live = gid < (long long)a.frames * a.g.blocks;
        const int f = live ? (int)(gid / a.g.blocks) : 0;
        const long long rem = live ? gid % a.g.blocks : 0;
        const int seg = (int)(rem / a.g.seg_blocks), b = (int)(rem % a.g.seg_blocks);
        const int k6 = b % 6;
        int v[8];
        if (live) {
            jp_load_row(a.src + (size_t)f * a.g.h * a.g.w * 3, a.g.w, a.g.h, seg, b / 6, k6, r, v);
            jpeg_fdct_pass(v, 1, 256, 9);
#pragma unroll
            for (int u = 0; u < 8; ++u) rows[lb][r][u] = v[u];
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int y = 0; y < 8; ++y) v[y] = rows[lb][y][r];
            jpeg_fdct_pass(v, 1, 65536, 17);
            const uint16_t* q = a.tab->q[k6 >= 4];
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                const int k = jpeg_zigzag_position(y * 8 + r);
                lev[lb][k] = (int16_t)jpeg_quantise(v[y], q[k], k > 0);
            }
        }
        __syncthreads();
    }
    const int lb = t & (JP_BLOCKS - 1), grp = t / JP_BLOCKS;      // the eight levels of group grp of block lb: one 16-byte store
    const long long gid = (long long)blockIdx.x * JP_BLOCKS + lb;
    if (gid >= (long long)a.frames * a.g.blocks) return;
    const int f = (int)(gid / a.g.blocks);
    const long long rem = gid % a.g.blocks;
    const int seg = (int)(rem / a.g.seg_blocks), b = (int)(rem % a.g.seg_blocks);
    const uint32_t* l2 = (const uint32_t*)&lev[lb][grp * 8];      // 4-byte aligned: a row of lev is 132 bytes
    int16_t* dst = a.levels + ((((size_t)f * a.g.mcu_h + seg) * 8 + grp) * a.g.seg_blocks + b) * 8;
    *(uint4*)dst = make_uint4(l2[0], l2[1], l2[2], l2[3]);
}

// exclusive scan of v over the workgroup's 256 lanes; *total: the sum.  sh: 4 words of LDS, free again on return
__device__ __forceinline__ int jp_scan(int v, int* sh, int t, int* total) {
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
    for (int w = 0; w < JP_THREADS / 64; ++w) {
        const int s = sh[w];
        if (w < (t >> 6)) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// `count` bits (<= 27), most significant first, at bit `pos` of a zeroed LDS buffer shared with the other lanes
__device__ __forceinline__ void jp_or_bits(uint32_t* buf, int pos, uint32_t bits, int count) {
    uint32_t hi, lo;
    jpeg_split_bits(pos, bits, count, &hi, &lo);
    atomicOr(&buf[pos >> 5], hi);
    if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}

// A block's bits on their way into that buffer: they gather in a register and leave a whole word at a time, one OR each -- the first and the
// last word are shared with the neighbouring blocks, so every word is ORed in.
struct JpBits {
    uint32_t* buf;
    unsigned long long acc;
    int n, word;
    __device__ __forceinline__ JpBits(uint32_t* b, int pos) : buf(b), acc(0), n(pos & 31), word(pos >> 5) {}
    __device__ __forceinline__ void put(uint32_t bits, int count) {      // n <= 31 here, count <= 27
        acc |= (unsigned long long)bits << (64 - n - count);
        n += count;
        if (n >= 32) {
            atomicOr(&buf[word++], (uint32_t)(acc >> 32));
            acc <<= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n) atomicOr(&buf[word], (uint32_t)(acc >> 32));
    }
};

__global__ __launch_bounds__(JP_THREADS) void jpeg_entropy_kernel(const JpArgs a) {
    __shared__ uint32_t buf[JP_BUF_WORDS];
    __shared__ uint32_t ac_tab[2][256];
    __shared__ uint32_t dc_tab[2][12];
    __shared__ int sh[JP_THREADS / 64];
    const int t = threadIdx.x;
    const int f = blockIdx.x / a.g.mcu_h, seg = blockIdx.x % a.g.mcu_h;
    const int nblk = a.g.seg_blocks;
    for (int i = t; i < 512; i += JP_THREADS) ac_tab[i >> 8][i & 255] = a.tab->ac[i >> 8][i & 255];
    if (t < 24) dc_tab[t / 12][t % 12] = a.tab->dc[t / 12][t % 12];
    __syncthreads();
    const int16_t* lv = a.levels + ((size_t)f * a.g.mcu_h + seg) * 64 * nblk;
    uint8_t* slot = a.segs + ((size_t)f * a.g.mcu_h + seg) * a.seg_slot;
    int out_pos = 0;                  // bytes of the segment written so far
    int carry_n = 0;                  // bits of the last partial byte, and their value
    uint32_t carry_v = 0;
    for (int c0 = 0; c0 < nblk; c0 += JP_THREADS) {
        const int b = c0 + t;
        const bool live = b < nblk;
        const int cls = live && (b % 6) >= 4;
        int diff = 0, nbits = 0;
        auto lev = [&](int g, int* l) {      // eight levels of the lane's block: one 16-byte load
            const uint4 q = *(const uint4*)(lv + ((size_t)g * nblk + b) * 8);
            l[0] = (int16_t)(q.x & 0xffffu); l[1] = (int16_t)(q.x >> 16);
            l[2] = (int16_t)(q.y & 0xffffu); l[3] = (int16_t)(q.y >> 16);
            l[4] = (int16_t)(q.z & 0xffffu); l[5] = (int16_t)(q.z >> 16);
            l[6] = (int16_t)(q.w & 0xffffu); l[7] = (int16_t)(q.w >> 16);
        };
        if (live) {
            const int pb = jpeg_dc_predecessor(b);
            diff = (int)lv[(size_t)b * 8] - (pb >= 0 ? (int)lv[(size_t)pb * 8] : 0);
            jpeg_code_block8(dc_tab[cls], ac_tab[cls], diff, lev, [&](uint32_t, int n) { nbits += n; });
        }
        int sum = 0;
        const int pos = carry_n + jp_scan(nbits, sh, t, &sum);
        const int total = carry_n + sum;
        for (int i = t; i < (total + 31) / 32 + 2; i += JP_THREADS) buf[i] = 0;     // <= JP_BUF_WORDS: total <= 7 + 256 * 1658
        __syncthreads();
        if (t == 0 && carry_n) jp_or_bits(buf, 0, carry_v, carry_n);
        if (live) {
            JpBits bits(buf, pos);
            jpeg_code_block8(dc_tab[cls], ac_tab[cls], diff, lev, [&](uint32_t v, int n) { bits.put(v, n); });
            bits.finish();
        }
        __syncthreads();
        const bool last = c0 + JP_THREADS >= nblk;
        const int rem = total & 7;
        int nbytes = total >> 3;
        if (last && rem) {           // J6: 1-bits up to the byte
            if (t == 0) jp_or_bits(buf, total, (1u << (8 - rem)) - 1u, 8 - rem);
            __syncthreads();
            ++nbytes;
        }
        carry_n = last ? 0 : rem;
        carry_v = carry_n ? jpeg_carry_bits(buf, nbytes, carry_n) : 0u;
        for (int w0 = 0; w0 * 4 < nbytes; w0 += JP_THREADS) {      // whole bytes, four per lane, 0x00 behind every 0xFF
            const int wi = w0 + t;
            const int nv = nbytes - 4 * wi < 0 ? 0 : (nbytes - 4 * wi > 4 ? 4 : nbytes - 4 * wi);
            const uint32_t w = nv ? buf[wi] : 0u;
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) cnt += 1 + (jpeg_word_byte(w, j) == 255u);
            int tile = 0;
            int o = out_pos + jp_scan(cnt, sh, t, &tile);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) {
                    const uint32_t v = jpeg_word_byte(w, j);
                    slot[o++] = (uint8_t)v;
                    if (v == 255u) slot[o++] = 0;
                }
            out_pos += tile;
        }
        __syncthreads();   // the carry and the bytes are read: the next 256 blocks may zero the buffer
    }
    if (t == 0) a.seg_len[(size_t)f * a.g.mcu_h + seg] = out_pos;
}

__global__ __launch_bounds__(JP_THREADS) void jpeg_assemble_kernel(const JpArgs a) {
    __shared__ long long red[2][JP_THREADS];
    const int t = threadIdx.x;
    const int f = blockIdx.x / a.g.mcu_h, seg = blockIdx.x % a.g.mcu_h;
    const int* len = a.seg_len + (size_t)f * a.g.mcu_h;
    long long before = 0, all = 0;
    for (int s = t; s < a.g.mcu_h; s += JP_THREADS) {
        const int n = len[s];
        all += n;
        if (s < seg) before += n;
    }
    red[0][t] = before;
    red[1][t] = all;
    __syncthreads();
    for (int d = JP_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) {
            red[0][t] += red[0][t + d];
            red[1][t] += red[1][t + d];
        }
        __syncthreads();
    }
    before = red[0][0];
    all = red[1][0];
    const long long length = (long long)JPEG_HEADER_BYTES + all + 2LL * (a.g.mcu_h - 1) + 2;
    const bool fits = length <= a.capacity;
    if (seg == 0 && t == 0) {
        a.lengths[f] = fits ? length : 0;
        a.flags[f] = fits ? 0 : JPEG_OVERFLOW;
        a.meta[2 * f] = fits ? length : 0;
        a.meta[2 * f + 1] = fits ? 0 : JPEG_OVERFLOW;
    }
    if (!fits) return;
    uint8_t* out = a.out + (size_t)f * a.capacity;
    if (seg == 0)
        for (int i = t; i < JPEG_HEADER_BYTES; i += JP_THREADS) out[i] = a.header[i];
    const long long at = (long long)JPEG_HEADER_BYTES + before + 2LL * seg;    // the RST markers of the segments before sit in front
    if (seg > 0 && t == 0) {
        out[at - 2] = 0xFF;
        out[at - 1] = (uint8_t)(0xD0 + ((seg - 1) & 7));
    }
    const uint8_t* src = a.segs + ((size_t)f * a.g.mcu_h + seg) * a.seg_slot;
    const int n = len[seg];
    for (int i = t; i < n; i += JP_THREADS) out[at + i] = src[i];
    if (seg == a.g.mcu_h - 1 && t == 0) {
        out[at + n] = 0xFF;
        out[at + n + 1] = 0xD9;
    }
}

}  // namespace

struct adas_jpeg {
    adas_jpeg_params p;
    JpegGeom g;
    int max_batch = 0;
    long long seg_slot = 0;
    JpegTables* d_tab = nullptr;
    uint8_t* d_header = nullptr;
    int16_t* d_levels = nullptr;
    uint8_t* d_segs = nullptr;
    int* d_seg_len = nullptr;
    uint8_t* d_out = nullptr;
    long long* d_len = nullptr;
    int32_t* d_flags = nullptr;
    long long* d_meta = nullptr;
    long long* h_meta = nullptr;  // pinned, [max_batch][2]: where a fetch lands a frame's length and flags
    hipStream_t last = nullptr;   // the stream of the last run: what the fetches drain
    int run_frames = 0;
};

void adas::jpeg_geometry_of(const adas_jpeg* h, int* width, int* height, int* max_batch) {
    *width = h ? h->p.width : 0;
    *height = h ? h->p.height : 0;
    *max_batch = h ? h->max_batch : 0;
}

static int jpeg_upload_tables(adas_jpeg* h, int quality) {
    JpegTables T;
    uint8_t hdr[JPEG_HEADER_BYTES];
    jpeg_build_tables(quality, &T);
    const int n = jpeg_build_header(h->p.width, h->p.height, quality, hdr);
    ADAS_REQUIRE(n == JPEG_HEADER_BYTES, ADAS_ERR_INVALID, "adas_jpeg: the header is %d bytes, not %d", n, JPEG_HEADER_BYTES);
    ADAS_HIP_TRY(hipDeviceSynchronize());   // a run in flight may still read the old tables
    ADAS_HIP_TRY(hipMemcpy(h->d_tab, &T, sizeof(T), hipMemcpyHostToDevice));
    ADAS_HIP_TRY(hipMemcpy(h->d_header, hdr, sizeof(hdr), hipMemcpyHostToDevice));
    h->p.quality = quality;
    return ADAS_OK;
}

extern "C" {

int adas_jpeg_default_params(adas_jpeg_params* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_jpeg_default_params: null argument");
    memset(p, 0, sizeof(*p));
    p->width = 1280;
    p->height = 720;
    p->quality = 90;
    p->capacity = 0;
    return ADAS_OK;
}

int64_t adas_jpeg_bound(int width, int height) {
    if (width < 1 || height < 1 || width > JPEG_MAX_DIM || height > JPEG_MAX_DIM) return 0;
    return (int64_t)jpeg_bound(width, height);
}

int adas_jpeg_destroy(adas_jpeg* h) {
    if (!h) return ADAS_OK;
    for (void* q : {(void*)h->d_tab, (void*)h->d_header, (void*)h->d_levels, (void*)h->d_segs, (void*)h->d_seg_len, (void*)h->d_out, (void*)h->d_len,
                    (void*)h->d_flags, (void*)h->d_meta})
        if (q) (void)hipFree(q);
    if (h->h_meta) (void)hipHostFree(h->h_meta);
    delete h;
    return ADAS_OK;
}

int adas_jpeg_create(const adas_jpeg_params* p, int max_batch, adas_jpeg** out) {
    const char* who = "adas_jpeg_create";
    ADAS_REQUIRE(p && out, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(p->width >= 1 && p->height >= 1 && p->width <= JPEG_MAX_DIM && p->height <= JPEG_MAX_DIM, ADAS_ERR_INVALID,
                 "%s: a %dx%d frame (width and height must be in 1..%d)", who, p->width, p->height, JPEG_MAX_DIM);
    ADAS_REQUIRE(p->quality >= 1 && p->quality <= 100, ADAS_ERR_INVALID, "%s: quality %d is outside 1..100", who, p->quality);
    ADAS_REQUIRE(max_batch >= 1, ADAS_ERR_INVALID, "%s: max_batch %d", who, max_batch);
    const long long cap = p->capacity ? (long long)p->capacity : (long long)p->width * p->height * 3;
    ADAS_REQUIRE(cap >= JPEG_HEADER_BYTES, ADAS_ERR_INVALID,
                 "%s: a capacity of %lld bytes per frame is below the %d header bytes (adas_jpeg_bound(%d, %d) = %lld always fits)", who, cap,
                 JPEG_HEADER_BYTES, p->width, p->height, jpeg_bound(p->width, p->height));
    adas_jpeg* h = new (std::nothrow) adas_jpeg();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->p = *p;
    h->p.capacity = cap;
    h->g = jpeg_geometry(p->width, p->height);
    h->max_batch = max_batch;
    h->seg_slot = (long long)h->g.seg_blocks * JPEG_BLOCK_MAX_BYTES;
    const size_t segs = (size_t)max_batch * h->g.mcu_h;
    hipError_t e = hipMalloc((void**)&h->d_tab, sizeof(JpegTables));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_header, JPEG_HEADER_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_levels, (size_t)max_batch * h->g.blocks * 64 * sizeof(int16_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_segs, segs * (size_t)h->seg_slot);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_seg_len, segs * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_out, (size_t)max_batch * (size_t)cap);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_len, (size_t)max_batch * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_flags, (size_t)max_batch * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_meta, (size_t)max_batch * 2 * sizeof(long long));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_meta, (size_t)max_batch * 2 * sizeof(long long), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemset(h->d_len, 0, (size_t)max_batch * sizeof(long long));
    if (e == hipSuccess) e = hipMemset(h->d_flags, 0, (size_t)max_batch * sizeof(int32_t));
    if (e != hipSuccess) {
        adas_jpeg_destroy(h);
        return hip_fail(e, "hipMalloc(jpeg)", __FILE__, __LINE__);
    }
    int rc = jpeg_upload_tables(h, p->quality);
    if (rc) {
        adas_jpeg_destroy(h);
        return rc;
    }
    *out = h;
    return ADAS_OK;
}

int adas_jpeg_set_quality(adas_jpeg* h, int quality) {
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "adas_jpeg_set_quality: null handle");
    ADAS_REQUIRE(quality >= 1 && quality <= 100, ADAS_ERR_INVALID, "adas_jpeg_set_quality: quality %d is outside 1..100", quality);
    return jpeg_upload_tables(h, quality);   // the tables keep their addresses: a captured run reads the new ones
}

int adas_jpeg_run(adas_jpeg* h, const uint8_t* d_frames_bgr, int batch, void* stream) {
    ADAS_REQUIRE(h && d_frames_bgr, ADAS_ERR_INVALID, "adas_jpeg_run: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "adas_jpeg_run: batch %d, the handle holds %d frames", batch, h->max_batch);
    hipStream_t st = (hipStream_t)stream;
    JpArgs a = {};
    a.g = h->g;
    a.frames = batch;
    a.capacity = h->p.capacity;
    a.seg_slot = h->seg_slot;
    a.src = d_frames_bgr;
    a.tab = h->d_tab; a.header = h->d_header; a.levels = h->d_levels; a.segs = h->d_segs; a.seg_len = h->d_seg_len;
    a.out = h->d_out; a.lengths = h->d_len; a.flags = h->d_flags; a.meta = h->d_meta;
    h->last = st;
    h->run_frames = batch;
    const long long blocks = (long long)batch * h->g.blocks;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((blocks + JP_BLOCKS - 1) / JP_BLOCKS)), dim3(JP_THREADS), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    const unsigned segs = (unsigned)batch * (unsigned)h->g.mcu_h;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(segs), dim3(JP_THREADS), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(jpeg_assemble_kernel, dim3(segs), dim3(JP_THREADS), 0, st, a);
    ADAS_HIP_TRY(hipGetLastError());
    return ADAS_OK;
}

int adas_jpeg_fetch_lengths(adas_jpeg* h, int batch, int64_t* n_bytes, int32_t* flags) {
    ADAS_REQUIRE(h && n_bytes, ADAS_ERR_INVALID, "adas_jpeg_fetch_lengths: null argument");
    ADAS_REQUIRE(batch >= 1 && batch <= h->run_frames, ADAS_ERR_INVALID, "adas_jpeg_fetch_lengths: %d frames, the last run encoded %d", batch, h->run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    static_assert(sizeof(long long) == sizeof(int64_t), "lengths are 64 bits");
    ADAS_HIP_TRY(hipMemcpy(n_bytes, h->d_len, (size_t)batch * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (flags) ADAS_HIP_TRY(hipMemcpy(flags, h->d_flags, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_jpeg_fetch(adas_jpeg* h, int frame, uint8_t* h_buf, int64_t h_cap, int64_t* n_bytes, int32_t* flags) {
    ADAS_REQUIRE(h && n_bytes, ADAS_ERR_INVALID, "adas_jpeg_fetch: null argument");
    ADAS_REQUIRE(frame >= 0 && frame < h->run_frames, ADAS_ERR_INVALID, "adas_jpeg_fetch: frame %d was not part of the last run (%d frames)", frame,
                 h->run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h->h_meta + 2 * frame, h->d_meta + 2 * frame, 2 * sizeof(long long), hipMemcpyDeviceToHost));
    const long long n = h->h_meta[2 * frame];
    const int32_t fl = (int32_t)h->h_meta[2 * frame + 1];
    *n_bytes = n;
    if (flags) *flags = fl;
    ADAS_REQUIRE(n == 0 || (h_buf && h_cap >= n), ADAS_ERR_INVALID, "adas_jpeg_fetch: frame %d holds %lld bytes, the buffer %lld", frame, n, (long long)h_cap);
    if (n) ADAS_HIP_TRY(hipMemcpy(h_buf, h->d_out + (size_t)frame * (size_t)h->p.capacity, (size_t)n, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_jpeg_device_view(adas_jpeg* h, const uint8_t** d_streams, const int64_t** d_lengths, int64_t* stride) {
    ADAS_REQUIRE(h && d_streams && d_lengths && stride, ADAS_ERR_INVALID, "adas_jpeg_device_view: null argument");
    *d_streams = h->d_out;
    *d_lengths = (const int64_t*)h->d_len;
    *stride = h->p.capacity;
    return ADAS_OK;
}

}  // extern "C"
