// overlay_kernels.hip -- the lane overlay on the device: the discs, the ego-lane polygon and the two alpha blends of the reference's
// Draw* block (ultrafastLaneDetectorV2.py:196-218, distanceMeasure.py:98, perspectiveTransformation.py:217-226) on BGR u8 frames that
// already sit in HBM.  The pixel rules are overlay_core.h (modelled on OpenCV 4.5, parity with a real cv2 build UNPINNED, lines not
// clipped before they are walked); this file is the kernels around them and the C ABI (adas_overlay_*).
//
// Coverage lives in HBM as bit planes, 32 columns to a word: per frame an ANY plane [H][rw] (rw = ceil(W / 32): W / 8 bytes per row, about
// 4 % of the frame) and a DETAIL plane [H][rw][8] (lanes 0..3, area, distance points; 2 spare words) that is read only where ANY is set.
// All planes are zero between runs.  A run is
//   overlay_mark_kernel    (i) preparation.  One workgroup owns a band of OV_BAND rows of one frame and builds their coverage in LDS: the
//                          polygon's edges that meet the band are listed, every (row, edge) pair ORs the edge's run on the row (closed form
//                          of the line walk) and toggles one bit per crossing, and a prefix XOR turns the toggles into the even-odd interior
//                          -- no crossing list, no sort, no cap; every disc whose rows meet the band ORs its spans.  Everything is an OR
//                          or an XOR, so no order matters: "the last disc wins" is resolved by the lane bit of the highest lane (lanes are
//                          drawn in order), colours by each frame's record.  The band's words that are not zero are stored; no global atomic.
//   overlay_stream_kernel  (ii) one pass: reads 3HW bytes and writes 3HW bytes per frame in 16-byte accesses aligned to the destination
//                          (a frame's first and last <= 15 bytes go byte by byte, as rows of 3W bytes start on every alignment) plus the
//                          ANY words of its columns; a 16-byte piece whose ANY words are zero is a copy.
//   overlay_clean_kernel   zeroes the words that were set (reads the ANY plane, writes only where it is not zero).
// The bird view's discs are written in place: the same mark kernel on the bird planes, then overlay_apply_kernel, one thread per ANY word,
// which writes the covered pixels and zeroes its words.
// Memory-bound by design: the yardstick is a device-to-device copy of the same frames (tools/bench_overlay.py).
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <initializer_list>
#include <new>
#include "overlay_core.h"

using namespace adas;

static_assert(sizeof(adas_overlay_params) == 88 && offsetof(adas_overlay_params, lane_alpha) == 32, "adas_overlay_params layout");

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_BAND = 8;          // rows of a mark workgroup (fewer for very wide images: the band's planes live in LDS)
constexpr int OV_PLANES = 7;        // LDS planes of a band: lanes 0..3, area, distance, toggles
constexpr int OV_LIST = 2048;       // polygon edges listed per pass
constexpr int OV_LDS_WORDS = 9216;  // LDS budget of the planes: 36 KB (+ 8 KB of edge list: under the 48 KB a launch may ask for)
constexpr int OV_MAXPTS = ADAS_UFLD_MAX_POINTS;

struct OvSources {                  // what one run reads, per frame q
    const int* lane_pts;            // [q][4][128][2]
    const int* lane_cnt;            // lane_cnt[q * lane_cnt_stride + l]
    int lane_cnt_stride;
    const int* poly;                // frame q's polygon at poly + q * poly_stride, (x, y) pairs
    size_t poly_stride;
    int poly_max;                   // points a frame's slab holds
    const int *poly_n0, *poly_n1;   // its count: poly_n0[q * poly_n_stride] (+ poly_n1[...] when non-null)
    int poly_n_stride;
    const int* area_on;             // area_on[q * area_on_stride] != 0: the polygon is drawn
    int area_on_stride;
    const int* offset_type;         // offset_type[q * offset_stride], null: UNKNOWN
    int offset_stride;
    const int* collision;           // collision[q * collision_stride] indexes collision_colors; null: area_bgr or the default
    int collision_stride;
    const uint8_t* area_bgr;        // [q][3] or null
    const int* dist_pts;            // [q][dist_cap][2]
    int dist_cap;
    const int* dist_cnt;            // dist_cnt[q * dist_cnt_stride]
    int dist_cnt_stride;
};

struct OvStyle {                    // colours packed as overlay_pack_bgr does
    uint32_t lane[4], offset, area, collision[4], dist;
    OverlayAlpha lane_w, area_w;
    int r_lane, r_dist;
};

struct OvDev {
    OvSources s;
    OvStyle st;
    int H, W, rw;                   // rw: words per plane row
    int band;                       // rows per mark workgroup
    uint32_t* any;                  // [frames][H][rw]
    uint32_t* detail;               // [frames][H][rw][8]
    int* flags;                     // [frames], null for the bird view
    int stages;                     // ADAS_OVERLAY_LANES | AREA | DISTANCE of this launch
    int direct;                     // lanes are written, not blended (the bird view)
    const uint8_t* src;
    uint8_t* dst;
};

__device__ __forceinline__ int ov_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ORs columns xl .. xr (inside the image) into a row's LDS words
__device__ __forceinline__ void ov_lds_span(uint32_t* roww, int xl, int xr) {
    for (int w = xl >> 5; w <= (xr >> 5); ++w) atomicOr(roww + w, overlay_word_mask(xl, xr, w));   // at most rw words: the span is clipped
}

struct LdsRowOps {   // overlay_poly_edge_row on a band's LDS bitmaps
    uint32_t *fillw, *togw;
    __device__ void fill(int xl, int xr) { ov_lds_span(fillw, xl, xr); }
    __device__ void set(int q) { atomicOr(fillw + (q >> 5), 1u << (q & 31)); }
    __device__ void toggle(int t) { atomicXor(togw + (t >> 5), 1u << (t & 31)); }
};

// grid (ceil(H / band), frames); dynamic LDS: OV_PLANES * band * rw words + OV_LIST ints.  One workgroup owns rows [y0, y0 + band) of one
// frame: it builds their coverage in LDS and stores the words that are not zero (the planes are zero between runs).
__global__ __launch_bounds__(OV_THREADS) void overlay_mark_kernel(OvDev d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int hw[2][ADAS_OVERLAY_MAX_RADIUS + 1];
    __shared__ int bad, listed;
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const int band = d.band, rw = d.rw, per = band * rw;
    uint32_t* planes = (uint32_t*)smem;                 // [OV_PLANES][band][rw]: lanes 0..3, area (edges, then the whole fill), distance, toggles
    int* list = (int*)(planes + OV_PLANES * per);       // [OV_LIST] edges that meet the band
    const int y0 = blockIdx.x * band;
    const int rows = d.H - y0 < band ? d.H - y0 : band;
    for (int i = tid; i < OV_PLANES * per; i += OV_THREADS) planes[i] = 0u;
    if (tid < 2) overlay_disc_halfwidths(tid == 0 ? d.st.r_lane : d.st.r_dist, hw[tid]);
    if (tid == 0) bad = 0;
    __syncthreads();
    // ---- the polygon
    int n = 0;
    if ((d.stages & ADAS_OVERLAY_AREA) && d.s.poly && d.s.area_on[f * d.s.area_on_stride] != 0) {
        n = d.s.poly_n0[f * d.s.poly_n_stride] + (d.s.poly_n1 ? d.s.poly_n1[f * d.s.poly_n_stride] : 0);
        n = ov_clampi(n, 0, d.s.poly_max);
    }
    const int* pts = d.s.poly + f * d.s.poly_stride;
    for (int i = tid; i < 2 * n; i += OV_THREADS)
        if (pts[i] > ADAS_OVERLAY_COORD_MAX || pts[i] < -ADAS_OVERLAY_COORD_MAX) bad = 1;   // every writer stores 1
    __syncthreads();
    const int skip = bad;
    if (blockIdx.x == 0 && tid == 0 && d.flags) d.flags[f] = skip ? ADAS_OVERLAY_POLY_RANGE : 0;
    if (skip) n = 0;
    for (int e0 = 0; e0 < n; e0 += OV_LIST) {   // edges in chunks of OV_LIST: those whose rows meet the band are listed, then (row, edge) pairs
        if (tid == 0) listed = 0;
        __syncthreads();
        const int e1 = e0 + OV_LIST < n ? e0 + OV_LIST : n;
        for (int e = e0 + tid; e < e1; e += OV_THREADS) {
            const int ya = pts[2 * e + 1], yb = pts[2 * (e + 1 == n ? 0 : e + 1) + 1];
            const int lo = ya < yb ? ya : yb, hi = ya < yb ? yb : ya;
            if (hi >= y0 && lo < y0 + rows) list[atomicAdd(&listed, 1)] = e;   // any order: everything below is an OR or an XOR
        }
        __syncthreads();
        const int m = listed;
        for (int t = tid; t < rows * m; t += OV_THREADS) {
            const int r = t / m, e = list[t - r * m];
            LdsRowOps ops{planes + 4 * per + r * rw, planes + 6 * per + r * rw};
            overlay_poly_edge_row(pts, n, e, y0 + r, d.W, ops);
        }
        __syncthreads();
    }
    // ---- discs: every slot of the lane table and every distance point whose rows meet the band
    if ((d.stages & ADAS_OVERLAY_LANES) && d.s.lane_pts) {
        const int R = d.st.r_lane;
        for (int t = tid; t < 4 * OV_MAXPTS; t += OV_THREADS) {
            const int l = t / OV_MAXPTS, i = t - l * OV_MAXPTS;
            if (i >= ov_clampi(d.s.lane_cnt[f * d.s.lane_cnt_stride + l], 0, OV_MAXPTS)) continue;
            const int* p = d.s.lane_pts + ((f * 4 + l) * OV_MAXPTS + i) * 2;
            const int cx = p[0], cy = p[1];
            for (int r = 0; r < rows; ++r) {
                const long long j = (long long)y0 + r - cy;
                int y, xl, xr;
                if (j >= -R && j <= R && overlay_disc_row(cx, cy, (int)j, hw[0][j < 0 ? -j : j], d.W, d.H, &y, &xl, &xr))
                    ov_lds_span(planes + l * per + r * rw, xl, xr);
            }
        }
    }
    if ((d.stages & ADAS_OVERLAY_DISTANCE) && d.s.dist_pts) {
        const int R = d.st.r_dist;
        const int nd = ov_clampi(d.s.dist_cnt[f * d.s.dist_cnt_stride], 0, d.s.dist_cap);
        for (int i = tid; i < nd; i += OV_THREADS) {
            const int* p = d.s.dist_pts + (f * d.s.dist_cap + i) * 2;
            const int cx = p[0], cy = p[1];
            for (int r = 0; r < rows; ++r) {
                const long long j = (long long)y0 + r - cy;
                int y, xl, xr;
                if (j >= -R && j <= R && overlay_disc_row(cx, cy, (int)j, hw[1][j < 0 ? -j : j], d.W, d.H, &y, &xl, &xr))
                    ov_lds_span(planes + 5 * per + r * rw, xl, xr);
            }
        }
    }
    __syncthreads();
    if (n > 0 && tid < rows) {   // the prefix XOR of a row is sequential in its words: one lane per row turns the toggles into the interior
        uint32_t carry = 0u;
        for (int w = 0; w < rw; ++w) {
            const uint32_t tg = planes[6 * per + tid * rw + w];
            uint32_t m = overlay_prefix_xor(tg, carry);
            carry ^= (uint32_t)__popc(tg) & 1u;
            if (w == rw - 1 && (d.W & 31)) m &= 0xffffffffu >> (32 - (d.W & 31));   // columns past the image
            planes[4 * per + tid * rw + w] |= m;
        }
    }
    __syncthreads();
    for (int i = tid; i < rows * rw; i += OV_THREADS) {
        const uint4 lo = make_uint4(planes[i], planes[per + i], planes[2 * per + i], planes[3 * per + i]);
        const uint32_t ar = planes[4 * per + i], di = planes[5 * per + i];
        const uint32_t any = lo.x | lo.y | lo.z | lo.w | ar | di;
        if (!any) continue;
        const size_t w = (f * d.H + y0) * (size_t)rw + i;
        uint4* q = reinterpret_cast<uint4*>(d.detail + w * 8);
        q[0] = lo;
        q[1] = make_uint4(ar, di, 0u, 0u);
        d.any[w] = any;
    }
}

// frame f's colours after the offset rule and the collision table
__device__ __forceinline__ OverlayStyle ov_frame_style(const OvDev& d, size_t f) {
    OverlayStyle o;
    const int off = d.s.offset_type ? d.s.offset_type[f * d.s.offset_stride] : ADAS_OFFSET_UNKNOWN;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const bool red = (l == 1 && off == ADAS_OFFSET_RIGHT) || (l == 2 && off == ADAS_OFFSET_LEFT);
        o.lane[l] = red ? d.st.offset : d.st.lane[l];
    }
    if (d.s.collision) {
        const int k = ov_clampi(d.s.collision[f * d.s.collision_stride], 0, 3);
        o.area = k == 0 ? d.st.collision[0] : k == 1 ? d.st.collision[1] : k == 2 ? d.st.collision[2] : d.st.collision[3];
    } else if (d.s.area_bgr) {
        o.area = (uint32_t)d.s.area_bgr[f * 3] | ((uint32_t)d.s.area_bgr[f * 3 + 1] << 8) | ((uint32_t)d.s.area_bgr[f * 3 + 2] << 16);
    } else {
        o.area = d.st.area;
    }
    o.dist = d.st.dist;
    o.lane_w = d.st.lane_w;
    o.area_w = d.st.area_w;
    o.lane_direct = d.direct;
    return o;
}

// the coverage words of 32 columns: a piece re-reads them only when it moves to another word
struct OvWord {
    size_t at;        // index of the cached word, ~0: none
    uint32_t any;
    uint4 lanes;
    uint2 rest;       // area, distance
};
__device__ __forceinline__ uint32_t ov_bits(const OvDev& d, OvWord& c, size_t f, int y, int x) {
    const size_t w = (f * d.H + y) * (size_t)d.rw + (x >> 5);
    if (w != c.at) {
        c.at = w;
        c.any = d.any[w];
        if (c.any) {
            c.lanes = *reinterpret_cast<const uint4*>(d.detail + w * 8);
            c.rest = *reinterpret_cast<const uint2*>(d.detail + w * 8 + 4);
        }
    }
    const uint32_t b = 1u << (x & 31);
    if (!(c.any & b)) return 0u;
    return ((c.lanes.x & b) ? 1u : 0u) | ((c.lanes.y & b) ? 2u : 0u) | ((c.lanes.z & b) ? 4u : 0u) | ((c.lanes.w & b) ? 8u : 0u) |
           ((c.rest.x & b) ? OV_BIT_AREA : 0u) | ((c.rest.y & b) ? OV_BIT_DIST : 0u);
}

struct __attribute__((packed, aligned(1))) OvPiece1 {   // a 16-byte piece at any address
    uint32_t w[4];
};

// Where bytes [b0, b0 + n) of a frame lie, and the coverage words fetched ahead for them
struct OvSpan {
    int y, x, c;      // row, column and channel of the first byte
    int x1;           // column of the last byte's pixel, when the bytes lie in one row (else -1)
    OvWord w;         // the first pixel's coverage word (at = ~0: not fetched)
    uint32_t quiet;   // 1: one row, and the ANY words of its columns are zero -- the bytes are a copy
};
__device__ __forceinline__ void ov_locate(const OvDev& d, size_t f, uint32_t b0, int n, OvSpan& s) {
    const uint32_t p0 = b0 / 3u, p1 = (b0 + n - 1) / 3u;
    s.c = (int)(b0 - p0 * 3u);
    s.y = (int)(p0 / (uint32_t)d.W);
    s.x = (int)(p0 - (uint32_t)s.y * d.W);
    s.x1 = s.x + (int)(p1 - p0) < d.W ? s.x + (int)(p1 - p0) : -1;
    s.w.at = ~(size_t)0;
    s.quiet = 0u;
    if (s.x1 >= 0) {   // the piece lies in one row: its columns span one or two ANY words
        const size_t w = (f * d.H + s.y) * (size_t)d.rw;
        s.w.at = w + (s.x >> 5);
        s.w.any = d.any[s.w.at];
        s.quiet = (s.w.any | d.any[w + (s.x1 >> 5)]) == 0u;
    }
}
// second step of the fetch: the first word's detail, when something is drawn there (issued for every piece of a thread before any is drawn)
__device__ __forceinline__ void ov_fetch_detail(const OvDev& d, OvSpan& s) {
    if (s.x1 >= 0 && s.w.any) {
        s.w.lanes = *reinterpret_cast<const uint4*>(d.detail + s.w.at * 8);
        s.w.rest = *reinterpret_cast<const uint2*>(d.detail + s.w.at * 8 + 4);
    }
}
// draws on the bytes held in v (byte k in bits 8 (k & 3) of v[k >> 2])
__device__ __forceinline__ void ov_draw_piece(const OvDev& d, size_t f, const OverlayStyle& st, int n, OvSpan& s, uint32_t v[4]) {
    if (s.quiet) return;
    int c = s.c, y = s.y, x = s.x;
    uint32_t bits = ov_bits(d, s.w, f, y, x);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < n) {
            if (bits) {
                const int sv = (int)((v[k >> 2] >> (8 * (k & 3))) & 0xffu);
                const int o = overlay_pixel(sv, bits, c, st);
                v[k >> 2] = (v[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((uint32_t)o << (8 * (k & 3)));
            }
            if (++c == 3) {
                c = 0;
                if (++x == d.W) { x = 0; ++y; }
                if (k + 1 < n) bits = ov_bits(d, s.w, f, y, x);
            }
        }
    }
}

constexpr int OV_UNROLL = 4;   // pieces a thread has in flight: the pass is a chain of dependent loads (frame bytes, ANY word, detail words)

// grid (blocks, frames); a frame's 3HW bytes = a head of < 16 bytes up to the destination's first 16-byte boundary, aligned pieces, a tail
__global__ __launch_bounds__(OV_THREADS) void overlay_stream_kernel(OvDev d) {
    const size_t f = blockIdx.y;
    const uint32_t FB = (uint32_t)d.H * d.W * 3u;   // < 2^28: the image limits
    const uint8_t* src = d.src + f * FB;   // may be dst: no restrict
    uint8_t* dst = d.dst + f * FB;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head > FB) head = FB;
    const uint32_t pieces = (FB - head) / 16u, tail = FB - head - pieces * 16u;
    const OverlayStyle st = ov_frame_style(d, f);
    const bool src_aligned = (((uintptr_t)src + head) & 15u) == 0;
    const uint32_t stride = gridDim.x * OV_THREADS;
    for (uint32_t i0 = blockIdx.x * OV_THREADS + threadIdx.x; i0 < pieces; i0 += stride * OV_UNROLL) {
        uint32_t v[OV_UNROLL][4];
        OvSpan sp[OV_UNROLL];
#pragma unroll
        for (int u = 0; u < OV_UNROLL; ++u) {
            const uint32_t i = i0 + u * stride;
            if (i < pieces) {
                const uint32_t b0 = head + i * 16u;
                if (src_aligned) {
                    const uint4 q = *reinterpret_cast<const uint4*>(src + b0);
                    v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
                } else {
                    const OvPiece1 q = *reinterpret_cast<const OvPiece1*>(src + b0);
                    v[u][0] = q.w[0]; v[u][1] = q.w[1]; v[u][2] = q.w[2]; v[u][3] = q.w[3];
                }
                ov_locate(d, f, b0, 16, sp[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < OV_UNROLL; ++u)
            if (i0 + u * stride < pieces) ov_fetch_detail(d, sp[u]);
#pragma unroll
        for (int u = 0; u < OV_UNROLL; ++u) {
            const uint32_t i = i0 + u * stride;
            if (i < pieces) {
                ov_draw_piece(d, f, st, 16, sp[u], v[u]);
                *reinterpret_cast<uint4*>(dst + head + i * 16u) = make_uint4(v[u][0], v[u][1], v[u][2], v[u][3]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {   // the head (thread 0) and the tail: byte by byte
        const uint32_t b0 = threadIdx.x == 0 ? 0u : head + pieces * 16u;
        const int n = (int)(threadIdx.x == 0 ? head : tail);
        if (n > 0) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            for (int k = 0; k < n; ++k) v[k >> 2] |= (uint32_t)src[b0 + k] << (8 * (k & 3));
            OvSpan sp;
            ov_locate(d, f, b0, n, sp);
            ov_fetch_detail(d, sp);
            ov_draw_piece(d, f, st, n, sp, v);
            for (int k = 0; k < n; ++k) dst[b0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// zeroes the words the mark kernel set: one thread per ANY word of frames [0, frames)
__global__ __launch_bounds__(OV_THREADS) void overlay_clean_kernel(OvDev d, size_t words) {
    for (size_t w = (size_t)blockIdx.x * OV_THREADS + threadIdx.x; w < words; w += (size_t)gridDim.x * OV_THREADS) {
        if (d.any[w] == 0u) continue;
        d.any[w] = 0u;
        uint4* q = reinterpret_cast<uint4*>(d.detail + w * 8);
        q[0] = make_uint4(0u, 0u, 0u, 0u);
        q[1] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// the bird view: discs written in place.  One thread per ANY word: it alone writes the word's 32 pixels and zeroes the word
__global__ __launch_bounds__(OV_THREADS) void overlay_apply_kernel(OvDev d, size_t words) {
    const size_t per_frame = (size_t)d.H * d.rw;
    for (size_t w = (size_t)blockIdx.x * OV_THREADS + threadIdx.x; w < words; w += (size_t)gridDim.x * OV_THREADS) {
        const uint32_t a = d.any[w];
        if (a == 0u) continue;
        const size_t f = w / per_frame, r = w - f * per_frame;
        const int y = (int)(r / d.rw), x0 = (int)(r - (size_t)y * d.rw) * 32;
        const OverlayStyle st = ov_frame_style(d, f);
        uint4* q = reinterpret_cast<uint4*>(d.detail + w * 8);
        const uint4 lanes = q[0];
        uint8_t* row = d.dst + ((f * d.H + y) * (size_t)d.W) * 3;
        for (int b = 0; b < 32; ++b) {
            if (!((a >> b) & 1u) || x0 + b >= d.W) continue;
            const uint32_t m = 1u << b;
            const uint32_t bits = ((lanes.x & m) ? 1u : 0u) | ((lanes.y & m) ? 2u : 0u) | ((lanes.z & m) ? 4u : 0u) | ((lanes.w & m) ? 8u : 0u);
            if (!bits) continue;
            uint8_t* p = row + (size_t)(x0 + b) * 3;
            for (int c = 0; c < 3; ++c) p[c] = (uint8_t)overlay_pixel(0, bits, c, st);   // written, not blended: the old byte is not read
        }
        d.any[w] = 0u;
        q[0] = make_uint4(0u, 0u, 0u, 0u);
        q[1] = make_uint4(0u, 0u, 0u, 0u);
    }
}

}  // namespace

struct adas_overlay {
    adas_overlay_params p;
    int max_batch = 0;
    int rw = 0, bird_rw = 0;
    uint32_t *any = nullptr, *detail = nullptr;             // the frame's planes
    uint32_t *bird_any = nullptr, *bird_detail = nullptr;   // the bird view's
    int* flags = nullptr;                                   // [max_batch]
    uint8_t* d_dst = nullptr;                               // the handle's own [max_batch][src_h][src_w][3], allocated when first asked for
    int dst_frames = 0;                                     // frames [0, dst_frames) of d_dst have been written by some run
    int run_frames = 0;
    hipStream_t last = 0;
    size_t frame_bytes() const { return (size_t)p.src_h * p.src_w * 3; }
};

namespace adas {
int overlay_geometry(const ::adas_overlay* h, int* src_h, int* src_w, int* bird_h, int* bird_w, int* max_batch) {
    if (!h) return 0;
    *src_h = h->p.src_h; *src_w = h->p.src_w; *bird_h = h->p.bird_h; *bird_w = h->p.bird_w; *max_batch = h->max_batch;
    return 1;
}
}  // namespace adas

static int overlay_own_buffer(adas_overlay* h) {
    if (!h->d_dst) ADAS_HIP_TRY(hipMalloc((void**)&h->d_dst, h->frame_bytes() * h->max_batch));
    return ADAS_OK;
}

static int overlay_check_style(const adas_overlay_params* p, const char* who) {
    ADAS_REQUIRE(p->lane_radius >= 0 && p->lane_radius <= ADAS_OVERLAY_MAX_RADIUS && p->distance_radius >= 0 &&
                     p->distance_radius <= ADAS_OVERLAY_MAX_RADIUS && p->bird_radius >= 0 && p->bird_radius <= ADAS_OVERLAY_MAX_RADIUS,
                 ADAS_ERR_INVALID, "%s: radii must be in [0, %d] (got %d, %d, %d)", who, ADAS_OVERLAY_MAX_RADIUS, p->lane_radius, p->distance_radius,
                 p->bird_radius);
    ADAS_REQUIRE(p->lane_alpha >= 0.0 && p->lane_alpha <= 1.0 && p->area_alpha >= 0.0 && p->area_alpha <= 1.0, ADAS_ERR_INVALID,
                 "%s: alphas must be in [0, 1] (got %g, %g)", who, p->lane_alpha, p->area_alpha);
    return ADAS_OK;
}

static void overlay_style(const adas_overlay_params& p, int bird, OvStyle* s) {
    for (int l = 0; l < 4; ++l) s->lane[l] = overlay_pack_bgr(p.lane_colors[l]);
    for (int k = 0; k < 4; ++k) s->collision[k] = overlay_pack_bgr(p.collision_colors[k]);
    s->offset = overlay_pack_bgr(p.offset_color);
    s->area = overlay_pack_bgr(p.area_color);
    s->dist = overlay_pack_bgr(p.distance_color);
    s->lane_w = overlay_alpha(p.lane_alpha);
    s->area_w = overlay_alpha(p.area_alpha);
    s->r_lane = bird ? p.bird_radius : p.lane_radius;
    s->r_dist = p.distance_radius;
}

static int overlay_band(int rw) {   // rows whose OV_PLANES planes fit the LDS budget: 8 up to 5248 columns, 2 at 16384
    const int b = OV_LDS_WORDS / (OV_PLANES * rw);
    return b < 1 ? 1 : (b > OV_BAND ? OV_BAND : b);
}

static unsigned overlay_grid(size_t items) {
    const size_t b = (items + OV_THREADS - 1) / OV_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// the launches of one run; `s` holds the sources, bird_pts / bird_cnt (stride bird_cnt_stride) the bird view's
static int overlay_launch(adas_overlay* h, const uint8_t* src, uint8_t* dst, OvSources s, const int* bird_pts, const int* bird_cnt, int bird_cnt_stride,
                          uint8_t* d_bird, int stages, int frames, hipStream_t st) {
    const int frame_stages = stages & (ADAS_OVERLAY_LANES | ADAS_OVERLAY_AREA | ADAS_OVERLAY_DISTANCE);
    if (frame_stages) {
        if (!dst) {
            int rc = overlay_own_buffer(h);
            if (rc) return rc;
        }
        OvDev d;
        memset(&d, 0, sizeof(d));
        d.s = s;
        overlay_style(h->p, 0, &d.st);
        d.H = h->p.src_h; d.W = h->p.src_w; d.rw = h->rw;
        d.any = h->any; d.detail = h->detail; d.flags = h->flags;
        d.stages = frame_stages;
        d.src = src;
        d.dst = dst ? dst : h->d_dst;
        d.band = overlay_band(d.rw);
        hipLaunchKernelGGL(overlay_mark_kernel, dim3((unsigned)((d.H + d.band - 1) / d.band), (unsigned)frames), dim3(OV_THREADS),
                           ((size_t)OV_PLANES * d.band * d.rw + OV_LIST) * 4, st, d);
        ADAS_HIP_TRY(hipGetLastError());
        const size_t pieces = h->frame_bytes() / 16 + 2;
        unsigned gx = overlay_grid(pieces);
        const unsigned per = (unsigned)((2048 + frames - 1) / frames);   // about 2048 workgroups in all, grid-stride the rest
        if (gx > per) gx = per;
        hipLaunchKernelGGL(overlay_stream_kernel, dim3(gx, (unsigned)frames), dim3(OV_THREADS), 0, st, d);
        ADAS_HIP_TRY(hipGetLastError());
        const size_t words = (size_t)frames * d.H * d.rw;
        hipLaunchKernelGGL(overlay_clean_kernel, dim3(overlay_grid(words)), dim3(OV_THREADS), 0, st, d, words);
        ADAS_HIP_TRY(hipGetLastError());
        if (!dst && frames > h->dst_frames) h->dst_frames = frames;
        h->run_frames = frames;
    }
    if (stages & ADAS_OVERLAY_BIRD) {
        OvDev d;
        memset(&d, 0, sizeof(d));
        d.s.lane_pts = bird_pts;
        d.s.lane_cnt = bird_cnt;
        d.s.lane_cnt_stride = bird_cnt_stride;
        d.s.offset_type = s.offset_type;
        d.s.offset_stride = s.offset_stride;
        overlay_style(h->p, 1, &d.st);
        d.H = h->p.bird_h; d.W = h->p.bird_w; d.rw = h->bird_rw;
        d.any = h->bird_any; d.detail = h->bird_detail; d.flags = nullptr;
        d.stages = ADAS_OVERLAY_LANES;
        d.direct = 1;
        d.dst = d_bird;
        d.band = overlay_band(d.rw);
        hipLaunchKernelGGL(overlay_mark_kernel, dim3((unsigned)((d.H + d.band - 1) / d.band), (unsigned)frames), dim3(OV_THREADS),
                           ((size_t)OV_PLANES * d.band * d.rw + OV_LIST) * 4, st, d);
        ADAS_HIP_TRY(hipGetLastError());
        const size_t words = (size_t)frames * d.H * d.rw;
        hipLaunchKernelGGL(overlay_apply_kernel, dim3(overlay_grid(words)), dim3(OV_THREADS), 0, st, d, words);
        ADAS_HIP_TRY(hipGetLastError());
    }
    h->last = st;
    return ADAS_OK;
}

#define OV_RUN_REQUIRE(name, frames)                                                                                                          \
    ADAS_REQUIRE(h && (frames) > 0 && (frames) <= h->max_batch, ADAS_ERR_INVALID, name ": bad argument (%d frames, the handle holds %d)", (int)(frames), \
                 h ? h->max_batch : 0);                                                                                                       \
    ADAS_REQUIRE(!(stages & ~15), ADAS_ERR_INVALID, name ": unknown stage bits 0x%x", stages);                                                \
    ADAS_REQUIRE(!(stages & 7) || d_src_bgr, ADAS_ERR_INVALID, name ": the frame stages need source frames");                                 \
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_BIRD) || (h->p.bird_h > 0 && d_bird_bgr), ADAS_ERR_INVALID,                                          \
                 name ": the bird stage needs a handle created with a bird-view size and a bird-view image")

extern "C" {

int adas_overlay_default_params(adas_overlay_params* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_overlay_default_params: null argument");
    memset(p, 0, sizeof(*p));
    p->lane_radius = 3; p->distance_radius = 4; p->bird_radius = 10;
    p->lane_alpha = 0.3; p->area_alpha = 0.85;
    const uint8_t lanes[4][3] = {{255, 0, 0}, {46, 139, 87}, {50, 205, 50}, {0, 255, 255}};
    const uint8_t coll[4][3] = {{0, 255, 255}, {0, 255, 0}, {0, 102, 255}, {0, 0, 255}};
    memcpy(p->lane_colors, lanes, 12);
    memcpy(p->collision_colors, coll, 12);
    p->offset_color[0] = 0; p->offset_color[1] = 0; p->offset_color[2] = 255;
    p->area_color[0] = 255; p->area_color[1] = 191; p->area_color[2] = 0;
    p->distance_color[0] = p->distance_color[1] = p->distance_color[2] = 255;
    return ADAS_OK;
}

int adas_overlay_create(const adas_overlay_params* p, int max_batch, adas_overlay** out) {
    ADAS_REQUIRE(p && out && max_batch > 0 && max_batch <= 65535, ADAS_ERR_INVALID, "adas_overlay_create: bad argument");
    ADAS_REQUIRE(p->src_h > 0 && p->src_h <= 4320 && p->src_w > 0 && p->src_w <= 16384, ADAS_ERR_INVALID,
                 "adas_overlay_create: frames must be 1..4320 rows by 1..16384 columns (got %dx%d)", p->src_h, p->src_w);
    ADAS_REQUIRE((p->bird_h == 0 && p->bird_w == 0) || (p->bird_h > 0 && p->bird_h <= 4320 && p->bird_w > 0 && p->bird_w <= 16384), ADAS_ERR_INVALID,
                 "adas_overlay_create: the bird view must be 0x0 (none) or 1..4320 rows by 1..16384 columns (got %dx%d)", p->bird_h, p->bird_w);
    int rc = overlay_check_style(p, "adas_overlay_create");
    if (rc) return rc;
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    adas_overlay* h = new (std::nothrow) adas_overlay();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->p = *p;
    h->max_batch = max_batch;
    h->rw = (p->src_w + 31) / 32;
    h->bird_rw = (p->bird_w + 31) / 32;
    const size_t B = max_batch, words = B * p->src_h * h->rw, bwords = B * p->bird_h * h->bird_rw;
    hipError_t e = hipMalloc((void**)&h->detail, words * 32);
    if (e == hipSuccess) e = hipMalloc((void**)&h->any, words * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->flags, B * 4);
    if (e == hipSuccess && bwords) e = hipMalloc((void**)&h->bird_detail, bwords * 32);
    if (e == hipSuccess && bwords) e = hipMalloc((void**)&h->bird_any, bwords * 4);
    if (e == hipSuccess) e = hipMemset(h->detail, 0, words * 32);   // the planes are zero between runs
    if (e == hipSuccess) e = hipMemset(h->any, 0, words * 4);
    if (e == hipSuccess) e = hipMemset(h->flags, 0, B * 4);
    if (e == hipSuccess && bwords) e = hipMemset(h->bird_detail, 0, bwords * 32);
    if (e == hipSuccess && bwords) e = hipMemset(h->bird_any, 0, bwords * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        adas_overlay_destroy(h);
        return hip_fail(e, "hipMalloc(overlay planes)", __FILE__, __LINE__);
    }
    *out = h;
    return ADAS_OK;
}

int adas_overlay_destroy(adas_overlay* h) {
    if (!h) return ADAS_OK;
    for (void* q : {(void*)h->any, (void*)h->detail, (void*)h->bird_any, (void*)h->bird_detail, (void*)h->flags, (void*)h->d_dst})
        if (q) (void)hipFree(q);
    delete h;
    return ADAS_OK;
}

int adas_overlay_set_style(adas_overlay* h, const adas_overlay_params* p) {
    ADAS_REQUIRE(h && p, ADAS_ERR_INVALID, "adas_overlay_set_style: bad argument");
    int rc = overlay_check_style(p, "adas_overlay_set_style");
    if (rc) return rc;
    adas_overlay_params n = *p;
    n.src_h = h->p.src_h; n.src_w = h->p.src_w; n.bird_h = h->p.bird_h; n.bird_w = h->p.bird_w;
    h->p = n;
    adas::bump_config_generation();   // a captured step holds the old style in its kernel arguments
    return ADAS_OK;
}

int adas_overlay_run(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode, adas_lane_geometry* geometry,
                     adas_analysis* analysis, uint8_t* d_bird_bgr, int stages, int n_streams, int n_frames, void* stream) {
    ADAS_REQUIRE(n_streams > 0 && n_frames > 0, ADAS_ERR_INVALID, "adas_overlay_run: bad argument (%d streams x %d frames)", n_streams, n_frames);
    const long long frames = (long long)n_streams * n_frames;
    OV_RUN_REQUIRE("adas_overlay_run", frames);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_LANES) || decode, ADAS_ERR_INVALID, "adas_overlay_run: the lane stage needs a decode handle");
    ADAS_REQUIRE(!decode || adas::decode_num_lanes(decode) == 4, ADAS_ERR_INVALID,
                 "adas_overlay_run: the decoder has num_lanes = %d (CurveLanes); the overlay draws the reference's four lane colours, num_lanes must be 4",
                 adas::decode_num_lanes(decode));
    ADAS_REQUIRE(!(stages & (ADAS_OVERLAY_AREA | ADAS_OVERLAY_BIRD)) || geometry, ADAS_ERR_INVALID,
                 "adas_overlay_run: the area and bird stages need a geometry handle");
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DISTANCE) || analysis, ADAS_ERR_INVALID, "adas_overlay_run: the distance stage needs an analysis handle");
    ADAS_REQUIRE((!decode || frames <= adas::handle_max_batch(decode)) && (!geometry || frames <= adas::handle_max_batch(geometry)), ADAS_ERR_INVALID,
                 "adas_overlay_run: %d frames, the decode handle holds %d, the geometry handle %d", (int)frames, adas::handle_max_batch(decode),
                 adas::handle_max_batch(geometry));
    int af = 0;
    ADAS_REQUIRE(!analysis || (adas::analysis_capacity(analysis, nullptr, &af) && frames <= af), ADAS_ERR_INVALID,
                 "adas_overlay_run: %d frames, the analysis handle holds %d", (int)frames, af);
    OvSources s;
    memset(&s, 0, sizeof(s));
    if (decode) {
        const int *cnt, *det, *pts;
        adas::decode_lane_views(decode, &cnt, &det, &pts);
        s.lane_pts = pts; s.lane_cnt = cnt; s.lane_cnt_stride = 4;
    }
    const int* bird_pts = nullptr;
    const int* bird_cnt = nullptr;
    if (geometry) {
        const int32_t *hdr = nullptr, *area = nullptr;
        const double* vals = nullptr;
        int32_t area_stride = 0;
        int rc = adas_lane_geometry_device_views(geometry, &hdr, &vals, &area, &area_stride);
        if (rc) return rc;
        s.poly = area; s.poly_stride = (size_t)area_stride; s.poly_max = area_stride / 2;
        s.poly_n0 = hdr + 1; s.poly_n1 = hdr + 2; s.poly_n_stride = 8;   // area_points = the left points, then the reversed right points
        s.area_on = hdr; s.area_on_stride = 8;
        bird_pts = adas::geometry_bird_points(geometry);
        bird_cnt = hdr + 4;
    }
    if (analysis) {
        const int *fr, *pts;
        int stride = 0, maxp = 0;
        adas::analysis_frame_views(analysis, &fr, &stride, &pts, &maxp);
        s.offset_type = fr + offsetof(adas_analysis_frame, offset_msg) / 4; s.offset_stride = stride;
        s.collision = fr + offsetof(adas_analysis_frame, collision_msg) / 4; s.collision_stride = stride;
        s.dist_pts = pts; s.dist_cap = maxp;
        s.dist_cnt = fr + offsetof(adas_analysis_frame, n_points) / 4; s.dist_cnt_stride = stride;
    }
    return overlay_launch(h, d_src_bgr, d_dst_bgr, s, bird_pts, bird_cnt, 8, d_bird_bgr, stages, (int)frames, (hipStream_t)stream);
}

int adas_overlay_run_arrays(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const int32_t* d_lane_points, const int32_t* d_lane_counts,
                            const int32_t* d_poly, int poly_cap, const int32_t* d_poly_counts, const int32_t* d_area_status,
                            const int32_t* d_offset_type, const uint8_t* d_area_bgr, const int32_t* d_dist_points, int dist_cap,
                            const int32_t* d_dist_counts, const int32_t* d_bird_points, const int32_t* d_bird_counts, uint8_t* d_bird_bgr, int stages,
                            int n_frames, void* stream) {
    OV_RUN_REQUIRE("adas_overlay_run_arrays", n_frames);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_LANES) || (d_lane_points && d_lane_counts), ADAS_ERR_INVALID,
                 "adas_overlay_run_arrays: the lane stage needs lane points and counts");
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_AREA) || (d_poly && poly_cap > 0 && d_poly_counts && d_area_status), ADAS_ERR_INVALID,
                 "adas_overlay_run_arrays: the area stage needs a polygon, its counts and the area flags");
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DISTANCE) || (d_dist_points && dist_cap > 0 && d_dist_counts), ADAS_ERR_INVALID,
                 "adas_overlay_run_arrays: the distance stage needs distance points and counts");
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_BIRD) || (d_bird_points && d_bird_counts), ADAS_ERR_INVALID,
                 "adas_overlay_run_arrays: the bird stage needs bird points and counts");
    OvSources s;
    memset(&s, 0, sizeof(s));
    s.lane_pts = d_lane_points; s.lane_cnt = d_lane_counts; s.lane_cnt_stride = 4;
    s.poly = d_poly; s.poly_stride = (size_t)(poly_cap > 0 ? poly_cap : 0) * 2; s.poly_max = poly_cap > 0 ? poly_cap : 0;
    s.poly_n0 = d_poly_counts; s.poly_n1 = nullptr; s.poly_n_stride = 1;
    s.area_on = d_area_status; s.area_on_stride = 1;
    s.offset_type = d_offset_type; s.offset_stride = 1;
    s.area_bgr = d_area_bgr;
    s.dist_pts = d_dist_points; s.dist_cap = dist_cap > 0 ? dist_cap : 0;
    s.dist_cnt = d_dist_counts; s.dist_cnt_stride = 1;
    if (!(stages & ADAS_OVERLAY_AREA)) s.poly = nullptr;
    return overlay_launch(h, d_src_bgr, d_dst_bgr, s, d_bird_points, d_bird_counts, 4, d_bird_bgr, stages, n_frames, (hipStream_t)stream);
}

int adas_overlay_fetch(adas_overlay* h, int frame, uint8_t* h_bgr) {
    ADAS_REQUIRE(h && h_bgr && frame >= 0 && frame < h->max_batch, ADAS_ERR_INVALID, "adas_overlay_fetch: bad argument");
    ADAS_REQUIRE(frame < h->dst_frames, ADAS_ERR_INVALID,
                 "adas_overlay_fetch: frame %d of the handle's own buffer was never written (largest batch run into it: %d)", frame, h->dst_frames);
    ADAS_HIP_TRY(hipMemcpyAsync(h_bgr, h->d_dst + (size_t)frame * h->frame_bytes(), h->frame_bytes(), hipMemcpyDeviceToHost, h->last));
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    return ADAS_OK;
}

int adas_overlay_device_view(adas_overlay* h, const uint8_t** d_bgr) {
    ADAS_REQUIRE(h && d_bgr, ADAS_ERR_INVALID, "adas_overlay_device_view: bad argument");
    int rc = overlay_own_buffer(h);
    if (rc) return rc;
    *d_bgr = h->d_dst;
    return ADAS_OK;
}

int adas_overlay_fetch_flags(adas_overlay* h, int frame, int32_t* flags) {
    ADAS_REQUIRE(h && flags && frame >= 0 && frame < h->max_batch, ADAS_ERR_INVALID, "adas_overlay_fetch_flags: bad argument");
    ADAS_REQUIRE(frame < h->run_frames, ADAS_ERR_INVALID, "adas_overlay_fetch_flags: frame %d was not part of the last run (%d frames)", frame,
                 h->run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(flags, h->flags + frame, 4, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

}  // extern "C"
