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
// The object layer (ADAS_OVERLAY_DETECTIONS / ADAS_OVERLAY_TRACKS: cornerRect's outline and arms, plot_bbox's outline and tint, rules D6-D9)
// carries a colour per box, which bit planes cannot: overlay_objects_kernel first turns the survivors and the live tracks into one 48-byte
// record per box ([frames][det_cap + trk_cap] slots, order kept, a filtered track an empty record), the mark kernel ORs every record's runs
// into the two spare detail planes ("some detection draws here", "some track draws or tints here"), and in the streaming pass a 16-byte
// piece with such a pixel walks the frame's records once, in order (the first OV_OBJ_LDS staged in LDS, a longer list goes on from HBM --
// nothing is truncated; a record whose box misses the piece's marked pixels is skipped) and evaluates the thick segments in closed form
// for each marked pixel.  A piece without those bits takes the path it took before; with both stages off the pass is
// overlay_stream_kernel, which holds no object code (with the layer: overlay_stream_objects_kernel), and the record kernel is not launched.
// The trajectories stage (ADAS_OVERLAY_TRAJECTORIES, rules D10-D12 of overlay_track_core.h) adds two launches of its own:
// overlay_track_prims_kernel turns every drawn track into its circles and its rectangle or arrows, and overlay_tracks_draw_kernel, behind
// the streaming pass, lists per band of rows the primitives that meet it, builds their coverage in LDS and writes the covered pixels.
// Host side a run is described once: the six public run entry points are a name and a stage mask over adas::overlay_run_handles (sources
// read from the other handles; the pipeline's step calls it too) or overlay_run_raw (an adas_overlay_arrays).  Both check their arguments and
// fill one OvRun -- the tracker's rows through one OvRows view -- for overlay_launch, the only place that launches.
// Memory-bound by design: the yardstick is a device-to-device copy of the same frames (tools/bench_overlay.py).
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <initializer_list>
#include <new>
#include "overlay_core.h"
#include "overlay_track_core.h"

using namespace adas;

static_assert(sizeof(adas_overlay_params) == 88 && offsetof(adas_overlay_params, lane_alpha) == 32, "adas_overlay_params layout");

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_BAND = 8;          // rows of a mark workgroup (fewer for very wide images: the band's planes live in LDS)
constexpr int OV_PLANES = 7;        // LDS planes of a band: lanes 0..3, area, distance, toggles
constexpr int OV_LIST = 2048;       // polygon edges listed per pass
constexpr int OV_LDS_WORDS = 9216;  // LDS budget of the planes: 36 KB (+ 8 KB of edge list: under the 48 KB a launch may ask for)
constexpr int OV_MAXPTS = ADAS_UFLD_MAX_POINTS;
constexpr int OV_OBJ_STAGES = ADAS_OVERLAY_DETECTIONS | ADAS_OVERLAY_TRACKS;
constexpr int OV_OBJ_PLANES = 9;    // with the object layer: + detections (plane 7), tracks (plane 8)
constexpr int OV_OBJ_LDS = 384;     // records the streaming pass stages in LDS (18 KB); a longer list goes on from HBM
constexpr int OV_OBJ_WAVES = 4;     // waves per SIMD the streaming pass with the object layer is compiled for
constexpr int OV_HW = 68;           // ints of one half-width table in LDS (ADAS_OVERLAY_MAX_RADIUS + 1, rounded up to 16 bytes)
static_assert(sizeof(OverlayObject) == 48, "OverlayObject is copied as three uint4");

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

struct OvObjects {                  // the boxes one run reads, per frame q (null / 0 with its stage off)
    const int* det_xyxy;            // [q][det_cap][4]
    const int* det_cls;             // [q][det_cap]
    const int* det_cnt;             // det_cnt[q * det_cnt_stride]
    int det_cap, det_cnt_stride;
    const unsigned char* trk_tlwh;  // row k of frame q: 4 doubles at trk_tlwh + q * trk_frame_bytes + k * trk_row_bytes
    const unsigned char* trk_cls;   // its class, an int at trk_cls + q * trk_cls_frame_bytes + k * trk_cls_row_bytes
    const unsigned char* trk_act;   // its is_activated, an int at the strides of trk_tlwh, or null: every row is
    const unsigned char* trk_cnt;   // rows of frame q: an int at trk_cnt + q * trk_cnt_bytes
    size_t trk_frame_bytes, trk_row_bytes, trk_cls_frame_bytes, trk_cls_row_bytes, trk_cnt_bytes;
    int trk_cap;
    const uint32_t *det_colors, *trk_colors;   // packed class colours
    int n_det_colors, n_trk_colors;
    double min_box_area;
    int radii;                      // overlay_obj_radii of the three thicknesses
    OverlayObject* recs;            // [q][det_cap + trk_cap]: detections in their slots, tracks behind det_cap
    int* rec_cnt;                   // [q][2]: detections, track rows
    int lds_recs;                   // records of a frame the streaming pass stages in LDS
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
    int stages;                     // ADAS_OVERLAY_LANES | AREA | DISTANCE | DETECTIONS | TRACKS of this launch
    int direct;                     // lanes are written, not blended (the bird view)
    const uint8_t* src;
    uint8_t* dst;
};

struct OvDevObj : OvDev {          // what the kernels of a run with the object layer take; the others take the OvDev they always took
    OvObjects o;
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

__device__ __forceinline__ OverlayObjStyle ov_obj_style(const OvDevObj& d, const int* hw) {   // hw: [3][OV_HW]
    OverlayObjStyle s;
    s.radii = d.o.radii;
    s.hw = hw;
    s.hw_stride = OV_HW;
    return s;
}
__device__ __forceinline__ void ov_obj_halfwidths(const OvDevObj& d, int which, int* hw) {
    overlay_disc_halfwidths((d.o.radii >> (8 * which)) & 0xff, hw + which * OV_HW);
}

// grid (frames): one record per box of the frame.  Only the records' bounds need the radii, not the half-widths.
__global__ __launch_bounds__(OV_THREADS) void overlay_objects_kernel(OvDevObj d) {
    const size_t f = blockIdx.x;
    const int slots = d.o.det_cap + d.o.trk_cap;
    OverlayObject* recs = d.o.recs + f * slots;
    const OverlayObjStyle s = ov_obj_style(d, nullptr);
    int nd = 0, nt = 0;
    if (d.stages & ADAS_OVERLAY_DETECTIONS) nd = ov_clampi(d.o.det_cnt[f * d.o.det_cnt_stride], 0, d.o.det_cap);
    if (d.stages & ADAS_OVERLAY_TRACKS) nt = ov_clampi(*(const int*)(d.o.trk_cnt + f * d.o.trk_cnt_bytes), 0, d.o.trk_cap);
    for (int i = threadIdx.x; i < nd; i += OV_THREADS) {
        const size_t r = f * d.o.det_cap + i;
        recs[i] = overlay_make_detection(d.o.det_xyxy + r * 4, overlay_class_colour(d.o.det_cls[r], d.o.det_colors, d.o.n_det_colors), s, d.W, d.H);
    }
    for (int k = threadIdx.x; k < nt; k += OV_THREADS) {
        const size_t at = f * d.o.trk_frame_bytes + k * d.o.trk_row_bytes;
        const int act = d.o.trk_act ? *(const int*)(d.o.trk_act + at) : 1;
        const int cls = *(const int*)(d.o.trk_cls + f * d.o.trk_cls_frame_bytes + k * d.o.trk_cls_row_bytes);
        recs[d.o.det_cap + k] = overlay_make_track((const double*)(d.o.trk_tlwh + at), act, d.o.min_box_area,
                                                   overlay_class_colour(cls, d.o.trk_colors, d.o.n_trk_colors), s, d.W, d.H);
    }
    if (threadIdx.x == 0) {
        d.o.rec_cnt[2 * f] = nd;
        d.o.rec_cnt[2 * f + 1] = nt;
    }
}

// grid (ceil(H / band), frames); dynamic LDS: nplanes * band * rw words + OV_LIST ints (+ 3 * OV_HW ints with the object layer).  One workgroup owns rows [y0, y0 + band) of one
// frame: it builds their coverage in LDS and stores the words that are not zero (the planes are zero between runs).
// OBJ: the kernel of a run with the object layer (two more planes, the boxes' runs).  Without it no object code is compiled in and the plane
// count is the constant it was: a run with both stages off, and the bird view's, execute the code they executed before the layer existed.
template <bool OBJ, class DEV>
__device__ __forceinline__ void overlay_mark_body(const DEV& d) {
    constexpr int NPLANES = OBJ ? OV_OBJ_PLANES : OV_PLANES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int hw[2][ADAS_OVERLAY_MAX_RADIUS + 1];
    __shared__ int bad, listed;
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x;
    const int band = d.band, rw = d.rw, per = band * rw;
    constexpr bool objs = OBJ;
    uint32_t* planes = (uint32_t*)smem;                 // [nplanes][band][rw]: lanes 0..3, area (edges, then the whole fill), distance, toggles,
                                                        // and with the object layer detections, tracks
    int* list = (int*)(planes + NPLANES * per);         // [OV_LIST] edges that meet the band
    int* ohw = list + OV_LIST;                          // [3][OV_HW], with the object layer only: the static LDS stays what it was without it
    const int y0 = blockIdx.x * band;
    const int rows = d.H - y0 < band ? d.H - y0 : band;
    for (int i = tid; i < NPLANES * per; i += OV_THREADS) planes[i] = 0u;
    if (tid < 2) overlay_disc_halfwidths(tid == 0 ? d.st.r_lane : d.st.r_dist, hw[tid]);
    else if constexpr (OBJ) {
        if (tid < 5) ov_obj_halfwidths(d, tid - 2, ohw);
    }
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
    if constexpr (OBJ) {   // ---- boxes: every (record, row) pair ORs the runs of the record's segments on the row, and a track its tint region's
        const OverlayObjStyle os = ov_obj_style(d, ohw);
        const int nd = d.o.rec_cnt[2 * f], nt = d.o.rec_cnt[2 * f + 1];
        const OverlayObject* recs = d.o.recs + f * (d.o.det_cap + d.o.trk_cap);
        for (int t = tid; t < (nd + nt) * rows; t += OV_THREADS) {
            const int i = t / rows, r = t - i * rows, y = y0 + r;
            const OverlayObject o = recs[i < nd ? i : d.o.det_cap + (i - nd)];
            if (y < o.by0 || y > o.by1) continue;   // an empty box (nothing inside the image, or a filtered track) fails this
            uint32_t* roww = planes + (o.kind == OV_OBJ_DET ? 7 : 8) * per + r * rw;
            const int ns = overlay_object_segments(o);
            for (int k = 0; k < ns; ++k) {
                long long ax, ay, bx, by, xl, xr;
                const int* shw;
                const int R = overlay_object_segment(o, k, os, &ax, &ay, &bx, &by, &shw);
                if (!overlay_seg_row(ax, ay, bx, by, R, shw, y, &xl, &xr)) continue;
                if (xl < 0) xl = 0;
                if (xr > d.W - 1) xr = d.W - 1;
                if (xl <= xr) ov_lds_span(roww, (int)xl, (int)xr);
            }
            if (o.kind == OV_OBJ_TRACK && y >= o.y1 && y < o.y2 && o.x1 < o.x2) ov_lds_span(roww, o.x1, o.x2 - 1);   // 0 <= x1, x2 <= W: clamped
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
        const uint32_t de = objs ? planes[7 * per + i] : 0u, tr = objs ? planes[8 * per + i] : 0u;
        const uint32_t any = lo.x | lo.y | lo.z | lo.w | ar | di | de | tr;
        if (!any) continue;
        const size_t w = (f * d.H + y0) * (size_t)rw + i;
        uint4* q = reinterpret_cast<uint4*>(d.detail + w * 8);
        q[0] = lo;
        q[1] = make_uint4(ar, di, de, tr);
        d.any[w] = any;
    }
}

__global__ __launch_bounds__(OV_THREADS) void overlay_mark_kernel(OvDev d) { overlay_mark_body<false>(d); }
__global__ __launch_bounds__(OV_THREADS) void overlay_mark_objects_kernel(OvDevObj d) { overlay_mark_body<true>(d); }

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
    uint4 rest;       // area, distance, detections, tracks
};
// OBJ: the kernel of a run with the object layer.  Without it (OBJ = false) the two spare detail words are not read and no object code
// is compiled in: a run with both stages off executes the code it executed before the layer existed.
template <bool OBJ>
__device__ __forceinline__ uint32_t ov_bits(const OvDev& d, OvWord& c, size_t f, int y, int x) {
    const size_t w = (f * d.H + y) * (size_t)d.rw + (x >> 5);
    if (w != c.at) {
        c.at = w;
        c.any = d.any[w];
        if (c.any) {
            c.lanes = *reinterpret_cast<const uint4*>(d.detail + w * 8);
            if (OBJ) {
                c.rest = *reinterpret_cast<const uint4*>(d.detail + w * 8 + 4);
            } else {
                const uint2 r = *reinterpret_cast<const uint2*>(d.detail + w * 8 + 4);
                c.rest = make_uint4(r.x, r.y, 0u, 0u);
            }
        }
    }
    const uint32_t b = 1u << (x & 31);
    if (!(c.any & b)) return 0u;
    return ((c.lanes.x & b) ? 1u : 0u) | ((c.lanes.y & b) ? 2u : 0u) | ((c.lanes.z & b) ? 4u : 0u) | ((c.lanes.w & b) ? 8u : 0u) |
           ((c.rest.x & b) ? OV_BIT_AREA : 0u) | ((c.rest.y & b) ? OV_BIT_DIST : 0u) |
           (OBJ ? (((c.rest.z & b) ? OV_BIT_DET : 0u) | ((c.rest.w & b) ? OV_BIT_TRK : 0u)) : 0u);
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
template <bool OBJ>
__device__ __forceinline__ void ov_fetch_detail(const OvDev& d, OvSpan& s) {
    if (s.x1 >= 0 && s.w.any) {
        s.w.lanes = *reinterpret_cast<const uint4*>(d.detail + s.w.at * 8);
        if (OBJ) {
            s.w.rest = *reinterpret_cast<const uint4*>(d.detail + s.w.at * 8 + 4);
        } else {
            const uint2 r = *reinterpret_cast<const uint2*>(d.detail + s.w.at * 8 + 4);
            s.w.rest = make_uint4(r.x, r.y, 0u, 0u);
        }
    }
}

// the frame's records as the streaming pass sees them: the first `nlds` of the list in LDS, the rest in their slots in HBM
struct OvObjCtx {
    int nd, n;                      // detections, detections + track rows
    int nlds, det_cap;
    const OverlayObject* lds;
    const OverlayObject* slots;     // the frame's [det_cap + trk_cap]
    OverlayObjStyle s;
};
// byte k (0 .. 15) of a piece held as two 64-bit halves, k not known at compile time: shifts, not an indexed register array
__device__ __forceinline__ int ov_get_byte(unsigned long long lo, unsigned long long hi, int k) {
    return (int)(((k < 8 ? lo : hi) >> (8 * (k & 7))) & 0xffull);
}
__device__ __forceinline__ void ov_put_byte(unsigned long long& lo, unsigned long long& hi, int k, int b) {
    const unsigned long long m = 0xffull << (8 * (k & 7)), q = (unsigned long long)(unsigned)b << (8 * (k & 7));
    if (k < 8) lo = (lo & ~m) | q;
    else hi = (hi & ~m) | q;
}
// D9 on the pixels of a piece that carry an object bit (bit p of `om`: pixel p of the piece; pixel 0 is (s.x, s.y), whose channel s.c is
// byte 0).  The frame's records are walked once, in order: a record whose box misses the box of the piece's marked pixels is skipped, the
// others ask each marked pixel for its membership (once per pixel) and rewrite that pixel's bytes of the piece -- every pixel still
// sees the records in order.  One copy of the rules per piece: the loops are not unrolled.
__device__ __forceinline__ void ov_fold_piece(const OvDev& d, const OvObjCtx& oc, int n, const OvSpan& s, uint32_t om, uint32_t v[4]) {
    unsigned long long lo = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32), hi = (unsigned long long)v[2] | ((unsigned long long)v[3] << 32);
    int xa = d.W, xb = -1, ya = d.H, yb = -1;
    {
        int x = s.x, y = s.y;
        for (uint32_t m = om; m; m >>= 1) {
            if (m & 1u) {
                xa = x < xa ? x : xa; xb = x > xb ? x : xb;
                ya = y < ya ? y : ya; yb = y > yb ? y : yb;
            }
            if (++x == d.W) { x = 0; ++y; }
        }
    }
    for (int i = 0; i < oc.n; ++i) {
        const OverlayObject* o = i < oc.nlds ? oc.lds + i : oc.slots + (i < oc.nd ? i : oc.det_cap + (i - oc.nd));
        if (o->bx0 > xb || o->bx1 < xa || o->by0 > yb || o->by1 < ya) continue;
        int x = s.x, y = s.y, k0 = -s.c;   // k0: where the pixel's channel 0 lies in the piece (outside it for a pixel cut by the piece's ends)
        for (uint32_t m = om; m; m >>= 1, k0 += 3) {
            if (m & 1u) {
                const int ops = overlay_object_ops(*o, x, y, oc.s);
                if (ops) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (k0 + c >= 0 && k0 + c < n) ov_put_byte(lo, hi, k0 + c, overlay_object_channel(ov_get_byte(lo, hi, k0 + c), ops, o->colour, c));
                }
            }
            if (++x == d.W) { x = 0; ++y; }
        }
    }
    v[0] = (uint32_t)lo; v[1] = (uint32_t)(lo >> 32); v[2] = (uint32_t)hi; v[3] = (uint32_t)(hi >> 32);
}
// draws on the bytes held in v (byte k in bits 8 (k & 3) of v[k >> 2])
template <bool OBJ>
__device__ __forceinline__ void ov_draw_piece(const OvDev& d, size_t f, const OverlayStyle& st, const OvObjCtx& oc, int n, OvSpan& s, uint32_t v[4]) {
    if (s.quiet) return;
    int c = s.c, y = s.y, x = s.x;
    uint32_t bits = ov_bits<OBJ>(d, s.w, f, y, x);
    uint32_t om = 0u, pbit = 1u;   // the piece's pixels that carry an object bit and no distance disc (DISTANCE overrides everything)
    if (OBJ && (bits & (OV_BIT_DET | OV_BIT_TRK)) && !(bits & OV_BIT_DIST)) om = 1u;
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
                if (k + 1 < n) {
                    bits = ov_bits<OBJ>(d, s.w, f, y, x);
                    if (OBJ) {
                        pbit <<= 1;
                        if ((bits & (OV_BIT_DET | OV_BIT_TRK)) && !(bits & OV_BIT_DIST)) om |= pbit;
                    }
                }
            }
        }
    }
    if (OBJ && om) ov_fold_piece(d, oc, n, s, om, v);   // no pixel of the piece has an object bit: the path ends here, as before the layer
}

constexpr int OV_UNROLL = 4;   // pieces a thread has in flight: the pass is a chain of dependent loads (frame bytes, ANY word, detail words)

// grid (blocks, frames); a frame's 3HW bytes = a head of < 16 bytes up to the destination's first 16-byte boundary, aligned pieces, a tail
// dynamic LDS, only with the object layer (OBJ): three half-width tables, then the frame's first lds_recs records
template <bool OBJ, class DEV>
__device__ __forceinline__ void overlay_stream_body(const DEV& d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ov_smem[];
    const size_t f = blockIdx.y;
    OvObjCtx oc;
    oc.nd = oc.n = oc.nlds = 0;
    if constexpr (OBJ) {
        int* ohw = (int*)ov_smem;
        uint4* lrec = (uint4*)(ov_smem + 3 * OV_HW * 4);
        if (threadIdx.x < 3) ov_obj_halfwidths(d, threadIdx.x, ohw);
        oc.nd = d.o.rec_cnt[2 * f];
        oc.n = oc.nd + d.o.rec_cnt[2 * f + 1];
        oc.nlds = oc.n < d.o.lds_recs ? oc.n : d.o.lds_recs;
        oc.det_cap = d.o.det_cap;
        oc.slots = d.o.recs + f * (d.o.det_cap + d.o.trk_cap);
        oc.lds = (const OverlayObject*)lrec;
        oc.s = ov_obj_style(d, ohw);
        for (int t = threadIdx.x; t < oc.nlds * 3; t += OV_THREADS) {
            const int i = t / 3, q = t - i * 3;
            lrec[t] = reinterpret_cast<const uint4*>(oc.slots + (i < oc.nd ? i : oc.det_cap + (i - oc.nd)))[q];
        }
        __syncthreads();
    }
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
            if (i0 + u * stride < pieces) ov_fetch_detail<OBJ>(d, sp[u]);
#pragma unroll
        for (int u = 0; u < OV_UNROLL; ++u) {
            const uint32_t i = i0 + u * stride;
            if (i < pieces) {
                ov_draw_piece<OBJ>(d, f, st, oc, 16, sp[u], v[u]);
                *reinterpret_cast<uint4*>(dst + head + i * 16u) = make_uint4(v[u][0], v[u][1], v[u][2], v[u][3]);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {   // the head (thread 0) and the tail: byte by byte
        const uint32_t b0 = threadIdx.x == 0 ? 0u : head + pieces * 16u;
        const int n = (int)(threadIdx.x == 0 ? head : tail);
        if (n > 0) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (OBJ) {   // the larger kernel keeps an indexed v[] in scratch: go through 64-bit shifts instead
                unsigned long long lo = 0ull, hi = 0ull;
                for (int k = 0; k < n; ++k) ov_put_byte(lo, hi, k, src[b0 + k]);
                v[0] = (uint32_t)lo; v[1] = (uint32_t)(lo >> 32); v[2] = (uint32_t)hi; v[3] = (uint32_t)(hi >> 32);
            } else {
                for (int k = 0; k < n; ++k) v[k >> 2] |= (uint32_t)src[b0 + k] << (8 * (k & 3));
            }
            OvSpan sp;
            ov_locate(d, f, b0, n, sp);
            ov_fetch_detail<OBJ>(d, sp);
            ov_draw_piece<OBJ>(d, f, st, oc, n, sp, v);
            if (OBJ) {
                const unsigned long long lo = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32), hi = (unsigned long long)v[2] | ((unsigned long long)v[3] << 32);
                for (int k = 0; k < n; ++k) dst[b0 + k] = (uint8_t)ov_get_byte(lo, hi, k);
            } else {
                for (int k = 0; k < n; ++k) dst[b0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// Two kernels, so that each has its own launch bounds: the pass without the object layer keeps the bounds (and the code) it had before the
// layer existed; the pass with it is held to the 4 waves per SIMD of the other one.
__global__ __launch_bounds__(OV_THREADS) void overlay_stream_kernel(OvDev d) { overlay_stream_body<false>(d); }
__global__ __launch_bounds__(OV_THREADS, OV_OBJ_WAVES) void overlay_stream_objects_kernel(OvDevObj d) { overlay_stream_body<true>(d); }

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

// ---- the trajectories stage (ADAS_OVERLAY_TRAJECTORIES: plot_trajectories' circles, plot_directions' rectangle or arrows; rules D10-D12 of
// overlay_track_core.h).  A sparse pass of its own beside the streaming pass, which it does not touch:
//   overlay_track_prims_kernel   one lane per track row: the trajectory ring -> at most ADAS_OVERLAY_TRACK_PRIMS 64-byte primitives in the
//                                track's slots, and a 32-byte head (their number, the box around them)
//   overlay_tracks_draw_kernel   behind the streaming pass and ahead of the clean-up, one workgroup per band of rows: the primitives that meet
//                                the band are listed in LDS, every (listed primitive, row) pair ORs its runs into one more plane -- which
//                                lives in LDS only --, and every marked pixel without a distance disc takes the colour of the last
//                                primitive that hits it, folded through the later tracks' outline and tint when TRACKS is on (the fold of
//                                overlay_track_core.h: no earlier pixel value is needed, so the pass is legal in place).
constexpr int OV_TRK_LANES = 64;    // tracks of a workgroup of the primitive kernel
constexpr int OV_TRK_WORK = 2 * (ADAS_OVERLAY_TRACK_RING - 1);   // doubles of one track's direction list
constexpr int OV_TRK_LIST = OV_THREADS;   // slots of a frame's primitive list a band takes at a time, one per thread (their records: 16 KB of LDS)
static_assert(sizeof(OverlayPrim) == 64 && sizeof(OverlayTrackHead) == 32, "the primitive records' layout");

struct OvTracks {                   // the tracks one run reads, per frame q
    const unsigned char* tlwh;      // row k: 4 doubles at tlwh + q * frame_bytes + k * row_bytes
    const unsigned char* cls;       // an int at cls + q * cls_frame_bytes + k * cls_row_bytes
    const unsigned char* act;       // is_activated, an int at the strides of tlwh, or null: every row is
    const unsigned char* cnt;       // rows of frame q: an int at cnt + q * cnt_bytes
    size_t frame_bytes, row_bytes, cls_frame_bytes, cls_row_bytes, cnt_bytes;
    int trk_cap;
    // row k's trajectory: ring `slot` of frame q, 30 x 4 doubles at ring + q * ring_frame_bytes + slot * 960
    const unsigned char* ring;
    size_t ring_frame_bytes;
    const unsigned char* slot_ids;  // null: slot = k, the ring is stored oldest first; else the slot is the int at slot_ids + q * slot_frame_bytes + k * 4
    size_t slot_frame_bytes;
    const unsigned char* len;       // slot_ids null: len(trajectory), an int at len + q * len_frame_bytes + k * 4; else the boxes ever appended,
    size_t len_frame_bytes, len_row_bytes;   // an int at len + q * len_frame_bytes + slot * len_row_bytes (entry i of the list lives at i % 30)
};

struct OvTrkDev {
    OvTracks t;
    int H, W, rw, band;
    const uint32_t* colors;         // packed class colours of the tracks
    int n_colors;
    double min_box_area;
    int tab[2 * ADAS_OVERLAY_TRACK_RING];   // overlay_mark_table: radii, then thicknesses
    OverlayPrim* prims;             // [q][trk_cap][ADAS_OVERLAY_TRACK_PRIMS]
    OverlayTrackHead* heads;        // [q][trk_cap]
    int* cnt;                       // [q]: track rows
    const uint32_t* detail;         // the frame's detail planes: word 5 of a group is the distance discs'
    int* flags;
    const OverlayObject* objs;      // TRACKS on: frame q's track records at objs + q * obj_stride, row k at [k]; else null
    size_t obj_stride;
    int radii;                      // overlay_obj_radii of the object style
    uint8_t* dst;
};

__global__ __launch_bounds__(OV_TRK_LANES) void overlay_track_prims_kernel(OvTrkDev d) {
    __shared__ double work[OV_TRK_WORK * OV_TRK_LANES];   // element j of lane l at work[j * OV_TRK_LANES + l]
    __shared__ int tab[2 * ADAS_OVERLAY_TRACK_RING];
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x, k = blockIdx.x * OV_TRK_LANES + tid;
    if (tid < 2 * ADAS_OVERLAY_TRACK_RING) tab[tid] = d.tab[tid];
    __syncthreads();
    const int nt = ov_clampi(*(const int*)(d.t.cnt + f * d.t.cnt_bytes), 0, d.t.trk_cap);
    if (blockIdx.x == 0 && tid == 0) d.cnt[f] = nt;
    if (k >= nt) return;
    const size_t at = f * d.t.frame_bytes + k * d.t.row_bytes;
    const int act = d.t.act ? *(const int*)(d.t.act + at) : 1;
    const int cls = *(const int*)(d.t.cls + f * d.t.cls_frame_bytes + k * d.t.cls_row_bytes);
    int slot = k, len = 0, start = 0;
    if (d.t.slot_ids) {   // the tracker's rings: through the slot the message row names
        slot = *(const int*)(d.t.slot_ids + f * d.t.slot_frame_bytes + (size_t)k * 4);
        if (slot >= 0 && slot < d.t.trk_cap) {
            const int n = *(const int*)(d.t.len + f * d.t.len_frame_bytes + slot * d.t.len_row_bytes);
            len = ov_clampi(n, 0, ADAS_OVERLAY_TRACK_RING);
            start = n > len ? (n - len) % ADAS_OVERLAY_TRACK_RING : 0;
        } else {
            slot = 0;   // not a slot of the table: no trajectory
        }
    } else {
        len = ov_clampi(*(const int*)(d.t.len + f * d.t.len_frame_bytes + (size_t)k * 4), 0, ADAS_OVERLAY_TRACK_RING);
    }
    const double* ring = (const double*)(d.t.ring + f * d.t.ring_frame_bytes + (size_t)slot * (ADAS_OVERLAY_TRACK_RING * 32));
    OverlayPrim* out = d.prims + (f * d.t.trk_cap + k) * ADAS_OVERLAY_TRACK_PRIMS;
    int range = 0;
    const int n = overlay_track_prims((const double*)(d.t.tlwh + at), act, d.min_box_area, overlay_class_colour(cls, d.colors, d.n_colors), ring, start,
                                      len, tab, tab + ADAS_OVERLAY_TRACK_RING, d.W, d.H, work + tid, OV_TRK_LANES, out, &range);
    d.heads[f * d.t.trk_cap + k] = overlay_track_head(out, n, range);
}

struct LdsFillOps {   // overlay_prim_row on a band's LDS bitmap
    uint32_t* roww;
    __device__ void fill(int xl, int xr) { ov_lds_span(roww, xl, xr); }
};

// grid (ceil(H / band), frames); dynamic LDS: 2 * band * rw words.  One workgroup owns rows [y0, y0 + band) of one frame.  The frame's slots
// (track k, primitive i: slot k * ADAS_OVERLAY_TRACK_PRIMS + i, the drawing order) are taken OV_TRK_LIST at a time, one per thread, from the
// LAST to the first: the primitives of the chunk that meet the band are copied to LDS in slot order (a ballot and a prefix count: the list
// stays sorted), every (listed primitive, row) pair ORs its runs into the band's plane, and every marked pixel that no later chunk has
// drawn walks the list from its end: the first hit is the last primitive drawn there, and the pixel takes the fold of
// overlay_track_core.h from it unless a distance disc covers it.  Nothing is truncated: a longer list is more chunks.
__global__ __launch_bounds__(OV_THREADS) void overlay_tracks_draw_kernel(OvTrkDev d) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int hw[(ADAS_OVERLAY_TRACK_MAX_R + 1) * ADAS_OVERLAY_TRACK_HW];
    __shared__ int ohw[3 * OV_HW];
    __shared__ __attribute__((aligned(16))) OverlayPrim list[OV_TRK_LIST];
    __shared__ int lslot[OV_TRK_LIST];
    __shared__ int wcount[OV_THREADS / 64];
    const size_t f = blockIdx.y;
    const int tid = threadIdx.x, rw = d.rw, per = d.band * rw;
    uint32_t* plane = (uint32_t*)smem;   // [band][rw]: this chunk's coverage
    uint32_t* done = plane + per;        // [band][rw]: drawn by a later chunk
    const int y0 = blockIdx.x * d.band;
    const int rows = d.H - y0 < d.band ? d.H - y0 : d.band;
    for (int i = tid; i < per; i += OV_THREADS) done[i] = 0u;
    if (tid <= ADAS_OVERLAY_TRACK_MAX_R) overlay_track_halfwidths(tid, hw);
    else if (tid < ADAS_OVERLAY_TRACK_MAX_R + 4) {
        const int which = tid - ADAS_OVERLAY_TRACK_MAX_R - 1;
        overlay_disc_halfwidths((d.radii >> (8 * which)) & 0xff, ohw + which * OV_HW);
    }
    const int nt = d.cnt[f];
    const OverlayTrackHead* heads = d.heads + f * d.t.trk_cap;
    const OverlayPrim* prims = d.prims + f * d.t.trk_cap * ADAS_OVERLAY_TRACK_PRIMS;
    const OverlayObject* objs = d.objs ? d.objs + f * d.obj_stride : nullptr;
    if (blockIdx.x == 0 && tid == 0 && d.flags) {   // behind the coverage kernel, which stores the frame's other flags
        int range = 0;
        for (int k = 0; k < nt; ++k) range |= heads[k].range;
        if (range) d.flags[f] |= ADAS_OVERLAY_TRACK_RANGE;
    }
    const OverlayTrackStyle s{hw};
    OverlayObjStyle os;
    os.radii = d.radii; os.hw = ohw; os.hw_stride = OV_HW;
    for (int c1 = nt * ADAS_OVERLAY_TRACK_PRIMS; c1 > 0; c1 -= OV_TRK_LIST) {
        const int c0 = c1 > OV_TRK_LIST ? c1 - OV_TRK_LIST : 0;
        for (int i = tid; i < per; i += OV_THREADS) plane[i] = 0u;
        const int q = c0 + tid;   // this thread's slot
        bool meets = false;
        if (q < c1) {
            const int k = q / ADAS_OVERLAY_TRACK_PRIMS, i = q - k * ADAS_OVERLAY_TRACK_PRIMS;
            const OverlayTrackHead h = heads[k];
            if (i < h.n && h.y1 >= y0 && h.y0 < y0 + rows) {
                const OverlayPrim* p = prims + q;
                const int px0 = p->x0, py0 = p->y0, px1 = p->x1, py1 = p->y1;
                meets = px0 <= px1 && py1 >= y0 && py0 < y0 + rows;
            }
        }
        const unsigned long long bal = __ballot(meets);
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) wcount[wv] = __popcll(bal);
        __syncthreads();   // also: the tables, `done`, the plane, and the previous chunk's pixels
        int at = __popcll(bal & ((1ull << lane) - 1ull)), m = 0;
        for (int w = 0; w < OV_THREADS / 64; ++w) {
            if (w < wv) at += wcount[w];
            m += wcount[w];
        }
        if (meets) {
            const uint4* src = reinterpret_cast<const uint4*>(prims + q);
            uint4* dst = reinterpret_cast<uint4*>(list + at);
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
            lslot[at] = q;
        }
        __syncthreads();
        if (m > 0) {   // uniform
            for (int t = tid; t < m * rows; t += OV_THREADS) {
                const int e = t / rows, r = t - e * rows;
                LdsFillOps ops{plane + r * rw};
                overlay_prim_row(list[e], s, y0 + r, d.W, ops);
            }
            __syncthreads();
            for (int t = tid; t < rows * rw * 32; t += OV_THREADS) {   // one lane per pixel of the band
                const int wi = t >> 5, b = t & 31;
                if (!(((plane[wi] & ~done[wi]) >> b) & 1u)) continue;
                const int r = wi / rw, x = (wi - r * rw) * 32 + b, y = y0 + r;
                int e = m - 1;
                while (e >= 0 && !overlay_prim_hit(list[e], s, x, y)) --e;   // the list is in drawing order: the first hit from its end
                if (e < 0) continue;   // (the runs and the test agree: not expected)
                const int best = lslot[e];
                atomicOr(done + wi, 1u << b);
                const size_t gw = (f * d.H + y) * (size_t)rw + (wi - r * rw);
                if ((d.detail[gw * 8 + 5] >> b) & 1u) continue;   // DISTANCE overrides everything
                const uint32_t c = list[e].colour;
                int bgr[3] = {(int)(c & 0xffu), (int)((c >> 8) & 0xffu), (int)((c >> 16) & 0xffu)};
                if (objs)
                    for (int j = best / ADAS_OVERLAY_TRACK_PRIMS + 1; j < nt; ++j) {
                        const int ops = overlay_object_ops(objs[j], x, y, os);
                        if (!ops) continue;
                        for (int ch = 0; ch < 3; ++ch) bgr[ch] = overlay_object_channel(bgr[ch], ops, objs[j].colour, ch);
                    }
                uint8_t* px = d.dst + ((f * d.H + y) * (size_t)d.W + x) * 3;
                px[0] = (uint8_t)bgr[0]; px[1] = (uint8_t)bgr[1]; px[2] = (uint8_t)bgr[2];
            }
        }
        __syncthreads();
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
    // the object layer
    adas_overlay_object_style os;
    uint32_t* colors[2] = {nullptr, nullptr};               // packed class colours: [0] detections, [1] tracks
    int n_colors[2] = {0, 0};
    OverlayObject* recs = nullptr;                          // [max_batch][rec_slots]
    int rec_slots = 0;
    int* rec_cnt = nullptr;                                 // [max_batch][2]
    // the trajectories stage: allocated when first asked for (overlay_reserve_tracks)
    OverlayPrim* trj_prims = nullptr;                       // [max_batch][trj_cap][ADAS_OVERLAY_TRACK_PRIMS]
    OverlayTrackHead* trj_heads = nullptr;                  // [max_batch][trj_cap]
    int* trj_cnt = nullptr;                                 // [max_batch]
    int trj_cap = 0;
    int trj_run_cap = 0, trj_run_frames = 0;                // the last run with the stage: its trk_cap and frames (0: none yet)
    adas::overlay_panels* panels = nullptr;                 // the UI panels' state (overlay_panels.hip), after adas_overlay_set_panels
    adas::overlay_text* text = nullptr;                     // the text's state (overlay_text.hip), after the first adas_overlay_set_font / _set_text_*
    adas::overlay_readout* readout = nullptr;               // the bird view's readouts (overlay_readout.hip), after the first style or run with the stage
    size_t frame_bytes() const { return (size_t)p.src_h * p.src_w * 3; }
};

namespace adas {
int overlay_geometry(const ::adas_overlay* h, int* src_h, int* src_w, int* bird_h, int* bird_w, int* max_batch) {
    if (!h) return 0;
    *src_h = h->p.src_h; *src_w = h->p.src_w; *bird_h = h->p.bird_h; *bird_w = h->p.bird_w; *max_batch = h->max_batch;
    return 1;
}
overlay_panels** overlay_panel_slot(::adas_overlay* h) { return &h->panels; }
overlay_text** overlay_text_slot(::adas_overlay* h) { return &h->text; }
overlay_readout** overlay_readout_slot(::adas_overlay* h) { return &h->readout; }
void overlay_class_colors(const ::adas_overlay* h, int which, const uint32_t** table, int* n) { *table = h->colors[which]; *n = h->n_colors[which]; }
void overlay_note_stream(::adas_overlay* h, void* stream) { h->last = (hipStream_t)stream; }
}  // namespace adas

static int overlay_own_buffer(adas_overlay* h) {
    if (!h->d_dst) ADAS_HIP_TRY(hipMalloc((void**)&h->d_dst, h->frame_bytes() * h->max_batch));
    return ADAS_OK;
}

int adas::overlay_own_frames(adas_overlay* h, uint8_t** d_bgr, int* frames_written) {
    int rc = overlay_own_buffer(h);
    if (rc) return rc;
    *d_bgr = h->d_dst;
    *frames_written = h->dst_frames;
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

static int overlay_band(int rw, int nplanes) {   // rows whose planes fit the LDS budget: 8 up to 5248 columns, 2 at 16384 (OV_PLANES planes)
    const int b = OV_LDS_WORDS / (nplanes * rw);
    return b < 1 ? 1 : (b > OV_BAND ? OV_BAND : b);
}

static unsigned overlay_grid(size_t items) {
    const size_t b = (items + OV_THREADS - 1) / OV_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// room for `slots` records per frame.  Allocates: not inside a stream capture (adas_pipeline_set_overlay_stages reserves ahead of the step)
static int overlay_reserve_records(adas_overlay* h, int slots) {
    if (slots <= h->rec_slots) return ADAS_OK;
    ADAS_HIP_TRY(hipDeviceSynchronize());   // a run in flight may still read the old table
    if (h->recs) (void)hipFree(h->recs);
    h->recs = nullptr;
    h->rec_slots = 0;
    ADAS_HIP_TRY(hipMalloc((void**)&h->recs, (size_t)h->max_batch * slots * sizeof(OverlayObject)));
    h->rec_slots = slots;
    adas::bump_config_generation();   // a captured step holds the old table's address in its kernel arguments
    return ADAS_OK;
}

// room for the primitives of trk_cap tracks per frame.  Allocates: not inside a stream capture
static int overlay_reserve_tracks(adas_overlay* h, int trk_cap) {
    if (!h->trj_cnt) {
        int* cnt = nullptr;
        hipError_t e = hipMalloc((void**)&cnt, (size_t)h->max_batch * 4);
        if (e == hipSuccess) e = hipMemset(cnt, 0, (size_t)h->max_batch * 4);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            if (cnt) (void)hipFree(cnt);
            return hip_fail(e, "hipMalloc(overlay track counts)", __FILE__, __LINE__);
        }
        h->trj_cnt = cnt;
        adas::bump_config_generation();
    }
    if (trk_cap <= h->trj_cap) return ADAS_OK;
    ADAS_HIP_TRY(hipDeviceSynchronize());   // a run in flight may still read the old tables
    if (h->trj_prims) (void)hipFree(h->trj_prims);
    if (h->trj_heads) (void)hipFree(h->trj_heads);
    h->trj_prims = nullptr;
    h->trj_heads = nullptr;
    h->trj_cap = 0;
    h->trj_run_cap = h->trj_run_frames = 0;
    ADAS_HIP_TRY(hipMalloc((void**)&h->trj_prims, (size_t)h->max_batch * trk_cap * ADAS_OVERLAY_TRACK_PRIMS * sizeof(OverlayPrim)));
    ADAS_HIP_TRY(hipMalloc((void**)&h->trj_heads, (size_t)h->max_batch * trk_cap * sizeof(OverlayTrackHead)));
    h->trj_cap = trk_cap;
    adas::bump_config_generation();   // a captured step holds the old tables' addresses in its kernel arguments
    return ADAS_OK;
}

namespace adas {
int overlay_reserve_objects(::adas_overlay* h, int det_cap, int trk_cap) { return h ? overlay_reserve_records(h, det_cap + trk_cap) : ADAS_OK; }
int overlay_reserve_trajectories(::adas_overlay* h, int trk_cap) { return h ? overlay_reserve_tracks(h, trk_cap) : ADAS_OK; }
}  // namespace adas

static int overlay_check_object_style(const adas_overlay_object_style* p, const char* who) {
    ADAS_REQUIRE(p->det_rect_thickness >= 1 && p->det_rect_thickness <= ADAS_OVERLAY_MAX_THICKNESS && p->det_arm_thickness >= 1 &&
                     p->det_arm_thickness <= ADAS_OVERLAY_MAX_THICKNESS && p->track_thickness >= 1 && p->track_thickness <= ADAS_OVERLAY_MAX_THICKNESS,
                 ADAS_ERR_INVALID, "%s: thicknesses must be in [1, %d] (got %d, %d, %d)", who, ADAS_OVERLAY_MAX_THICKNESS, p->det_rect_thickness,
                 p->det_arm_thickness, p->track_thickness);
    ADAS_REQUIRE(p->min_box_area == p->min_box_area, ADAS_ERR_INVALID, "%s: min_box_area is not a number", who);
    return ADAS_OK;
}

// a tracker's rows as the tracks and the trajectories stage read them, per frame q: OvObjects::trk_* and the head of OvTracks hold a copy each
struct OvRows {
    const unsigned char *tlwh, *cls, *act, *cnt;   // act null: every row is activated
    size_t frame_bytes, row_bytes, cls_frame_bytes, cls_row_bytes, cnt_bytes;
    int cap;
};

// the live table of `tracker` (rows in the layout of adas_track); returns the streams it holds
static int overlay_rows_of_tracker(const adas_bytetrack* tracker, OvRows* r) {
    int ts = 0;
    adas::tracker_live_views(tracker, &r->cnt, &r->tlwh, &r->frame_bytes, &ts, &r->cap);
    r->cnt += offsetof(adas_track_header, n_tracked);
    r->cnt_bytes = r->cls_frame_bytes = r->frame_bytes;
    r->row_bytes = r->cls_row_bytes = sizeof(adas_track);
    r->cls = r->tlwh + offsetof(adas_track, class_id);
    r->act = r->tlwh + offsetof(adas_track, is_activated);
    return ts;
}

static void overlay_rows_of_arrays(const adas_overlay_arrays& a, OvRows* r) {
    r->tlwh = (const unsigned char*)a.d_trk_tlwh; r->frame_bytes = (size_t)a.trk_cap * 32; r->row_bytes = 32;
    r->cls = (const unsigned char*)a.d_trk_cls; r->cls_frame_bytes = (size_t)a.trk_cap * 4; r->cls_row_bytes = 4; r->act = nullptr;
    r->cnt = (const unsigned char*)a.d_trk_counts; r->cnt_bytes = 4; r->cap = a.trk_cap;
}

static void overlay_rows_to_objects(const OvRows& r, OvObjects* o) {
    o->trk_tlwh = r.tlwh; o->trk_cls = r.cls; o->trk_act = r.act; o->trk_cnt = r.cnt; o->trk_cap = r.cap;
    o->trk_frame_bytes = r.frame_bytes; o->trk_row_bytes = r.row_bytes; o->trk_cnt_bytes = r.cnt_bytes;
    o->trk_cls_frame_bytes = r.cls_frame_bytes; o->trk_cls_row_bytes = r.cls_row_bytes;
}

static void overlay_rows_to_tracks(const OvRows& r, OvTracks* t) {
    t->tlwh = r.tlwh; t->cls = r.cls; t->act = r.act; t->cnt = r.cnt; t->trk_cap = r.cap;
    t->frame_bytes = r.frame_bytes; t->row_bytes = r.row_bytes; t->cnt_bytes = r.cnt_bytes;
    t->cls_frame_bytes = r.cls_frame_bytes; t->cls_row_bytes = r.cls_row_bytes;
}

struct OvRun {                      // one run as overlay_launch takes it; what a stage that is off would read stays zero
    const uint8_t* src; uint8_t* dst;   // dst null: the handle's own buffer
    OvSources s;
    const int *bird_pts, *bird_cnt; // the bird view's lane points and counts, bird_cnt[q * bird_cnt_stride + l]
    int bird_cnt_stride;
    uint8_t* d_bird;
    OvObjects obj;                  // the boxes (stages 16 / 32)
    OvTracks trk;                   // the tracks (stage 128)
    adas::overlay_readout_sources ro;   // the readouts (stage 256)
    int stages, frames;
    hipStream_t st;
};

// the launches of one run
static int overlay_launch(adas_overlay* h, const OvRun& r) {
    const int stages = r.stages, frames = r.frames; const hipStream_t st = r.st;
    const int frame_stages = stages & (ADAS_OVERLAY_LANES | ADAS_OVERLAY_AREA | ADAS_OVERLAY_DISTANCE | OV_OBJ_STAGES);
    const bool traj = (stages & ADAS_OVERLAY_TRAJECTORIES) != 0;   // two launches of its own; without it neither, and nothing else changes
    if (frame_stages || traj) {
        if (!r.dst) {
            int rc = overlay_own_buffer(h);
            if (rc) return rc;
        }
        OvDevObj d;
        memset(&d, 0, sizeof(d));
        d.s = r.s;
        overlay_style(h->p, 0, &d.st);
        d.H = h->p.src_h; d.W = h->p.src_w; d.rw = h->rw;
        d.any = h->any; d.detail = h->detail; d.flags = h->flags;
        d.stages = frame_stages;
        d.src = r.src;
        d.dst = r.dst ? r.dst : h->d_dst;
        int nplanes = OV_PLANES;
        size_t stream_lds = 0;
        if (frame_stages & OV_OBJ_STAGES) {   // one more launch, ahead of the coverage: the boxes' records
            d.o = r.obj;
            if (!(frame_stages & ADAS_OVERLAY_DETECTIONS)) d.o.det_cap = 0;
            if (!(frame_stages & ADAS_OVERLAY_TRACKS)) d.o.trk_cap = 0;
            int rc = overlay_reserve_records(h, d.o.det_cap + d.o.trk_cap);
            if (rc) return rc;
            d.o.det_colors = h->colors[0]; d.o.n_det_colors = h->n_colors[0];
            d.o.trk_colors = h->colors[1]; d.o.n_trk_colors = h->n_colors[1];
            d.o.min_box_area = h->os.min_box_area;
            d.o.radii = overlay_obj_radii(h->os.det_rect_thickness, h->os.det_arm_thickness, h->os.track_thickness);
            d.o.recs = h->recs; d.o.rec_cnt = h->rec_cnt;
            d.o.lds_recs = d.o.det_cap + d.o.trk_cap < OV_OBJ_LDS ? d.o.det_cap + d.o.trk_cap : OV_OBJ_LDS;
            nplanes = OV_OBJ_PLANES;
            stream_lds = (size_t)3 * OV_HW * 4 + (size_t)d.o.lds_recs * sizeof(OverlayObject);
            hipLaunchKernelGGL(overlay_objects_kernel, dim3((unsigned)frames), dim3(OV_THREADS), 0, st, d);
            ADAS_HIP_TRY(hipGetLastError());
        }
        OvTrkDev td;
        if (traj) {   // the tracks' primitives, beside the boxes' records
            int rc = overlay_reserve_tracks(h, r.trk.trk_cap);
            if (rc) return rc;
            memset(&td, 0, sizeof(td));
            td.t = r.trk;
            td.H = d.H; td.W = d.W; td.rw = d.rw;
            td.band = overlay_band(d.rw, 2);
            td.colors = h->colors[1]; td.n_colors = h->n_colors[1];
            td.min_box_area = h->os.min_box_area;
            overlay_mark_table(td.tab, td.tab + ADAS_OVERLAY_TRACK_RING);
            td.prims = h->trj_prims; td.heads = h->trj_heads; td.cnt = h->trj_cnt;
            td.detail = h->detail; td.flags = h->flags;
            if (frame_stages & ADAS_OVERLAY_TRACKS) {   // the later tracks' outline and tint fold over a primitive's colour
                td.objs = h->recs + d.o.det_cap;
                td.obj_stride = (size_t)d.o.det_cap + d.o.trk_cap;
            }
            td.radii = overlay_obj_radii(h->os.det_rect_thickness, h->os.det_arm_thickness, h->os.track_thickness);
            td.dst = d.dst;
            hipLaunchKernelGGL(overlay_track_prims_kernel, dim3((unsigned)((r.trk.trk_cap + OV_TRK_LANES - 1) / OV_TRK_LANES), (unsigned)frames),
                               dim3(OV_TRK_LANES), 0, st, td);
            ADAS_HIP_TRY(hipGetLastError());
            h->trj_run_cap = r.trk.trk_cap;
            h->trj_run_frames = frames;
        }
        d.band = overlay_band(d.rw, nplanes);
        const OvDev plain = d;   // the kernels without the object layer take the arguments they always took
        if (frame_stages & OV_OBJ_STAGES)
            hipLaunchKernelGGL(overlay_mark_objects_kernel, dim3((unsigned)((d.H + d.band - 1) / d.band), (unsigned)frames), dim3(OV_THREADS),
                               ((size_t)OV_OBJ_PLANES * d.band * d.rw + OV_LIST + 3 * OV_HW) * 4, st, d);
        else
            hipLaunchKernelGGL(overlay_mark_kernel, dim3((unsigned)((d.H + d.band - 1) / d.band), (unsigned)frames), dim3(OV_THREADS),
                               ((size_t)OV_PLANES * d.band * d.rw + OV_LIST) * 4, st, plain);
        ADAS_HIP_TRY(hipGetLastError());
        const size_t pieces = h->frame_bytes() / 16 + 2;
        unsigned gx = overlay_grid(pieces);
        const unsigned per = (unsigned)((2048 + frames - 1) / frames);   // about 2048 workgroups in all, grid-stride the rest
        if (gx > per) gx = per;
        if (frame_stages & OV_OBJ_STAGES) hipLaunchKernelGGL(overlay_stream_objects_kernel, dim3(gx, (unsigned)frames), dim3(OV_THREADS), stream_lds, st, d);
        else hipLaunchKernelGGL(overlay_stream_kernel, dim3(gx, (unsigned)frames), dim3(OV_THREADS), 0, st, plain);
        ADAS_HIP_TRY(hipGetLastError());
        const size_t words = (size_t)frames * d.H * d.rw;
        if (traj) {   // behind the streaming pass, whose bytes it overwrites, and ahead of the clean-up: it reads the distance discs' plane
            hipLaunchKernelGGL(overlay_tracks_draw_kernel, dim3((unsigned)((td.H + td.band - 1) / td.band), (unsigned)frames), dim3(OV_THREADS),
                               (size_t)2 * td.band * td.rw * 4, st, td);
            ADAS_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(overlay_clean_kernel, dim3(overlay_grid(words)), dim3(OV_THREADS), 0, st, plain, words);
        ADAS_HIP_TRY(hipGetLastError());
        if (!r.dst && frames > h->dst_frames) h->dst_frames = frames;
        h->run_frames = frames;
    }
    if (stages & ADAS_OVERLAY_READOUTS) {   // two launches of its own, ahead of the discs; without it neither
        int rc = adas::overlay_readout_launch(h, r.ro, r.d_bird, frames, (void*)st);
        if (rc) return rc;
    }
    if (stages & ADAS_OVERLAY_BIRD) {
        OvDev d;
        memset(&d, 0, sizeof(d));
        d.s.lane_pts = r.bird_pts;
        d.s.lane_cnt = r.bird_cnt;
        d.s.lane_cnt_stride = r.bird_cnt_stride;
        d.s.offset_type = r.s.offset_type;
        d.s.offset_stride = r.s.offset_stride;
        overlay_style(h->p, 1, &d.st);
        d.H = h->p.bird_h; d.W = h->p.bird_w; d.rw = h->bird_rw;
        d.any = h->bird_any; d.detail = h->bird_detail; d.flags = nullptr;
        d.stages = ADAS_OVERLAY_LANES;
        d.direct = 1;
        d.dst = r.d_bird;
        d.band = overlay_band(d.rw, OV_PLANES);
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

// what every run checks first.  who: the entry point's name; mask: the stage bits it accepts
static int overlay_check_run(const char* who, int mask, const adas_overlay* h, long long frames, int stages, const void* d_src_bgr, const void* d_bird_bgr) {
    ADAS_REQUIRE(h && frames > 0 && frames <= h->max_batch, ADAS_ERR_INVALID, "%s: bad argument (%d frames, the handle holds %d)", who, (int)frames,
                 h ? h->max_batch : 0);
    ADAS_REQUIRE(!(stages & ~mask), ADAS_ERR_INVALID, "%s: unknown stage bits 0x%x", who, stages);
    ADAS_REQUIRE(!(stages & mask & ~(ADAS_OVERLAY_BIRD | ADAS_OVERLAY_READOUTS)) || d_src_bgr, ADAS_ERR_INVALID, "%s: the frame stages need source frames", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_BIRD) || (h->p.bird_h > 0 && d_bird_bgr), ADAS_ERR_INVALID,
                 "%s: the bird stage needs a handle created with a bird-view size and a bird-view image", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_READOUTS) || (h->p.bird_h > 0 && d_bird_bgr), ADAS_ERR_INVALID,
                 "%s: the readouts stage needs a handle created with a bird-view size and a bird-view image", who);
    return ADAS_OK;
}

// every run from the handles' device arrays: the three adas_overlay_run* entry points and the pipeline's step are masks over it
int adas::overlay_run_handles(const char* who, int mask, adas_overlay* h, const adas::overlay_handles& a) {
    const int stages = a.stages, n_streams = a.n_streams, n_frames = a.n_frames;
    ADAS_REQUIRE(n_streams > 0 && n_frames > 0, ADAS_ERR_INVALID, "%s: bad argument (%d streams x %d frames)", who, n_streams, n_frames);
    const long long frames = (long long)n_streams * n_frames;
    int rc = overlay_check_run(who, mask, h, frames, stages, a.d_src_bgr, a.d_bird_bgr);
    if (rc) return rc;
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_LANES) || a.decode, ADAS_ERR_INVALID, "%s: the lane stage needs a decode handle", who);
    ADAS_REQUIRE(!a.decode || adas::decode_num_lanes(a.decode) == 4, ADAS_ERR_INVALID,
                 "%s: the decoder has num_lanes = %d (CurveLanes); the overlay draws the reference's four lane colours, num_lanes must be 4", who,
                 adas::decode_num_lanes(a.decode));
    ADAS_REQUIRE(!(stages & (ADAS_OVERLAY_AREA | ADAS_OVERLAY_BIRD)) || a.geometry, ADAS_ERR_INVALID, "%s: the area and bird stages need a geometry handle",
                 who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_READOUTS) || a.geometry, ADAS_ERR_INVALID,
                 "%s: the readouts stage needs a geometry handle (its direction, curvature, offset and veh_pos)", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DISTANCE) || a.analysis, ADAS_ERR_INVALID, "%s: the distance stage needs an analysis handle", who);
    ADAS_REQUIRE((!a.decode || frames <= adas::handle_max_batch(a.decode)) && (!a.geometry || frames <= adas::handle_max_batch(a.geometry)),
                 ADAS_ERR_INVALID, "%s: %d frames, the decode handle holds %d, the geometry handle %d", who, (int)frames, adas::handle_max_batch(a.decode),
                 adas::handle_max_batch(a.geometry));
    int af = 0;
    ADAS_REQUIRE(!a.analysis || (adas::analysis_capacity(a.analysis, nullptr, &af) && frames <= af), ADAS_ERR_INVALID,
                 "%s: %d frames, the analysis handle holds %d", who, (int)frames, af);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DETECTIONS) || a.post, ADAS_ERR_INVALID, "%s: the detections stage needs a yolo_post handle", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_TRACKS) || a.tracker, ADAS_ERR_INVALID, "%s: the tracks stage needs a bytetrack handle", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_TRAJECTORIES) || a.tracker, ADAS_ERR_INVALID, "%s: the trajectories stage needs a bytetrack handle", who);
    OvRun r = {};
    if (stages & ADAS_OVERLAY_DETECTIONS) {
        ADAS_REQUIRE(frames <= adas::handle_max_batch(a.post), ADAS_ERR_INVALID, "%s: %d frames, the yolo_post handle holds %d", who, (int)frames,
                     adas::handle_max_batch(a.post));
        const int* cnt = nullptr;
        adas::post_survivor_views(a.post, &r.obj.det_xyxy, &r.obj.det_cls, &cnt, &r.obj.det_cap);
        r.obj.det_cnt = cnt + 2; r.obj.det_cnt_stride = 4;   // counts[4]: n_found, n_candidates, n_keep, flags
    }
    if (stages & (ADAS_OVERLAY_TRACKS | ADAS_OVERLAY_TRAJECTORIES)) {   // both read the tracker's live table: one view of its rows
        const char* stage = (stages & ADAS_OVERLAY_TRACKS) ? "tracks" : "trajectories";
        ADAS_REQUIRE(n_frames == 1, ADAS_ERR_INVALID,
                     "%s: the %s stage draws the tracker's live table, which holds the last frame only: n_frames must be 1 (got %d)", who, stage, n_frames);
        OvRows rows;
        const int ts = overlay_rows_of_tracker(a.tracker, &rows);
        ADAS_REQUIRE(n_streams <= ts, ADAS_ERR_INVALID, "%s: %d streams, the bytetrack handle holds %d", who, n_streams, ts);
        if (stages & ADAS_OVERLAY_TRACKS) overlay_rows_to_objects(rows, &r.obj);
        if (stages & ADAS_OVERLAY_TRAJECTORIES) {
            overlay_rows_to_tracks(rows, &r.trk);
            adas::tracker_ring_views(a.tracker, &r.trk.slot_ids, &r.trk.len, &r.trk.len_row_bytes, &r.trk.ring);   // the rings, through the slot each row names
            r.trk.slot_frame_bytes = r.trk.len_frame_bytes = r.trk.ring_frame_bytes = rows.frame_bytes;
        }
    }
    OvSources& s = r.s;
    if (a.decode) {
        const int *cnt, *det, *pts;
        adas::decode_lane_views(a.decode, &cnt, &det, &pts);
        s.lane_pts = pts; s.lane_cnt = cnt; s.lane_cnt_stride = 4;
    }
    if (a.geometry) {
        const int32_t *hdr = nullptr, *area = nullptr;
        const double* vals = nullptr;
        int32_t area_stride = 0;
        rc = adas_lane_geometry_device_views(a.geometry, &hdr, &vals, &area, &area_stride);
        if (rc) return rc;
        s.poly = area; s.poly_stride = (size_t)area_stride; s.poly_max = area_stride / 2;
        s.poly_n0 = hdr + 1; s.poly_n1 = hdr + 2; s.poly_n_stride = 8;   // area_points = the left points, then the reversed right points
        s.area_on = hdr; s.area_on_stride = 8;
        r.bird_pts = adas::geometry_bird_points(a.geometry); r.bird_cnt = hdr + 4;
        if (stages & ADAS_OVERLAY_READOUTS) {
            rc = adas::overlay_readout_check(who, h);
            if (rc) return rc;
            r.ro.dir = hdr + 3; r.ro.dir_stride = 8;
            r.ro.veh = adas::geometry_veh_pos(a.geometry);
            r.ro.cur = vals; r.ro.off = vals + 1; r.ro.val_stride = 2;
        }
    }
    if (a.analysis) {
        const int *fr, *pts;
        int stride = 0, maxp = 0;
        adas::analysis_frame_views(a.analysis, &fr, &stride, &pts, &maxp);
        s.offset_type = fr + offsetof(adas_analysis_frame, offset_msg) / 4; s.offset_stride = stride;
        s.collision = fr + offsetof(adas_analysis_frame, collision_msg) / 4; s.collision_stride = stride;
        s.dist_pts = pts; s.dist_cap = maxp;
        s.dist_cnt = fr + offsetof(adas_analysis_frame, n_points) / 4; s.dist_cnt_stride = stride;
    }
    r.src = a.d_src_bgr; r.dst = a.d_dst_bgr; r.d_bird = a.d_bird_bgr; r.bird_cnt_stride = 8;
    r.stages = stages; r.frames = (int)frames; r.st = (hipStream_t)a.stream;
    return overlay_launch(h, r);
}

// every run from raw device arrays: the three adas_overlay_run_arrays* entry points are masks over it
static int overlay_run_raw(const char* who, int mask, adas_overlay* h, const adas_overlay_arrays& a, const adas_overlay_readout_arrays* ra = nullptr) {
    const int stages = a.stages;
    int rc = overlay_check_run(who, mask, h, a.n_frames, stages, a.d_src_bgr, a.d_bird_bgr);
    if (rc) return rc;
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_READOUTS) || (ra && ra->d_direction && ra->d_veh_pos && ra->d_curvature && ra->d_offset), ADAS_ERR_INVALID,
                 "%s: the readouts stage needs the direction, veh_pos, curvature and offset arrays", who);
    if (stages & ADAS_OVERLAY_READOUTS) {
        rc = adas::overlay_readout_check(who, h);
        if (rc) return rc;
    }
    const bool rows_given = a.d_trk_tlwh && a.trk_cap > 0 && a.d_trk_cls && a.d_trk_counts;
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_TRAJECTORIES) || (rows_given && a.d_traj_tlbr && a.d_traj_len), ADAS_ERR_INVALID,
                 "%s: the trajectories stage needs the tracks' boxes, classes and counts, and their trajectories and lengths", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_LANES) || (a.d_lane_points && a.d_lane_counts), ADAS_ERR_INVALID,
                 "%s: the lane stage needs lane points and counts", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_AREA) || (a.d_poly && a.poly_cap > 0 && a.d_poly_counts && a.d_area_status), ADAS_ERR_INVALID,
                 "%s: the area stage needs a polygon, its counts and the area flags", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DISTANCE) || (a.d_dist_points && a.dist_cap > 0 && a.d_dist_counts), ADAS_ERR_INVALID,
                 "%s: the distance stage needs distance points and counts", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_BIRD) || (a.d_bird_points && a.d_bird_counts), ADAS_ERR_INVALID, "%s: the bird stage needs bird points and counts",
                 who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DETECTIONS) || (a.d_det_xyxy && a.det_cap > 0 && a.d_det_cls && a.d_det_counts), ADAS_ERR_INVALID,
                 "%s: the detections stage needs boxes, classes and counts", who);
    ADAS_REQUIRE(!(stages & ADAS_OVERLAY_TRACKS) || rows_given, ADAS_ERR_INVALID, "%s: the tracks stage needs boxes, classes and counts", who);
    ADAS_REQUIRE(a.det_cap <= (1 << 24) && a.trk_cap <= (1 << 24), ADAS_ERR_INVALID, "%s: capacities above 2^24 boxes per frame (%d, %d)", who, a.det_cap,
                 a.trk_cap);
    OvRun r = {};
    OvSources& s = r.s;
    s.lane_pts = a.d_lane_points; s.lane_cnt = a.d_lane_counts; s.lane_cnt_stride = 4;
    s.poly_max = a.poly_cap > 0 ? a.poly_cap : 0;
    s.poly = (stages & ADAS_OVERLAY_AREA) ? a.d_poly : nullptr; s.poly_stride = (size_t)s.poly_max * 2;
    s.poly_n0 = a.d_poly_counts; s.poly_n_stride = 1; s.area_on = a.d_area_status; s.area_on_stride = 1;
    s.offset_type = a.d_offset_type; s.offset_stride = 1; s.area_bgr = a.d_area_bgr;
    s.dist_pts = a.d_dist_points; s.dist_cap = a.dist_cap > 0 ? a.dist_cap : 0; s.dist_cnt = a.d_dist_counts; s.dist_cnt_stride = 1;
    if (stages & ADAS_OVERLAY_DETECTIONS) {
        r.obj.det_xyxy = a.d_det_xyxy; r.obj.det_cls = a.d_det_cls; r.obj.det_cnt = a.d_det_counts; r.obj.det_cap = a.det_cap; r.obj.det_cnt_stride = 1;
    }
    if (stages & (ADAS_OVERLAY_TRACKS | ADAS_OVERLAY_TRAJECTORIES)) {
        OvRows rows;
        overlay_rows_of_arrays(a, &rows);
        if (stages & ADAS_OVERLAY_TRACKS) overlay_rows_to_objects(rows, &r.obj);
        if (stages & ADAS_OVERLAY_TRAJECTORIES) {
            overlay_rows_to_tracks(rows, &r.trk);
            r.trk.ring = (const unsigned char*)a.d_traj_tlbr; r.trk.ring_frame_bytes = (size_t)a.trk_cap * ADAS_OVERLAY_TRACK_RING * 32;
            r.trk.len = (const unsigned char*)a.d_traj_len; r.trk.len_frame_bytes = (size_t)a.trk_cap * 4; r.trk.len_row_bytes = 4;
        }
    }
    r.src = a.d_src_bgr; r.dst = a.d_dst_bgr; r.d_bird = a.d_bird_bgr;
    r.bird_pts = a.d_bird_points; r.bird_cnt = a.d_bird_counts; r.bird_cnt_stride = 4;
    if (stages & ADAS_OVERLAY_READOUTS) {
        r.ro.dir = ra->d_direction; r.ro.dir_stride = 1;
        r.ro.veh = ra->d_veh_pos; r.ro.cur = ra->d_curvature; r.ro.off = ra->d_offset; r.ro.val_stride = 1;
    }
    r.stages = stages; r.frames = a.n_frames; r.st = (hipStream_t)a.stream;
    return overlay_launch(h, r);
}

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
    (void)adas_overlay_default_object_style(&h->os);
    h->max_batch = max_batch;
    h->rw = (p->src_w + 31) / 32;
    h->bird_rw = (p->bird_w + 31) / 32;
    const size_t B = max_batch, words = B * p->src_h * h->rw, bwords = B * p->bird_h * h->bird_rw;
    hipError_t e = hipMalloc((void**)&h->detail, words * 32);
    if (e == hipSuccess) e = hipMalloc((void**)&h->any, words * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->flags, B * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->rec_cnt, B * 8);
    if (e == hipSuccess) e = hipMemset(h->rec_cnt, 0, B * 8);
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
    for (void* q : {(void*)h->any, (void*)h->detail, (void*)h->bird_any, (void*)h->bird_detail, (void*)h->flags, (void*)h->d_dst,
                    (void*)h->rec_cnt, (void*)h->recs, (void*)h->colors[0], (void*)h->colors[1], (void*)h->trj_prims, (void*)h->trj_heads,
                    (void*)h->trj_cnt})
        if (q) (void)hipFree(q);
    adas::overlay_panels_free(h->panels);
    adas::overlay_text_free(h->text);
    adas::overlay_readout_free(h->readout);
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

// The six run entry points: each is its name and the stage bits it accepts over overlay_run_handles / overlay_run_raw.
int adas_overlay_run(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode, adas_lane_geometry* geometry,
                     adas_analysis* analysis, uint8_t* d_bird_bgr, int stages, int n_streams, int n_frames, void* stream) {
    return adas::overlay_run_handles("adas_overlay_run", 15, h,
                                     {d_src_bgr, d_dst_bgr, decode, geometry, analysis, nullptr, nullptr, d_bird_bgr, stages, n_streams, n_frames, stream});
}

int adas_overlay_run_objects(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode, adas_lane_geometry* geometry,
                             adas_analysis* analysis, adas_yolo_post* post, adas_bytetrack* tracker, uint8_t* d_bird_bgr, int stages, int n_streams,
                             int n_frames, void* stream) {
    return adas::overlay_run_handles("adas_overlay_run_objects", 63, h,
                                     {d_src_bgr, d_dst_bgr, decode, geometry, analysis, post, tracker, d_bird_bgr, stages, n_streams, n_frames, stream});
}

int adas_overlay_run_trajectories(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode,
                                  adas_lane_geometry* geometry, adas_analysis* analysis, adas_yolo_post* post, adas_bytetrack* tracker, uint8_t* d_bird_bgr,
                                  int stages, int n_streams, int n_frames, void* stream) {
    return adas::overlay_run_handles("adas_overlay_run_trajectories", 63 | ADAS_OVERLAY_TRAJECTORIES, h,
                                     {d_src_bgr, d_dst_bgr, decode, geometry, analysis, post, tracker, d_bird_bgr, stages, n_streams, n_frames, stream});
}

int adas_overlay_run_arrays_objects(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const int32_t* d_lane_points,
                                    const int32_t* d_lane_counts, const int32_t* d_poly, int poly_cap, const int32_t* d_poly_counts,
                                    const int32_t* d_area_status, const int32_t* d_offset_type, const uint8_t* d_area_bgr, const int32_t* d_dist_points,
                                    int dist_cap, const int32_t* d_dist_counts, const int32_t* d_bird_points, const int32_t* d_bird_counts,
                                    uint8_t* d_bird_bgr, const int32_t* d_det_xyxy, int det_cap, const int32_t* d_det_cls, const int32_t* d_det_counts,
                                    const double* d_trk_tlwh, int trk_cap, const int32_t* d_trk_cls, const int32_t* d_trk_counts, int stages,
                                    int n_frames, void* stream) {
    adas_overlay_arrays a = {};
    a.d_src_bgr = d_src_bgr; a.d_dst_bgr = d_dst_bgr; a.d_lane_points = d_lane_points; a.d_lane_counts = d_lane_counts;
    a.d_poly = d_poly; a.poly_cap = poly_cap; a.d_poly_counts = d_poly_counts; a.d_area_status = d_area_status;
    a.d_offset_type = d_offset_type; a.d_area_bgr = d_area_bgr; a.d_dist_points = d_dist_points; a.dist_cap = dist_cap; a.d_dist_counts = d_dist_counts;
    a.d_bird_points = d_bird_points; a.d_bird_counts = d_bird_counts; a.d_bird_bgr = d_bird_bgr; a.stages = stages; a.n_frames = n_frames; a.stream = stream;
    a.d_det_xyxy = d_det_xyxy; a.det_cap = det_cap; a.d_det_cls = d_det_cls; a.d_det_counts = d_det_counts;
    a.d_trk_tlwh = d_trk_tlwh; a.trk_cap = trk_cap; a.d_trk_cls = d_trk_cls; a.d_trk_counts = d_trk_counts;
    return overlay_run_raw("adas_overlay_run_arrays_objects", 63, h, a);
}

int adas_overlay_run_arrays(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const int32_t* d_lane_points, const int32_t* d_lane_counts,
                            const int32_t* d_poly, int poly_cap, const int32_t* d_poly_counts, const int32_t* d_area_status,
                            const int32_t* d_offset_type, const uint8_t* d_area_bgr, const int32_t* d_dist_points, int dist_cap,
                            const int32_t* d_dist_counts, const int32_t* d_bird_points, const int32_t* d_bird_counts, uint8_t* d_bird_bgr, int stages,
                            int n_frames, void* stream) {
    adas_overlay_arrays a = {};
    a.d_src_bgr = d_src_bgr; a.d_dst_bgr = d_dst_bgr; a.d_lane_points = d_lane_points; a.d_lane_counts = d_lane_counts;
    a.d_poly = d_poly; a.poly_cap = poly_cap; a.d_poly_counts = d_poly_counts; a.d_area_status = d_area_status;
    a.d_offset_type = d_offset_type; a.d_area_bgr = d_area_bgr; a.d_dist_points = d_dist_points; a.dist_cap = dist_cap; a.d_dist_counts = d_dist_counts;
    a.d_bird_points = d_bird_points; a.d_bird_counts = d_bird_counts; a.d_bird_bgr = d_bird_bgr; a.stages = stages; a.n_frames = n_frames; a.stream = stream;
    return overlay_run_raw("adas_overlay_run_arrays", 15, h, a);
}

int adas_overlay_run_arrays_trajectories(adas_overlay* h, const adas_overlay_arrays* a) {
    ADAS_REQUIRE(a, ADAS_ERR_INVALID, "adas_overlay_run_arrays_trajectories: null argument");
    return overlay_run_raw("adas_overlay_run_arrays_trajectories", 63 | ADAS_OVERLAY_TRAJECTORIES, h, *a);
}

int adas_overlay_run_readouts(adas_overlay* h, const uint8_t* d_src_bgr, uint8_t* d_dst_bgr, const adas_ufld_decode* decode, adas_lane_geometry* geometry,
                              adas_analysis* analysis, adas_yolo_post* post, adas_bytetrack* tracker, uint8_t* d_bird_bgr, int stages, int n_streams, int n_frames,
                              void* stream) {
    return adas::overlay_run_handles("adas_overlay_run_readouts", 63 | ADAS_OVERLAY_TRAJECTORIES | ADAS_OVERLAY_READOUTS, h,
                                     {d_src_bgr, d_dst_bgr, decode, geometry, analysis, post, tracker, d_bird_bgr, stages, n_streams, n_frames, stream});
}

int adas_overlay_run_arrays_readouts(adas_overlay* h, const adas_overlay_arrays* a, const adas_overlay_readout_arrays* r) {
    ADAS_REQUIRE(a, ADAS_ERR_INVALID, "adas_overlay_run_arrays_readouts: null argument");
    return overlay_run_raw("adas_overlay_run_arrays_readouts", 63 | ADAS_OVERLAY_TRAJECTORIES | ADAS_OVERLAY_READOUTS, h, *a, r);
}

int adas_overlay_fetch_track_marks(adas_overlay* h, int frame, adas_overlay_track_mark* marks, int max_marks, int32_t* n_marks) {
    ADAS_REQUIRE(h && n_marks && max_marks >= 0 && (marks || max_marks == 0) && frame >= 0 && frame < h->max_batch, ADAS_ERR_INVALID,
                 "adas_overlay_fetch_track_marks: bad argument");
    ADAS_REQUIRE(frame < h->trj_run_frames, ADAS_ERR_INVALID,
                 "adas_overlay_fetch_track_marks: frame %d was not part of a run with the trajectories stage (the last one had %d frames)", frame,
                 h->trj_run_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    const int cap = h->trj_run_cap;
    int nt = 0;
    ADAS_HIP_TRY(hipMemcpy(&nt, h->trj_cnt + frame, 4, hipMemcpyDeviceToHost));
    nt = nt < 0 ? 0 : (nt > cap ? cap : nt);
    OverlayTrackHead* heads = new (std::nothrow) OverlayTrackHead[nt > 0 ? nt : 1];
    OverlayPrim* prims = new (std::nothrow) OverlayPrim[(size_t)(nt > 0 ? nt : 1) * ADAS_OVERLAY_TRACK_PRIMS];
    hipError_t e = hipSuccess;
    if (heads && prims && nt > 0) {
        e = hipMemcpy(heads, h->trj_heads + (size_t)frame * cap, (size_t)nt * sizeof(OverlayTrackHead), hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(prims, h->trj_prims + (size_t)frame * cap * ADAS_OVERLAY_TRACK_PRIMS, (size_t)nt * ADAS_OVERLAY_TRACK_PRIMS * sizeof(OverlayPrim),
                          hipMemcpyDeviceToHost);
    }
    int n = 0;
    if (heads && prims && e == hipSuccess) {
        for (int k = 0; k < nt; ++k) {
            const OverlayPrim* p = prims + (size_t)k * ADAS_OVERLAY_TRACK_PRIMS;
            n = overlay_track_marks(p, heads[k].n, k, marks, max_marks, n);
        }
    }
    const bool oom = !heads || !prims;
    delete[] heads;
    delete[] prims;
    ADAS_REQUIRE(!oom, ADAS_ERR_INVALID, "out of host memory");
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(overlay track marks)", __FILE__, __LINE__);
    *n_marks = n;
    return ADAS_OK;
}

int adas_overlay_default_object_style(adas_overlay_object_style* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_overlay_default_object_style: null argument");
    memset(p, 0, sizeof(*p));
    p->min_box_area = 10.0;
    p->det_rect_thickness = 1; p->det_arm_thickness = 5; p->track_thickness = 2;
    return ADAS_OK;
}

int adas_overlay_set_object_style(adas_overlay* h, const adas_overlay_object_style* p) {
    ADAS_REQUIRE(h && p, ADAS_ERR_INVALID, "adas_overlay_set_object_style: bad argument");
    int rc = overlay_check_object_style(p, "adas_overlay_set_object_style");
    if (rc) return rc;
    h->os = *p;
    adas::bump_config_generation();   // a captured step holds the old style in its kernel arguments
    return ADAS_OK;
}

int adas_overlay_set_class_colors(adas_overlay* h, int which, const uint8_t (*bgr)[3], int n) {
    ADAS_REQUIRE(h && (which == ADAS_OVERLAY_DETECTIONS || which == ADAS_OVERLAY_TRACKS) && n >= 0 && (bgr || n == 0), ADAS_ERR_INVALID,
                 "adas_overlay_set_class_colors: bad argument (which must be ADAS_OVERLAY_DETECTIONS or ADAS_OVERLAY_TRACKS)");
    const int t = which == ADAS_OVERLAY_TRACKS;
    uint32_t* table = nullptr;
    if (n > 0) {
        uint32_t* packed = new (std::nothrow) uint32_t[n];
        ADAS_REQUIRE(packed, ADAS_ERR_INVALID, "out of host memory");
        for (int i = 0; i < n; ++i) packed[i] = overlay_pack_bgr(bgr[i]);
        hipError_t e = hipMalloc((void**)&table, (size_t)n * 4);
        if (e == hipSuccess) e = hipMemcpy(table, packed, (size_t)n * 4, hipMemcpyHostToDevice);
        delete[] packed;
        if (e != hipSuccess) {
            if (table) (void)hipFree(table);
            return hip_fail(e, "hipMalloc(overlay class colours)", __FILE__, __LINE__);
        }
    }
    ADAS_HIP_TRY(hipDeviceSynchronize());   // a run in flight may still read the old table
    if (h->colors[t]) (void)hipFree(h->colors[t]);
    h->colors[t] = table;
    h->n_colors[t] = n;
    adas::bump_config_generation();   // a captured step holds the old table's address in its kernel arguments
    return ADAS_OK;
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
