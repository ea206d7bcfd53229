// remap_kernels.hip -- camera frames rectified on the device, in front of the fused step: cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) of BGR u8
// frames that already sit in HBM through a fixed-point map per stream, the map either the caller's (cv2's CV_16SC2 + CV_16UC1 pair) or built
// here from a lens model as cv2.initUndistortRectifyMap writes it.  The rules and every byte address are remap_core.h (U1-U6); this file is
// the kernels around its work items and the C ABI (adas_remap_*).  Every run takes remap_kernel unless ADAS_REMAP_STAGED=1 is set.
//   remap_build_kernel   a thread per map entry evaluates rule U3 in fp64 and stores the entry.  Runs when a camera is set, off the hot path.
//   remap_kernel         the hot path, direct form.  A thread per run of 4 consecutive pixels of a destination row, a workgroup per 4 rows by
//                        64 runs, frames along grid.z; neighbouring lanes take neighbouring runs, so a wave reads 1 KB of (sx, sy) and 512 B of
//                        fractions in 16- and 8-byte loads and writes 768 contiguous bytes as dwords.  The taps are warp_sample's 8-byte row
//                        loads, gathered through L1 / L2 as they are.  No LDS.  Any pointer, any size.
//   remap_tile_kernel    the staged form, opt-in (ADAS_REMAP_STAGED=1: it measured slower), for a 16-byte aligned source whose
//                        rows are multiples of 16 bytes (the camera sizes): the same workgroup first finds the bounding box of its taps (an
//                        LDS min / max), brings the box into LDS in 16-byte pieces and reads the taps from LDS; a workgroup whose box
//                        exceeds 16 KB gathers directly.  Same bytes.
// Memory-bound: 3 B read and 3 B written per pixel plus 6 B of map.  adas_remap_run is one plain launch without allocation or host
// synchronisation: capturable once the maps are set.
#include "common.h"
#include <stddef.h>
#include <string.h>
#include <new>
#include <vector>
#include "remap_core.h"

using namespace adas;

static_assert(sizeof(adas_remap_camera) == sizeof(RemapCamera) && offsetof(adas_remap_camera, D) == offsetof(RemapCamera, D) &&
                  offsetof(adas_remap_camera, new_K) == offsetof(RemapCamera, new_K) && offsetof(adas_remap_camera, R) == offsetof(RemapCamera, R),
              "adas_remap_camera is RemapCamera");
static_assert(sizeof(adas_remap_params) == 24, "adas_remap_params is six ints and _lib.RemapParams");

namespace {

constexpr int REMAP_THREADS = 256;
constexpr int REMAP_RUNS = REMAP_TILE_RUNS, REMAP_ROWS = REMAP_TILE_ROWS;   // both remap kernels' workgroup: 64 runs of each of 4 rows
static_assert(REMAP_RUNS * REMAP_ROWS == REMAP_THREADS, "");

__global__ __launch_bounds__(REMAP_THREADS) void remap_build_kernel(RemapGeom g, RemapModel m, int16_t* __restrict__ xy, uint16_t* __restrict__ frac,
                                                                   int map) {
    const long long i = (long long)blockIdx.x * REMAP_THREADS + threadIdx.x;
    if (i >= (long long)g.dh * g.dw) return;
    remap_build_item(g, m, xy, frac, map, i);
}

// a workgroup is REMAP_ROWS destination rows by REMAP_RUNS runs: a wave takes 64 neighbouring runs of one row, and no index needs a division
__global__ __launch_bounds__(REMAP_THREADS) void remap_kernel(RemapGeom g, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             const int16_t* __restrict__ xy, const uint16_t* __restrict__ frac,
                                                             const int* __restrict__ map_of_stream) {
    const int run = (int)(blockIdx.x * REMAP_RUNS + threadIdx.x), y = (int)(blockIdx.y * REMAP_ROWS + threadIdx.y);
    if (run >= remap_runs(g.dw) || y >= g.dh) return;
    const int f = (int)blockIdx.z;
    const int map = remap_ld_table(map_of_stream, f % g.n_streams);   // workgroup-uniform; the table holds checked indices only
    remap_item(g, src, dst, xy, frac, map, f, y, run);
}

__global__ __launch_bounds__(REMAP_THREADS) void remap_tile_kernel(RemapGeom g, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                  const int16_t* __restrict__ xy, const uint16_t* __restrict__ frac,
                                                                  const int* __restrict__ map_of_stream) {
    __shared__ uint4 box[(REMAP_TILE_LDS + REMAP_TILE_PAD) / 16];
    __shared__ int ext[4];
    uint8_t* lds = (uint8_t*)box;
    const int tid = (int)(threadIdx.y * REMAP_RUNS + threadIdx.x);
    const int run = (int)(blockIdx.x * REMAP_RUNS + threadIdx.x), y = (int)(blockIdx.y * REMAP_ROWS + threadIdx.y);
    const bool live = run < remap_runs(g.dw) && y < g.dh;
    const int f = (int)blockIdx.z;
    const int map = remap_ld_table(map_of_stream, f % g.n_streams);
    if (tid == 0) {
        ext[0] = ext[2] = 0x7fffffff;
        ext[1] = ext[3] = -1;
    }
    __syncthreads();
    uint32_t mx[4], mf[4], px[4];
    int n = 0;
    if (live) {
        n = remap_run_entries(g, xy, frac, map, y, run, mx, mf);
        int e[4] = {0x7fffffff, -1, 0x7fffffff, -1};
        remap_run_extent(g, n, mx, e);
        if (e[1] >= e[0]) {
            atomicMin(&ext[0], e[0]);
            atomicMax(&ext[1], e[1]);
            atomicMin(&ext[2], e[2]);
            atomicMax(&ext[3], e[3]);
        }
    }
    __syncthreads();
    const int box_ext[4] = {ext[0], ext[1], ext[2], ext[3]};
    const RemapTile T = remap_tile_of(box_ext);
    if (!remap_tile_fits(T)) {   // workgroup-uniform: no barrier follows
        if (live) {
            remap_run_gather(g, src, f, n, mx, mf, px);
            remap_run_store(g, dst, f, y, run, n, px);
        }
        return;
    }
    for (int p = tid; p < remap_tile_pieces(T); p += REMAP_THREADS) remap_tile_load(g, T, src, f, lds, p);
    __syncthreads();
    if (live) {
        remap_run_sample_tile(g, T, lds, n, mx, mf, px);
        remap_run_store(g, dst, f, y, run, n, px);
    }
}

// ADAS_REMAP_STAGED=1: a run that meets remap_tile_ok takes the staged form.  It measured 3.3 to 3.8 times slower than the direct form at the
// camera size (profiles/r08/remap.txt) and is kept as a measured experiment only: off unless asked for, and read at every
// run, so that one process can measure both forms in alternation
bool remap_staged_on() { return env_on("ADAS_REMAP_STAGED"); }

}  // namespace

struct adas_remap {
    RemapGeom g;
    int max_batch = 0;
    int16_t* d_xy = nullptr;             // [n_maps][map_stride][2]
    uint16_t* d_frac = nullptr;          // [n_maps][map_stride]
    int* d_table = nullptr;              // [n_streams] map of stream
    uint8_t* d_dst = nullptr;            // [max_batch][dst_h][dst_w][3]
    std::vector<int> table;              // the host copy of d_table
    std::vector<unsigned char> is_set;   // per map: a camera or a caller's map has been set
    int dst_frames = 0;                  // frames [0, dst_frames) of d_dst have been written by some run
    hipStream_t last = nullptr;          // the stream of the last run: set calls and fetches order themselves behind it
    size_t frame_bytes() const { return (size_t)g.dh * g.dw * 3; }
    size_t entries() const { return (size_t)g.dh * g.dw; }
};

void adas::remap_geometry_of(const adas_remap* h, int* src_h, int* src_w, int* dst_h, int* dst_w, int* n_streams, int* max_batch) {
    *src_h = h ? h->g.sh : 0;
    *src_w = h ? h->g.sw : 0;
    *dst_h = h ? h->g.dh : 0;
    *dst_w = h ? h->g.dw : 0;
    *n_streams = h ? h->g.n_streams : 0;
    *max_batch = h ? h->max_batch : 0;
}
uint8_t* adas::remap_frames(adas_remap* h) { return h ? h->d_dst : nullptr; }
void adas::remap_forget_stream(adas_remap* h) {
    if (h) h->last = nullptr;
}

// The handle is host state until a call needs the device: the two map tables, the stream table and the handle's own frames then come in one go
// (a refusal of U4 needs no device).  Every run follows a set call, so a run never allocates.
static int remap_device(adas_remap* h) {
    if (h->d_xy) return ADAS_OK;
    ADAS_REQUIRE(adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    const size_t map_entries = (size_t)h->g.n_maps * (size_t)h->g.map_stride;
    int16_t* xy = nullptr;
    uint16_t* frac = nullptr;
    int* table = nullptr;
    uint8_t* dst = nullptr;
    hipError_t e = hipMalloc((void**)&xy, map_entries * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&frac, map_entries * 2);
    if (e == hipSuccess) e = hipMalloc((void**)&table, h->table.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&dst, h->frame_bytes() * h->max_batch);
    if (e == hipSuccess) e = hipMemset(xy, 0, map_entries * 4);   // an unset map is refused by the run; zero is a legal entry all the same
    if (e == hipSuccess) e = hipMemset(frac, 0, map_entries * 2);
    if (e == hipSuccess) e = hipMemcpy(table, h->table.data(), h->table.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (xy) (void)hipFree(xy);
        if (frac) (void)hipFree(frac);
        if (table) (void)hipFree(table);
        if (dst) (void)hipFree(dst);
        return hip_fail(e, "hipMalloc(remap)", __FILE__, __LINE__);
    }
    h->d_frac = frac; h->d_table = table; h->d_dst = dst; h->d_xy = xy;
    return ADAS_OK;
}

static int remap_push_table(adas_remap* h) {
    if (!h->d_xy) return ADAS_OK;   // the device table is filled from the host copy when it is allocated
    ADAS_HIP_TRY(hipMemcpyAsync(h->d_table, h->table.data(), h->table.size() * sizeof(int), hipMemcpyHostToDevice, h->last));
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    return ADAS_OK;
}

extern "C" {

int adas_remap_destroy(adas_remap* h) {
    if (!h) return ADAS_OK;
    if (h->d_xy) (void)hipFree(h->d_xy);
    if (h->d_frac) (void)hipFree(h->d_frac);
    if (h->d_table) (void)hipFree(h->d_table);
    if (h->d_dst) (void)hipFree(h->d_dst);
    delete h;
    return ADAS_OK;
}

int adas_remap_create(const adas_remap_params* p, int max_batch, adas_remap** out) {
    const char* who = "adas_remap_create";
    ADAS_REQUIRE(p && out, ADAS_ERR_INVALID, "%s: null argument", who);
    const int why = remap_check_sizes(p->src_h, p->src_w, p->dst_h, p->dst_w);
    ADAS_REQUIRE(why == REMAP_OK, ADAS_ERR_INVALID, "%s: %s (source %dx%d, destination %dx%d)", who, remap_why(why), p->src_h, p->src_w, p->dst_h, p->dst_w);
    ADAS_REQUIRE(p->n_streams >= 1 && p->n_streams <= 65535, ADAS_ERR_INVALID, "%s: n_streams %d (1..65535)", who, p->n_streams);
    ADAS_REQUIRE(p->n_maps >= 1 && p->n_maps <= 65535, ADAS_ERR_INVALID, "%s: n_maps %d (1..65535)", who, p->n_maps);
    ADAS_REQUIRE(max_batch >= 1 && max_batch <= 65535, ADAS_ERR_INVALID, "%s: max_batch %d (1..65535)", who, max_batch);
    adas_remap* h = new (std::nothrow) adas_remap();
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "out of host memory");
    h->g.sh = p->src_h; h->g.sw = p->src_w; h->g.dh = p->dst_h; h->g.dw = p->dst_w;
    h->g.n_streams = p->n_streams; h->g.n_maps = p->n_maps;
    h->g.map_stride = remap_map_stride(p->dst_h, p->dst_w);
    h->max_batch = max_batch;
    h->table.resize(p->n_streams);
    for (int s = 0; s < p->n_streams; ++s) h->table[s] = remap_default_map(s, p->n_maps);
    h->is_set.assign(p->n_maps, 0);
    *out = h;
    return ADAS_OK;
}

int adas_remap_set_camera(adas_remap* h, int map, const adas_remap_camera* cam) {
    const char* who = "adas_remap_set_camera";
    ADAS_REQUIRE(h && cam, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(map == -1 || remap_check_map(map, h->g.n_maps) == REMAP_OK, ADAS_ERR_INVALID, "%s: %s (map %d of %d)", who, remap_why(REMAP_BAD_MAP), map,
                 h->g.n_maps);
    RemapCamera c;
    memcpy(&c, cam, sizeof(c));
    RemapModel m;
    const int why = remap_model_of(c, &m);
    ADAS_REQUIRE(why == REMAP_OK, ADAS_ERR_INVALID, "%s: %s", who, remap_why(why));
    const int rc = remap_device(h);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((h->entries() + REMAP_THREADS - 1) / REMAP_THREADS);
    for (int k = map < 0 ? 0 : map; k < (map < 0 ? h->g.n_maps : map + 1); ++k) {
        hipLaunchKernelGGL(remap_build_kernel, dim3(blocks), dim3(REMAP_THREADS), 0, h->last, h->g, m, h->d_xy, h->d_frac, k);
        ADAS_HIP_TRY(hipGetLastError());
        h->is_set[k] = 1;
    }
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));   // off the hot path: a run on any stream that follows reads the finished map
    return ADAS_OK;
}

int adas_remap_set_map(adas_remap* h, int map, const int16_t* h_xy, const uint16_t* h_frac) {
    const char* who = "adas_remap_set_map";
    ADAS_REQUIRE(h && h_xy && h_frac, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(remap_check_map(map, h->g.n_maps) == REMAP_OK, ADAS_ERR_INVALID, "%s: %s (map %d of %d)", who, remap_why(REMAP_BAD_MAP), map, h->g.n_maps);
    const int rc = remap_device(h);
    if (rc) return rc;
    const size_t at = (size_t)map * (size_t)h->g.map_stride;
    ADAS_HIP_TRY(hipMemcpyAsync(h->d_xy + 2 * at, h_xy, h->entries() * 4, hipMemcpyHostToDevice, h->last));
    ADAS_HIP_TRY(hipMemcpyAsync(h->d_frac + at, h_frac, h->entries() * 2, hipMemcpyHostToDevice, h->last));
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    h->is_set[map] = 1;
    return ADAS_OK;
}

int adas_remap_assign(adas_remap* h, int stream, int map) {
    const char* who = "adas_remap_assign";
    ADAS_REQUIRE(h, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(stream >= 0 && stream < h->g.n_streams, ADAS_ERR_INVALID, "%s: stream %d of %d", who, stream, h->g.n_streams);
    ADAS_REQUIRE(remap_check_map(map, h->g.n_maps) == REMAP_OK, ADAS_ERR_INVALID, "%s: %s (map %d of %d)", who, remap_why(REMAP_BAD_MAP), map, h->g.n_maps);
    h->table[stream] = map;
    return remap_push_table(h);
}

int adas_remap_fetch_map(adas_remap* h, int map, int16_t* h_xy, uint16_t* h_frac) {
    const char* who = "adas_remap_fetch_map";
    ADAS_REQUIRE(h && h_xy && h_frac, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(remap_check_map(map, h->g.n_maps) == REMAP_OK, ADAS_ERR_INVALID, "%s: %s (map %d of %d)", who, remap_why(REMAP_BAD_MAP), map, h->g.n_maps);
    ADAS_REQUIRE(h->is_set[map], ADAS_ERR_INVALID, "%s: map %d was never set (adas_remap_set_camera / _set_map)", who, map);
    const size_t at = (size_t)map * (size_t)h->g.map_stride;
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_xy, h->d_xy + 2 * at, h->entries() * 4, hipMemcpyDeviceToHost));
    ADAS_HIP_TRY(hipMemcpy(h_frac, h->d_frac + at, h->entries() * 2, hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_remap_run(adas_remap* h, const uint8_t* d_src_bgr, int batch, uint8_t* d_dst_bgr, void* stream) {
    const char* who = "adas_remap_run";
    ADAS_REQUIRE(h && d_src_bgr, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(batch >= 1 && batch <= h->max_batch, ADAS_ERR_INVALID, "%s: batch %d, the handle holds %d frames", who, batch, h->max_batch);
    for (int s = 0; s < h->g.n_streams && s < batch; ++s)
        ADAS_REQUIRE(h->is_set[h->table[s]], ADAS_ERR_INVALID, "%s: map %d of stream %d was never set (adas_remap_set_camera / _set_map)", who, h->table[s],
                     s);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((remap_runs(h->g.dw) + REMAP_RUNS - 1) / REMAP_RUNS), (unsigned)((h->g.dh + REMAP_ROWS - 1) / REMAP_ROWS), (unsigned)batch);
    const bool staged = remap_staged_on() && remap_tile_ok(h->g, d_src_bgr);
    hipLaunchKernelGGL(staged ? remap_tile_kernel : remap_kernel, grid, dim3(REMAP_RUNS, REMAP_ROWS), 0, st, h->g, d_src_bgr, d_dst_bgr ? d_dst_bgr : h->d_dst, h->d_xy, h->d_frac,
                       h->d_table);
    ADAS_HIP_TRY(hipGetLastError());
    h->last = st;
    if (!d_dst_bgr && batch > h->dst_frames) h->dst_frames = batch;
    return ADAS_OK;
}

int adas_remap_fetch(adas_remap* h, int frame, uint8_t* h_bgr) {
    const char* who = "adas_remap_fetch";
    ADAS_REQUIRE(h && h_bgr, ADAS_ERR_INVALID, "%s: null argument", who);
    ADAS_REQUIRE(frame >= 0 && frame < h->dst_frames, ADAS_ERR_INVALID,
                 "%s: frame %d of the handle's own buffer was never written (largest batch run into it: %d)", who, frame, h->dst_frames);
    ADAS_HIP_TRY(hipStreamSynchronize(h->last));
    ADAS_HIP_TRY(hipMemcpy(h_bgr, h->d_dst + (size_t)frame * h->frame_bytes(), h->frame_bytes(), hipMemcpyDeviceToHost));
    return ADAS_OK;
}

int adas_remap_device_view(adas_remap* h, const uint8_t** d_frames_bgr) {
    ADAS_REQUIRE(h && d_frames_bgr, ADAS_ERR_INVALID, "adas_remap_device_view: null argument");
    const int rc = remap_device(h);
    if (rc) return rc;
    *d_frames_bgr = h->d_dst;
    return ADAS_OK;
}

}  // extern "C"
