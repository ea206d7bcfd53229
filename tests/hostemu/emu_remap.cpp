// Host build of the rectification stage's rules (csrc/remap_core.h; g++, one thread): the work the two device kernels run -- remap_build_item over
// every map entry, remap_item over every frame and run -- through the same address arithmetic, with every map load, table load and store
// audited: a load must lie inside the tables the caller handed over, a store inside the `batch` destination frames (or the map being built),
// a wide access must be aligned as the device needs it (an access that fails is counted and not made), and every destination byte and every
// entry of a built map must be stored exactly once (U6).  The staged form runs as its kernel does, workgroup by workgroup with a loop over the
// lanes at every barrier, its 16-byte source loads audited against the source frames and its LDS a heap block of the kernel's size.  The direct
// form's taps are warp_core.h's warp_sample, unchanged; their addresses, like the staged form's LDS reads, are what
// tests/hostemu/remap_bounds_main.cpp runs under a sanitizer over heap blocks of exactly the frames' size.  The CPU suite compares the results
// with tests/remap_ref.py, the GPU suite the device's bytes with these.  Test scaffolding only; never loaded by the product.
#include <stddef.h>
#include <stdlib.h>
#include <vector>
#define REMAP_AUDIT 1
#include "remap_core.h"
#include "adas_hip.h"

using namespace adas;

namespace {
struct Range {
    const uint8_t *lo = nullptr, *hi = nullptr;
};
struct Audit {
    Range r[7];                  // by kind: xy loads, fraction loads, frame stores, table loads, xy stores, fraction stores, staged source loads
    std::vector<uint8_t> hits;   // stores per destination byte (kind 2) or per built entry's xy byte (kind 4), saturating at 255
    std::vector<uint8_t> hits2;  // stores per built entry's fraction byte (kind 5)
    long long outside = 0, misaligned = 0, loads = 0, stores = 0, wide_loads = 0, wide_stores = 0, staged_loads = 0, direct_tiles = 0;
} A;
}  // namespace

namespace adas {
bool remap_audit(const void* p, int bytes, int align, int kind) {
    const uint8_t* q = (const uint8_t*)p;
    const Range& r = A.r[kind];
    const bool inside = r.lo && q >= r.lo && q + bytes <= r.hi;
    const bool store = kind == 2 || kind == 4 || kind == 5;
    if (!inside) ++A.outside;
    if ((uintptr_t)q % (uintptr_t)align) ++A.misaligned;
    ++(store ? A.stores : A.loads);
    if (kind == 2 && bytes > 1) ++A.wide_stores;
    if (kind == 6) ++A.staged_loads;
    if ((kind == 0 && bytes > 4) || (kind == 1 && bytes > 2)) ++A.wide_loads;
    if (inside && store) {
        std::vector<uint8_t>& hits = kind == 5 ? A.hits2 : A.hits;
        for (int i = 0; i < bytes; ++i) {
            uint8_t& h = hits[(size_t)(q - r.lo) + i];
            if (h < 255) ++h;
        }
    }
    return inside;   // any other access is counted, not made
}
}  // namespace adas

extern "C" {

// sizeof and the field offsets of adas_remap_params (src_h, src_w, dst_h, dst_w, n_streams, n_maps) as g++ lays the public header out, then
// sizeof and the offsets of K, D, new_K, R of the rules' RemapCamera
void emu_remap_layout(int* out) {
    const int v[12] = {(int)sizeof(adas_remap_params),           (int)offsetof(adas_remap_params, src_h),     (int)offsetof(adas_remap_params, src_w),
                       (int)offsetof(adas_remap_params, dst_h),   (int)offsetof(adas_remap_params, dst_w),     (int)offsetof(adas_remap_params, n_streams),
                       (int)offsetof(adas_remap_params, n_maps),  (int)sizeof(RemapCamera),                    (int)offsetof(RemapCamera, K),
                       (int)offsetof(RemapCamera, D),             (int)offsetof(RemapCamera, new_K),           (int)offsetof(RemapCamera, R)};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

int emu_remap_check_sizes(int sh, int sw, int dh, int dw) { return remap_check_sizes(sh, sw, dh, dw); }
int emu_remap_check_map(int map, int n_maps) { return remap_check_map(map, n_maps); }
int emu_remap_check_camera(const RemapCamera* c) {
    RemapModel m;
    return remap_model_of(*c, &m);
}
const char* emu_remap_why(int code) { return remap_why(code); }
long long emu_remap_map_stride(int dh, int dw) { return remap_map_stride(dh, dw); }
int emu_remap_default_map(int stream, int n_maps) { return remap_default_map(stream, n_maps); }

// The build kernel's work: map `map` of tables that hold n_maps maps (xy: n_maps * map_stride * 4 bytes, frac: * 2 bytes), every entry through
// remap_build_item.  info [4] = accesses outside, misaligned accesses, stores, bytes of the map's dst_h * dst_w entries not stored exactly once.
// Returns remap_model_of's verdict (nothing runs unless it is 0).
int emu_remap_build(const RemapCamera* cam, int dh, int dw, int map, int n_maps, int16_t* xy, uint16_t* frac, long long* info) {
    RemapModel m;
    const int why = remap_model_of(*cam, &m);
    if (why != REMAP_OK) return why;
    RemapGeom g;
    g.sh = g.sw = 0; g.dh = dh; g.dw = dw; g.n_streams = 1; g.n_maps = n_maps;
    g.map_stride = remap_map_stride(dh, dw);
    const long long n = (long long)dh * dw;
    A = Audit();
    // the map's own entries, not the padding behind them and not another map's
    A.r[4].lo = (const uint8_t*)(xy + 2 * map * g.map_stride);
    A.r[4].hi = A.r[4].lo + n * 4;
    A.r[5].lo = (const uint8_t*)(frac + map * g.map_stride);
    A.r[5].hi = A.r[5].lo + n * 2;
    A.hits.assign((size_t)n * 4, 0);
    A.hits2.assign((size_t)n * 2, 0);
    for (long long i = 0; i < n; ++i) remap_build_item(g, m, xy, frac, map, i);
    long long not_once = 0;
    for (uint8_t h : A.hits) not_once += h != 1;
    for (uint8_t h : A.hits2) not_once += h != 1;
    const long long v[4] = {A.outside, A.misaligned, A.stores, not_once};
    for (int i = 0; i < 4; ++i) info[i] = v[i];
    return REMAP_OK;
}

// The staged form as remap_tile_kernel runs it: the phases of remap_core.h in the kernel's order, a loop over the lanes where the kernel has a
// barrier; the LDS is a heap block of exactly the kernel's static size, filled with junk before every workgroup
static void run_tiles(const RemapGeom& g, const uint8_t* src, uint8_t* dst, const int16_t* xy, const uint16_t* frac, const int* table, int batch) {
    const int lanes = REMAP_TILE_ROWS * REMAP_TILE_RUNS, runs = remap_runs(g.dw);
    uint8_t* lds = (uint8_t*)malloc(REMAP_TILE_LDS + REMAP_TILE_PAD);
    static uint32_t mx[REMAP_TILE_ROWS * REMAP_TILE_RUNS][4], mf[REMAP_TILE_ROWS * REMAP_TILE_RUNS][4];
    static int n[REMAP_TILE_ROWS * REMAP_TILE_RUNS];
    for (int f = 0; f < batch; ++f)
        for (int by = 0; by * REMAP_TILE_ROWS < g.dh; ++by)
            for (int bx = 0; bx * REMAP_TILE_RUNS < runs; ++bx) {
                const int map = remap_ld_table(table, f % g.n_streams);
                memset(lds, 0xEE, REMAP_TILE_LDS + REMAP_TILE_PAD);
                int ext[4] = {0x7fffffff, -1, 0x7fffffff, -1};
                for (int t = 0; t < lanes; ++t) {
                    const int run = bx * REMAP_TILE_RUNS + t % REMAP_TILE_RUNS, y = by * REMAP_TILE_ROWS + t / REMAP_TILE_RUNS;
                    n[t] = -1;
                    if (run >= runs || y >= g.dh) continue;
                    n[t] = remap_run_entries(g, xy, frac, map, y, run, mx[t], mf[t]);
                    remap_run_extent(g, n[t], mx[t], ext);
                }
                const RemapTile T = remap_tile_of(ext);
                const bool fits = remap_tile_fits(T);
                if (!fits) ++A.direct_tiles;
                for (int p = 0; fits && p < remap_tile_pieces(T); ++p) remap_tile_load(g, T, src, f, lds, p);
                for (int t = 0; t < lanes; ++t) {
                    if (n[t] < 0) continue;
                    const int run = bx * REMAP_TILE_RUNS + t % REMAP_TILE_RUNS, y = by * REMAP_TILE_ROWS + t / REMAP_TILE_RUNS;
                    uint32_t px[4];
                    if (fits) remap_run_sample_tile(g, T, lds, n[t], mx[t], mf[t], px);
                    else remap_run_gather(g, src, f, n[t], mx[t], mf[t], px);
                    remap_run_store(g, dst, f, y, run, n[t], px);
                }
            }
    free(lds);
}

// A run as adas_remap_run makes it: `batch` frames from src (src_bytes) into dst (dst_bytes), through tables of n_maps maps and the stream
// table [n_streams], walking every work item.  path: -1 as remap_tile_ok decides for this source pointer, 0 the direct form.  info [8] =
// accesses outside, misaligned accesses, loads, stores, wide (16- and 8-byte) map loads, 12-byte stores, destination bytes (of the first
// dst_bytes) not stored exactly once, and the form taken: 0 direct, else 1 + 16-byte staged source loads + 1000000 * workgroups whose box
// did not fit.  Returns remap_check_sizes' verdict, or REMAP_BAD_MAP for a table word outside the maps.
int emu_remap_run(int sh, int sw, int dh, int dw, int n_streams, int n_maps, const uint8_t* src, long long src_bytes, uint8_t* dst, long long dst_bytes,
                  const int16_t* xy, const uint16_t* frac, const int* table, int batch, int path, long long* info) {
    const int why = remap_check_sizes(sh, sw, dh, dw);
    if (why != REMAP_OK) return why;
    for (int s = 0; s < n_streams; ++s)
        if (remap_check_map(table[s], n_maps) != REMAP_OK) return REMAP_BAD_MAP;
    RemapGeom g;
    g.sh = sh; g.sw = sw; g.dh = dh; g.dw = dw; g.n_streams = n_streams; g.n_maps = n_maps;
    g.map_stride = remap_map_stride(dh, dw);
    A = Audit();
    A.r[0].lo = (const uint8_t*)xy;
    A.r[0].hi = A.r[0].lo + (long long)n_maps * g.map_stride * 4;
    A.r[1].lo = (const uint8_t*)frac;
    A.r[1].hi = A.r[1].lo + (long long)n_maps * g.map_stride * 2;
    A.r[2].lo = dst;
    A.r[2].hi = dst + dst_bytes;
    A.r[3].lo = (const uint8_t*)table;
    A.r[3].hi = A.r[3].lo + (long long)n_streams * 4;
    A.r[6].lo = src;
    A.r[6].hi = src + src_bytes;
    A.hits.assign((size_t)dst_bytes, 0);
    const bool staged = path != 0 && remap_tile_ok(g, src);
    if (staged) run_tiles(g, src, dst, xy, frac, table, batch);
    for (int f = 0; !staged && f < batch; ++f) {
        const int map = remap_ld_table(table, f % n_streams);
        for (int y = 0; y < dh; ++y)
            for (int run = 0; run < remap_runs(dw); ++run) remap_item(g, src, dst, xy, frac, map, f, y, run);
    }
    long long not_once = 0;
    for (uint8_t h : A.hits) not_once += h != 1;
    const long long v[8] = {A.outside, A.misaligned, A.loads, A.stores, A.wide_loads, A.wide_stores, not_once,
                            staged ? 1 + A.staged_loads + 1000000 * A.direct_tiles : 0};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return REMAP_OK;
}

}  // extern "C"
