// Host build of the scaling stage's rules (csrc/scale_core.h; g++, one thread): the work the device kernels run -- scale_item over every
// canvas and item index, or the staged blocks' phases lane by lane in the kernel's order, through the same address arithmetic (S8) -- with
// every load and store audited: a source load must lie inside the
// `batch` source frames, a store inside the canvases the run owns, a state load inside the state array, all inside the arrays the caller
// handed over (an access that does not is counted and not made), a 16-byte store must be aligned as the device needs it, and every canvas
// byte must be stored exactly once.  The CPU suite compares the canvases with tests/scale_ref.py, the GPU suite the device's canvases with
// these.  Test scaffolding only; never loaded by the product.
#include <stddef.h>
#include <stdlib.h>
#include <vector>
#define SCALE_AUDIT 1
#include "scale_core.h"

using namespace adas;

namespace {
struct Audit {
    const uint8_t *src = nullptr, *src_hi = nullptr;
    const uint8_t *state = nullptr, *state_hi = nullptr;
    uint8_t *dst = nullptr, *dst_hi = nullptr;
    std::vector<uint8_t> hits;   // stores per canvas byte, saturating at 255
    long long outside = 0, misaligned = 0, loads = 0, stores = 0, wide = 0, state_loads = 0;
} A;
}  // namespace

namespace adas {
bool scale_audit(const void* p, int bytes, int align, int kind) {
    const uint8_t* q = (const uint8_t*)p;
    const uint8_t* lo = kind == 1 ? A.dst : (kind == 2 ? A.state : A.src);
    const uint8_t* hi = kind == 1 ? A.dst_hi : (kind == 2 ? A.state_hi : A.src_hi);
    const bool inside = lo && q >= lo && q + bytes <= hi;
    if (!inside) ++A.outside;
    if ((uintptr_t)q % (uintptr_t)align) ++A.misaligned;
    if (kind == 1 && bytes > 1) ++A.wide;
    ++(kind == 1 ? A.stores : (kind == 2 ? A.state_loads : A.loads));
    if (inside && kind == 1)
        for (int i = 0; i < bytes; ++i) {
            uint8_t& h = A.hits[(size_t)(q - lo) + i];
            if (h < 255) ++h;
        }
    return inside;   // any other access is counted, not made
}
}  // namespace adas

namespace {
template <int MODE>
void run_items(const ScaleParams& p, bool vec, int batch, const uint8_t* src, const uint8_t* state, long long stride, uint8_t* dst) {
    const uint32_t items = scale_items_per_canvas(p, vec);
    const int canvases = scale_canvases(p, batch);
    for (int k = 0; k < canvases; ++k)
        for (uint32_t t = 0; t < items; ++t) scale_item<MODE>(p, vec, batch, src, state, stride, dst, k, t);
}

// the staged path as scale_area_kernel runs it: the phases of scale_core.h in the kernel's order, a loop over the lanes where the kernel has
// a barrier; the LDS is a heap block of exactly the launch's dynamic size
void run_blocks(const ScaleParams& p, const ScaleStaged& sg, int batch, const uint8_t* src, const uint8_t* state, long long stride, uint8_t* dst) {
    const uint32_t blocks = scale_staged_blocks_per_canvas(p, sg);
    const int canvases = scale_canvases(p, batch);
    uint8_t* lds = (uint8_t*)malloc((size_t)scale_staged_lds_bytes(sg));
    uint8_t* lds_out = lds + 2 * sg.lds_row;
    static uint32_t acc[SCALE_BLOCK][3];
    static ScalePiece v[SCALE_BLOCK][SCALE_STAGE_PIECES];
    for (int k = 0; k < canvases; ++k)
        for (uint32_t b = 0; b < blocks; ++b) {
            const ScaleBlock B = scale_block(p, sg, batch, state, stride, k, b);
            memset(acc, 0, sizeof(acc));
            memset(lds, 0xEE, (size_t)scale_staged_lds_bytes(sg));   // what an earlier block left: nothing may depend on it
            if (B.y_lo < B.y_hi)
                for (int t = 0; t < SCALE_BLOCK; ++t)
                    for (int i = 0; i < SCALE_STAGE_PIECES; ++i) scale_stage_write(sg, lds, t, i, scale_stage_load(p, B, src, B.y_lo, t, i));
            for (int sy = B.y_lo; sy < B.y_hi; ++sy) {
                const int cur = (sy - B.y_lo) & 1;
                for (int t = 0; t < SCALE_BLOCK; ++t) {
                    if (sy + 1 < B.y_hi)
                        for (int i = 0; i < SCALE_STAGE_PIECES; ++i) v[t][i] = scale_stage_load(p, B, src, sy + 1, t, i);
                    scale_block_accumulate(p, B, lds + cur * sg.lds_row, sy, t, acc[t]);
                }
                if (sy + 1 < B.y_hi)
                    for (int t = 0; t < SCALE_BLOCK; ++t)
                        for (int i = 0; i < SCALE_STAGE_PIECES; ++i) scale_stage_write(sg, lds + (cur ^ 1) * sg.lds_row, t, i, v[t][i]);
            }
            for (int t = 0; t < SCALE_BLOCK; ++t) scale_block_finish(p, B, lds_out, t, acc[t]);
            for (int t = 0; t < SCALE_BLOCK; ++t) scale_block_store(B, lds_out, dst, t);
        }
    free(lds);
}
}  // namespace

extern "C" {

// sizeof and the offsets of src_w, src_h, dst_w, dst_h, mode, cols, rows, border, background, border_bgr
void emu_scale_params_layout(int* out) {
    const int v[11] = {(int)sizeof(ScaleParams),         (int)offsetof(ScaleParams, src_w), (int)offsetof(ScaleParams, src_h),
                       (int)offsetof(ScaleParams, dst_w), (int)offsetof(ScaleParams, dst_h), (int)offsetof(ScaleParams, mode),
                       (int)offsetof(ScaleParams, cols),  (int)offsetof(ScaleParams, rows),  (int)offsetof(ScaleParams, border),
                       (int)offsetof(ScaleParams, background), (int)offsetof(ScaleParams, border_bgr)};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}

int emu_scale_check(const ScaleParams* p) { return scale_check(*p); }
long long emu_scale_canvas_bytes(const ScaleParams* p) { return scale_check(*p) == SCALE_OK ? scale_canvas_bytes(*p) : 0; }
int emu_scale_canvases(const ScaleParams* p, int batch) { return scale_check(*p) == SCALE_OK ? scale_canvases(*p, batch) : 0; }
int emu_scale_vector_ok(const ScaleParams* p, const void* src, const void* dst) { return scale_vector_ok(*p, src, dst) ? 1 : 0; }
// the run's path for these two pointers, as scale_path decides: 0 generic items, 1 vector items, 2 staged blocks
int emu_scale_path(const ScaleParams* p, const void* src, const void* dst) {
    ScaleStaged sg;
    return scale_path(*p, src, dst, &sg);
}

// S5's span and weights of destination index d: lo, hi and the weights of lo .. hi - 1 into w (room for sn)
void emu_scale_area_weights(int d, int dn, int sn, int* lo, int* hi, int* w) {
    scale_area_span(d, dn, sn, lo, hi);
    for (int s = *lo; s < *hi; ++s) w[s - *lo] = scale_area_weight(s, d, dn, sn);
}

// A run as adas_scale_run makes it: `batch` frames from src into the canvases at dst, walking every work item.  [src, src + src_bytes),
// [dst, dst + dst_bytes) and [state, state + state_bytes) are what the items may touch.  path: -1 as scale_path decides, 0 generic items.
// info [8] = the path taken (scale_path's), accesses outside the arrays, misaligned accesses, source loads, stores, 16-byte stores, state
// loads, canvas bytes (of the first dst_bytes) not stored exactly once.  Returns scale_check's verdict (nothing runs unless it is 0).
int emu_scale_run(const ScaleParams* pp, const uint8_t* src, long long src_bytes, const uint8_t* state, long long state_bytes, long long state_stride,
                  uint8_t* dst, long long dst_bytes, int batch, int path, long long* info) {
    const ScaleParams p = *pp;
    const int why = scale_check(p);
    if (why != SCALE_OK) return why;
    ScaleStaged sg;
    const int way = path == 0 ? SCALE_PATH_GENERIC : scale_path(p, src, dst, &sg);
    const bool vec = way == SCALE_PATH_PIECES;
    A = Audit();
    A.src = src;
    A.src_hi = src + src_bytes;
    A.state = state;
    A.state_hi = state ? state + state_bytes : nullptr;
    A.dst = dst;
    A.dst_hi = dst + dst_bytes;
    A.hits.assign((size_t)dst_bytes, 0);
    if (way == SCALE_PATH_STAGED)
        run_blocks(p, sg, batch, src, state, state_stride, dst);
    else if (p.mode == SCALE_MODE_LINEAR)
        run_items<SCALE_MODE_LINEAR>(p, vec, batch, src, state, state_stride, dst);
    else
        run_items<SCALE_MODE_AREA>(p, vec, batch, src, state, state_stride, dst);
    if (info) {
        long long not_once = 0;
        for (uint8_t h : A.hits) not_once += h != 1;
        const long long v[8] = {way, A.outside, A.misaligned, A.loads, A.stores, A.wide, A.state_loads, not_once};
        for (int i = 0; i < 8; ++i) info[i] = v[i];
    }
    return SCALE_OK;
}

}  // extern "C"
