// TEST SCAFFOLDING ONLY -- never loaded by the product.
// Compiles the two-pass EfficientDet tail of csrc/post_core.h (effdet_scan_chunk over every chunk, then effdet_tail_finish) with g++ as
// single-thread host code (Ctx{tid=0,nthr=1}): chunk geometry, staging offsets, the joining of the per-row segments, the list layout and
// the gather are checked on the GPU-less build container.  Wave prefixes and barriers are only exercised by the -m gpu tests.
#include <cstdlib>
#include <cstring>
#include <vector>
#include "post_core.h"
using namespace adas;

extern "C" {

// reg_all / cls_all: the five levels behind one another ([A][4], [A][nc]).  misalign: floats by which the class logits are shifted off a
// 16-byte boundary before the pass reads them (0..3), so that the staging's head / body / tail split is walked in every phase.
int emu_effdet_tail2(const float* reg_all, const float* cls_all, int in_h, int in_w, int nc, int cap, int max_det, double score_thr, double iou_thr,
                     double anchor_scale, int chunk, int tile, int parts, int misalign, int* count, float* boxes, int* ids, float* confs,
                     int* n_chunks_out, int* chunk_counts) {
    EffdetTailCfg cfg{in_h, in_w, nc, cap, max_det, score_thr, iou_thr, anchor_scale};
    EffdetScanCfg sc{chunk, tile, parts};
    const int total = effdet_total_rows(cfg), n_chunks = effdet_scan_chunks(cfg, sc);
    std::vector<float> shifted((size_t)total * nc + 8);
    float* base = shifted.data();
    while (((uintptr_t)base & 15) != 0) ++base;
    base += misalign & 3;
    memcpy(base, cls_all, (size_t)total * nc * sizeof(float));
    EffdetTailFrame f;
    const float* cls[5];
    size_t row = 0;
    for (int l = 0; l < 5; ++l) {
        f.reg[l] = reg_all + row * 4;
        f.cls[l] = cls[l] = base + row * nc;
        row += (size_t)effdet_level_rows(cfg, l);
    }
    f.count = count; f.boxes = boxes; f.ids = ids; f.confs = confs;
    // lists start out as garbage: every entry the finish pass reads must have been written by the class-max pass
    std::vector<float> l_score(total, -7.f);
    std::vector<int> l_anchor(total, -7), l_cid(total, -7), l_count(n_chunks, -7);
    EffdetScanLists lists{l_score.data(), l_anchor.data(), l_cid.data(), l_count.data()};
    Ctx c{0, 1};
    std::vector<unsigned char> lds(effdet_scan_lds_bytes(sc, nc, 1) + 64);
    for (int k = 0; k < n_chunks; ++k) {
        int level, row0, n, a0;
        effdet_scan_chunk_span(cfg, sc, k, level, row0, n, a0);
        if (n < 1 || n > chunk || row0 + n > effdet_level_rows(cfg, level)) return 1;   // a chunk never straddles two levels
        effdet_scan_chunk(c, cfg, sc, cls, k, lists, lds.data());
        if (l_count[k] < 0 || l_count[k] > n) return 2;
    }
    std::vector<unsigned char> lds2(effdet_finish_lds_bytes(cap, 1) + 64);
    effdet_tail_finish(c, cfg, sc, f, lists, lds2.data());
    *n_chunks_out = n_chunks;
    if (chunk_counts) memcpy(chunk_counts, l_count.data(), (size_t)n_chunks * sizeof(int));
    return 0;
}

}  // extern "C"
