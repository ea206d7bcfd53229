// Stand-alone bounds program of the scaling stage (csrc/scale_core.h): for every src_w,src_h,dst_w,dst_h,mode,cols,rows,batch,border,align on
// its command line it allocates the source frames, the states and the canvases as heap blocks that end exactly where the data ends (malloc,
// the data `align` bytes behind the block's start: nothing to spare behind them, so a sanitizer build sees any access outside), fills the
// frames from a fixed generator and walks the device kernel's work items (emu_scale.cpp) over them.  Its own main, nothing preloaded:
//     g++ -O1 -g -fsanitize=address,undefined -I <csrc> scale_bounds_main.cpp -o scale_bounds && ./scale_bounds 50,18,25,9,0,2,2,5,1,1
// Prints one line per case with the canvases' checksum and the audit's counts; tests/test_scale_cpu.py reproduces it from tests/scale_ref.py.
#include <stdio.h>
#include <stdlib.h>
#include "emu_scale.cpp"

static uint32_t lcg_state;
static uint8_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (uint8_t)(lcg_state >> 24);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int v[10];
        if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9) != 10 || v[7] < 1 || v[9] < 0 ||
            v[9] > 15) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        ScaleParams p;
        memset(&p, 0, sizeof(p));
        p.src_w = v[0]; p.src_h = v[1]; p.dst_w = v[2]; p.dst_h = v[3]; p.mode = v[4]; p.cols = v[5]; p.rows = v[6]; p.border = v[8];
        const int batch = v[7], align = v[9];
        const uint8_t bg[3] = {9, 8, 7}, col[4][3] = {{0, 255, 255}, {0, 255, 0}, {0, 102, 255}, {0, 0, 255}};
        memcpy(p.background, bg, 3);
        for (int k = 0; k < 4; ++k) memcpy(p.border_bgr[k], col[k], 3);
        if (scale_check(p) != SCALE_OK) {
            fprintf(stderr, "refused case %s: %d\n", argv[a], scale_check(p));
            return 2;
        }
        const long long ns = scale_frame_bytes(p) * batch, nd = scale_canvas_bytes(p) * scale_canvases(p, batch);
        uint8_t* src_block = (uint8_t*)malloc((size_t)ns + align);
        uint8_t* dst_block = (uint8_t*)malloc((size_t)nd + align);
        int32_t* states = (int32_t*)malloc(sizeof(int32_t) * batch);
        if (!src_block || !dst_block || !states) return 3;
        uint8_t *src = src_block + align, *dst = dst_block + align;
        lcg_state = 12345u;
        for (long long i = 0; i < ns; ++i) src[i] = lcg();
        for (int f = 0; f < batch; ++f) states[f] = f % 6 - 1;   // -1, 0, 1, 2, 3, 4: both sides of the enum
        memset(dst, 0xA5, (size_t)nd);
        long long info[8];
        const int rc = emu_scale_run(&p, src, ns, (const uint8_t*)states, (long long)sizeof(int32_t) * batch, 4, dst, nd, batch, -1, info);
        if (rc) return 4;
        uint32_t sum = 2166136261u;   // FNV-1a over the canvases
        for (long long i = 0; i < nd; ++i) sum = (sum ^ dst[i]) * 16777619u;
        printf("%s %08x path %lld outside %lld misaligned %lld not_once %lld\n", argv[a], sum, info[0], info[1], info[2], info[7]);
        free(src_block);
        free(dst_block);
        free(states);
    }
    return 0;
}
