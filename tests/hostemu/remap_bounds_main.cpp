// Stand-alone bounds program of the rectification stage (csrc/remap_core.h): for every src_w,src_h,dst_w,dst_h,n_streams,n_maps,batch,lens,align
// on its command line it allocates the source frames, the two map tables, the stream table and the destination frames as heap blocks that end
// exactly where the data ends (malloc, the frames `align` bytes behind the block's start: nothing to spare behind them, so a sanitizer build
// sees any access outside -- warp_sample's taps included), builds every map with the build kernel's work items (lens 0 identity, 1 barrel,
// 2 rational, 3 pincushion, map m with its centre moved by m pixels; lens 4: the crafted table of saturated and edge entries), fills the frames
// from a fixed generator and walks the remap kernel's work items (emu_remap.cpp) over them.  Its own main, nothing preloaded:
//     g++ -O1 -g -fsanitize=address,undefined -I <csrc> -I <include> remap_bounds_main.cpp -o remap_bounds && ./remap_bounds 29,23,37,25,3,2,5,1,1
// Prints one line per case with the frames' checksum and the audit's counts; tests/test_remap_cpu.py reproduces it from tests/remap_ref.py.
#include <stdio.h>
#include <stdlib.h>
#include "emu_remap.cpp"

static uint32_t lcg_state;
static uint8_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (uint8_t)(lcg_state >> 24);
}

static const double LENS[4][8] = {{0, 0, 0, 0, 0, 0, 0, 0},
                                  {-0.2, 0.05, 0.001, -0.001, 0, 0, 0, 0},
                                  {-0.2, 0.05, 0.001, -0.001, 0.01, 0.1, 0.02, 0.003},
                                  {0.15, 0.02, 0.001, -0.001, 0, 0, 0, 0}};

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int v[9];
        if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) != 9 || v[4] < 1 || v[5] < 1 || v[6] < 1 ||
            v[7] < 0 || v[7] > 4 || v[8] < 0 || v[8] > 15 || remap_check_sizes(v[1], v[0], v[3], v[2]) != REMAP_OK) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        const int sw = v[0], sh = v[1], dw = v[2], dh = v[3], n_streams = v[4], n_maps = v[5], batch = v[6], lens = v[7], align = v[8];
        const long long stride = remap_map_stride(dh, dw), n = (long long)dh * dw, entries = (n_maps - 1) * stride + n;
        const long long ns = (long long)sh * sw * 3 * batch, nd = n * 3 * batch;
        uint8_t* src_block = (uint8_t*)malloc((size_t)ns + align);
        uint8_t* dst_block = (uint8_t*)malloc((size_t)nd + align);
        int16_t* xy = (int16_t*)malloc((size_t)entries * 4);
        uint16_t* frac = (uint16_t*)malloc((size_t)entries * 2);
        int* table = (int*)malloc(sizeof(int) * n_streams);
        if (!src_block || !dst_block || !xy || !frac || !table) return 3;
        memset(xy, 0, (size_t)entries * 4);
        memset(frac, 0, (size_t)entries * 2);
        long long bad = 0;
        for (int m = 0; m < n_maps; ++m) {
            if (lens < 4) {
                RemapCamera c;
                memset(&c, 0, sizeof(c));
                c.K[0] = c.K[1] = c.new_K[0] = c.new_K[1] = 20.0;
                c.K[2] = (sw - 1) * 0.5; c.K[3] = (sh - 1) * 0.5;
                c.new_K[2] = (dw - 1) * 0.5 + m; c.new_K[3] = (dh - 1) * 0.5;
                memcpy(c.D, LENS[lens], sizeof(c.D));
                c.R[0] = c.R[4] = c.R[8] = 1.0;
                long long info[4];
                if (emu_remap_build(&c, dh, dw, m, n_maps, xy, frac, info)) return 4;
                bad += info[0] + info[1] + info[3];
            } else {
                const int SX[9] = {-32768, -2, -1, 0, sw - 3, sw - 2, sw - 1, sw, 32767}, SY[9] = {-32768, -2, -1, 0, sh - 3, sh - 2, sh - 1, sh, 32767};
                const int F[4] = {0, 1, 16, 31};
                for (long long i = 0; i < n; ++i) {
                    const long long e = m * stride + i, j = i + m;
                    xy[2 * e] = (int16_t)SX[j % 9];
                    xy[2 * e + 1] = (int16_t)SY[(j / 9) % 9];
                    frac[e] = (uint16_t)(F[(j / 324) % 4] * 32 + F[(j / 81) % 4] + ((j & 1) ? 0xfc00 : 0));   // the top 6 bits are ignored (U1)
                }
            }
        }
        for (int s = 0; s < n_streams; ++s) table[s] = remap_default_map(s, n_maps);
        uint8_t *src = src_block + align, *dst = dst_block + align;
        lcg_state = 12345u;
        for (long long i = 0; i < ns; ++i) src[i] = lcg();
        memset(dst, 0xA5, (size_t)nd);
        long long info[8];
        if (emu_remap_run(sh, sw, dh, dw, n_streams, n_maps, src, ns, dst, nd, xy, frac, table, batch, -1, info)) return 5;
        uint32_t sum = 2166136261u;   // FNV-1a over the frames
        for (long long i = 0; i < nd; ++i) sum = (sum ^ dst[i]) * 16777619u;
        printf("%s %08x staged %d outside %lld misaligned %lld not_once %lld build_bad %lld\n", argv[a], sum, info[7] ? 1 : 0, info[0], info[1], info[6], bad);
        free(src_block);
        free(dst_block);
        free(xy);
        free(frac);
        free(table);
    }
    return 0;
}
