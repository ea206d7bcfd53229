// Stand-alone bounds program of the YUV conversion (csrc/yuv_core.h): for every geometry on its command line it allocates a source of exactly
// (batch - 1) * frame_stride + yuv_frame_extent bytes and a destination of exactly batch * w * h * 3 bytes (malloc: nothing to spare on
// either side, so a sanitizer build sees any access outside), fills the source from a fixed generator, walks every work item as the device
// kernel does, and folds the destination into a checksum.  Its own main, nothing preloaded:
//     g++ -O1 -g -fsanitize=address,undefined -I <csrc> yuv_bounds_main.cpp -o yuv_bounds && ./yuv_bounds GEOMETRY...
// GEOMETRY = format,matrix,w,h,batch,frame_stride,y_offset,y_pitch,u_offset,u_pitch,v_offset,v_pitch.  Prints one line per geometry and the
// checksum; tests/test_yuv_cpu.py reproduces the checksum from tests/yuv_ref.py.
#include <stdio.h>
#include <stdlib.h>
#include "yuv_core.h"

using namespace adas;

template <int FORMAT>
static void run_items(const YuvGeom& g, bool vec, const uint8_t* src, uint8_t* dst, int batch) {
    const uint32_t items = (uint32_t)yuv_items_per_frame(g, vec);
    for (int f = 0; f < batch; ++f)
        for (uint32_t t = 0; t < items; ++t) {
            if (g.matrix == YUV_MATRIX_FULL)
                yuv_item<FORMAT, YUV_MATRIX_FULL>(g, vec, src, dst, f, t);
            else
                yuv_item<FORMAT, YUV_MATRIX_VIDEO>(g, vec, src, dst, f, t);
        }
}

int main(int argc, char** argv) {
    unsigned long long sum = 0;
    for (int a = 1; a < argc; ++a) {
        long long v[12];
        if (sscanf(argv[a], "%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10,
                   v + 11) != 12) {
            fprintf(stderr, "bad geometry %s\n", argv[a]);
            return 2;
        }
        YuvGeom g;
        g.format = (int)v[0]; g.matrix = (int)v[1]; g.w = (int)v[2]; g.h = (int)v[3];
        const int batch = (int)v[4];
        g.frame_stride = v[5]; g.y_offset = v[6]; g.y_pitch = v[7]; g.u_offset = v[8]; g.u_pitch = v[9]; g.v_offset = v[10]; g.v_pitch = v[11];
        const int why = yuv_check(g);
        if (why != YUV_OK || batch < 1) {
            fprintf(stderr, "geometry %s refused (%d)\n", argv[a], why);
            return 2;
        }
        const size_t ns = (size_t)(batch - 1) * (size_t)g.frame_stride + (size_t)yuv_frame_extent(g), nd = (size_t)batch * (size_t)yuv_out_bytes(g.w, g.h);
        uint8_t* src = (uint8_t*)malloc(ns);
        uint8_t* dst = (uint8_t*)malloc(nd);
        if (!src || !dst) return 3;
        uint32_t x = 12345u + (uint32_t)a;
        for (size_t i = 0; i < ns; ++i) {
            x = x * 1664525u + 1013904223u;
            src[i] = (uint8_t)(x >> 24);
        }
        for (size_t i = 0; i < nd; ++i) dst[i] = 0;
        const bool vec = yuv_vector_ok(g, src, dst);
        switch (g.format) {
            case YUV_NV12: run_items<YUV_NV12>(g, vec, src, dst, batch); break;
            case YUV_NV21: run_items<YUV_NV21>(g, vec, src, dst, batch); break;
            case YUV_I420: run_items<YUV_I420>(g, vec, src, dst, batch); break;
            case YUV_YUYV: run_items<YUV_YUYV>(g, vec, src, dst, batch); break;
            default: run_items<YUV_UYVY>(g, vec, src, dst, batch); break;
        }
        unsigned long long s = 0;
        for (size_t i = 0; i < nd; ++i) s += (unsigned long long)dst[i] * (unsigned long long)(i + 1);
        sum = sum * 31ull + s;
        printf("%s %s src %zu dst %zu sum %llu\n", argv[a], vec ? "vector" : "generic", ns, nd, s);
        free(src);
        free(dst);
    }
    printf("checksum %llu\n", sum);
    return 0;
}
