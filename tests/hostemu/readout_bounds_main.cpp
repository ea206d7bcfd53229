// Stand-alone bounds program of the bird view's readouts (csrc/overlay_readout_core.h): for every W,H,frames,align,zoom,veh_pos,offset,curvature
// on its command line it allocates the bird images as one heap block of frames * H * W * 3 bytes between two runs of 32 guard bytes, builds a
// font from a fixed generator, and runs the layout and the draw walk of the two device kernels (emu_overlay_readout.cpp) over them; frame q
// is drawn at veh_pos + 7 q.  Guard bytes that changed, or a walk that refuses, end it with a non-zero status.  Its own main, nothing preloaded:
//     g++ -O1 -g -fsanitize=address,undefined -I <csrc> -I <include> readout_bounds_main.cpp -o readout_bounds && ./readout_bounds 101,37,2,1,2,50.5,0.25,1234.56
// Prints one line per case with the frames' checksum; tests/test_overlay_readout_cpu.py reproduces it from tests/readout_ref.py.
#include <stdio.h>
#include <stdlib.h>
#include "emu_overlay_readout.cpp"

static uint32_t lcg_state;
static uint8_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (uint8_t)(lcg_state >> 24);
}

int main(int argc, char** argv) {
    const int GUARD = 32;
    for (int a = 1; a < argc; ++a) {
        int W, H, frames, align, zoom;
        double veh, off, cur;
        if (sscanf(argv[a], "%d,%d,%d,%d,%d,%lf,%lf,%lf", &W, &H, &frames, &align, &zoom, &veh, &off, &cur) != 8 || W < 1 || H < 1 || frames < 1 || align < 0 ||
            align > 15 || zoom < 1 || zoom > READOUT_MAX_ZOOM) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        lcg_state = 12345u;
        TextFont f;
        memset(&f, 0, sizeof(f));
        f.cell_h = 9; f.baseline_row = 6; f.size_h = 7; f.size_w_extra = 0x18000; f.set = 1; f.scale = 1.0;
        int x = 1;
        for (int g = 0; g < TEXT_GLYPHS; ++g) {
            f.glyph_w[g] = g ? 1 + (g * 7) % 9 : 0;
            f.glyph_x[g] = x;
            x += f.glyph_w[g] + 1;
            f.bearing_x[g] = (g * 5) % 5 - 2;
            f.advance[g] = ((f.glyph_w[g] + 1) << 16) + (g * 4099) % 65536;
        }
        f.atlas_w = x;
        uint8_t* atlas = (uint8_t*)malloc((size_t)f.cell_h * f.atlas_w);   // exactly sized
        if (!atlas) return 3;
        for (int i = 0; i < f.cell_h * f.atlas_w; ++i) atlas[i] = lcg();
        f.atlas = atlas;
        const size_t total = (size_t)frames * H * W * 3;
        uint8_t* block = (uint8_t*)malloc(total + 2 * GUARD);
        if (!block) return 3;
        memset(block, 0xA5, GUARD);
        memset(block + GUARD + total, 0x5A, GUARD);
        uint8_t* buf = block + GUARD;
        for (size_t i = 0; i < total; ++i) buf[i] = lcg();
        ReadoutStyle st;
        readout_default_style(&st);
        st.zoom = zoom;
        st.offset_x = -3; st.offset_y = 9 * zoom / 2;          // clipped at the left and the top
        st.radius_x = W / 2; st.radius_y = H - 2;              // and at the right and the bottom
        std::vector<int> dir(frames);
        std::vector<double> vv(frames), oo(frames), cc(frames);
        for (int q = 0; q < frames; ++q) {
            dir[q] = q == 1 ? 0 : 3;                           // frame 1 fails the gate
            vv[q] = veh + 7.0 * q; oo[q] = off; cc[q] = cur;
        }
        std::vector<ReadoutRecord> recs(frames);
        emu_readout_layout(dir.data(), vv.data(), cc.data(), oo.data(), frames, W, H, &st, &f, recs.data());
        const int rc = emu_readout_draw(buf, frames, H, W, align, &st, &f, recs.data(), 8);
        if (rc) {
            fprintf(stderr, "%s: draw walk refused (%d)\n", argv[a], rc);
            return 4;
        }
        for (int i = 0; i < GUARD; ++i)
            if (block[i] != 0xA5 || block[GUARD + total + i] != 0x5A) {
                fprintf(stderr, "%s: guard byte %d changed\n", argv[a], i);
                return 5;
            }
        unsigned long long s = 0;
        for (size_t i = 0; i < total; ++i) s += (unsigned long long)buf[i] * (unsigned long long)(i + 1);
        printf("%s flags %d sum %llu\n", argv[a], recs[0].flags, s);
        free(block);
        free(atlas);
    }
    return 0;
}
