// Stand-alone bounds program of the overlay text (csrc/overlay_text_core.h): for every W,H,frames,align on its command line it allocates the
// frames as one heap block of exactly frames * H * W * 3 bytes (malloc: nothing to spare on either side, so a sanitizer build sees any access
// outside), builds a font and a scene of strings and label boxes clipped at all four edges from a fixed generator, and runs the layout and
// the draw walk of the two device kernels (emu_overlay_text.cpp) over them.  Its own main, nothing preloaded:
//     g++ -O1 -g -fsanitize=address,undefined -I <csrc> text_bounds_main.cpp -o text_bounds && ./text_bounds 101,37,2,1 64,16,1,15
// Prints one line per geometry with the frames' checksum; tests/test_overlay_text_cpu.py reproduces it from tests/text_ref.py.
#include <stdio.h>
#include <stdlib.h>
#include "emu_overlay_text.cpp"

static uint32_t lcg_state;
static uint8_t lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (uint8_t)(lcg_state >> 24);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int W, H, frames, align;
        if (sscanf(argv[a], "%d,%d,%d,%d", &W, &H, &frames, &align) != 4 || W < 1 || H < 1 || frames < 1 || align < 0 || align > 15) {
            fprintf(stderr, "bad geometry %s\n", argv[a]);
            return 2;
        }
        lcg_state = 12345u;
        TextFont fonts[TEXT_FONTS];
        memset(fonts, 0, sizeof(fonts));
        TextFont& f = fonts[0];
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
        uint8_t* atlas = (uint8_t*)malloc((size_t)f.cell_h * f.atlas_w);   // exactly sized too
        if (!atlas) return 3;
        for (int i = 0; i < f.cell_h * f.atlas_w; ++i) atlas[i] = lcg();
        f.atlas = atlas;
        const size_t total = (size_t)frames * H * W * 3;
        uint8_t* buf = (uint8_t*)malloc(total);
        if (!buf) return 3;
        for (size_t i = 0; i < total; ++i) buf[i] = lcg();
        const struct { int x, y; const char* s; } L[TEXT_MAX_LINES] = {{-4, H / 2, "Left edge"}, {W - 7, H / 2 + 3, "Right edge"}, {W / 3, 2, "Top"},
                                                                      {W / 4, H + 4, "Bottom"}, {W + 40, 5, "outside"},    {W / 2, H / 2, ""},
                                                                      {W / 2, H - 4, "a\x7f" "b\xe9"},  {-300, -300, "far"}};
        TextLine lines[TEXT_MAX_LINES];
        memset(lines, 0, sizeof(lines));
        for (int k = 0; k < TEXT_MAX_LINES; ++k) {
            lines[k].x = L[k].x; lines[k].y = L[k].y; lines[k].slot = 0;
            lines[k].color[0] = (uint8_t)(40 * k); lines[k].color[1] = (uint8_t)(255 - 30 * k); lines[k].color[2] = (uint8_t)(7 * k);
            lines[k].len = (uint8_t)strlen(L[k].s);
            memcpy(lines[k].text, L[k].s, lines[k].len);
        }
        const int n_det = 4;
        std::vector<int32_t> xyxy((size_t)frames * n_det * 4), cls((size_t)frames * n_det), cnt(frames, n_det);
        for (int q = 0; q < frames; ++q) {
            const int b[n_det][2] = {{3 + q, 0}, {W / 2, H / 2}, {W - 12, H - 3 + q}, {-6, 14}};
            for (int k = 0; k < n_det; ++k) {
                xyxy[((size_t)q * n_det + k) * 4] = b[k][0]; xyxy[((size_t)q * n_det + k) * 4 + 1] = b[k][1];
                xyxy[((size_t)q * n_det + k) * 4 + 2] = b[k][0] + 9; xyxy[((size_t)q * n_det + k) * 4 + 3] = b[k][1] + 9;
                cls[(size_t)q * n_det + k] = k == 1 ? 9 : k % 2;
            }
        }
        const char names[2][TEXT_LABEL_BYTES] = {"car", "person"};
        const uint32_t colors[2] = {0x0040ffu, 0x19c814u};
        EmuTextArrays arr = {};
        arr.det_xyxy = xyxy.data(); arr.det_cls = cls.data(); arr.det_counts = cnt.data(); arr.det_cap = n_det;
        EmuTextTables tb = {};
        tb.fonts = fonts; tb.det_names = &names[0][0]; tb.n_det_names = 2; tb.det_colors = colors; tb.n_det_colors = 2; tb.lines = lines; tb.n_lines = TEXT_MAX_LINES;
        TextStyle st;
        memset(&st, 0, sizeof(st));
        st.show_ratio = 0.25; st.min_box_area = 10.0; st.max_text_items = 256;
        st.det_label_dx = 2; st.det_label_dy = -7; st.det_box_pad = 3;
        st.label_color[0] = st.label_color[1] = st.label_color[2] = 255;
        std::vector<TextItem> items((size_t)frames * st.max_text_items);
        std::vector<int> heads((size_t)frames * 4);
        emu_text_layout(&arr, &tb, &st, W, H, TEXT_DETECTIONS | TEXT_LINES, frames, st.max_text_items, items.data(), heads.data());
        const int rc = emu_text_draw(buf, frames, H, W, align, fonts, items.data(), heads.data(), st.max_text_items, 8);
        if (rc) {
            fprintf(stderr, "%s: draw walk refused (%d)\n", argv[a], rc);
            return 4;
        }
        unsigned long long s = 0;
        for (size_t i = 0; i < total; ++i) s += (unsigned long long)buf[i] * (unsigned long long)(i + 1);
        printf("%s items %d sum %llu\n", argv[a], heads[0], s);
        free(buf);
        free(atlas);
    }
    return 0;
}
