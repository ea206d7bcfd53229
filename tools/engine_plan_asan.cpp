// engine_plan_asan.cpp -- csrc/engine_load.cpp's read / validate / plan path and csrc/engine_schedule.cpp's plan_schedule under
// AddressSanitizer + UBSan, on the CPU, as a stand-alone program: it is linked from those two files compiled with the sanitizers (so the sanitizer runtime is the program's own) against
// libadas_hip.so for the kernels' predicates, and plans and schedules every table file it is given.  No device is touched.  tools/engine_plan_asan.py
// builds it, writes the tables of three shipped graphs and the damaged tables of tests/test_engine_plan_cpu.py, and runs it.
//   engine_plan_asan <file>.<precision>.tables ...     (precision: ADAS_PREC_* as a number; max_batch 64 and 1 each)
// Exit status 0: every file was planned or refused with an error code; a sanitizer report ends the program with its own status.
#include "../include/adas_hip.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

int main(int argc, char** argv) {
    int planned = 0, refused = 0, scheduled = 0;
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[i]); return 2; }
        std::vector<unsigned char> in;
        unsigned char chunk[65536];
        for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) in.insert(in.end(), chunk, chunk + n);
        fclose(f);
        // an exact-size heap copy: a read past the tables is a read past the allocation
        unsigned char* tables = (unsigned char*)malloc(in.size() ? in.size() : 1);
        memcpy(tables, in.data(), in.size());
        const char* dot = strrchr(argv[i], '.');            // <name>.<precision>.tables
        int prec = -1;
        for (const char* p = dot ? dot - 1 : argv[i]; p >= argv[i] && *p != '.'; --p) prec = *p - '0';
        for (int max_batch : {64, 1}) {
            int32_t n_ops = 0;
            uint64_t weight_bytes = 0;
            int rc = adas_debug_engine_plan(tables, in.size(), prec, max_batch, nullptr, 0, &n_ops, &weight_bytes);
            if (rc == ADAS_OK) {
                std::vector<int64_t> rows((size_t)n_ops * ADAS_PLAN_COLS);
                rc = adas_debug_engine_plan(tables, in.size(), prec, max_batch, rows.data(), n_ops, &n_ops, &weight_bytes);
            }
            // the launch schedule of the same tables (csrc/engine_schedule.cpp), at the engine's own batch size and at one frame
            for (int batch : {max_batch, 1}) {
                if (rc != ADAS_OK) break;
                int32_t n_steps = 0;
                std::vector<int32_t> step_of(n_ops), role(n_ops);
                std::vector<char> labels((size_t)n_ops * ADAS_LABEL_CAP);
                rc = adas_debug_engine_schedule(tables, in.size(), prec, max_batch, batch, step_of.data(), role.data(), labels.data(), n_ops, &n_ops, &n_steps);
                if (rc == ADAS_OK) ++scheduled;
            }
            if (rc == ADAS_OK) ++planned;
            else if (rc == ADAS_ERR_FORMAT) ++refused;
            else { fprintf(stderr, "%s: error %d: %s\n", argv[i], rc, adas_last_error()); free(tables); return 3; }
        }
        free(tables);
    }
    printf("engine_plan_asan: %d planned, %d schedules, %d refused, no sanitizer report\n", planned, scheduled, refused);
    return 0;
}
