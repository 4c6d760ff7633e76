// stage_host_check.cpp - the host side of the stage API (stages.cpp) that runs before any device call, as a stand-alone program for a
// sanitizer build on a machine WITHOUT a GPU: argument validation of every stcn_stage_* / stcn_aggregate_wbg / stcn_fusion_model_create
// export and the growth rule of the bank staging.  Build and run:  make -C eva_vos_amd/csrc stage-host-check
// (host code with -fsanitize=address,undefined; the program links the library's objects, nothing is loaded into another process).
#include <cstdio>
#include <cstring>

#include "../../eva_vos_amd/csrc/engine.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s   (last error: %s)\n", __FILE__, __LINE__, #cond, stcn_last_error()); } } while (0)
static bool says(const char *what) { return std::strstr(stcn_last_error(), what) != nullptr; }

int main() {
    float dummy[4] = {0.f, 0.f, 0.f, 0.f};
    float *p = dummy;                       // a valid host pointer: never followed, every call fails its checks first
    stcn_stage *st = nullptr;
    EXPECT(stcn_stage_create(nullptr, 128, 160, 1, nullptr, &st) == STCN_E_INVALID && says("null") && !st);
    EXPECT(stcn_stage_create(nullptr, 100, 160, 1, nullptr, &st) == STCN_E_INVALID && says("nh=100"));
    EXPECT(stcn_stage_create(nullptr, 128, 0, 1, nullptr, &st) == STCN_E_INVALID && says("nw=0"));
    EXPECT(stcn_stage_create(nullptr, 128, 160, 0, nullptr, &st) == STCN_E_INVALID && says("max_objects=0"));
    EXPECT(stcn_stage_create(nullptr, 128, 160, STCN_MAX_OBJECTS + 1, nullptr, &st) == STCN_E_INVALID && says("max_objects=33"));
    EXPECT(stcn_stage_destroy(nullptr) == STCN_OK);
    const int bad_k[] = {0, -1, STCN_MAX_OBJECTS + 1};
    for (int k : bad_k) {
        EXPECT(stcn_stage_encode_value(nullptr, p, p, p, k, p) == STCN_E_INVALID && says("k="));
        EXPECT(stcn_stage_segment(nullptr, p, 80, p, 80, 0, 1, k, p, p, p, p, p) == STCN_E_INVALID && says("k="));
        EXPECT(stcn_aggregate_wbg(nullptr, p, k, 100, 1, 0, p) == STCN_E_INVALID && says("k="));
    }
    EXPECT(stcn_stage_segment(nullptr, p, 80, p, 80, 0, 0, 1, p, p, p, p, p) == STCN_E_INVALID && says("T=0"));
    EXPECT(stcn_stage_attention(nullptr, p, p, p, p, 0, p) == STCN_E_INVALID && says("b=0"));
    EXPECT(stcn_stage_attention(nullptr, p, p, p, p, STCN_MAX_OBJECTS + 2, p) == STCN_E_INVALID && says("b=34"));
    EXPECT(stcn_stage_encode_key(nullptr, p, p, p, p, p, p) == STCN_E_INVALID && says("null"));
    EXPECT(stcn_stage_encode_value(nullptr, p, p, p, 1, p) == STCN_E_INVALID && says("null"));
    EXPECT(stcn_stage_segment(nullptr, p, 80, p, 80, 0, 1, 1, p, p, p, p, p) == STCN_E_INVALID && says("null"));
    EXPECT(stcn_stage_attention(nullptr, p, p, p, p, 2, p) == STCN_E_INVALID && says("null"));
    EXPECT(stcn_stage_fusion(nullptr, p, p, p, p, 0.5f, 0.5f, p) == STCN_E_INVALID && says("null"));
    EXPECT(stcn_aggregate_wbg(nullptr, nullptr, 1, 100, 1, 0, p) == STCN_E_INVALID);
    EXPECT(stcn_aggregate_wbg(nullptr, p, 1, 100, 1, 0, nullptr) == STCN_E_INVALID);
    EXPECT(stcn_aggregate_wbg(nullptr, p, 1, 0, 1, 0, p) == STCN_E_INVALID && says("npix=0"));
    stcn_model *m = nullptr;
    EXPECT(stcn_fusion_model_create(0, nullptr, 12, &m) == STCN_E_INVALID && !m);
    stcn_weight_desc d{};
    EXPECT(stcn_fusion_model_create(0, &d, 0, &m) == STCN_E_INVALID);
    EXPECT(stcn_fusion_model_create(0, &d, 1, nullptr) == STCN_E_INVALID);
    EXPECT(stcn_fusion_model_create(0, &d, 1, &m) == STCN_E_INVALID && says("descriptor") && !m);      // a descriptor without name / data
    EXPECT(stcn_test_transpose(nullptr, p, p, 1, 8, 6, 8, 0, 1) == STCN_E_INVALID);
    EXPECT(stcn_test_transpose(nullptr, p, p, 1, 8, 4, 7, 0, 1) == STCN_E_INVALID);
    // a bank of 2^24 rows (the read kernels' key descriptor, (unsigned)N * 256 bytes, wraps there) is refused where the hooks fill a read
    EXPECT(stcn_test_memory_read(nullptr, p, p, p, 1 << 24, 97, 1, nullptr, nullptr, p) == STCN_E_INVALID && says("2^24"));
    float ms = 0.f;
    EXPECT(stcn_bench_memory_read(nullptr, p, p, p, 1 << 24, 97, 1, 1, p, &ms, nullptr) == STCN_E_INVALID && says("2^24"));
    // the bank staging: never shrinks, holds what is asked, and a memory growing one frame per call (80 rows at a time up to 100 frames)
    // allocates a logarithmic number of times
    EXPECT(stcn::stage_grow(0, 80) == 80 && stcn::stage_grow(80, 80) == 80 && stcn::stage_grow(80, 10) == 80 && stcn::stage_grow(80, 81) == 160 && stcn::stage_grow(80, 1000) == 1000);
    long cap = 0; int grows = 0;
    for (long rows = 80; rows <= 8000; rows += 80) { const long c = stcn::stage_grow(cap, rows); EXPECT(c >= rows && c >= cap); if (c != cap) ++grows; cap = c; }
    EXPECT(grows <= 8 && cap < 2 * 8000);
    std::printf(failures ? "stage_host_check: %d FAILED\n" : "stage_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
