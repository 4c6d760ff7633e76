// stage_host_check.cpp - the host side of the stage API (stages.cpp) that runs before any device call, as a stand-alone program for a
// sanitizer build on a machine WITHOUT a GPU: argument validation of every stcn_stage_* / stcn_aggregate_wbg / stcn_fusion_model_create
// export, the growth rule of the bank staging and the engine plan (plan_engine, bank_slots_needed) at its extremes.  Build and run:  make -C eva_vos_amd/csrc stage-host-check
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
    // the key-cache slot layout: ten fields, increasing, each at a multiple of 4 floats, nothing behind the last one, and as many floats as
    // the formula engine_alloc_common used to spell out beside slot_ptrs' walk
    const int frames[][2] = {{128, 160}, {480, 864}, {16, 16}};
    for (const auto &f : frames) {
        stcn::Dims dm; dm.set(f[0], f[1]);
        const stcn::SlotLayout l = stcn::slot_layout(dm);
        for (int i = 0; i < stcn::SLOT_FIELDS; ++i) {
            EXPECT(l.off[i] % 4 == 0 && l.ext[i] > 0);
            if (i) EXPECT(l.off[i] > l.off[i - 1] && l.off[i] >= l.off[i - 1] + l.ext[i - 1]);
        }
        EXPECT(l.off[0] == 0 && l.off[stcn::SLOT_VC] + l.ext[stcn::SLOT_VC] == l.total);
        EXPECT(l.total == (size_t)dm.hw16 * (64 + 512 + 1024) + (size_t)(dm.hw16 + 3) / 4 * 4 + (size_t)dm.hw8 * 512 + (size_t)dm.hw4 * 256 + (size_t)4 * dm.hw16 * 512);
    }
    {   // the retire queue hands out the smallest retired buffer that fits, none when nothing fits, and removes exactly what it handed out.
        // The entries are host addresses that stand for buffers: every one is taken back (release) before an owner could free it
        static char mem[4];
        const size_t sizes[4] = {300, 100, 200, 100};
        stcn::RetireQueue q;
        for (int i = 0; i < 4; ++i) { stcn::PoolBuf<> b; b.p = &mem[i]; q.push(std::move(b), sizes[i]); }
        stcn::PoolBuf<> got; size_t cap = 0;
        EXPECT(!q.take_fitting(301, &got, &cap) && !got && q.bufs.size() == 4);
        EXPECT(q.take_fitting(150, &got, &cap) && got.release() == &mem[2] && cap == 200 && q.bufs.size() == 3);
        EXPECT(q.take_fitting(100, &got, &cap) && got.release() == &mem[1] && cap == 100 && q.bufs.size() == 2);      // of two equal ones the older
        EXPECT(q.bufs[0].first.p == &mem[0] && q.bufs[1].first.p == &mem[3]);
        EXPECT(q.take_fitting(1, &got, &cap) && got.release() == &mem[3] && cap == 100);
        EXPECT(!q.take_fitting(301, &got, &cap) && q.take_fitting(300, &got, &cap) && got.release() == &mem[0] && q.bufs.empty());
        EXPECT(!q.take_fitting(0, &got, &cap));
    }
    {   // the engine plan at its extremes: one frame, one frame more than the key cache, the most objects, a bank insertion at every frame
        // and none at all.  Whatever is asked for, every workspace is built for >= 1 frame and the bank holds a whole-clip sweep
        const stcn::EngineEnv env;                     // the defaults: this program reads no environment
        const stcn_engine_opts none{-1, -1, -1, -1}, wild{1 << 30, 1 << 30, 1 << 30, 1 << 30}, zero{0, 0, 0, 0};
        const int shapes[][3] = {{1, 1, 1}, {1, 1, 5}, {2, STCN_MAX_OBJECTS, 1}, {3, 1, 1000}, {106, 1, 1}, {107, 1, 1}, {107, STCN_MAX_OBJECTS, 200}, {9, STCN_MAX_OBJECTS, 5}};
        for (const auto &s : shapes)
            for (const stcn_engine_opts &o : {none, wild, zero})
                for (int fuse = 0; fuse < 2; ++fuse) {
                    const int T = s[0], k = s[1], mf = s[2];
                    const stcn::EnginePlan p = stcn::plan_engine(T, k, mf, fuse != 0, o, env);
                    EXPECT(p.n_slots == (T < 106 ? T : 106) && p.mem_freq == mf);
                    EXPECT(p.group >= 1 && p.group <= stcn::MAX_DECODE_GROUP && p.group <= (mf > 1 ? mf : 1) && (p.group == 1 || p.group * k <= 16));
                    EXPECT(p.key_batch >= 1 && p.key_batch <= 8);
                    EXPECT(p.main.key_batch >= 1 && p.main.group == p.group && p.side.key_batch >= 1 && p.side.group == 1);
                    EXPECT(!p.dual_sweep || (T >= 3 && T <= p.n_slots && p.lookahead > 0));
                    EXPECT(!p.fuse_side || (fuse && p.has_side));
                    EXPECT(p.bank_lo == (p.dual_sweep ? (T - 1) / mf + 2 : 0));
                    EXPECT(p.bank_initial == stcn::bank_slots_needed(p, T - 1, 8) && p.bank_initial == p.bank_lo + (T - 1) / mf + 1 + 8);
                    // an interaction next to an interacted frame (span 0) still has room for its certain slot; longer spans never need less
                    EXPECT(stcn::bank_slots_needed(p, 0, 1) == p.bank_lo + 2);
                    EXPECT(stcn::bank_slots_needed(p, T - 1, 60) >= stcn::bank_slots_needed(p, T / 2, 60));
                }
        const stcn::EnginePlan a = stcn::plan_engine(107, 1, 1, true, none, env);      // a clip that recycles its cache keeps fuse_side, nothing else
        EXPECT(a.lookahead == 0 && a.lookahead_req == 2 && a.fuse_side && a.has_side && !a.dual_sweep && a.side.key_batch == 1 && a.bank_initial == 115);
        const stcn::EnginePlan b = stcn::plan_engine(106, 1, 1, true, none, env);
        EXPECT(b.lookahead == 2 && b.dual_sweep && b.bank_lo == 107 && b.bank_initial == 107 + 106 + 8);
    }
    std::printf(failures ? "stage_host_check: %d FAILED\n" : "stage_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
