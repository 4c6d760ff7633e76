// stages.cpp - the reference's stage-level interface (PropagationNetwork.encode_key / encode_value / segment_with_query / get_attention,
// FusionNet.forward, aggregate_wbg) as C-ABI entry points on the reference's own tensor layouts (see include/stcn_hip.h).
// A stage context owns what a call needs - a workspace, the row-layout copies of the call's tensors, the bank staging - so a call only
// converts layouts (layout.hip) and enqueues the engine's own stage functions (engine.h) on the context's stream.
#include <algorithm>
#include <cmath>

#include "engine.h"

using namespace stcn;

struct stcn_stage {
    const Model *model = nullptr;
    hipStream_t stream = nullptr;
    int max_k = 0;
    Work w;                              // sized for max_k objects; w.k and the planning capacity w.wino_v_floats are set per call (stage_batch)
    size_t v_alloc = 0;                  // Winograd V floats allocated
    PoolBuf<float> img4;                 // [npix][4] the call's frame
    PoolBuf<float> k16, thin, f16, f8, f4;     // the frame's features as rows
    PoolBuf<float> s8, s4;               // decoder skip convs of f8 / f4
    PoolBuf<float> val;                  // [max_k][hw16][512] encode_value's output as rows
    PoolBuf<float> qsq;                  // [hw16 + MEMREAD_MSQ_PAD] |k16|^2 (segment: of the queries, km; attention: of the memory key)
    PoolBuf<float> mk1;                  // [hw16][64] attention's memory key
    // bank staging of segment: the memory as rows, grown geometrically (stage_grow) to the largest (rows, objects) seen
    long bank_rows = 0; int bank_k = 0;
    PoolBuf<float> bank_key, bank_msq, bank_val;
    PoolBuf<int32_t> centre;             // kernelized read: row centres of one frame of queries
    // the buffers go back to the pool: nothing of this context may still run
    ~stcn_stage() { if (model) (void)hipSetDevice(model->device); (void)hipStreamSynchronize(stream); }
};

namespace stcn {
// capacity after growing `cap` to hold `need`: at least twice the old one, so n growing calls allocate O(log n) times
long stage_grow(long cap, long need) { return need <= cap ? cap : std::max(need, 2 * cap); }
}  // namespace stcn

namespace {
// room for a memory of `rows` rows and k objects.  Growing waits for the context's stream first (earlier calls may still read the old
// staging, and a buffer handed back to the pool can be another context's the next moment) - the one place a stage call waits at all
int bank_reserve(stcn_stage *s, long rows, int k) {
    if (rows <= s->bank_rows && k <= s->bank_k) return STCN_OK;
    const long nr = stage_grow(s->bank_rows, rows);
    const int nk = (int)std::min<long>(STCN_MAX_OBJECTS, stage_grow(s->bank_k, k));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->bank_key.reset(); s->bank_msq.reset(); s->bank_val.reset(); s->centre.reset();
    s->bank_rows = 0; s->bank_k = 0;                   // a failure below leaves no staging
    HIPCHK(s->bank_key.alloc((size_t)nr * 64 * 4));
    HIPCHK(s->bank_msq.alloc(((size_t)nr + MEMREAD_MSQ_PAD) * 4));
    HIPCHK(s->bank_val.alloc((size_t)nk * nr * 512 * 4));
    HIPCHK(s->centre.alloc((size_t)memread_centre_stride((int)nr) * 4));
    s->bank_rows = nr; s->bank_k = nk;
    return STCN_OK;
}
// |x|^2 of n rows of 64 behind which the read kernels may fetch MEMREAD_MSQ_PAD more
int rows_msq(const float *x, long n, float *msq, hipStream_t st) {
    HIPCHK(hipMemsetAsync(msq, 0, ((size_t)n + MEMREAD_MSQ_PAD) * 4, st));
    rowsumsq_launch(x, (int)n, 64, msq, st);
    return STCN_OK;
}
// A call over k objects runs as in a context created for exactly k: the planners choose a conv's kernel family by what fits the Winograd
// workspace, so a result must not depend on how many objects the context happens to have room for
void stage_batch(stcn_stage *s, int k) {
    s->w.k = k;
    s->w.wino_v_floats = std::min(s->v_alloc, wino_v_capacity(s->w.d, k));
}
// what every stage call checks first: the context, that its model has the propagation network, 1 <= k <= the context's objects
int stage_check(const stcn_stage *s, const char *who, int k, bool need_prop = true) {
    if (k < 1 || k > STCN_MAX_OBJECTS) { set_error("%s: k=%d outside 1..%d", who, k, STCN_MAX_OBJECTS); return STCN_E_INVALID; }
    if (!s) { set_error("%s: null stage context", who); return STCN_E_INVALID; }
    if (k > s->max_k) { set_error("%s: k=%d, the context was created for max_objects=%d", who, k, s->max_k); return STCN_E_INVALID; }
    if (need_prop && !s->model->has_prop) { set_error("%s: the context's model is a FusionNet alone (stcn_fusion_model_create)", who); return STCN_E_STATE; }
    return STCN_OK;
}
}  // namespace

extern "C" {

int stcn_stage_create(const stcn_model *m, int nh, int nw, int max_objects, void *stream, stcn_stage **out) {
    if (nh < 16 || nw < 16 || nh % 16 || nw % 16) { set_error("stcn_stage_create: nh=%d nw=%d must be positive multiples of 16 (frames arrive padded)", nh, nw); return STCN_E_INVALID; }
    if ((long)nh * nw > MAX_FRAME_PIXELS) { set_error("stcn_stage_create: a frame of nh=%d x nw=%d pixels, at most 2^24 = %ld", nh, nw, MAX_FRAME_PIXELS); return STCN_E_INVALID; }
    if (max_objects < 1 || max_objects > STCN_MAX_OBJECTS) { set_error("stcn_stage_create: max_objects=%d outside 1..%d", max_objects, STCN_MAX_OBJECTS); return STCN_E_INVALID; }
    if (!m || !out) { set_error("stcn_stage_create: null arguments"); return STCN_E_INVALID; }
    HIPCHK(hipSetDevice(m->m.device));
    std::unique_ptr<stcn_stage> s(new stcn_stage());       // a failure below destroys it: whatever it took so far goes back
    s->model = &m->m; s->stream = (hipStream_t)stream; s->max_k = max_objects;
    RC(s->w.init(nh, nw, max_objects));
    s->v_alloc = s->w.wino_v_floats;
    const Dims &d = s->w.d;
    const size_t sizes[] = {(size_t)d.npix * 4, (size_t)d.hw16 * 64, (size_t)d.hw16 * 512, (size_t)d.hw16 * 1024, (size_t)d.hw8 * 512, (size_t)d.hw4 * 256,
                            (size_t)d.hw8 * 512, (size_t)d.hw4 * 256, (size_t)max_objects * d.hw16 * 512, (size_t)d.hw16 + MEMREAD_MSQ_PAD, (size_t)d.hw16 * 64};
    PoolBuf<float> *bufs[] = {&s->img4, &s->k16, &s->thin, &s->f16, &s->f8, &s->f4, &s->s8, &s->s4, &s->val, &s->qsq, &s->mk1};
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) HIPCHK(bufs[i]->alloc(sizes[i] * sizeof(float)));
    *out = s.release();
    return STCN_OK;
}

int stcn_stage_destroy(stcn_stage *s) {
    if (s) delete s;
    return STCN_OK;
}

int stcn_stage_encode_key(stcn_stage *s, const float *frame, float *k16, float *f16_thin, float *f16, float *f8, float *f4) {
    RC(stage_check(s, "stcn_stage_encode_key", 1));
    if (!frame) { set_error("stcn_stage_encode_key: null frame"); return STCN_E_INVALID; }
    HIPCHK(hipSetDevice(s->model->device));
    const Dims &d = s->w.d;
    hipStream_t st = s->stream;
    stage_batch(s, 1);
    pack_image_launch(frame, s->img4, d.nh, d.nw, d.nh, d.nw, 0, 0, st);
    const KeyOut ko{s->k16, nullptr, f16_thin ? s->thin : nullptr, s->f16, nullptr, nullptr, f8 ? s->f8 : nullptr, f4 ? s->f4 : nullptr};
    RC(encode_key(*s->model, s->w, st, s->img4, ko));
    if (k16) rows_to_planes_launch(s->k16, 0, k16, d.hw16, 0, 1, d.hw16, 64, st);
    if (f16_thin) rows_to_planes_launch(s->thin, 0, f16_thin, d.hw16, 0, 1, d.hw16, 512, st);
    if (f16) rows_to_planes_launch(s->f16, 0, f16, d.hw16, 0, 1, d.hw16, 1024, st);
    if (f8) rows_to_planes_launch(s->f8, 0, f8, d.hw8, 0, 1, d.hw8, 512, st);
    if (f4) rows_to_planes_launch(s->f4, 0, f4, d.hw4, 0, 1, d.hw4, 256, st);
    return launch_status("stage encode_key");
}

int stcn_stage_encode_value(stcn_stage *s, const float *frame, const float *kf16, const float *masks, int k, float *out) {
    RC(stage_check(s, "stcn_stage_encode_value", k));
    if (!frame || !kf16 || !masks || !out) { set_error("stcn_stage_encode_value: null arguments"); return STCN_E_INVALID; }
    HIPCHK(hipSetDevice(s->model->device));
    const Dims &d = s->w.d;
    hipStream_t st = s->stream;
    stage_batch(s, k);
    pack_image_launch(frame, s->img4, d.nh, d.nw, d.nh, d.nw, 0, 0, st);
    planes_to_rows_launch(kf16, d.hw16, 0, s->f16, 0, 1, d.hw16, 1024, st);
    RC(encode_value(*s->model, s->w, st, s->img4, s->f16, masks, d.npix, s->val, 0));
    rows_to_planes_launch(s->val, (long)d.hw16 * 512, out, d.hw16, (long)d.hw16 * 512, k, d.hw16, 512, st);
    return launch_status("stage encode_value");
}

int stcn_stage_segment(stcn_stage *s, const float *mk16, long mk_plane_stride, const float *mv16, long mv_plane_stride, long mv_object_stride,
                       int T, int k, const float *qf8, const float *qf4, const float *qk16, const float *qv16, float *prob) {
    const char *who = "stcn_stage_segment";
    if (T < 1) { set_error("%s: T=%d, a memory of at least one frame is required", who, T); return STCN_E_INVALID; }
    RC(stage_check(s, who, k));
    if (!mk16 || !mv16 || !qf8 || !qf4 || !qk16 || !qv16 || !prob) { set_error("%s: null arguments", who); return STCN_E_INVALID; }
    const Dims &d = s->w.d;
    const long N = (long)T * d.hw16;
    if (N >= MEMREAD_MAX_ROWS) { set_error("%s: a memory of T * h16 * w16 = %ld rows, the read addresses fewer than 2^24 = %ld", who, N, MEMREAD_MAX_ROWS); return STCN_E_INVALID; }
    if (mk_plane_stride < N || mv_plane_stride < N || mv_object_stride < 0) {
        set_error("%s: bad strides (plane strides >= T * h16 * w16 = %ld; mk %ld, mv %ld)", who, N, mk_plane_stride, mv_plane_stride);
        return STCN_E_INVALID;
    }
    const Model &m = *s->model;
    if (N < m.top_k) { set_error("%s: the memory has T * h16 * w16 = %ld rows, fewer than top_k = %d (the reference's topk raises as well)", who, N, m.top_k); return STCN_E_INVALID; }
    HIPCHK(hipSetDevice(m.device));
    hipStream_t st = s->stream;
    Work &w = s->w;
    stage_batch(s, k);
    RC(bank_reserve(s, N, k));
    // the bank, read in place from the caller's (possibly T-sliced) tensors
    planes_to_rows_launch(mk16, mk_plane_stride, 0, s->bank_key, 0, 1, (int)N, 64, st);
    RC(rows_msq(s->bank_key, N, s->bank_msq, st));
    planes_to_rows_launch(mv16, mv_plane_stride, mv_object_stride, s->bank_val, N * 512, k, (int)N, 512, st);
    // the query frame
    planes_to_rows_launch(qk16, d.hw16, 0, s->k16, 0, 1, d.hw16, 64, st);
    planes_to_rows_launch(qv16, d.hw16, 0, s->thin, 0, 1, d.hw16, 512, st);
    planes_to_rows_launch(qf8, d.hw8, 0, s->f8, 0, 1, d.hw8, 512, st);
    planes_to_rows_launch(qf4, d.hw4, 0, s->f4, 0, 1, d.hw4, 256, st);
    RC(run_conv(m, w, st, "decoder.up_16_8.skip_conv", ConvArgs(s->f8, 512, 1, d.h8, d.w8).out(s->s8)));
    RC(run_conv(m, w, st, "decoder.up_8_4.skip_conv", ConvArgs(s->f4, 256, 1, d.h4, d.w4).out(s->s4)));
    const bool km = m.km > 0.f;
    if (km) rowsumsq_launch(s->k16, d.hw16, 64, s->qsq, st);
    const MemReadKm kmo{m.km, d.h16, d.w16, s->qsq, (long)d.hw16, s->centre, nullptr};
    MemRead r{};
    r.mk = s->bank_key; r.msq = s->bank_msq; r.mv = s->bank_val; r.mv_os = N * 512; r.N = (int)N;
    r.qk = s->k16; r.Q = d.hw16; r.k = k; r.top_k = m.top_k; r.readout = w.readout; r.ro_os = (long)d.hw16 * 512; r.km = km ? &kmo : nullptr;
    memory_read_launch(r, MemReadScratch{w.cand_v, w.cand_i, w.cand_n, w.gmax, w.tau}, st);
    RC(launch_status("stage memory read"));
    RC(decode_logit4(m, w, st, w.readout, s->thin, s->s8, s->s4));
    up4_sigmoid_launch(w.logit4, k, d.h4, d.w4, prob, st);
    return launch_status("stage segment");
}

int stcn_stage_attention(stcn_stage *s, const float *mk16, const float *pos, const float *neg, const float *qk16, int b, float *attn) {
    const char *who = "stcn_stage_attention";
    if (b < 1 || b > STCN_MAX_OBJECTS + 1) { set_error("%s: b=%d outside 1..%d", who, b, STCN_MAX_OBJECTS + 1); return STCN_E_INVALID; }
    RC(stage_check(s, who, 1));
    if (b > s->max_k + 1) { set_error("%s: b=%d mask planes, the context was created for max_objects=%d (+ background)", who, b, s->max_k); return STCN_E_INVALID; }
    if (!mk16 || !pos || !neg || !qk16 || !attn) { set_error("%s: null arguments", who); return STCN_E_INVALID; }
    HIPCHK(hipSetDevice(s->model->device));
    const Dims &d = s->w.d;
    hipStream_t st = s->stream;
    Work &w = s->w;
    planes_to_rows_launch(mk16, d.hw16, 0, s->mk1, 0, 1, d.hw16, 64, st);
    planes_to_rows_launch(qk16, d.hw16, 0, s->k16, 0, 1, d.hw16, 64, st);
    RC(rows_msq(s->mk1, d.hw16, s->qsq, st));
    attention_read_launch(s->mk1, s->qsq, s->k16, pos, neg, b, d.h16, d.w16, w.pooled, w.amap, attn, AttnScratch{w.gmax, w.cand_v}, st);
    return launch_status("stage attention");
}

int stcn_stage_fusion(stcn_stage *s, const float *im, const float *seg1, const float *seg2, const float *attn, float nc, float nr, float *logit) {
    RC(stage_check(s, "stcn_stage_fusion", 1, false));
    if (!im || !seg1 || !seg2 || !attn || !logit) { set_error("stcn_stage_fusion: null arguments"); return STCN_E_INVALID; }
    if (!std::isfinite(nc) || !std::isfinite(nr)) { set_error("stcn_stage_fusion: time = (%f, %f) is not finite", (double)nc, (double)nr); return STCN_E_INVALID; }
    HIPCHK(hipSetDevice(s->model->device));
    const Dims &d = s->w.d;
    stage_batch(s, 1);
    pack_image_launch(im, s->img4, d.nh, d.nw, d.nh, d.nw, 0, 0, s->stream);
    RC(fusion_logit(*s->model, s->w, s->stream, s->img4, seg1, seg2, attn, nc, nr, logit));
    return launch_status("stage fusion");
}

int stcn_aggregate_wbg(void *stream, const float *prob, int k, long npix, int keep_bg, int hard, float *out) {
    if (k < 1 || k > STCN_MAX_OBJECTS) { set_error("stcn_aggregate_wbg: k=%d outside 1..%d", k, STCN_MAX_OBJECTS); return STCN_E_INVALID; }
    if (!prob || !out || npix < 1) { set_error("stcn_aggregate_wbg: null arguments or npix=%ld < 1", npix); return STCN_E_INVALID; }
    aggregate_wbg_launch(prob, k, npix, keep_bg, hard, out, (hipStream_t)stream);
    return launch_status("aggregate_wbg");
}

int stcn_test_transpose(void *stream, const float *src, float *dst, int B, int R, int C, long ld, long planes_bs, int to_rows) {
    if (!src || !dst || B < 1 || R < 1 || C < 4 || C % 4 || ld < R || planes_bs < 0) { set_error("stcn_test_transpose: bad arguments (C %% 4 == 0, ld >= R)"); return STCN_E_INVALID; }
    if (to_rows) planes_to_rows_launch(src, ld, planes_bs, dst, (long)R * C, B, R, C, (hipStream_t)stream);
    else rows_to_planes_launch(src, (long)R * C, dst, ld, planes_bs, B, R, C, (hipStream_t)stream);
    return launch_status("transpose");
}

}  // extern "C"
