// hooks.cpp - stage-level C-ABI entry points used by tests/ and bench.py (see include/stcn_hip.h).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"

using namespace stcn;

namespace {
struct TmpWork {
    Work w;
    int rc;
    TmpWork(int nh, int nw, int k) { rc = w.init(nh, nw, k); }
    ~TmpWork() { (void)hipDeviceSynchronize(); }      // then w gives its buffers back
};
struct DevBuf {
    float *p = nullptr;
    int alloc(size_t floats) { HIPCHK(hipMalloc((void **)&p, floats * 4)); return STCN_OK; }
    ~DevBuf() { if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); } }
};
// the one-layer model of the conv hooks: layer "t", weights not yet bound
ConvW test_convw(int Cin, int Cout, int KH, int KW) {
    ConvW cw;
    cw.cout = Cout; cw.cin = Cin; cw.cin_p = Cin; cw.kh = KH; cw.kw = KW;
    cw.K = KH * KW * Cin; cw.Kp = (cw.K + 31) / 32 * 32;
    return cw;
}
// V of either Winograd form: 16 positions x tiles of 2x2 padded to 64, or 36 positions x tiles of 4x4 padded to 128 (for a
// handful of tiles the padded F(4x4) workspace is the larger one - sized for F(2x2) alone such a case fell back silently)
size_t test_wino_v_floats(int B, int OH, int OW, int Cin) {
    const size_t v2 = (size_t)16 * Cin * (((size_t)B * ((OH + 1) / 2) * ((OW + 1) / 2) + 63) / 64 * 64);
    const size_t v4 = (size_t)36 * Cin * (((size_t)B * ((OH + 3) / 4) * ((OW + 3) / 4) + 127) / 128 * 128);
    return v2 > v4 ? v2 : v4;
}
// the one-layer model (layer "t") and workspace stcn_test_conv / stcn_bench_conv run.  hw: host copy of the weights [Cout][Kp] of a
// stride-1 3x3 conv - it gets the Winograd weights the engine would make (f4: as a decoder layer) and a V workspace - else null
struct ConvRig {
    Model m;
    Work w;
    DevBuf wv, ws;
    ~ConvRig() { (void)hipDeviceSynchronize(); for (void *p : m.allocs) (void)hipFree(p); }
    int init(ConvW cw, const std::vector<float> *hw, bool f4, int B, int OH, int OW, size_t slab_floats) {
        if (hw) {
            RC(make_wino(m, cw, *hw));
            RC(make_wino_fusion12(m, cw, *hw));
            if (f4) RC(make_wino4(m, cw, *hw));
            w.wino_v_floats = test_wino_v_floats(B, OH, OW, cw.cin_p);
            RC(wv.alloc(w.wino_v_floats));
            w.wino_v = wv.p;
        }
        m.conv["t"] = cw;
        w.splitk_floats = slab_floats;
        RC(ws.alloc(w.splitk_floats));
        w.splitk = ws.p;
        return STCN_OK;
    }
};
// The device-free set-up of stcn_test_conv's conv (stcn_test_conv_path / stcn_test_conv_plan): the same ConvW and Work sizes, planned but
// neither allocated nor launched.  The planners test wino_u, wino4_u, partial, bias and res for null only, so one non-null constant
// stands in for every buffer.  No residual.
int plan_test_conv(int B, int H, int W, int Cin, int Cout, int K, int stride, int flags, int splitk, ConvP &p, ConvPlan &pl) {
    static float buf[4];
    Model m;
    ConvW cw = test_convw(Cin, Cout, K, K);
    cw.w = cw.bias = buf;
    const int OH = (H + 2 * (K / 2) - K) / stride + 1, OW = (W + 2 * (K / 2) - K) / stride + 1;
    Work w;
    if (K == 3 && stride == 1) {
        if (wants_wino(cw) || wants_wino_fusion12(cw)) cw.wino_u = buf;
        if (flags & 4) { if (wants_wino4(cw)) cw.wino4_u = buf; m.wino4_min_wg = 0; }
        w.wino_v_floats = test_wino_v_floats(B, OH, OW, Cin);
        w.wino_v = buf;
    }
    m.conv["t"] = cw;
    w.splitk_floats = (size_t)16 * 1024 * 1024;
    w.splitk = buf;
    return plan_conv(m, w, "t", ConvArgs(buf, Cin, B, H, W).strided(stride).out(buf).relu(flags & 1, (flags >> 1) & 1).splitk(splitk), p, pl);
}
// The read stcn_test_memory_read_km runs once and stcn_bench_memory_read_km times: the arguments checked (`who` names the hook in the
// message), |mk|^2 and the scratch allocated - sized by memread_scratch_floats and nothing else -, the km scratch (|qk|^2 per query, the
// packed row centres) when h16 / w16 / km / centres are not all zero, and the descriptor filled
struct ReadRig {
    DevBuf msq, cv, ci, cn, gm, tau, qsq, cen;
    MemReadKm km{};
    MemRead r{};
    MemReadScratch scr{};
    int init(const char *who, hipStream_t s, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k, int h16, int w16,
             float sigma, int32_t *centres, int32_t *topk_idx, float *topk_w, float *readout) {
        const bool bad = !mk || !mv || !qk || !readout || top_k < 1 || top_k > STCN_MAX_TOP_K || N < top_k || Q < 1 || k < 1;
        if (bad) { set_error("%s: bad arguments (1 <= top_k <= %d, N >= top_k; top_k=%d N=%d)", who, STCN_MAX_TOP_K, top_k, N); return STCN_E_INVALID; }
        if (N >= MEMREAD_MAX_ROWS) { set_error("%s: a bank of N=%d rows, the read addresses fewer than 2^24 = %ld", who, N, MEMREAD_MAX_ROWS); return STCN_E_INVALID; }
        const bool with_km = h16 != 0 || w16 != 0 || sigma != 0.f || centres;      // all zero: the plain read
        // the kernelized read: km > 0 finite, the Q queries whole frames of h16 x w16 positions (16-bit coordinates)
        const bool km_ok = std::isfinite(sigma) && sigma > 0.f && h16 >= 1 && w16 >= 1 && h16 < 32768 && w16 < 32768 && (long)h16 * w16 <= Q && Q % (h16 * w16) == 0;
        if (with_km && !km_ok) { set_error("%s_km: bad arguments (km > 0 finite, Q a multiple of h16 * w16; km=%f h16=%d w16=%d Q=%d)", who, (double)sigma, h16, w16, Q); return STCN_E_INVALID; }
        const MemReadScratchSizes sz = memread_scratch_floats(Q);
        RC(msq.alloc((size_t)N + MEMREAD_MSQ_PAD)); RC(cv.alloc(sz.cand_v)); RC(ci.alloc(sz.cand_i)); RC(cn.alloc(sz.cand_n)); RC(gm.alloc(sz.gmax)); RC(tau.alloc(sz.tau));
        scr = MemReadScratch{cv.p, reinterpret_cast<int32_t *>(ci.p), reinterpret_cast<int32_t *>(cn.p), gm.p, tau.p};
        if (with_km) {
            RC(qsq.alloc(Q)); RC(cen.alloc((size_t)(Q / (h16 * w16)) * memread_centre_stride(N)));
            rowsumsq_launch(qk, Q, 64, qsq.p, s);
            km = MemReadKm{sigma, h16, w16, qsq.p, (long)h16 * w16, reinterpret_cast<int32_t *>(cen.p), centres};
        }
        HIPCHK(hipMemsetAsync(msq.p, 0, ((size_t)N + MEMREAD_MSQ_PAD) * 4, s));
        rowsumsq_launch(mk, N, 64, msq.p, s);
        r.mk = mk; r.msq = msq.p; r.mv = mv; r.mv_os = (long)N * 512; r.N = N; r.qk = qk; r.Q = Q; r.k = k; r.top_k = top_k;
        r.readout = readout; r.ro_os = (long)Q * 512; r.topk_idx = topk_idx; r.topk_w = topk_w; r.km = with_km ? &km : nullptr;
        return STCN_OK;
    }
};
void export_memread_plan(int N, int Q, int32_t *plan7) {
    const MemReadPlan pl = memread_plan(N, Q);
    const int32_t v[7] = {pl.steps, pl.ss, pl.ns, pl.nc1, pl.spc1, pl.nc2, pl.spc2};
    for (int i = 0; i < 7; ++i) plan7[i] = v[i];
}
// stcn_test_kernel: the kernels of kernels.h it reaches, with the argument counts include/stcn_hip.h documents
struct SmallKernel { const char *name; int nptr, ni, nf; unsigned wide; };     // wide: bit i set = integer i is a long (a stride or an element count)
const SmallKernel SMALL_KERNELS[] = {
    {"maxpool3x3s2", 2, 4, 0, 0}, {"upsample2x_add", 3, 6, 0, 1u << 4}, {"up4_sigmoid_aggregate", 2, 8, 0, 1u << 3 | 1u << 4 | 1u << 6 | 1u << 7},
    {"up4_sigmoid", 2, 3, 0, 0}, {"sigmoid_aggregate", 2, 3, 0, 1u << 1 | 1u << 2}, {"argmax", 2, 3, 0, 1u << 2}, {"rowsumsq", 2, 5, 0, 1u << 3 | 1u << 4},
    {"pack_image", 2, 6, 0, 0}, {"pack_value_input", 3, 3, 0, 1u << 0}, {"pack_fusion_input", 5, 1, 2, 1u << 0}, {"interact_mask", 5, 9, 0, 1u << 7},
    {"cbam", 7, 3, 1, 0}, {"copy_rows", 2, 4, 0, 1u << 0 | 1u << 1 | 1u << 3}, {"copy2", 4, 2, 0, 1u << 0 | 1u << 1}, {"fill", 1, 1, 1, 1u << 0},
};
}  // namespace

extern "C" {

int stcn_test_conv(void *stream, const float *x, const float *wgt, const float *bias, const float *res, float *y, int B,
                   int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int flags, int splitk) {
    return stcn_test_conv_ex(stream, x, wgt, bias, res, y, B, H, W, Cin, Cout, KH, KW, stride, pad, flags, splitk, nullptr, 0, CONV_DENSE, CONV_DENSE,
                             CONV_DENSE, 0, CONV_DENSE);
}

// The one rig of the conv hooks: the operands in every form ConvArgs takes (a second source, batch strides of the input, the residual and
// the output, the per-frame residual of a batch laid out [object][frame]).  plan_conv's own refusals pass through with its message.
int stcn_test_conv_ex(void *stream, const float *x, const float *wgt, const float *bias, const float *res, float *y, int B,
                      int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int flags, int splitk,
                      const float *x1, int c1, long bs0, long bs1, long res_bs, int res_bmod, long y_bs) {
    if (!x || !wgt || !y || B < 1 || H < 1 || W < 1 || Cin < 4 || Cout < 1 || stride < 1 || Cin % 4 || pad != KH / 2 || KH != KW) {
        set_error("stcn_test_conv_ex: x, w and y, B, H, W, Cout, stride >= 1, Cin%%4==0, square kernel, pad=K/2 required"); return STCN_E_INVALID;
    }
    if ((x1 != nullptr) != (c1 > 0) || c1 % 4 || bs0 < CONV_DENSE || bs1 < CONV_DENSE || res_bs < CONV_DENSE || res_bmod < 0 || y_bs < CONV_DENSE) {
        set_error("stcn_test_conv_ex: a second source has c1 > 0 channels (c1%%4==0); strides are -1 (dense), 0 (broadcast) or elements; res_bmod >= 0");
        return STCN_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    ConvW cw = test_convw(Cin + c1, Cout, KH, KW);
    DevBuf wpad;
    RC(wpad.alloc((size_t)Cout * cw.Kp));
    HIPCHK(hipMemsetAsync(wpad.p, 0, (size_t)Cout * cw.Kp * 4, s));
    HIPCHK(hipMemcpy2DAsync(wpad.p, (size_t)cw.Kp * 4, wgt, (size_t)cw.K * 4, (size_t)cw.K * 4, Cout, hipMemcpyDeviceToDevice, s));
    cw.w = wpad.p; cw.bias = const_cast<float *>(bias);
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
    const bool wino = KH == 3 && stride == 1 && !x1;   // stride-1 3x3 of one source: the Winograd path, as in the engine
    std::vector<float> hw;
    if (wino) {
        HIPCHK(hipStreamSynchronize(s));
        hw.resize((size_t)Cout * cw.Kp);
        HIPCHK(hipMemcpy(hw.data(), wpad.p, hw.size() * 4, hipMemcpyDeviceToHost));
    }
    ConvRig r;
    RC(r.init(cw, wino ? &hw : nullptr, flags & 4, B, OH, OW, (size_t)16 * 1024 * 1024));    // flags bit 2: as a decoder layer (F(4x4,3x3))
    if (wino && (flags & 4)) r.m.wino4_min_wg = 0;
    if (Cout == 1) {
        const bool dense = !x1 && bs0 == CONV_DENSE && y_bs == CONV_DENSE && !res;
        if (stride != 1 || !dense) { set_error("Cout==1 path is stride 1, one dense source, dense output, no residual"); return STCN_E_INVALID; }
        float b0 = 0.f;
        if (bias) HIPCHK(hipMemcpy(&b0, bias, 4, hipMemcpyDeviceToHost));
        conv_n1_launch(x, wpad.p, b0, y, B, H, W, Cin, KH, flags & 1, s);
        set_conv_path("n1");
    } else {
        RC(run_conv(r.m, r.w, s, "t", ConvArgs(x, Cin, B, H, W, bs0).concat(x1, c1, x1 ? bs1 : 0).strided(stride).out(y, y_bs == CONV_DENSE ? 0 : y_bs)
                                          .residual(res, res_bs, res_bmod).relu(flags & 1, (flags >> 1) & 1).splitk(splitk)));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// The plan stcn_test_conv's conv would take, as its path string: the same ConvW and Work sizes, but nothing is allocated on a device
// and nothing is launched (works without a GPU).
int stcn_test_conv_path(int B, int H, int W, int Cin, int Cout, int K, int stride, int flags, int splitk, char *out, int n) {
    if (Cin % 4 || !out || n < 1) { set_error("stcn_test_conv_path: Cin%%4==0 and an output buffer required"); return STCN_E_INVALID; }
    ConvP p;
    ConvPlan pl;
    RC(plan_test_conv(B, H, W, Cin, Cout, K, stride, flags, splitk, p, pl));
    format_conv_path(pl, out, (size_t)n);
    return STCN_OK;
}

// ... and the same plan in numbers (the path string leaves most of it out); the order is the one include/stcn_hip.h documents.
// Fields of other families than the plan's are zero.
int stcn_test_conv_plan(int B, int H, int W, int Cin, int Cout, int K, int stride, int flags, int splitk, int32_t *iv, int n, double *dv) {
    if (Cin % 4 || !iv || n < STCN_CONV_PLAN_INTS || !dv) { set_error("stcn_test_conv_plan: Cin%%4==0, STCN_CONV_PLAN_INTS ints and 2 doubles required"); return STCN_E_INVALID; }
    ConvP p;
    ConvPlan pl;
    RC(plan_test_conv(B, H, W, Cin, Cout, K, stride, flags, splitk, p, pl));
    const bool w2 = pl.family == CONV_WINO2, w4 = pl.family == CONV_WINO4, direct = pl.family == CONV_DIRECT;
    const WinoGeom g = w2 || w4 ? pl.geo : WinoGeom{};
    const W4Plan q = w4 ? pl.w4 : W4Plan{};
    const int32_t v[STCN_CONV_PLAN_INTS] = {
        pl.family, pl.splitk, pl.ppw, pl.tail, pl.n_in, pl.n_gemm, pl.reduce,
        g.TH, g.TW, g.Mt, g.Mt_pad, g.KB, w2 ? pl.w2.kb_per_split : 0,
        q.mb, q.tiles_m, q.tiles_n, q.grid, q.full_wg, q.pieces, q.per, q.chunks, q.tm_per_chunk,
        direct ? p.tile_big : 0, direct ? p.rem_full : 0, direct ? p.rem_split : 0, direct ? p.rem_per : 0, direct ? p.chain : 0};
    for (int i = 0; i < STCN_CONV_PLAN_INTS; ++i) iv[i] = v[i];
    if (n > STCN_CONV_PLAN_INTS) iv[STCN_CONV_PLAN_INTS] = direct ? p.affine_out : 0;
    dv[0] = (double)pl.v_floats; dv[1] = pl.fl_exec;
    return STCN_OK;
}

int stcn_bench_conv(void *stream, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int splitk,
                    int iters, float *avg_ms, double *flops_per_launch) {
    hipStream_t s = (hipStream_t)stream;
    (void)pad;
    ConvW cw = test_convw(Cin, Cout, KH, KW);
    const int OH = (H + 2 * (KH / 2) - KH) / stride + 1, OW = (W + 2 * (KW / 2) - KW) / stride + 1;
    DevBuf x, wt, b, y;
    RC(x.alloc((size_t)B * H * W * Cin)); RC(wt.alloc((size_t)Cout * cw.Kp)); RC(b.alloc(Cout));
    RC(y.alloc((size_t)B * OH * OW * Cout));
    // non-trivial data (zero operands raise the clock: cdna_hip_programming.md rule 25)
    std::vector<float> h((size_t)B * H * W * Cin);
    unsigned st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 32768.f - 1.f; };
    for (auto &v : h) v = rnd();
    HIPCHK(hipMemcpy(x.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    h.assign((size_t)Cout * cw.Kp, 0.f);
    for (auto &v : h) v = rnd() * 0.05f;
    HIPCHK(hipMemcpy(wt.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(b.p, 0, Cout * 4, s));
    cw.w = wt.p; cw.bias = b.p;
    ConvRig r;                                                    // STCN_BENCH_CONV_F4: time the layer as a decoder layer
    RC(r.init(cw, KH == 3 && stride == 1 ? &h : nullptr, getenv("STCN_BENCH_CONV_F4") != nullptr, B, OH, OW, (size_t)32 * 1024 * 1024));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    DevBuf resb;                                                  // STCN_BENCH_CONV_RES=1: with a residual operand (the ResNet conv3 layers)
    const long obs = (long)OH * OW * Cout;
    if (getenv("STCN_BENCH_CONV_RES")) { RC(resb.alloc((size_t)B * obs)); HIPCHK(hipMemsetAsync(resb.p, 0, (size_t)B * obs * 4, s)); }
    const ConvArgs args = ConvArgs(x.p, Cin, B, H, W).strided(stride).out(y.p).residual(resb.p).relu(0, 1).splitk(splitk);
    for (int i = 0; i < 3; ++i)
        RC(run_conv(r.m, r.w, s, "t", args));
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        RC(run_conv(r.m, r.w, s, "t", args));
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (avg_ms) *avg_ms = ms / iters;
    if (flops_per_launch) *flops_per_launch = 2.0 * B * OH * OW * (double)Cout * KH * KW * Cin;
    return STCN_OK;
}

static int pack_one(const float *img_chw, int nh, int nw, float *img4, hipStream_t s) {
    pack_image_launch(img_chw, img4, nh, nw, nh, nw, 0, 0, s);
    return STCN_OK;
}

int stcn_test_encode_key(const stcn_model *m, void *stream, const float *img, int nh, int nw, float *k16, float *f16_thin,
                         float *f16, float *f8, float *f4) {
    if (!m || !img || nh % 16 || nw % 16) { set_error("stcn_test_encode_key: bad arguments"); return STCN_E_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    TmpWork t(nh, nw, 1);
    RC(t.rc);
    const Dims &d = t.w.d;
    DevBuf img4, tf16, tk16, tmsq;
    RC(img4.alloc((size_t)d.npix * 4)); RC(tf16.alloc((size_t)d.hw16 * 1024)); RC(tk16.alloc((size_t)d.hw16 * 64));
    RC(tmsq.alloc(d.hw16));
    RC(pack_one(img, nh, nw, img4.p, s));
    KeyOut ko{k16 ? k16 : tk16.p, tmsq.p, f16_thin, f16 ? f16 : tf16.p, nullptr, nullptr, f8, f4, nullptr, nullptr};
    RC(encode_key(m->m, t.w, s, img4.p, ko));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_test_encode_value(const stcn_model *m, void *stream, const float *img, const float *f16, const float *masks, int k,
                           int nh, int nw, float *out) {
    if (!m || !img || !f16 || !masks || !out || k < 1 || k > STCN_MAX_OBJECTS) { set_error("stcn_test_encode_value: bad arguments"); return STCN_E_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    TmpWork t(nh, nw, k);
    RC(t.rc);
    DevBuf img4;
    RC(img4.alloc((size_t)t.w.d.npix * 4));
    RC(pack_one(img, nh, nw, img4.p, s));
    RC(encode_value(m->m, t.w, s, img4.p, f16, masks, t.w.d.npix, out, 0));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_test_memory_read(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k,
                          int32_t *topk_idx, float *topk_w, float *readout) {
    return stcn_test_memory_read_k(stream, mk, mv, qk, N, Q, k, STCN_MAX_TOP_K, topk_idx, topk_w, readout);
}

int stcn_test_memory_read_k(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k,
                            int32_t *topk_idx, float *topk_w, float *readout) {
    return stcn_test_memory_read_km(stream, mk, mv, qk, N, Q, k, top_k, 0, 0, 0.f, nullptr, topk_idx, topk_w, readout);
}

int stcn_test_memory_read_km(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k, int h16, int w16,
                             float km, int32_t *centres, int32_t *topk_idx, float *topk_w, float *readout) {
    hipStream_t s = (hipStream_t)stream;
    ReadRig rig;
    RC(rig.init("stcn_test_memory_read", s, mk, mv, qk, N, Q, k, top_k, h16, w16, km, centres, topk_idx, topk_w, readout));
    memory_read_launch(rig.r, rig.scr, s);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// Timed memory reads on caller-provided device data: `iters` whole reads (pass 1, threshold, pass 2, merge + gather) between
// two HIP events on `stream`; scratch is allocated once, outside the timed region.  ms = average per read.
int stcn_bench_memory_read(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int iters,
                           float *readout, float *ms, int32_t *plan7) {
    return stcn_bench_memory_read_k(stream, mk, mv, qk, N, Q, k, STCN_MAX_TOP_K, iters, readout, ms, plan7);
}

int stcn_bench_memory_read_k(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k, int iters,
                             float *readout, float *ms, int32_t *plan7) {
    return stcn_bench_memory_read_km(stream, mk, mv, qk, N, Q, k, top_k, 0, 0, 0.f, iters, readout, ms, plan7);
}

int stcn_bench_memory_read_km(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k, int h16, int w16,
                              float km, int iters, float *readout, float *ms, int32_t *plan7) {
    hipStream_t s = (hipStream_t)stream;
    if (!ms || iters < 1) { set_error("stcn_bench_memory_read: bad arguments (ms and iters >= 1 required; top_k=%d N=%d)", top_k, N); return STCN_E_INVALID; }
    ReadRig rig;
    RC(rig.init("stcn_bench_memory_read", s, mk, mv, qk, N, Q, k, top_k, h16, w16, km, nullptr, nullptr, nullptr, readout));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int it = 0; it < 2; ++it) memory_read_launch(rig.r, rig.scr, s);
    HIPCHK(hipEventRecord(e0, s));
    for (int it = 0; it < iters; ++it) memory_read_launch(rig.r, rig.scr, s);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    *ms /= (float)iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (plan7) export_memread_plan(N, Q, plan7);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_test_sweep_plan(int idx, int closest, int mem_freq, int cap, int32_t *out, int n, int32_t *count) {
    if (mem_freq < 1 || cap < 1 || n < 0 || (n > 0 && !out) || !count) { set_error("stcn_test_sweep_plan: bad arguments"); return STCN_E_INVALID; }
    const std::vector<SweepGroup> groups = plan_sweep(idx, closest, mem_freq, cap);
    *count = (int32_t)groups.size();
    for (int i = 0; i < n && i < (int)groups.size(); ++i) {
        const SweepGroup &g = groups[i];
        const int32_t v[4] = {g.first, g.t_lo, g.G, g.inserts ? 1 : 0};
        for (int j = 0; j < 4; ++j) out[4 * i + j] = v[j];
    }
    return STCN_OK;
}

int stcn_memread_plan(int N, int Q, int32_t *plan7) {
    if (!plan7 || N < 1 || Q < 1) { set_error("stcn_memread_plan: bad arguments"); return STCN_E_INVALID; }
    export_memread_plan(N, Q, plan7);
    return STCN_OK;
}

int stcn_attention_plan(int hw, int32_t *plan5) {
    if (!plan5 || hw < 1) { set_error("stcn_attention_plan: bad arguments"); return STCN_E_INVALID; }
    const AttnPlan pl = attention_plan(hw);
    const int32_t v[5] = {pl.steps, pl.qblocks, pl.NC, pl.spc, pl.NCeff};
    for (int i = 0; i < 5; ++i) plan5[i] = v[i];
    return STCN_OK;
}

int stcn_memread_scratch(int Q, int64_t *sizes5) {
    if (!sizes5 || Q < 1) { set_error("stcn_memread_scratch: bad arguments"); return STCN_E_INVALID; }
    const MemReadScratchSizes sz = memread_scratch_floats(Q);
    for (size_t i = 0, v[5] = {sz.cand_v, sz.cand_i, sz.cand_n, sz.gmax, sz.tau}; i < 5; ++i) sizes5[i] = (int64_t)v[i];
    return STCN_OK;
}

int stcn_test_decode(const stcn_model *m, void *stream, const float *readout, const float *f16_thin, const float *f8,
                     const float *f4, int k, int nh, int nw, float *logit4, float *agg) {
    if (!m || !readout || !f16_thin || !f8 || !f4 || !agg) { set_error("stcn_test_decode: bad arguments"); return STCN_E_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    TmpWork t(nh, nw, k);
    RC(t.rc);
    const Dims &d = t.w.d;
    DevBuf s8, s4;
    RC(s8.alloc((size_t)d.hw8 * 512)); RC(s4.alloc((size_t)d.hw4 * 256));
    // one frame as a broadcast source (batch stride 0), as the hook always ran these two
    RC(run_conv(m->m, t.w, s, "decoder.up_16_8.skip_conv", ConvArgs(f8, 512, 1, d.h8, d.w8, 0).out(s8.p)));
    RC(run_conv(m->m, t.w, s, "decoder.up_8_4.skip_conv", ConvArgs(f4, 256, 1, d.h4, d.w4, 0).out(s4.p)));
    RC(decode(m->m, t.w, s, readout, f16_thin, s8.p, s4.p, agg, d.npix));
    if (logit4) HIPCHK(hipMemcpyAsync(logit4, t.w.logit4, (size_t)k * d.hw4 * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_test_attention(void *stream, const float *mk, const float *qk, const float *pos, const float *neg, int kk, int nh,
                        int nw, float *attn) {
    if (!pos || !neg) { set_error("stcn_test_attention: bad arguments"); return STCN_E_INVALID; }
    return stcn_test_attention_ex(stream, mk, qk, pos, neg, kk, nh, nw, nullptr, nullptr, nullptr, nullptr, attn);
}

int stcn_test_attention_ex(void *stream, const float *mk, const float *qk, const float *pos, const float *neg, int kk, int nh, int nw,
                           const float *msq_in, const float *pooled_in, float *pooled_out, float *amap_out, float *attn) {
    const char *who = "stcn_test_attention_ex";
    if (!mk || !qk || !attn || kk < 1 || kk > STCN_MAX_OBJECTS + 1) { set_error("%s: bad arguments (mk, qk, attn non-null, 1 <= kk <= %d; kk=%d)", who, STCN_MAX_OBJECTS + 1, kk); return STCN_E_INVALID; }
    if (nh < 16 || nw < 16 || nh % 16 || nw % 16 || (long)nh * nw > MAX_FRAME_PIXELS) { set_error("%s: bad frame %d x %d (multiples of 16, at most 2^24 pixels)", who, nh, nw); return STCN_E_INVALID; }
    // the masks of the interaction, or their pooled means from an earlier call - one of the two
    if (pooled_in ? (pos || neg) : (!pos || !neg)) { set_error("%s: pos and neg, or pooled_in alone", who); return STCN_E_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const int h = nh / 16, w = nw / 16, nchp = attention_nchp(2 * kk);
    DevBuf msq, pooled, amap, gm, part;
    RC(gm.alloc((size_t)256 * h * w)); RC(part.alloc(attention_part_floats(kk, h * w)));
    RC(pooled.alloc((size_t)std::max(20, nchp) * h * w)); RC(amap.alloc((size_t)kk * 2 * h * w));
    if (!msq_in) {
        RC(msq.alloc(h * w + MEMREAD_MSQ_PAD));
        HIPCHK(hipMemsetAsync(msq.p, 0, (size_t)(h * w + MEMREAD_MSQ_PAD) * 4, s));
        rowsumsq_launch(mk, h * w, 64, msq.p, s);
    }
    if (pooled_in) HIPCHK(hipMemcpyAsync(pooled.p, pooled_in, (size_t)nchp * h * w * 4, hipMemcpyDeviceToDevice, s));
    attention_read_launch(mk, msq_in ? msq_in : msq.p, qk, pos, neg, kk, h, w, pooled.p, amap.p, attn, AttnScratch{gm.p, part.p}, s);
    if (pooled_out) HIPCHK(hipMemcpyAsync(pooled_out, pooled.p, (size_t)nchp * h * w * 4, hipMemcpyDeviceToDevice, s));
    if (amap_out) HIPCHK(hipMemcpyAsync(amap_out, amap.p, (size_t)kk * 2 * h * w * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_test_fusion(const stcn_model *m, void *stream, const float *img, const float *prev, const float *curr,
                     const float *attn, float nc, float nr, int nh, int nw, float *logit) {
    if (!m || !img || !prev || !curr || !attn || !logit) { set_error("stcn_test_fusion: bad arguments"); return STCN_E_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    TmpWork t(nh, nw, 1);
    RC(t.rc);
    DevBuf img4;
    RC(img4.alloc((size_t)t.w.d.npix * 4));
    RC(pack_one(img, nh, nw, img4.p, s));
    RC(fusion_logit(m->m, t.w, s, img4.p, prev, curr, attn, nc, nr, logit));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// ---- J / F metrics: every argument is checked before any device call --------------------------------------------------------------------
static int bound_radius(int H, int W) { return (int)std::ceil(0.008 * std::sqrt((double)H * H + (double)W * W)); }      // interactions/metrics.py:119-120

// What all the entry points check: k where the call has one (label maps), the shape - min_hw = 2 where a boundary map can be built, 1 for
// the binary J-only call - the disk radius where the call builds boundary maps (`disk`: disk_scan squares up to r + 1 in int, see
// METRICS_MAX_RADIUS; the J-only forms have no disk and take any shape) and every pointer the call dereferences.
static bool metric_args_ok(const char *who, bool has_k, int k, int T, int H, int W, int min_hw, bool disk, std::initializer_list<const void *> ptrs) {
    if (has_k && (k < 1 || k > STCN_MAX_OBJECTS)) { set_error("%s: k = %d outside 1..%d (STCN_MAX_OBJECTS)", who, k, STCN_MAX_OBJECTS); return false; }
    if (T < 1 || H < min_hw || W < min_hw) { set_error("%s: bad shape (T >= 1, H, W >= %d required; T=%d H=%d W=%d)", who, min_hw, T, H, W); return false; }
    if (disk && bound_radius(H, W) > METRICS_MAX_RADIUS) {
        set_error("%s: H=%d W=%d take a disk of radius %d, above the limit of %d (METRICS_MAX_RADIUS)", who, H, W, bound_radius(H, W), METRICS_MAX_RADIUS);
        return false;
    }
    for (const void *p : ptrs)
        if (!p) { set_error("%s: null pointer", who); return false; }
    return true;
}

int stcn_metrics_jf_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int T, int H, int W,
                           int32_t *counts_dev, uint8_t *scratch_dev) {
    if (!metric_args_ok("stcn_metrics_jf_counts", false, 0, T, H, W, 2, true, {gt_dev, pred_dev, counts_dev, scratch_dev})) return STCN_E_INVALID;
    jf_counts_launch(gt_dev, pred_dev, T, H, W, bound_radius(H, W), scratch_dev, counts_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_metrics_j_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int T, int H, int W, int32_t *counts_dev) {
    if (!metric_args_ok("stcn_metrics_j_counts", false, 0, T, H, W, 1, false, {gt_dev, pred_dev, counts_dev})) return STCN_E_INVALID;
    jf_counts_launch(gt_dev, pred_dev, T, H, W, -1, nullptr, counts_dev, (hipStream_t)stream);       // radius < 0: intersection / union only
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// ---- frame distances (frame_select.hip): the generic entry; stcn_engine_frame_distances (engine.cpp) runs the same launch on the key cache
static bool frame_gram_shape_ok(const char *who, int T, int64_t K) {
    if (T < 1 || T > FRAME_GRAM_MAX_T) { set_error("%s: T=%d outside 1..%d", who, T, FRAME_GRAM_MAX_T); return false; }
    if (K < 4 || K % 4 != 0) { set_error("%s: K=%lld is not a multiple of 4 that is >= 4", who, (long long)K); return false; }
    return true;
}

int stcn_frame_gram_scratch(int T, int64_t K, int64_t *bytes, int32_t *slices) {
    if (!frame_gram_shape_ok("stcn_frame_gram_scratch", T, K)) return STCN_E_INVALID;
    if (bytes) *bytes = (int64_t)frame_gram_scratch_bytes(T, (long)K);
    if (slices) *slices = frame_gram_plan(T, (long)K).slices;
    return STCN_OK;
}

int stcn_frame_sq_distances(void *stream, const float *x_dev, int T, int64_t K, int64_t stride, void *scratch_dev, double *dist_dev) {
    const char *who = "stcn_frame_sq_distances";
    if (!x_dev || !scratch_dev || !dist_dev) { set_error("%s: null pointer (x_dev=%p scratch_dev=%p dist_dev=%p)", who, (const void *)x_dev, scratch_dev, (void *)dist_dev); return STCN_E_INVALID; }
    if (!frame_gram_shape_ok(who, T, K)) return STCN_E_INVALID;
    if (stride < K || stride % 4 != 0) { set_error("%s: stride=%lld is not a multiple of 4 that is >= K=%lld", who, (long long)stride, (long long)K); return STCN_E_INVALID; }
    if ((uintptr_t)x_dev % 16 != 0 || (uintptr_t)scratch_dev % 8 != 0 || (uintptr_t)dist_dev % 8 != 0) {
        set_error("%s: x_dev=%p must be 16-byte aligned (scratch_dev, dist_dev: 8)", who, (const void *)x_dev);
        return STCN_E_INVALID;
    }
    FrameIndex index;
    for (int t = 0; t < FRAME_GRAM_MAX_T; ++t) index.v[t] = t < T ? t : 0;
    frame_gram_launch(x_dev, index, (long)stride, T, (long)K, static_cast<double *>(scratch_dev), dist_dev, (hipStream_t)stream);
    return launch_status("frame distances");
}

int stcn_metrics_objects_scratch(int k, int T, int H, int W, int64_t *bytes) {
    if (!metric_args_ok("stcn_metrics_objects_scratch", true, k, T, H, W, 2, true, {bytes})) return STCN_E_INVALID;
    *bytes = (int64_t)label_scratch_bytes(k, T, H, W);
    return STCN_OK;
}

int stcn_metrics_objects_jf_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int k, int T, int H, int W, int32_t *counts_dev,
                                   void *scratch_dev) {
    if (!metric_args_ok("stcn_metrics_objects_jf_counts", true, k, T, H, W, 2, true, {gt_dev, pred_dev, counts_dev, scratch_dev})) return STCN_E_INVALID;
    label_counts_launch(gt_dev, pred_dev, k, T, H, W, bound_radius(H, W), scratch_dev, counts_dev, T, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_metrics_objects_j_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int k, int T, int H, int W, int32_t *counts_dev) {
    if (!metric_args_ok("stcn_metrics_objects_j_counts", true, k, T, H, W, 2, false, {gt_dev, pred_dev, counts_dev})) return STCN_E_INVALID;
    label_counts_launch(gt_dev, pred_dev, k, T, H, W, -1, nullptr, counts_dev, T, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// Both round entry points.  labels: label maps of k objects, flags = present; else binary masks, flags = noobj, no object_quality.  Frames
// [t0, t1) are composed and counted now; the counts (and gen) of the other frames are the caller's from earlier rounds.
static int metrics_round(const char *who, bool labels, void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev,
                         const uint8_t *annotated_dev, const uint8_t *flags_dev, int k, int T, int H, int W, int t0, int t1, int j_only, double no_object,
                         uint8_t *gen_dev, void *scratch_dev, int32_t *counts_dev, double *object_quality_dev, double *quality_dev, int32_t *select_dev,
                         bool typed = false, const uint8_t *annot_dev = nullptr) {
    const void *unused = who;       // in the place of a pointer that this form of the call does not read
    if (!metric_args_ok(who, labels, k, T, H, W, 2, !j_only, {masks_dev, gt_dev, annotated_dev, flags_dev, gen_dev, counts_dev, labels ? object_quality_dev : unused,
                                                    quality_dev, select_dev, j_only ? unused : scratch_dev, typed ? annot_dev : unused}))
        return STCN_E_INVALID;
    if (lh < 0 || lw < 0 || lh + H > nh || lw + W > nw) { set_error("%s: the %d x %d crop at (%d, %d) leaves the %d x %d tensor", who, H, W, lh, lw, nh, nw); return STCN_E_INVALID; }
    if (t0 < 0 || t1 > T || t0 >= t1) { set_error("%s: frames [%d, %d) are not a non-empty range inside [0, %d)", who, t0, t1, T); return STCN_E_INVALID; }
    const size_t hw = (size_t)H * W;
    void *scratch = j_only ? nullptr : (char *)scratch_dev + (labels ? label_scratch_bytes(k, t0, H, W) : t0 * hw);      // the scratch of frame t0
    round_score_launch(masks_dev + (size_t)t0 * nh * nw, nh, nw, lh, lw, gt_dev + t0 * hw, annotated_dev + t0, flags_dev, labels ? k : 0, t1 - t0, H, W,
                       j_only ? -1 : bound_radius(H, W), no_object, gen_dev + t0 * hw, scratch, counts_dev + (size_t)t0 * 6, T, object_quality_dev,
                       quality_dev, select_dev, (hipStream_t)stream, t0, typed ? annot_dev + t0 * hw : nullptr);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_metrics_round_typed(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev, const uint8_t *type_dev,
                             const uint8_t *annot_dev, const uint8_t *noobj_dev, int T, int H, int W, int t0, int t1, int j_only, double no_object,
                             uint8_t *gen_dev, uint8_t *scratch_dev, int32_t *counts_dev, double *quality_dev, int32_t *select_dev) {
    return metrics_round("stcn_metrics_round_typed", false, stream, masks_dev, nh, nw, lh, lw, gt_dev, type_dev, noobj_dev, 0, T, H, W, t0, t1, j_only,
                         no_object, gen_dev, scratch_dev, counts_dev, nullptr, quality_dev, select_dev, true, annot_dev);
}

int stcn_metrics_round(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev, const uint8_t *annotated_dev,
                       const uint8_t *noobj_dev, int T, int H, int W, int t0, int t1, int j_only, double no_object, uint8_t *gen_dev, uint8_t *scratch_dev,
                       int32_t *counts_dev, double *quality_dev, int32_t *select_dev) {
    return metrics_round("stcn_metrics_round", false, stream, masks_dev, nh, nw, lh, lw, gt_dev, annotated_dev, noobj_dev, 0, T, H, W, t0, t1, j_only,
                         no_object, gen_dev, scratch_dev, counts_dev, nullptr, quality_dev, select_dev);
}

int stcn_metrics_trial(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev, const uint8_t *annotated_dev,
                       const uint8_t *noobj_dev, int candidate, int T, int H, int W, int t0, int t1, int j_only, double no_object,
                       const int32_t *counts_dev, uint8_t *span_gen_dev, uint8_t *scratch_dev, int32_t *span_counts_dev, double *quality_dev) {
    const char *who = "stcn_metrics_trial";
    const void *unused = who;
    if (!metric_args_ok(who, false, 0, T, H, W, 2, !j_only, {masks_dev, gt_dev, annotated_dev, noobj_dev, counts_dev, span_gen_dev, span_counts_dev, quality_dev,
                                                    j_only ? unused : scratch_dev}))
        return STCN_E_INVALID;
    if (lh < 0 || lw < 0 || lh + H > nh || lw + W > nw) { set_error("%s: the %d x %d crop at (%d, %d) leaves the %d x %d tensor", who, H, W, lh, lw, nh, nw); return STCN_E_INVALID; }
    if (t0 < 0 || t1 > T || t0 > t1) { set_error("%s: frames [%d, %d) are not a range inside [0, %d)", who, t0, t1, T); return STCN_E_INVALID; }
    if (candidate < 0 || candidate >= T) { set_error("%s: candidate frame %d outside [0, %d)", who, candidate, T); return STCN_E_INVALID; }
    const size_t hw = (size_t)H * W;
    trial_score_launch(masks_dev + (size_t)t0 * nh * nw, nh, nw, lh, lw, gt_dev + t0 * hw, annotated_dev + t0, noobj_dev,
                       candidate >= t0 && candidate < t1 ? candidate - t0 : -1, T, H, W, t0, t1, j_only ? -1 : bound_radius(H, W), no_object, counts_dev,
                       span_gen_dev, scratch_dev, span_counts_dev, quality_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_metrics_objects_round(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev,
                               const uint8_t *annotated_dev, const uint8_t *present_dev, int k, int T, int H, int W, int t0, int t1, int j_only,
                               double no_object, uint8_t *gen_dev, void *scratch_dev, int32_t *counts_dev, double *object_quality_dev,
                               double *quality_dev, int32_t *select_dev) {
    return metrics_round("stcn_metrics_objects_round", true, stream, masks_dev, nh, nw, lh, lw, gt_dev, annotated_dev, present_dev, k, T, H, W, t0, t1,
                         j_only, no_object, gen_dev, scratch_dev, counts_dev, object_quality_dev, quality_dev, select_dev);
}

// ---- the simulated user (robot.hip): every argument is checked before any device call ---------------------------------------------------
static bool robot_args_ok(const char *who, int H, int W, std::initializer_list<const void *> ptrs) {
    if (H < 1 || W < 1 || (long)H * W > MAX_FRAME_PIXELS) { set_error("%s: bad frame %d x %d (1 <= H * W <= 2^24 pixels)", who, H, W); return false; }
    for (const void *p : ptrs)
        if (!p) { set_error("%s: null pointer", who); return false; }
    return true;
}

int stcn_robot_scratch(int H, int W, int64_t *bytes) {
    if (!robot_args_ok("stcn_robot_scratch", H, W, {bytes})) return STCN_E_INVALID;
    *bytes = (int64_t)robot_scratch_bytes(H, W);
    return STCN_OK;
}

int stcn_robot_click(void *stream, const uint8_t *pred_dev, const uint8_t *gt_dev, int H, int W, int mode, int use_iou, double iou, void *scratch_dev,
                     int32_t *record_dev, uint8_t *component_dev) {
    const char *who = "stcn_robot_click";
    if (mode != STCN_ROBOT_INTERACT && mode != STCN_ROBOT_MIDDLE) { set_error("%s: mode %d is neither STCN_ROBOT_INTERACT nor STCN_ROBOT_MIDDLE", who, mode); return STCN_E_INVALID; }
    const void *unused = who;
    if (!robot_args_ok(who, H, W, {mode == STCN_ROBOT_MIDDLE ? unused : pred_dev, gt_dev, scratch_dev, record_dev})) return STCN_E_INVALID;
    if ((uintptr_t)scratch_dev % 8 != 0) { set_error("%s: scratch_dev=%p must be 8-byte aligned", who, scratch_dev); return STCN_E_INVALID; }
    robot_click_launch(pred_dev, gt_dev, H, W, mode == STCN_ROBOT_MIDDLE, use_iou && iou < 0.1, scratch_dev, record_dev, component_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_robot_bbox(void *stream, const uint8_t *mask_dev, int H, int W, int32_t *record_dev) {
    if (!robot_args_ok("stcn_robot_bbox", H, W, {mask_dev, record_dev})) return STCN_E_INVALID;
    robot_bbox_launch(mask_dev, H, W, record_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_robot_best_mask(void *stream, const uint8_t *cand_dev, const uint8_t *target_dev, int M, int H, int W, int32_t *out_dev) {
    const char *who = "stcn_robot_best_mask";
    if (M < 1 || M > STCN_ROBOT_MAX_CANDIDATES) { set_error("%s: M = %d outside 1..%d (STCN_ROBOT_MAX_CANDIDATES)", who, M, STCN_ROBOT_MAX_CANDIDATES); return STCN_E_INVALID; }
    if (!robot_args_ok(who, H, W, {cand_dev, target_dev, out_dev})) return STCN_E_INVALID;
    robot_best_mask_launch(cand_dev, target_dev, M, H, W, out_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// ---- masks as network input (resize.hip): every argument is checked before any device call ---------------------------------------------
int stcn_masks_resize_nearest(void *stream, const uint8_t *src, int T, int H, int W, const int32_t *frames_dev, int n, int out_h, int out_w, int channels,
                              float *out) {
    const char *who = "stcn_masks_resize_nearest";
    if (!src || !out) { set_error("%s: null pointer (%s)", who, !src ? "src" : "out"); return STCN_E_INVALID; }
    if (T < 1 || H < 1 || W < 1) { set_error("%s: bad source [%d, %d, %d]: every size is at least 1", who, T, H, W); return STCN_E_INVALID; }
    if (out_h < 1 || out_w < 1 || channels < 1 || (long)out_h * out_w > MAX_FRAME_PIXELS) {
        set_error("%s: bad output [n, %d, %d, %d]: every size is at least 1, out_h * out_w at most 2^24", who, channels, out_h, out_w);
        return STCN_E_INVALID;
    }
    if (frames_dev && n <= 0) { set_error("%s: frames_dev is given with n = %d (at least 1 frame)", who, n); return STCN_E_INVALID; }
    if (!frames_dev && (n <= 0 || n > T)) { set_error("%s: n = %d without frames_dev means the first n of the T = %d frames (1 <= n <= T)", who, n, T); return STCN_E_INVALID; }
    if (n > 65535) { set_error("%s: n = %d frames in one call, at most 65535", who, n); return STCN_E_INVALID; }
    masks_resize_nearest_launch(src, T, H, W, frames_dev, n, out_h, out_w, channels, out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// ---- frames as stored images (rgb8.hip): every argument is checked before any device call -------------------------------------------------
int stcn_frames_to_rgb8(void *stream, const float *clip_dev, int T, int H, int W, const int32_t *frames_dev, int n, void *scratch_dev, uint8_t *out_dev) {
    const char *who = "stcn_frames_to_rgb8";
    if (!clip_dev || !scratch_dev || !out_dev) {
        set_error("%s: null pointer (%s)", who, !clip_dev ? "clip_dev" : !scratch_dev ? "scratch_dev" : "out_dev");
        return STCN_E_INVALID;
    }
    if (n < 0 || n > 65535) { set_error("%s: n = %d frames in one call (0 <= n <= 65535)", who, n); return STCN_E_INVALID; }
    if (T < 1 || H < 1 || W < 1 || (long)H * W > MAX_FRAME_PIXELS) {
        set_error("%s: bad clip [%d, 3, %d, %d]: every size is at least 1, H * W at most 2^24", who, T, H, W);
        return STCN_E_INVALID;
    }
    if ((uintptr_t)clip_dev % 4 != 0 || (uintptr_t)scratch_dev % 4 != 0) {
        set_error("%s: clip_dev=%p and scratch_dev=%p must be 4-byte aligned", who, (const void *)clip_dev, scratch_dev);
        return STCN_E_INVALID;
    }
    if (n == 0) return STCN_OK;
    frames_to_rgb8_launch(clip_dev, T, H, W, frames_dev, n, scratch_dev, out_dev, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

// ---- a clip at a working resolution (rescale.hip): every argument is checked before any device call -------------------------------------
int stcn_prob_upsample_argmax(void *stream, const float *prob, int k1, int T, int nh, int nw, int lh, int lw, int h, int w, int H, int W, int t0, int t1,
                              uint8_t *masks_out) {
    const char *who = "stcn_prob_upsample_argmax";
    if (!prob || !masks_out) { set_error("%s: null pointer (%s)", who, !prob ? "prob" : "masks_out"); return STCN_E_INVALID; }
    if (k1 < 2 || k1 > STCN_MAX_OBJECTS + 1) { set_error("%s: k1 = %d channels outside 2..%d (background + 1..%d objects)", who, k1, STCN_MAX_OBJECTS + 1, STCN_MAX_OBJECTS); return STCN_E_INVALID; }
    if (T < 1 || nh < 1 || nw < 1) { set_error("%s: bad prob [%d, T = %d, 1, nh = %d, nw = %d]: every size is at least 1", who, k1, T, nh, nw); return STCN_E_INVALID; }
    if (h < 1 || w < 1 || lh < 0 || lw < 0 || (long)lh + h > nh || (long)lw + w > nw) {
        set_error("%s: the window h = %d x w = %d at lh = %d, lw = %d is empty or outside the padded plane nh = %d x nw = %d", who, h, w, lh, lw, nh, nw);
        return STCN_E_INVALID;
    }
    if (H < 1 || W < 1 || (long)H * W > MAX_FRAME_PIXELS) { set_error("%s: bad output [T, H = %d, W = %d]: every size is at least 1, H * W at most 2^24", who, H, W); return STCN_E_INVALID; }
    if (t0 < 0 || t1 > T || t0 > t1) { set_error("%s: frames [t0 = %d, t1 = %d) are no range inside [0, T = %d]", who, t0, t1, T); return STCN_E_INVALID; }
    if (t0 == t1) return STCN_OK;
    prob_upsample_argmax_launch(prob, k1, T, nh, nw, lh, lw, h, w, H, W, t0, t1, masks_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_frames_downsample_aa(void *stream, const float *src, int planes, int H, int W, int h, int w, float *dst) {
    const char *who = "stcn_frames_downsample_aa";
    if (!src || !dst) { set_error("%s: null pointer (%s)", who, !src ? "src" : "dst"); return STCN_E_INVALID; }
    if (planes < 1) { set_error("%s: planes = %d, at least 1", who, planes); return STCN_E_INVALID; }
    if (H < 1 || W < 1 || (long)H * W > MAX_FRAME_PIXELS) { set_error("%s: bad source [planes, H = %d, W = %d]: every size is at least 1, H * W at most 2^24", who, H, W); return STCN_E_INVALID; }
    if (h < 1 || w < 1) { set_error("%s: bad output [planes, h = %d, w = %d]: every size is at least 1", who, h, w); return STCN_E_INVALID; }
    if (h > H || w > W) { set_error("%s: h = %d > H = %d or w = %d > W = %d: frames are never enlarged", who, h, H, w, W); return STCN_E_INVALID; }
    HIPCHK(frames_downsample_aa_launch(src, planes, H, W, h, w, dst, (hipStream_t)stream));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

int stcn_bench_mfma_rate(void *stream, int ms_target, float *tflops, float *ms_out) {
    if (!tflops || ms_target < 1 || ms_target > 2000) { set_error("stcn_bench_mfma_rate: bad arguments"); return STCN_E_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    const int cus = device_cus();
    DevBuf out;
    RC(out.alloc(64));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    // one wave-iteration = 12 MFMAs x 64 cycles x 3 waves per SIMD: ~1.15 us at 2 GHz; warm-up launch, then the timed one
    const int iters = ((int)(ms_target * 1000.0 / 1.15) + 3) / 4 * 4;         // the kernel walks 4 iterations per loop trip
    (void)mfma_probe_launch(out.p, 2 * cus, (iters / 8 + 3) / 4 * 4, s);
    HIPCHK(hipEventRecord(e0, s));
    const double fl = mfma_probe_launch(out.p, 2 * cus, iters, s);              // two workgroups per CU in turn (one resident: 768 threads x 2 fit)
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    *tflops = (float)(fl / (ms * 1e-3) / 1e12);
    if (ms_out) *ms_out = ms;
    return STCN_OK;
}

// One launch of a small kernel by name (include/stcn_hip.h lists the arguments of each).  Names and counts are checked before any device call.
int stcn_test_kernel(const char *name, void *stream, void *const *ptrs, int nptr, const int64_t *iv, int ni, const double *fv, int nf) {
    const SmallKernel *k = nullptr;
    for (const SmallKernel &c : SMALL_KERNELS)
        if (name && !strcmp(name, c.name)) k = &c;
    if (!k) { set_error("stcn_test_kernel: unknown kernel '%s'", name ? name : "(null)"); return STCN_E_INVALID; }
    bool ok = nptr == k->nptr && ni == k->ni && nf == k->nf && ptrs && iv && (nf == 0 || fv);
    for (int i = 0; ok && i < nptr; ++i) ok = ptrs[i] != nullptr;
    for (int i = 0; ok && i < ni; ++i) ok = iv[i] >= 0 && iv[i] <= ((k->wide >> i) & 1 ? (1LL << 40) : (long long)INT_MAX);      // the int parameters are not narrowed
    if (!ok) {
        set_error("stcn_test_kernel: '%s' takes %d non-null pointers, %d non-negative integers and %d doubles (got %d, %d, %d); sizes fit an int, strides 2^40",
                  k->name, k->nptr, k->ni, k->nf, nptr, ni, nf);
        return STCN_E_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const std::string n = k->name;
    auto F = [&](int i) { return static_cast<float *>(ptrs[i]); };
    auto I = [&](int i) { return (int)iv[i]; };
    // the sizes the kernels take on trust: object counts within the register arrays, channel counts in whole 16-byte accesses
    auto objects = [&](int64_t v) { return v >= 1 && v <= STCN_MAX_OBJECTS; };
    auto bad = [&](const char *what) { set_error("stcn_test_kernel: '%s' needs %s", k->name, what); return STCN_E_INVALID; };
    DevBuf scratch;
    if (n == "maxpool3x3s2") {
        if (iv[3] % 4 || iv[3] < 4 || iv[1] < 2 || iv[2] < 2 || iv[0] < 1) return bad("B >= 1, H, W >= 2, C % 4 == 0");
        maxpool3x3s2_launch(F(0), F(1), I(0), I(1), I(2), I(3), s);
    } else if (n == "upsample2x_add") {
        if (iv[3] % 4 || iv[3] < 4 || iv[0] < 1 || iv[1] < 1 || iv[2] < 1) return bad("B, h, w >= 1, C % 4 == 0");
        upsample2x_add_launch(F(0), F(1), F(2), I(0), I(1), I(2), I(3), s, (long)iv[4], I(5));
    } else if (n == "up4_sigmoid_aggregate") {
        if (!objects(iv[0]) || iv[1] < 1 || iv[2] < 1 || iv[5] < 1) return bad("1 <= k <= STCN_MAX_OBJECTS, h4, w4, G >= 1");
        up4_sigmoid_aggregate_launch(F(0), I(0), I(1), I(2), F(1), (long)iv[3], s, (long)iv[4], I(5), (long)iv[6], (long)iv[7]);
    } else if (n == "up4_sigmoid") {
        if (!objects(iv[0]) || iv[1] < 1 || iv[2] < 1) return bad("1 <= k <= STCN_MAX_OBJECTS, h4, w4 >= 1");
        up4_sigmoid_launch(F(0), I(0), I(1), I(2), F(1), s);
    } else if (n == "sigmoid_aggregate") {
        if (!objects(iv[0]) || iv[1] < 1) return bad("1 <= k <= STCN_MAX_OBJECTS, npix >= 1");
        sigmoid_aggregate_launch(F(0), I(0), (long)iv[1], F(1), (long)iv[2], s);
    } else if (n == "argmax") {
        if (iv[0] < 1 || iv[0] > 256 || iv[1] < 1 || iv[2] < 1) return bad("1 <= kk <= 256 (uint8 masks), T, npix >= 1");
        argmax_launch(F(0), I(0), I(1), (long)iv[2], static_cast<uint8_t *>(ptrs[1]), s);
    } else if (n == "rowsumsq") {
        if (iv[0] < 1 || iv[1] % 4 || iv[1] < 4 || iv[2] < 1) return bad("n, B >= 1, C % 4 == 0");
        rowsumsq_launch(F(0), I(0), I(1), F(1), s, I(2), (long)iv[3], (long)iv[4]);
    } else if (n == "pack_image") {
        if (iv[0] < 1 || iv[1] < 1 || iv[4] + iv[1] > iv[3] || iv[5] + iv[0] > iv[2]) return bad("H, W >= 1, lh + H <= nh, lw + W <= nw");
        pack_image_launch(F(0), F(1), I(0), I(1), I(2), I(3), I(4), I(5), s);
    } else if (n == "pack_value_input") {
        if (!objects(iv[1]) || iv[2] < 1) return bad("1 <= k <= STCN_MAX_OBJECTS, npix >= 1");
        pack_value_input_launch(F(0), F(1), (long)iv[0], I(1), I(2), F(2), s);
    } else if (n == "pack_fusion_input") {
        if (iv[0] < 1) return bad("npix >= 1");
        pack_fusion_input_launch(F(0), F(1), F(2), F(3), (float)fv[0], (float)fv[1], (long)iv[0], F(4), s);
    } else if (n == "interact_mask") {
        if (iv[8] < 1 || (iv[0] != 1 && iv[0] != iv[8]) || iv[1] < 1 || iv[2] < 1 || iv[6] + iv[1] > iv[3] || iv[5] + iv[2] > iv[4])
            return bad("kk >= 1, mc 1 or kk, H, W >= 1, lh + H <= nh, lw + W <= nw");
        interact_mask_launch(F(0), I(0), I(1), I(2), I(3), I(4), I(5), I(6), F(1), (long)iv[7], I(8), F(2), F(3), F(4), s);
    } else if (n == "cbam") {
        if (iv[0] < 1 || iv[1] < 1 || iv[2] < 1) return bad("B, h, w >= 1");
        RC(scratch.alloc((size_t)iv[0] * (16 * 1024 + 512 + 2 * (size_t)(iv[1] * iv[2]))));      // the size kernels.h states
        cbam_launch(F(0), F(1), I(0), I(1), I(2), CbamW{F(2), F(3), F(4), F(5), F(6), (float)fv[0]}, scratch.p, s);
    } else if (n == "copy_rows") {
        if (iv[2] < 1 || iv[3] < 1) return bad("rows, n >= 1");
        copy_rows_launch(F(0), (long)iv[0], F(1), (long)iv[1], I(2), (long)iv[3], s);
    } else if (n == "copy2") {
        if (iv[0] % 4) return bad("na % 4 == 0");
        copy2_launch(F(0), F(1), (long)iv[0], F(2), F(3), (long)iv[1], s);
    } else {
        fill_launch(F(0), (float)fv[0], (long)iv[0], s);
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return STCN_OK;
}

}  // extern "C"
