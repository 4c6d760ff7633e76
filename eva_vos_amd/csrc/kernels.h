// kernels.h - launch wrappers of the gfx950 kernels (host-callable, enqueue on a stream).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "../../include/stcn_hip.h"   // STCN_MAX_OBJECTS

namespace stcn {

// ---------------------------------------------------------------- division by a launch invariant
// An integer division by a run-time value costs ~25 VALU instructions on gfx950 (float reciprocal + correction), also for
// wave-uniform operands; the conv kernels did 5-10 of them per workgroup in set-up / epilogue code, which the fp32 MFMA of the
// co-resident workgroups cannot hide.  q = (x * magic) >> (31 + s) with magic = floor(2^(31+s) / d) + 1, s = ceil(log2 d), is
// exact for 0 <= x < 2^31 (x * (magic * d - 2^(31+s)) <= x * d < 2^(31+s)): one v_mul_hi + one shift.
struct FastDiv {
    unsigned magic, shift, d;       // shift = s - 1 (after the mul_hi's 32); d == 1: identity
};
static inline FastDiv fastdiv_make(unsigned d) {
    FastDiv f{0, 0, d};
    if (d <= 1) return f;
    unsigned s = 0;
    while ((1ull << s) < d) ++s;
    f.magic = (unsigned)(((1ull << (31 + s)) / d) + 1);
    f.shift = s - 1;
    return f;
}
#if defined(__HIPCC__)
__device__ __forceinline__ int fastdiv(int x, const FastDiv f) {
    return f.d <= 1 ? x : (int)(__umulhi((unsigned)x, f.magic) >> f.shift);
}
// Workgroups are dealt round-robin over the 8 XCDs (each with its own 4 MB L2): blocks b and b + 8 share one.  Kernels whose
// NEIGHBOURING blocks share input (stencil halos, bilinear taps, im2col rows) walk their index space in this order instead: every XCD
// gets one contiguous eighth, so shared lines are fetched into ONE L2 (bijective for any grid size; speed only, never correctness).
__device__ __forceinline__ int xcd_contiguous_block(int bid, int nblk) {
    const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}
#endif

// ---------------------------------------------------------------- process-level switches and the device's size
// A switch that holds for the whole process is a function-local `static const` initialised from one of these, so the variable is read
// once, at the first use (not per workspace as the Knobs below: moving one there would change when it takes effect).
static inline int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
static inline bool env_on(const char *name, bool dflt = true) { return env_int(name, dflt) != 0; }
// compute units of the current device at the first call (256 when it cannot be asked); read once per process
int device_cus();

// ---------------------------------------------------------------- launch-level tunables
// Read from the environment ONCE per workspace (= once per engine, once per stage-hook call) by Knobs::from_env() and carried in
// every ConvP - never read per launch: a driver may change os.environ between legs while host threads of other lanes launch.
struct Knobs {
    int wino_min_cin = 128;     // STCN_WINO_MIN_CIN: fewest input channels for which a stride-1 3x3 conv takes the F(2x2) path
    int wino_ppw = 0;           // STCN_WINO_PPW: 1 / 2 pins the F(2x2) GEMM instance (positions per wave), 0 = by shape
    int wino4_chunk_mb = 160;   // STCN_WINO4_CHUNK_MB: V bytes per slice of a chunked F(4x4) launch (0: unchunked)
    int fusion_conv12 = 0;      // STCN_FUSION_CONV12: FusionNet conv1 on the direct FusionNet kernel
    int fusion_wino = 1;        // STCN_FUSION_WINO: FusionNet convs as Winograd F(2x2) inside the workgroup
    int pw_chain = 2;           // STCN_PW_CHAIN: large pointwise convs on the chain kernel (several tiles per workgroup, one pipeline): 0 off,
                                // 1 consecutive tiles per workgroup, 2 tiles strided over the grid (default)
    // how the 32-tile F(4x4) GEMM is fed (neither changes a bit of any output):
    int wino4_piece_xcd = 1;    // STCN_WINO4_PIECE_XCD: K-piece workgroups in 2-D blocks per XCD (0: tile-major order, pieces inside)
    int wino4_share_v = 1;     // STCN_WINO4_SHARE_V: a conv that says so reuses V of the previous transform of the same input (0: always transforms)
    static Knobs from_env();
};

// ---------------------------------------------------------------- implicit-GEMM convolution
// Activations NHWC fp32.  Input = channel-concat of up to two sources (second may be batch-broadcast).
struct ConvP {
    const float *x0, *x1;   // sources; x1 == nullptr when unused
    int c0, c1;             // channels of each source (multiples of 4)
    long bs0, bs1;          // batch strides in elements (0 = broadcast over the batch)
    unsigned x0_bytes, x1_bytes, w_bytes;   // extents for the buffer descriptors (hardware bounds check)
    int B, H, W;            // input batch / spatial
    int OH, OW;
    int KH, KW, stride, pad;
    int Cin;                // c0 + c1
    int M, N;               // M = B*OH*OW rows, N = Cout
    int K, Kp;              // K = KH*KW*Cin, Kp = K rounded up to 32 (weights zero-padded)
    const float *w;         // [N][Kp], k ordered (kh, kw, cin)
    const float *bias;      // [N] or nullptr
    const float *res;       // residual [B][OH*OW][N] or nullptr
    long res_bs;            // batch stride of res (0 = broadcast)
    int res_bmod;           // > 0: the residual of batch element b is res + (b % res_bmod) * res_bs (a per-FRAME tensor under a
                            // batch laid out [object][frame]: decode groups of multi-object engines)
    float *y;               // [M][N]
    long y_bs;              // output batch stride in elements (0 = dense OH*OW*N)
    int relu_in, relu_out;
    int splitk;             // >= 1
    float *partial;         // [splitk][M][N] workspace when splitk > 1
    // tail balancing (splitk == 1 only, see conv_plan): tiles [0, rem_full) run whole; each of the remaining tiles is
    // cut into rem_split K pieces of rem_per K tiles whose tile-local partial sums go to `partial`
    // ([(tile - rem_full) * rem_split + piece][BM][BN]) and are summed by conv_reduce_tiles_kernel
    int rem_full, rem_split, rem_per;
    const float *wino_u;    // Winograd-transformed weights [16][Cin/8][N][8] (stride-1 3x3 convs with Cin >= 64, N % 64 == 0) or nullptr
    const float *wino4_u;   // Winograd F(4x4,3x3) weights [36][Cin/8][N][8] (decoder layers only: winograd4.hip) or nullptr
    FastDiv fd_ohw, fd_ow;  // divisions by OH*OW and OW
    FastDiv fd_cin, fd_kw;  // divisions by Cin and KW (the stem instance decodes (tap, channel) of its K index per thread and K tile)
    int pointwise;          // 1x1, stride 1, no padding, one dense source: im2col row m IS activation row m (no row decode)
    int affine_out;         // y (and res, if any) are dense [M][N]: element (m, n) at (m * N + n) * 4 bytes, < 4 GiB
    int tile_big;           // 1 = 128x128 workgroup tiles (fp32 kernel)
    int panel;              // > 0: tiles are walked in panels of this many n-tiles (fp32 kernel)
    int chain;              // > 0: pointwise chain kernel, this many consecutive tiles per workgroup (conv_plan)
    Knobs kn;               // the workspace's snapshot of the launch-level tunables
};
// ---------------------------------------------------------------- the plan of one convolution
// Filled ONCE per run_conv call (engine.cpp plan_conv) by the planning function of the family that takes the conv; the accounting, the
// profiling event pairs, the path string of the tests and the family's launch function all read this one object - nothing plans again.
constexpr int W4_MAX_CHUNKS = 16;       // most slices of a chunked F(4x4) launch (wino4_plan); one profiling event pair per slice
// tile geometry of a Winograd conv (wino_geom): TH x TW output tiles per image, Mt of them in the batch, padded to whole workgroup tiles;
// KB k-blocks of 8 input channels
struct WinoGeom { int TH, TW, Mt, Mt_pad, KB; };
// launch plan of the F(2x2) GEMM: ntile = (Mt_pad / 64) x tiles_n workgroup tiles, each cut into ConvPlan::splitk ranges of kb_per_split k-blocks
struct W2Plan { int tiles_n, ntile, kb_per_split; };
// launch plan of the F(4x4) GEMM: 64- or 32-tile workgroups, and (32-tile only) the tail split.  judge_wg: the workgroup count that
// eligibility holds against Model::wino4_min_wg (wino4_gemm_plan says how it differs from grid)
struct W4Plan { int tiles_m, tiles_n, mb, grid, full_wg, pieces, per, chunks, tm_per_chunk, judge_wg; };
enum ConvFamily { CONV_LITERAL = 0, CONV_FUSION = 1, CONV_WINO4 = 2, CONV_WINO2 = 3, CONV_DIRECT = 4 };
struct ConvPlan {
    int family = CONV_LITERAL;
    bool fusion_wino = false;       // CONV_FUSION: Winograd F(2x2,3x3) inside the workgroup (else the direct FusionNet kernel)
    WinoGeom geo{};                 // CONV_WINO4, CONV_WINO2
    W4Plan w4{};                    // CONV_WINO4
    W2Plan w2{};                    // CONV_WINO2
    int splitk = 1;                 // CONV_WINO2: split-K of the Winograd GEMM; CONV_DIRECT: p.splitk
    int ppw = 0;                    // CONV_WINO2: GEMM instance (positions per wave)
    const char *variant = "";       // CONV_DIRECT: conv_variant_name() (the tile plan itself is in ConvP: the kernels read it)
    bool tail = false;              // CONV_DIRECT: tail balancing (p.rem_split > 1)
    size_t v_floats = 0;            // Winograd families: V workspace floats
    int n_in = 0, n_gemm = 1;       // input-transform / GEMM launches (the chunks of an F(4x4) launch; n_in = 0 when run_conv found V in the workspace)
    bool reduce = false;            // a reduce launch follows
    double fl = 0;                  // algorithmic FLOP (set before the family plans)
    double fl_exec = 0;             // FLOP the matrix cores execute (Winograd: fewer)
};
// Per family one planning function (true when the family takes p, its part of pl filled) and one launch function, which takes that plan
// and does not plan.  ev_*: optional {start, stop} event pairs attached to the dispatches themselves (launch(): kernel begin/end
// timestamps, no extra barrier packets).
// direct implicit GEMM (always eligible): fills the launch plan of p (tile variant, split-K or tail balancing); force_splitk > 0 pins
// a plain split-K; workspace_floats = capacity of p.partial
void conv_plan(ConvP &p, int force_splitk, size_t workspace_floats, ConvPlan &pl);
void conv_launch(const ConvP &p, hipStream_t s, hipEvent_t *ev_gemm = nullptr, hipEvent_t *ev_red = nullptr);
// split-K tail of a conv whose slabs p.partial [p.splitk][M][N] are filled: sum + bias / residual / ReLU -> y
void conv_reduce_launch(const ConvP &p, hipStream_t s, hipEvent_t *ev_red = nullptr);
// Winograd F(2x2,3x3) path (winograd.hip): not eligible, or V needs more than v_cap floats -> false.  slab_floats = capacity of p.partial
bool wino_plan(const ConvP &p, size_t v_cap, size_t slab_floats, ConvPlan &pl);
void wino_launch(const ConvP &p, const ConvPlan &pl, float *V, hipStream_t s, hipEvent_t *ev_in = nullptr, hipEvent_t *ev_gemm = nullptr,
                 hipEvent_t *ev_red = nullptr);
void wino_transform_weights(const float *w, int N, int Cin, int Kp, float *U);
// fewest input channels of an F(4x4) layer.  64 (8 k-blocks, one K piece) since round 5: the 64-channel 3x3 convs of the value encoder's
// ResNet-18 layer1 over the objects of a multi-object engine (129 600 rows at k = 5) take 56 instead of 98 us each - config 3 219 -> 224 frames/s;
// at one object they have 52 workgroups and stay on the direct kernel (wino4_min_wg).  The key encoder's 64-channel res2 convs are flagged too since the
// key trunk moved to F(4x4) (engine.cpp wino4_layer; STCN_WINO4_KEY=0 at model creation takes the whole key trunk off F(4x4) again).
#ifndef W4_MIN_CIN
#define W4_MIN_CIN 64
#endif
// Winograd F(4x4,3x3) path (winograd4.hip, decoder layers): not eligible, fewer than min_wg workgroups, or V needs more than v_cap floats -> false
bool wino4_plan(const ConvP &p, int min_wg, size_t v_cap, size_t slab_floats, ConvPlan &pl);
// ev_in / ev_gemm: one {start, stop} pair per chunk (pl.w4.chunks: the transform and the GEMM alternate over slices of the tiles
// when V would not stay in the memory-side cache)
void wino4_launch(const ConvP &p, const ConvPlan &pl, float *V, hipStream_t s, hipEvent_t *const *ev_in = nullptr,
                  hipEvent_t *const *ev_gemm = nullptr, hipEvent_t *ev_red = nullptr);
void wino4_transform_weights(const float *w, int N, int Cin, int Kp, float *U);
// The family switches, read once per process: STCN_WINOGRAD (0: no F(2x2) weights or launches; the V workspace
// is shared and exists while either family is on) and STCN_WINO4
// (0 off, 1 on for flagged layers with enough workgroups (default), 2 whenever the shape allows)
bool wino_enabled();
int wino4_mode();

// FusionNet convs (fusion_conv.hip): 3x3, stride 1, Cout = 32, Cin = 32 or 12, one dense image: weights in registers, patch in LDS
bool fusion_conv_plan(const ConvP &p, ConvPlan &pl);
void fusion_conv_launch(const ConvP &p, const ConvPlan &pl, hipStream_t s, hipEvent_t *ev_gemm = nullptr);

// Cout == 1 convolution (decoder.pred, FusionNet.final_conv): one dot product per output pixel.
// x [B,H,W,C] (C multiple of 4), w [KH*KW*C], y [B*H*W]; stride 1, "same" padding.
void conv_n1_launch(const float *x, const float *w, float bias, float *y, int B, int H, int W, int C,
                    int KH, int relu_in, hipStream_t s);

// ---------------------------------------------------------------- elementwise / pooling
void maxpool3x3s2_launch(const float *x, float *y, int B, int H, int W, int C, hipStream_t s);
// NCHW image [3,H,W] (unpadded) -> NHWC4 padded [nh,nw,4] with zero border (pad lw, lh)
void pack_image_launch(const float *img_chw, float *out, int H, int W, int nh, int nw, int lw, int lh,
                       hipStream_t s);
// value-encoder input [k,nh,nw,8] = (rgb from NHWC4 image, mask_i, sum_{j!=i} mask_j, 0,0,0)
void pack_value_input_launch(const float *img4, const float *masks, long mask_stride, int k, int npix,
                             float *out, hipStream_t s);
// u[b] = skip[b * skip_bs] (skip_bs 0: broadcast over b) + bilinear_up2x(x[b]); x [B,h,w,C] -> u [B,2h,2w,C]
// skip_bmod > 0: the skip of batch element b is skip + (b % skip_bmod) * skip_bs
void upsample2x_add_launch(const float *x, const float *skip, float *u, int B, int h, int w, int C,
                           hipStream_t s, long skip_bs = 0, int skip_bmod = 0);
// logit4 [k,h4*w4] -> bilinear x4 -> sigmoid -> aggregate_wbg -> agg [k+1][nh*nw] (row stride agg_stride)
// obj_stride: floats between the logit planes of consecutive objects (0 = h4*w4)
// G > 1: G frames in one launch - frame g reads logit4 + g * logit_gs and writes agg + g * agg_gs
void up4_sigmoid_aggregate_launch(const float *logit4, int k, int h4, int w4, float *agg,
                                  long agg_stride, hipStream_t s, long obj_stride = 0, int G = 1, long logit_gs = 0, long agg_gs = 0);
// the same tail without the aggregation: logit4 [k,h4*w4] -> bilinear x4 -> sigmoid -> prob [k][nh*nw] (segment_with_query, prop_net.py:192)
void up4_sigmoid_launch(const float *logit4, int k, int h4, int w4, float *prob, hipStream_t s);
// aggregate_wbg (aggregate.py:22-37) on probabilities: prob [k][npix] -> out [k+1][npix] (keep_bg) or [k][npix]; hard: logits x 1000
void aggregate_wbg_launch(const float *prob, int k, long npix, int keep_bg, int hard, float *out, hipStream_t s);
// logits [k,npix] -> sigmoid -> aggregate -> agg rows (fusion output)
void sigmoid_aggregate_launch(const float *logit, int k, long npix, float *agg, long agg_stride,
                              hipStream_t s);
// masks[t] = argmax over rows of prob [(k+1), T, npix] for all t (first max wins)
void argmax_launch(const float *prob, int kk, int T, long npix, uint8_t *masks, hipStream_t s);
// rows [n, C] -> msq[n] = sum_c x^2
// B > 1: B batch elements in one launch (element b at x + b * x_bs -> out + b * out_bs)
void rowsumsq_launch(const float *x, int n, int C, float *out, hipStream_t s, int B = 1, long x_bs = 0, long out_bs = 0);
void fill_launch(float *p, float v, long n, hipStream_t s);
void spin_launch(int us, hipStream_t s);        // test aid: one wave that keeps stream s busy for `us` microseconds
void copy_rows_launch(const float *src, long src_stride, float *dst, long dst_stride, int rows, long n,
                      hipStream_t s);
// a [na floats, na % 4 == 0] -> da and b [nb floats] -> db in one launch
void copy2_launch(const float *a, float *da, long na, const float *b, float *db, long nb, hipStream_t s);
// interaction mask handling (inference_core.py:220-226): pads mask [mc,H,W] into [mc,nh,nw] planes,
// writes pos/neg = clamp(+-(mask - prob[:,idx])) for all kk rows, then prob[:,idx] = mask (broadcast)
void interact_mask_launch(const float *mask, int mc, int H, int W, int nh, int nw, int lw, int lh,
                          float *prob_idx, long prob_row_stride, int kk, float *padded, float *pos,
                          float *neg, hipStream_t s);

// ---------------------------------------------------------------- NCHW <-> rows (layout.hip)
// B planes-tensors [C][ld] (R <= ld elements of every channel plane are read; ld: elements between channel planes) <-> B row-tensors [R][C];
// batch element b at planes + b * planes_bs and rows + b * rows_bs.  C % 4 == 0; R, ld and the alignment of `planes` are free.
void planes_to_rows_launch(const float *planes, long ld, long planes_bs, float *rows, long rows_bs, int B, int R, int C, hipStream_t s);
void rows_to_planes_launch(const float *rows, long rows_bs, float *planes, long ld, long planes_bs, int B, int R, int C, hipStream_t s);

// ---------------------------------------------------------------- CBAM (cbam.py:21-77)
struct CbamW { const float *w1, *b1, *w2, *b2, *wsp; float bsp; };  // 512->32->512 MLP, 7x7 [2] conv
// x [B,hw,512] -> out = x + CBAM(x); scratch >= B*(16*1024 + 512 + 2*hw) floats
void cbam_launch(const float *x, float *out, int B, int h, int w, const CbamW &cw, float *scratch,
                 hipStream_t s);

// ---------------------------------------------------------------- space-time memory read
// the largest top_k the read is built for (every capacity below is sized for it; STCN_MAX_TOP_K of the C ABI) and the default model's
constexpr int MEMREAD_MAX_TOPK = 50;
// launch plan of the top-k read (it does not depend on top_k): `steps` 64-row steps of the bank; pass 1 visits every ss-th step (ns of them) in nc1 chunks of
// spc1 sampled steps, pass 2 all steps in nc2 chunks of spc2
struct MemReadPlan { int steps, ss, ns, nc1, spc1, nc2, spc2; };
MemReadPlan memread_plan(int N, int Q);
struct MemReadCost { double flop, bytes; };      // algorithmic FLOP and bytes of one read, as the profiler accounts them (km: the kernelized read)
MemReadCost memread_cost(int N, int Q, int k, int top_k, bool km);
// Scratch of a read of Q queries.  memread_scratch_floats(Q) is the one statement of its layout (memread.hip): the element counts of the five
// buffers, for every bank size, top_k and object count.  Whoever allocates a MemReadScratch sizes it from these and from nothing else.
struct MemReadScratch { float *cand_v; int32_t *cand_i; int32_t *cand_n; float *gmax; float *tau; };
struct MemReadScratchSizes { size_t cand_v, cand_i, cand_n, gmax, tau; };
MemReadScratchSizes memread_scratch_floats(int Q);
constexpr long MAX_FRAME_PIXELS = 1L << 24;      // padded frame nh * nw an engine or a stage context is created for: the per-frame launches size their grids in 32 bits
// largest disk radius r of the boundary measure (metrics.hip): disk_scan evaluates squares up to (r + 1)^2 in int, and 46340^2 =
// 2 147 395 600 <= INT_MAX = 2 147 483 647 < 46341^2 = 2 147 488 281.  The entry points that build boundary maps refuse a larger one.
constexpr int METRICS_MAX_RADIUS = 46339;
static_assert((long)(METRICS_MAX_RADIUS + 1) * (METRICS_MAX_RADIUS + 1) <= 0x7fffffffL && (long)(METRICS_MAX_RADIUS + 2) * (METRICS_MAX_RADIUS + 2) > 0x7fffffffL,
              "METRICS_MAX_RADIUS is the largest r with (r + 1)^2 <= INT_MAX");
constexpr long MEMREAD_MAX_ROWS = 1L << 24;      // bank rows of one read: the read kernels build their key descriptor as (unsigned)N * 256 bytes, which wraps there
constexpr int MEMREAD_MSQ_PAD = 64;     // readable floats behind the N values of msq: the read kernels fetch |mk|^2 in whole 64-row steps
// dynamic LDS above 64 KB has to be opted into once per (device, kernel function)
void allow_big_lds(const void *kernel, size_t lds);
#if defined(__HIPCC__)
// The one way the conv families and the memory read launch a kernel.  ev: {start, stop} event pair that the dispatch itself fills (profiling on), or null -
// then a plain launch: the engine is launch-bound and an unprofiled launch must ask the runtime for nothing more than that.
template <typename... KArgs, typename... Args>
static inline void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, hipEvent_t *ev, const Args &...args) {
    if (lds_bytes > 64 * 1024) allow_big_lds(reinterpret_cast<const void *>(kernel), lds_bytes);
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, s, ev[0], ev[1], 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
}
#endif
// The kernelized read (EvalMemoryReader(top_k, km), prop_net.py:92-99): a Gaussian of standard deviation `sigma` around the query each bank row
// matches best weights the affinity before the cut.  The Q queries are Q / (h16 * w16) whole frames of h16 x w16 positions; qsq: |qk|^2 of frame
// f at qsq + f * qsq_fs; centre: scratch of (Q / (h16 * w16)) * memread_centre_stride(N) int32; centre_idx (may be null): [frames][N], the
// best query of every row within each frame
struct MemReadKm { float sigma; int h16, w16; const float *qsq; long qsq_fs; int32_t *centre; int32_t *centre_idx; };
long memread_centre_stride(int N);
// One read, described once; its callers (the engine's read_decode, the test hook, the bench hook) fill the fields by name.
struct MemRead {
    const float *mk, *msq, *mv; long mv_os; int N;      // bank: mk [N,64], msq [N] (+ MEMREAD_MSQ_PAD readable floats), mv [k][N][512] with object stride mv_os
    const float *qk; int Q;                             // queries: qk [Q,64]
    int k, top_k;                                       // objects; rows per query, 1 .. MEMREAD_MAX_TOPK, N >= top_k
    float *readout; long ro_os; int32_t *topk_idx; float *topk_w;       // readout [k][Q][512] with object stride ro_os; topk_idx / topk_w optional [Q,top_k]
    const MemReadKm *km;                                // null: the plain read, the kernels it always ran
};
void memory_read_launch(const MemRead &r, const MemReadScratch &scr, hipStream_t s);
// fusion attention read: mk,qk [hw,64]; pos,neg [kk][16h*16w planes] -> attn [kk][2][nh*nw]; pooled: scratch of attention_nchp(2 kk) * h * w floats
struct AttnScratch { float *gmax, *part; };   // [256][hw], attention_part_floats(kk, hw) ([16][hw][19] up to 8 objects)
int attention_nchp(int nch);                          // channels 2 kk padded to the widths the pass kernel is instantiated for
size_t attention_part_floats(int kk, int hw);
// launch plan of the attention read of hw = h * w memory rows and as many queries: `steps` 64-row steps of the memory, `qblocks` workgroups of 64
// queries, each walking NCeff chunks of spc steps (the last chunk may be shorter, none is empty); NC: the chunk count asked for before rounding
// spc up (about 512 workgroups, at most 16 chunks - gmax holds 16 group maxima per chunk - and at most one per step)
struct AttnPlan { int steps, qblocks, NC, spc, NCeff; };
AttnPlan attention_plan(int hw);
// pos == nullptr: `pooled` already holds attention_pool_launch's output for this interaction
void attention_pool_launch(const float *pos, const float *neg, int kk, int h, int w, float *pooled, hipStream_t s);
void attention_read_launch(const float *mk, const float *msq, const float *qk, const float *pos,
                           const float *neg, int kk, int h, int w, float *pooled, float *amap,
                           float *attn, AttnScratch scr, hipStream_t s);
// fusion input [nh*nw,12] = (rgb, prev, curr, attn_pos, attn_neg, nc, nr, 0,0,0)
void pack_fusion_input_launch(const float *img4, const float *prev, const float *curr,
                              const float *attn2, float nc, float nr, long npix, float *out,
                              hipStream_t s);

// ---------------------------------------------------------------- J / F metric counts (interactions/metrics.py)
// gt, pred uint8 [T,H,W] (non-zero = object); bmap scratch [T*H*W]; counts [T][6] =
// (intersection, union, gt boundary px, pred boundary px, matched gt boundary px, matched pred boundary px)
void jf_counts_launch(const uint8_t *gt, const uint8_t *pred, int T, int H, int W, int radius, uint8_t *bmap,
                      int *counts, hipStream_t s);

// ---- the same for LABEL MAPS of k objects (0 = background, o in 1..k = object o; a label above k counts as background) ----
// counts [k][T_all][6]: per object the six integers jf_counts_launch gives for the binary masks (gt == o), (pred == o).  The boundary scratch
// holds per pixel the SET of objects the pixel is a boundary pixel of, one word for the gt map and one for the pred map, bit o - 1 = object o:
// bytes for k <= 8, 32-bit words above.  label_scratch_bytes is the one statement of its size.
size_t label_scratch_bytes(int k, int T, int H, int W);
// gt / pred / bsets / counts point at the first of the Tn frames to count; T_all = frames per object in counts (the object stride)
void label_counts_launch(const uint8_t *gt, const uint8_t *pred, int k, int Tn, int H, int W, int radius, void *bsets, int *counts, int T_all,
                         hipStream_t s);
// One annotation round scored on the device: gen = engine mask / GT on annotated frames, J or J&F counts, fp64 quality per frame, arg-min.
// k = 0: binary masks (flags = noobj [T_all], scratch = bmap, object_quality unused); k >= 1: label maps of k objects (flags = present
// [k][T_all], scratch = bsets): per-object quality [k][T_all], frame quality = mean over the objects present in the frame, ascending o.
// Pointers at the first of the Tn frames to recount; quality / arg-min over the T_all frames of the clip, t0 = index of that first frame.
void round_score_launch(const uint8_t *masks, int nh, int nw, int lh, int lw, const uint8_t *gt, const uint8_t *annotated, const uint8_t *flags, int k,
                        int Tn, int H, int W, int radius, double no_object, uint8_t *gen, void *scratch, int *counts, int T_all,
                        double *object_quality, double *quality, int *select, hipStream_t s, int t0, const uint8_t *annot = nullptr);
// A trial round of a binary session (stcn_metrics_trial): frames [t0, t1) composed - frame t0 + also counting as annotated, -1: none - and
// counted into span_gen / bmap / span_counts, then quality [T_all] from span_counts inside the span and the const base counts outside.
void trial_score_launch(const uint8_t *masks, int nh, int nw, int lh, int lw, const uint8_t *gt, const uint8_t *annotated, const uint8_t *noobj, int also,
                        int T_all, int H, int W, int t0, int t1, int radius, double no_object, const int *base, uint8_t *span_gen, uint8_t *bmap,
                        int *span_counts, double *quality, hipStream_t s);

// ---------------------------------------------------------------- the simulated user (robot.hip; robots/click_robot.py, bbox_robot.py)
// Masks uint8 [H,W], non-zero = object, H * W <= MAX_FRAME_PIXELS.  All three enqueue only; the number of launches depends on (H, W) and
// middle_only alone.  robot_scratch_bytes is the one statement of the click call's scratch size (pure host code).
size_t robot_scratch_bytes(int H, int W);
// record int32 [STCN_ROBOT_RECORD_INTS]; component: optional uint8 [H,W] OUT; middle_only: pred is not read; two_clicks: the iou < 0.1 branch
void robot_click_launch(const uint8_t *pred, const uint8_t *gt, int H, int W, int middle_only, int two_clicks, void *scratch, int *record,
                        uint8_t *component, hipStream_t s);
void robot_bbox_launch(const uint8_t *mask, int H, int W, int *record, hipStream_t s);                  // record int32 [STCN_ROBOT_BBOX_INTS]
void robot_best_mask_launch(const uint8_t *cand, const uint8_t *target, int M, int H, int W, int *out, hipStream_t s);      // out int32 [STCN_ROBOT_BEST_INTS]

// ---------------------------------------------------------------- masks as network input (resize.hip)
// src uint8 [T,H,W] -> out fp32 [n,channels,out_h,out_w]: nearest (torch's rule in fp32), the byte's value as a float, every channel the same
// plane.  frames: device int32 [n] or nullptr = frames 0..n-1; an index outside [0,T) is not read, its planes become NaN.  out_h * out_w <=
// MAX_FRAME_PIXELS, n <= 65535 (checked by the caller).  Enqueues one launch.
void masks_resize_nearest_launch(const uint8_t *src, int T, int H, int W, const int *frames, int n, int out_h, int out_w, int channels, float *out,
                                 hipStream_t s);

// ---------------------------------------------------------------- frames as stored images (rgb8.hip)
// clip fp32 [T,3,H,W] (4-byte aligned, finite) -> out uint8 [n,H,W,3]: per frame (x - min) / max(max - min, 1e-8f) * 255 in correctly rounded
// fp32, truncated.  frames: device int32 [n] or nullptr = frames 0..n-1; an index outside [0,T) is not read, its image becomes zeros.
// scratch: n * 8 bytes, 4-byte aligned, initialised by the call.  H * W <= MAX_FRAME_PIXELS, 1 <= n <= 65535 (checked by the caller).
// Enqueues three launches.
void frames_to_rgb8_launch(const float *clip, int T, int H, int W, const int *frames, int n, void *scratch, uint8_t *out, hipStream_t s);

// ---------------------------------------------------------------- a clip at a working resolution (rescale.hip)
// prob fp32 [k1,T,1,nh,nw] -> out uint8 [T,H,W], frames [t0,t1) only: the h x w window at (lh, lw) of every channel, bilinear
// (align_corners=False, torch's fp32 evaluation) to H x W, arg-max over the channels with the lowest index winning a tie.  Nothing outside the
// window is read, no other frame is written; out may start at any byte.  2 <= k1, the window inside the plane, H * W <= MAX_FRAME_PIXELS
// (checked by the caller).  Enqueues one launch per 65535 frames.
void prob_upsample_argmax_launch(const float *prob, int k1, int T, int nh, int nw, int lh, int lw, int h, int w, int H, int W, int t0, int t1,
                                 uint8_t *out, hipStream_t s);
// src fp32 [planes,H,W] -> dst fp32 [planes,h,w], h <= H, w <= W: antialiased bicubic (A = -0.5, align_corners=False), horizontal then vertical,
// fp64 sums rounded once.  The taps of (H -> h) and (W -> w) are built on the host and uploaded on first use, per device (a blocking copy, then
// cached for the life of the process): the error of that upload comes back.  Enqueues one launch per 65535 planes.
hipError_t frames_downsample_aa_launch(const float *src, int planes, int H, int W, int h, int w, float *dst, hipStream_t s);

// ---------------------------------------------------------------- frame distances (frame_select.hip)
// dist [T][T] fp64 = squared L2 distances between T vectors of K fp32 values, vector t at x + index.v[t] * stride (16-byte aligned: x and
// stride multiples of 4 floats, K % 4 == 0, K >= 4, 1 <= T <= FRAME_GRAM_MAX_T).  The Gram matrix is accumulated in fp64 on the matrix cores
// (v_mfma_f64_16x16x4_f64), K cut into plan.slices slices of plan.len values - a multiple of the k-step, slices * len >= K, no slice empty -
// whose partial 16 x 16 tiles [slices][pairs][16][16] go through `scratch` and are summed in slice order: symmetric, zero diagonal, the same
// bits on every run.  index travels as a kernel argument.
constexpr int FRAME_GRAM_MAX_T = 106;           // the frames of the key cache
constexpr int FRAME_GRAM_KSTEP = 32;            // k values a wave consumes per step
constexpr int FRAME_GRAM_MAX_SLICES = 512;      // two workgroups of four waves per compute unit
struct FrameIndex { int v[FRAME_GRAM_MAX_T]; };
struct FrameGramPlan { int slices; long len; int nt, pairs; };      // nt tiles of 16 frames, pairs = nt (nt + 1) / 2 tiles of the upper triangle
FrameGramPlan frame_gram_plan(int T, long K);                       // pure host code
size_t frame_gram_scratch_bytes(int T, long K);                     // from that plan and from nothing else: slices * pairs * 2048
void frame_gram_launch(const float *x, const FrameIndex &index, long stride, int T, long K, double *scratch, double *dist, hipStream_t s,
                       hipEvent_t *ev_gram = nullptr, hipEvent_t *ev_red = nullptr);

// pure fp32-MFMA load (no memory traffic): launches `grid` workgroups of 12 waves x iters x 12 MFMAs, returns the FLOP of the launch
double mfma_probe_launch(float *out, int grid, int iters, hipStream_t s);

}  // namespace stcn
