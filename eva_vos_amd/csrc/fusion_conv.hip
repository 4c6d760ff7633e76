// fusion_conv.hip - the 3x3 convolutions of FusionNet (reference mivos/model/fusion_net.py:12-30,38-48) on gfx950.
//
// Rounds >= 2 of an annotation session fuse every frame between two interacted frames (inference_core.py:184-207): five
// 3x3 convs with 32 output channels at FULL resolution (480x864: M = 414 720 rows, N = 32, K = 288 / 108) per fused frame and
// object - 33 GFLOP, a third of what the decoder of that frame costs.  As implicit GEMMs of the generic kernel (128x32 tiles, K
// tile 32: 9 barriers and 9 im2col re-stagings of the same pixels per tile) they ran far below the matrix rate.  Shape-specific
// structure instead:
//   * the WHOLE weight matrix lives in registers: the B operand of v_mfma_f32_32x32x2_f32 is one VGPR per MFMA, K = 288 means
//     144 VGPRs per lane hold every B fragment of the layer (loaded once per workgroup, 36 x 16 B per lane);
//   * the input patch of the workgroup (PH output rows x 32 columns + halo) is staged ONCE into LDS in full 128-byte pixel
//     lines (coalesced), pixel stride padded to CINP + 4 floats so that the A fragments (lane = pixel, lane half = 4-channel
//     group, one ds_read_b128 per 4 MFMAs, k-permuted exactly like the weights) are bank-conflict free; the nine taps are
//     nine shifted reads of the same patch: no im2col copy, one barrier per workgroup;
//   * a wave owns PH / 4 output rows of 32 pixels: 144 MFMAs per row back to back, nothing but ds_reads between them;
//   * persistent workgroups, the next patch's global loads in flight under the MFMAs of the current one;
//   * bias / residual / ReLU in the epilogue, 128-byte stores.
// CIN = 12 (conv1: 9 channels padded to 12 in HBM) runs as 16 channels per tap in LDS / registers (zero filled).
#include <hip/hip_ext.h>

#include "kernels.h"

namespace stcn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int CIN, int PH, bool RELU_OUT, bool HAS_RES>
__global__ __launch_bounds__(256, 2) void fusion_conv_kernel(const float *__restrict__ x, const float *__restrict__ w, int Kp,
                                                             const float *__restrict__ bias, const float *__restrict__ res,
                                                             float *__restrict__ y, int H, int W, int tiles_x, int n_patches) {
    constexpr int CINP = (CIN + 7) / 8 * 8, KB = CINP / 8, LP = CINP + 4;      // channels per tap in LDS, k-blocks, pixel stride
    constexpr int PW = 32, RB = PH / 4;                                       // patch columns, output rows per wave
    constexpr int CH = CIN / 4;                                               // 16-byte chunks per pixel in HBM
    extern __shared__ __attribute__((aligned(16))) float patch[];            // [2][(PH + 2)][(PW + 2)][LP]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;

    // PERSISTENT workgroups (two per CU): a workgroup walks the patches blockIdx.x, + gridDim.x, ...  The first version (one
    // workgroup per 8-row patch) staged, then computed, and lost the tail of its 3.2 rounds: 64 TFLOP/s, slower than the generic
    // kernel's 82.  Here the global loads of the NEXT patch are issued before the MFMAs of this one (registers), the weights are
    // loaded once per workgroup, and 4-row patches (3240 at 480x864) leave a tail of 6.3 -> 7 rounds instead of 3.2 -> 4:
    // 95 TFLOP/s on the 32 -> 32 layers (the MFMA loop alone, without any global access: 108 - the clock the chip holds).
    // staging: thread t moves the 16-byte part (t % CHP) of the pixels t / CHP + (256 / CHP) i of the patch.  Everything per
    // chunk (pixel row / column, validity, addresses) is recomputed per patch from two registers - hoisted out of the patch
    // loop it cost 30 VGPRs and spilled (the weights alone take 144).
    constexpr int CHP = CH > 4 ? 8 : 4, PPI = 256 / CHP;                       // lanes per pixel (power of two), pixels per pass
    constexpr int NPIX = (PH + 2) * (PW + 2), NIT = (NPIX + PPI - 1) / PPI;
    f32x4 st[NIT];
    int p0 = t / CHP;
    const int part = t % CHP;
    auto gload = [&](int pidx) {                                              // out-of-image pixels are zero (the conv's padding)
        const int by = pidx / tiles_x, bx = pidx - by * tiles_x;
        const int x0 = bx * PW, y0 = by * PH;
        asm volatile("" : "+v"(p0));                                          // keeps the per-chunk index math inside the loop
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int p = p0 + PPI * i;
            const int py = p / (PW + 2), px = p - py * (PW + 2);
            const int gy = y0 - 1 + py, gx = x0 - 1 + px;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (p < NPIX && part < CH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
                v = *reinterpret_cast<const f32x4 *>(x + ((long)gy * W + gx) * CIN + 4 * part);
            st[i] = v;
        }
    };
    constexpr int PBUF = NPIX * LP;                                           // floats per patch buffer
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int p = p0 + PPI * i;
            if (p < NPIX && part < CH) *reinterpret_cast<f32x4 *>(patch + buf * PBUF + p * LP + 4 * part) = st[i];
        }
    };
    int pidx = blockIdx.x;
    gload(pidx);
    // ---- the layer's weights -> registers: wr[tap][kb] = W[n = l31][tap * CIN + 8 kb + 4 h .. + 3] (zero beyond CIN)
    f32x4 wr[9][KB];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int c0 = 8 * kb + 4 * h;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c0 < CIN) v = *reinterpret_cast<const f32x4 *>(w + (long)l31 * Kp + tap * CIN + c0);
            wr[tap][kb] = v;
        }
    const float bv = bias[l31];
    if (CINP != CIN) {                                                        // the zero channels CIN .. CINP - 1 of every pixel (once)
        for (int p = t; p < 2 * NPIX; p += 256) *reinterpret_cast<f32x4 *>(patch + p * LP + CIN) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    sstore(0);
    const float *pa0 = patch + ((wave * RB) * (PW + 2) + l31) * LP + 4 * h;
    // Two patch buffers, ONE barrier per patch: the next patch's global loads are issued at the top, written to the other
    // buffer in the MIDDLE of this patch's MFMA stream (half a patch of matrix time after the loads: they have landed), and the
    // barrier at the top of the next iteration finds both the stores and every reader of the old buffer done.  (Single buffer:
    // barrier - compute - barrier - store, and the two co-resident workgroups of a CU, sharing the pipes fairly, arrive at those
    // phases together.)
    int buf = 0;
    for (; pidx < n_patches; pidx += gridDim.x, buf ^= 1) {
        __syncthreads();                                                      // patch `buf` is in LDS, nobody reads `buf ^ 1` any more
        const float *pa = pa0 + buf * PBUF;
        const int nxt = pidx + gridDim.x;
        if (nxt < n_patches) gload(nxt);                                              // lands while the MFMAs below run
        __builtin_amdgcn_sched_barrier(0);
        // ---- RB output rows of 32 pixels per wave; acc rows = pixels, columns = output channels
        f32x16 acc[RB];
#pragma unroll
        for (int b = 0; b < RB; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;
        // 9 taps x KB k-blocks = NG fragment groups of 4 MFMAs per row; the fragments of group g + 2 are requested before the
        // MFMAs of group g (three register sets, pinned: left alone hipcc issues each ds_read right in front of its first use
        // and every group pays the LDS latency: 0.61 of the matrix rate)
        constexpr int NG = 9 * KB;
        f32x4 fa[3][RB];
        auto fread = [&](int g2, f32x4 (&dst)[RB]) {
            const int tap = g2 / KB, kb = g2 - tap * KB, dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
            for (int b = 0; b < RB; ++b) dst[b] = *reinterpret_cast<const f32x4 *>(pa + ((b + dy) * (PW + 2) + dx) * LP + 8 * kb);
        };
        fread(0, fa[0]);
        fread(1, fa[1]);
#pragma unroll
        for (int g2 = 0; g2 < NG; ++g2) {
            if (g2 + 2 < NG) fread(g2 + 2, fa[(g2 + 2) % 3]);
            __builtin_amdgcn_sched_barrier(0);
            if (g2 == NG / 2 && nxt < n_patches) {
                sstore(buf ^ 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int tap = g2 / KB, kb = g2 - tap * KB;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < RB; ++b)
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g2 % 3][b][j], wr[tap][kb][j], acc[b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- epilogue: C/D layout column (channel) = lane & 31, row (pixel) = (r & 3) + 8 (r >> 2) + 4 h
        const int by = pidx / tiles_x, bx = pidx - by * tiles_x;
        const int x0 = bx * PW, y0 = by * PH;
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int oy = y0 + wave * RB + b;
            if (oy >= H) continue;
            const long rowo = ((long)oy * W + x0) * 32 + l31;
            float rv[16];                                                     // residual: all 16 loads in flight before the first use
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int px = min((r & 3) + 8 * (r >> 2) + 4 * h, W - 1 - x0);
                rv[r] = HAS_RES ? res[rowo + px * 32] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                rv[r] += acc[b][r] + bv;
                if (RELU_OUT) rv[r] = fmaxf(rv[r], 0.f);
                asm volatile("" : "+v"(rv[r]));                                 // pinned in front of the masked stores
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int px = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (x0 + px < W) y[rowo + px * 32] = rv[r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- 32 -> 32 as Winograd F(2x2,3x3)
// The direct kernel above runs at 0.8 of the matrix rate the chip holds: the only way down is fewer MFMAs.  F(2x2,3x3) needs 16
// multiplies per 2x2 outputs instead of 36 (exact-fp32 arithmetic: the transforms add, subtract and halve), and at 32 channels
// everything fits a workgroup:
//   * same persistent structure and patches (4 output rows x 32 columns = 2 x 16 tiles = ONE 32-row MFMA block, 6 x 34 input
//     pixels in LDS, the next patch's global loads in flight under the MFMAs);
//   * wave xi (of 4) owns the vertical transform index xi: its 4 positions (xi, nu) x 4 k-blocks of U live in 64 registers for
//     the whole launch; it builds its A fragments straight from the patch - row transform B^T needs just two input rows per xi
//     (d0 - d2, d1 + d2, d2 - d1, d1 - d3), the column transform four shifted pixels: 8 ds_read_b128 + 32 VALU per k-block, no V
//     array anywhere - and runs 64 MFMAs per patch (the direct kernel: 144);
//   * output transform: along nu in registers (u0 = m0 + m1 + m2, u1 = m1 - m2 - m3), along xi through a 32 KB LDS exchange
//     (the four waves hold the four xi): work item = (tile, output column, 4 channels), 16-byte reads / residual loads / stores.
// CIN = 12 (conv1: 9 channels padded to 12 in HBM): 16 channels per pixel in LDS (zero filled), two k-blocks, U built from the
// zero-padded weights.
template <int CIN, bool RELU_OUT, bool HAS_RES>
__global__ __launch_bounds__(256, 2) void fusion_wino_kernel(const float *__restrict__ x, const float *__restrict__ U,
                                                             const float *__restrict__ bias, const float *__restrict__ res,
                                                             float *__restrict__ y, int H, int W, int tiles_x, int n_patches) {
    constexpr int CINP = (CIN + 7) / 8 * 8, KB = CINP / 8, LP = CINP + 4, PH = 4, PW = 32;
    constexpr int NPIX = (PH + 2) * (PW + 2), PBUF = NPIX * LP;
    constexpr int CH = CIN / 4, CHP = CH > 4 ? 8 : 4, PPI = 256 / CHP, NIT = (NPIX + PPI - 1) / PPI;
    extern __shared__ __attribute__((aligned(16))) float patch[];            // [(PH + 2)][(PW + 2)][LP], then the exchange [4 xi][2 j][32 tiles][32 ch]
    float *ex = patch + PBUF;
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, h = lane >> 5;
    const int xi = __builtin_amdgcn_readfirstlane(t >> 6);

    f32x4 st[NIT];
    int p0 = t / CHP;
    const int part = t % CHP;
    auto gload = [&](int pidx) {                                              // out-of-image pixels are zero (the conv's padding)
        const int by = pidx / tiles_x, bx = pidx - by * tiles_x;
        const int x0 = bx * PW, y0 = by * PH;
        asm volatile("" : "+v"(p0));                                          // keeps the per-chunk index math inside the loop
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int p = p0 + PPI * i;
            const int py = p / (PW + 2), px = p - py * (PW + 2);
            const int gy = y0 - 1 + py, gx = x0 - 1 + px;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (p < NPIX && part < CH && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W)
                v = *reinterpret_cast<const f32x4 *>(x + ((long)gy * W + gx) * CIN + 4 * part);
            st[i] = v;
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int p = p0 + PPI * i;
            if (p < NPIX && part < CH) *reinterpret_cast<f32x4 *>(patch + p * LP + 4 * part) = st[i];
        }
    };
    int pidx = blockIdx.x;
    gload(pidx);
    if (CINP != CIN) {                                                        // the zero channels CIN .. CINP - 1 of every pixel (once)
        for (int p = t; p < NPIX; p += 256) *reinterpret_cast<f32x4 *>(patch + p * LP + CIN) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // ---- this wave's slice of U [16][KB][32][8] -> registers: ur[nu][kb] = U[pos = 4 xi + nu][kb][n = l31][4 h .. 4 h + 3]
    f32x4 ur[4][KB];
#pragma unroll
    for (int nu = 0; nu < 4; ++nu)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) ur[nu][kb] = *reinterpret_cast<const f32x4 *>(U + ((((4 * xi + nu) * KB + kb) * 32 + l31) << 3) + 4 * h);
    sstore();
    // lane = tile (ty, tx) of the patch; B^T row xi = d[ra] + sb d[rb]: (0, 2, -), (1, 2, +), (2, 1, -), (1, 3, -)
    const int ty = l31 >> 4, tx = l31 & 15;
    const int ra = xi == 0 ? 0 : (xi == 2 ? 2 : 1), rb = xi == 0 ? 2 : (xi == 1 ? 2 : (xi == 2 ? 1 : 3));
    const float sb = xi == 1 ? 1.f : -1.f;
    const float *pa = patch + ((2 * ty + ra) * (PW + 2) + 2 * tx) * LP + 4 * h;
    const float *pb = patch + ((2 * ty + rb) * (PW + 2) + 2 * tx) * LP + 4 * h;
    const int cq = t & 7, tile = (t >> 3) & 31;                               // combine: thread = (tile, 4 channels); column j = pass
    const int oty = tile >> 4, otx = tile & 15;
    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 4 * cq);
    for (; pidx < n_patches; pidx += gridDim.x) {
        __syncthreads();                                                      // the patch is in LDS, the exchange is free
        const int nxt = pidx + gridDim.x;
        if (nxt < n_patches) gload(nxt);                                      // lands while the MFMAs below run
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[4];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[nu][e] = 0.f;
        f32x4 da[4], db[4], v[4];
        auto dread = [&](int kb) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                da[c] = *reinterpret_cast<const f32x4 *>(pa + c * LP + 8 * kb);
                db[c] = *reinterpret_cast<const f32x4 *>(pb + c * LP + 8 * kb);
            }
        };
        auto vmake = [&]() {
            f32x4 tt[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) tt[c] = da[c] + db[c] * sb;
            v[0] = tt[0] - tt[2]; v[1] = tt[1] + tt[2]; v[2] = tt[2] - tt[1]; v[3] = tt[1] - tt[3];
        };
        dread(0);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            vmake();
            if (kb + 1 < KB) dread(kb + 1);                                   // the next k-block's pixels under this one's MFMAs
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int nu = 0; nu < 4; ++nu) acc[nu] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[nu][j], ur[nu][kb][j], acc[nu], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- residual block of the combine step: requested now, used after the barrier
        const int by = pidx / tiles_x, bx = pidx - by * tiles_x;
        const int x0 = bx * PW, y0 = by * PH;
        const int oy = y0 + 2 * oty, ox = x0 + 2 * otx;
        long po[2][2];
        f32x4 rv[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                po[j][i] = ((long)min(oy + i, H - 1) * W + min(ox + j, W - 1)) * 32 + 4 * cq;
                rv[j][i] = HAS_RES ? *reinterpret_cast<const f32x4 *>(res + po[j][i]) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        // ---- output transform along nu, then the exchange: ex[xi][j][tile row of the C layout][channel]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            ex[((xi * 2 + 0) * 32 + row) * 32 + l31] = acc[0][r] + acc[1][r] + acc[2][r];
            ex[((xi * 2 + 1) * 32 + row) * 32 + l31] = acc[1][r] - acc[2][r] - acc[3][r];
        }
        __syncthreads();                                                      // every wave is past its patch reads; the exchange is full
        if (nxt < n_patches) sstore();
        const f32x4 *ex4 = reinterpret_cast<const f32x4 *>(ex) + tile * 8 + cq;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 e0 = ex4[(0 * 2 + j) * 256], e1 = ex4[(1 * 2 + j) * 256], e2 = ex4[(2 * 2 + j) * 256], e3 = ex4[(3 * 2 + j) * 256];
            f32x4 o[2] = {e0 + e1 + e2, e1 - e2 - e3};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                o[i] += bv + rv[j][i];
                if (RELU_OUT) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[i][c] = fmaxf(o[i][c], 0.f);
                }
                asm volatile("" : "+v"(o[i]));                                 // pinned in front of the masked stores
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (oy + i < H && ox + j < W) *reinterpret_cast<f32x4 *>(y + po[j][i]) = o[i];
        }
    }
}

// conv1 (9 -> 12 channels in HBM, 16 per tap here: a quarter of its MFMAs multiply zeros) measured 53 us on this kernel, 49 us
// on the generic one: off by default (STCN_FUSION_CONV12=1 switches it on; the instance stays tested)
static bool fusion_conv_winograd(const ConvP &p) { return (p.Cin == 32 || p.Cin == 12) && p.wino_u && p.kn.fusion_wino; }

static bool fusion_conv_eligible(const ConvP &p) {
    constexpr bool on = true;
    return on && p.N == 32 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.B == 1 && !p.x1 && !p.relu_in &&
           (p.Cin == 32 || (p.Cin == 12 && (p.kn.fusion_conv12 || fusion_conv_winograd(p)))) &&
           p.K == 9 * p.Cin && (p.y_bs == 0) && (!p.res || !p.res_bmod) && p.bias;
}

bool fusion_conv_plan(const ConvP &p, ConvPlan &pl) {
    if (!fusion_conv_eligible(p)) return false;
    pl.family = CONV_FUSION;
    pl.fusion_wino = fusion_conv_winograd(p);
    pl.n_in = 0; pl.n_gemm = 1; pl.reduce = false;
    pl.fl_exec = pl.fusion_wino ? 2.0 * 16.0 * ((p.H + 3) / 4 * 2) * (double)((p.W + 31) / 32 * 16) * ((p.Cin + 7) / 8 * 8) * p.N : pl.fl;
    return true;
}

void fusion_conv_launch(const ConvP &p, const ConvPlan &pl, hipStream_t s, hipEvent_t *ev) {
    constexpr int PH = 4;
    const int tiles_x = (p.W + 31) / 32, tiles_y = (p.H + PH - 1) / PH, n_patches = tiles_x * tiles_y;
    const int resident = 2 * device_cus();            // two workgroups per CU (206 VGPRs: two waves per SIMD)
    const dim3 grid((unsigned)(n_patches < resident ? n_patches : resident));
    if (pl.fusion_wino) {
        const size_t ldsw = (size_t)((PH + 2) * 34 * ((p.Cin + 7) / 8 * 8 + 4) + 4 * 2 * 32 * 32) * sizeof(float);
#define STCN_FW(RL_, RS_) (p.Cin == 12 ? fusion_wino_kernel<12, RL_, RS_> : fusion_wino_kernel<32, RL_, RS_>)
        auto kfn = STCN_FW(false, false);
        switch ((p.relu_out ? 2 : 0) | (p.res ? 1 : 0)) {
            case 0: break;
            case 1: kfn = STCN_FW(false, true); break;
            case 2: kfn = STCN_FW(true, false); break;
            default: kfn = STCN_FW(true, true); break;
        }
#undef STCN_FW
        launch(kfn, grid, dim3(256), ldsw, s, ev, p.x0, p.wino_u, p.bias, p.res, p.y, p.H, p.W, tiles_x, n_patches);
        return;
    }
    const int cinp = (p.Cin + 7) / 8 * 8;
    const size_t lds = (size_t)2 * (PH + 2) * 34 * (cinp + 4) * sizeof(float);
#define STCN_FC(CIN_, RL_, RS_) kfn = fusion_conv_kernel<CIN_, PH, RL_, RS_>
    auto STCN_FC(32, false, false);
    const int key = (p.Cin == 12 ? 4 : 0) | (p.relu_out ? 2 : 0) | (p.res ? 1 : 0);
    switch (key) {
        case 0: break;
        case 1: STCN_FC(32, false, true); break;
        case 2: STCN_FC(32, true, false); break;
        case 3: STCN_FC(32, true, true); break;
        case 4: STCN_FC(12, false, false); break;
        case 5: STCN_FC(12, false, true); break;
        case 6: STCN_FC(12, true, false); break;
        default: STCN_FC(12, true, true); break;
    }
#undef STCN_FC
    launch(kfn, grid, dim3(256), lds, s, ev, p.x0, p.w, p.Kp, p.bias, p.res, p.y, p.H, p.W, tiles_x, n_patches);
}

}  // namespace stcn
