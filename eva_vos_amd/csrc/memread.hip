// memread.hip - space-time memory read of STCN on gfx950:
//   affinity S = (2 mk.qk - |mk|^2 - |qk|^2)/sqrt(64)          (reference prop_net.py:80-90)
//   per query column: top-K over the T*H*W memory rows, softmax over the K (prop_net.py:53-60); K = the model's top_k
//     (prop_net.py:141), 1 .. 50, 50 in the description below
//   readout = sum_j w_j * mv[idx_j]                             (prop_net.py:108-115)
// The reference materialises the dense [T*HW x HW] affinity and multiplies by the dense matrix; here S
// only ever lives in registers.  Exact two-pass selection:
//   pass 1 (affinity_pass<false>): S tiles on v_mfma_f32_16x16x4_f32 (A = memory keys as 16-B fragments
//     straight from global/L2, double-buffered in registers; B = the wave's 16 query keys, resident;
//     -|mk|^2/2 is the initial accumulator).  Every lane keeps running maxima over disjoint row groups
//     of its query column.  The 50th largest of a query's G >= 50 group maxima is a lower bound of its
//     true 50th largest score (they are 50 distinct elements), and a tight one (expected rank ~ 63 for
//     G = 128 groups): threshold_kernel computes it with a wave-wide radix select.
//   pass 2 (affinity_pass<true>): the same MFMA walk; a register-level pre-filter against the now GLOBAL
//     threshold makes candidates rare (~1.3 x 50 per query over the whole bank), they are appended to
//     per-(query, chunk) LDS lists with LDS atomics; an overflowing list is cut back to its best 50 by
//     the radix select (only adversarial orderings get there).
//   merge_readout: one wave per query merges the chunk lists, softmaxes the 50 with wavefront
//     reductions and gathers 50 value rows (2 KB each, NHWC bank) per object.
//   The column-constant -|qk|^2 term cancels in exp(v - v_max) and is dropped.
// top_k: a wave-uniform kernel argument K (1 .. TOPK = 50) of every kernel that depends on the cut - the selects compare counts with it,
//   the softmax and the gathers run over K lanes / rows.  A compile-time 50 beside it was measured and bought nothing (profiles/topk_default_ab.txt:
//   the read and the headline are the same within the repeats of one box), so there is ONE instantiation.  Every capacity is sized for 50 and
//   does not move: candidate lists keep a stride of 50, CAP2 = 64 stays above the cut, merge_readout stages MAXCHUNK2 * 50 entries, one lane
//   per selected row.  top_k = None of the reference (a dense softmax over the whole bank) is another kernel family and is not built.
// km (the kernelized read, EvalMemoryReader(top_k, km), prop_net.py:33-51,92-99): every memory row n takes the query it matches best in the
//   frame being read, (cy_n, cx_n), and its affinities to that frame are weighted by a Gaussian of standard deviation km around that
//   position BEFORE the cut: exp(S - max) * g.  In the log domain that is an additive bias on the score,
//     B[n,q] = S[n,q] - ((y_q - cy_n)^2 + (x_q - cx_n)^2) / (2 km^2),
//   and exp(S - max) * g is monotone in B: selection, near-tie re-score, softmax and gather are the plain read's, applied to B.
//   row_centre_kernel finds the centres (one more affinity walk, roles of keys and queries swapped, per frame of a decode group);
//   the KM instantiations of affinity_tile_kernel / merge_readout_kernel add the bias in the tile epilogue / to the fp64 re-score.
//   Without km the launch path runs the instantiations it always ran.
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "kernels.h"

namespace stcn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

// device side of the kernelized read: centre [frames][cstride] holds (cy << 16 | cx) of every bank row for every frame of the queries,
// frame f owning the queries [f * hw16, (f + 1) * hw16); inv2s = 1 / (2 km^2)
struct KmArgs { const int32_t *centre; long cstride; int hw16, w16; float inv2s; };
// squared distance of the packed positions a, b = (x, y) as 16-bit halves: one packed subtract, one dot product
__device__ __forceinline__ int km_dist2(s16x2 a, int b) {
    const s16x2 d = a - __builtin_bit_cast(s16x2, b);
    return __builtin_amdgcn_sdot2(d, d, 0, false);
}

static constexpr int TOPK = MEMREAD_MAX_TOPK;   // the largest cut, the default model's, and the stride of every candidate list
static constexpr int CAP = 128;       // per-(query, chunk) candidate list capacity (>= TOPK + 64)
static constexpr int TROWS = 128;     // memory rows per tile of the attention read
static constexpr int HROWS = 64;      // rows per step of the top-k passes
static constexpr int SLD = 132;       // attention-read S slab row stride (floats)
static constexpr int MAXCHUNK = 16;   // row chunks (grid.y) of the attention read
static constexpr int NGRP = 16;       // attention read: running maxima per lane-group: 4 lane groups x 4 row blocks
static constexpr int MAXCHUNK1 = 8;   // row chunks of pass 1 of the top-k read (64 maxima each: threshold_kernel takes <= 512)
static constexpr int MAXCHUNK2 = 32;  // row chunks of pass 2 (merge_readout stages MAXCHUNK2 * 50 entries per query)
static constexpr float RESCORE_W = 1e-4f;   // half-width of the fp32-score window around the cut that merge_readout_kernel re-scores in fp64

__device__ __forceinline__ unsigned f2key(float f) {          // order-preserving float -> uint
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) {
    return __popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Keep the best K of the n (K <= n <= 128) entries of a wave-owned list (values lv, payload li): bitwise
// radix select on order-preserving keys (ballot + popcount per bit), ties by list position.
// Returns the K-th best value; the list is compacted to exactly K entries.
__device__ __forceinline__ float wave_select128(float *lv, int *li, int n, int lane, const int K) {
    lds_fence();
    const float f0 = lane < n ? lv[lane] : 0.f, f1 = lane + 64 < n ? lv[lane + 64] : 0.f;
    const int i0 = lane < n ? li[lane] : 0, i1 = lane + 64 < n ? li[lane + 64] : 0;
    const unsigned k0 = lane < n ? f2key(f0) : 0u, k1 = lane + 64 < n ? f2key(f1) : 0u;   // key 0 < every real key
    unsigned prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        const int c = __popcll(__ballot(k0 >= cand)) + __popcll(__ballot(k1 >= cand));
        if (c >= K) prefix = cand;
    }
    const unsigned long long g0 = __ballot(k0 > prefix), g1 = __ballot(k1 > prefix);
    const unsigned long long e0 = __ballot(k0 == prefix), e1 = __ballot(k1 == prefix);
    const int need = K - (__popcll(g0) + __popcll(g1));                 // >= 1 ties to keep
    const bool keep0 = (k0 > prefix) || (k0 == prefix && lanes_below(e0, lane) < need);
    const bool keep1 = (k1 > prefix) || (k1 == prefix && __popcll(e0) + lanes_below(e1, lane) < need);
    const unsigned long long b0 = __ballot(keep0), b1 = __ballot(keep1);
    lds_fence();
    if (keep0) { const int p = lanes_below(b0, lane); lv[p] = f0; li[p] = i0; }
    if (keep1) { const int p = __popcll(b0) + lanes_below(b1, lane); lv[p] = f1; li[p] = i1; }
    lds_fence();
    return key2f(prefix);
}

// A fragments of one 64-row step: a[rb][kb] = mk[row0 + 16 rb + (lane&15)][16 kb + 4 (lane>>4) .. +3]
// (k-permuted like the conv kernel) and the accumulator init -|mk|^2/2 for this lane's C rows.
struct HalfFrag { f32x4 a[4][4]; f32x4 c[4]; };
__device__ __forceinline__ void load_half(const float *__restrict__ mk, const float *__restrict__ msq, int N,
                                          int row0, int lane, HalfFrag &h) {
    const int g = lane >> 4, col = lane & 15;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        int r = row0 + rb * 16 + col;
        r = r < N ? r : N - 1;
        const float *ap = mk + (long)r * 64 + 4 * g;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) h.a[rb][kb] = *reinterpret_cast<const f32x4 *>(ap + 16 * kb);
        // C layout 16x16: col = lane&15, row = 4*(lane>>4) + reg.  msq is padded by >= 64 readable floats.
        h.c[rb] = *reinterpret_cast<const f32x4 *>(msq + row0 + rb * 16 + 4 * g);
    }
}
// acc[rb][j] = (mk[row] . qk[col] - msq[row]/2) / 4 with row = row0 + 16 rb + 4 (lane>>4) + j, col = lane&15
__device__ __forceinline__ void mfma_half(const HalfFrag &h, const f32x4 (&bq)[4], f32x4 (&acc)[4]) {
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) acc[rb] = h.c[rb] * -0.5f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(h.a[rb][kb].x, bq[kb].x, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(h.a[rb][kb].y, bq[kb].y, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(h.a[rb][kb].z, bq[kb].z, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(h.a[rb][kb].w, bq[kb].w, acc[rb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) acc[rb] = acc[rb] * 0.25f;
}

__device__ __forceinline__ void load_bq(const float *__restrict__ qk, int Q, int q0, int lane, f32x4 (&bq)[4]) {
    int q = q0 + (lane & 15);
    q = q < Q ? q : Q - 1;
    const float *bp = qk + (long)q * 64 + 4 * (lane >> 4);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) bq[kb] = *reinterpret_cast<const f32x4 *>(bp + 16 * kb);
}

// ------------------------------------------------------------------------------------------------
// Tile kernel of the top-50 read (both passes).  One workgroup = 4 waves = 64 queries (16 per wave, resident in
// registers as MFMA B fragments) x one chunk of 64-row steps of the bank.  The 64x64 key tile of a step (+ its 64 |mk|^2)
// is staged ONCE per workgroup: global -> registers (issued a whole step ahead) -> LDS (double-buffered, 16-byte chunks
// XOR-swizzled by the row so both the ds_write_b128 of the staging and the ds_read_b128 of the A fragments are
// conflict-free) and shared by the 4 waves - the first version of this read fetched the tile once per wave
// straight from L2 and ran at ~0.4 of the fp32 MFMA rate on L2 bandwidth.
//   COLLECT == false (pass 1): visits only every `ss`-th step (a strided SAMPLE of the bank) and keeps 16 running maxima
//     per lane over disjoint row sets: gmax[q][chunk*64 + 16*(lane>>4) + 4*rb + j].  The 50th largest of >= 50 maxima of
//     disjoint subsets of the rows is a lower bound of the query's true 50th best score whatever the subsets are, so
//     sampling costs tightness (expected rank ~ 52*ss instead of ~ 52), never exactness - and 1/ss of the MFMA work.
//   COLLECT == true (pass 2): the full walk; scores above the query's threshold are appended to per-(query, chunk) lists
//     in LDS (LDS atomics); a list that could overflow within the next 32 rows is cut back to its best 50 by the wave
//     radix select, which also raises that query's threshold (only adversarial orderings get there).
static constexpr int CAP2 = 64;                                         // list capacity (any value in (TOPK, 128] works, see below)
static constexpr int KT_FLOATS = HROWS * 64 + HROWS;                    // key tile + (-|mk|^2 / 2) of one step
static constexpr int LISTS_PER_WAVE = 2 * 16 * CAP2 + 32;               // LV, LI, CNT, TAU
static constexpr int NGRP2 = 64;                                        // pass-1 maxima per query per chunk

//   K: the cut of pass 2 (1 .. TOPK, wave-uniform).  Pass 1 does not depend on it.
//   KM: both passes work on the biased score B = S - d^2 / (2 km^2) (in the kernel's units: U - 4 d^2 / (2 km^2)), d = distance of the lane's
//     query position from the row's centre in the query's frame.  The lane's packed position and frame are resident; a step's 16 centres per
//     lane (4 loads of 16 bytes, the same address for the 16 lanes of a lane group within one frame) are requested with the step's first
//     fragments and used in the epilogue: subtract, dot product, convert, fma per score - nothing in the MFMA loop.  Both passes evaluate the
//     same expression on the same accumulator, so pass 1's bound holds for what pass 2 sees.
template <bool COLLECT, bool SINGLE = false, bool KM = false>
__global__ __launch_bounds__(256, SINGLE ? 3 : 2) void affinity_tile_kernel(
    const float *__restrict__ mk, const float *__restrict__ msq, const float *__restrict__ qk, int N, int Q, int ns,
    int ss, int spc, float *__restrict__ gmax, const float *__restrict__ tau_in, float *__restrict__ cand_v,
    int32_t *__restrict__ cand_i, int32_t *__restrict__ cand_n, const int K, const KmArgs km) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int NBUF = SINGLE ? 1 : 2;                                // SINGLE: one key tile buffer, two barriers per step, 3 workgroups per CU
    float *KT = smem;                                                   // [NBUF][KT_FLOATS]
    float *LV = smem + NBUF * KT_FLOATS + wave * LISTS_PER_WAVE;        // [16][CAP2]      (pass 2 only)
    int *LI = reinterpret_cast<int *>(LV + 16 * CAP2);                  // [16][CAP2]
    int *CNT = LI + 16 * CAP2;                                          // [16]
    float *TAU = reinterpret_cast<float *>(CNT + 16);                   // [16]

    const int q0 = (blockIdx.x * 4 + wave) * 16;                        // may be >= Q: the wave still stages tiles
    const int chunk = blockIdx.y;
    const int j0 = chunk * spc, j1 = min(ns, j0 + spc);                 // (sampled) steps of this chunk
    const int g = lane >> 4, col = lane & 15;
    const int qcol = min(q0 + col, Q - 1);

    f32x4 bq[4];
    load_bq(qk, Q, min(q0, Q - 1), lane, bq);
    s16x2 pq = {0, 0};                                                  // KM: the lane's query position (x, y) in its frame
    const int32_t *cl = nullptr;                                        // KM: centres of the lane's frame, at the lane's first C row
    float nkb = 0.f;
    if constexpr (KM) {
        const int fq = qcol / km.hw16, p = qcol - fq * km.hw16, y = p / km.w16;
        pq = s16x2{(short)(p - y * km.w16), (short)y};
        cl = km.centre + (long)fq * km.cstride + 4 * g;
        nkb = -4.f * km.inv2s;
    }
    // the kernel works on U = mk.qk - |mk|^2/2 = 4 S (S = the reference's affinity up to the per-query constant): maxima
    // and thresholds are compared unscaled, a score is multiplied by 1/4 (exact) when it leaves the kernel
    float tcol = -__builtin_inff();
    f32x4 gm[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) gm[rb] = f32x4{tcol, tcol, tcol, tcol};
    if (COLLECT) {
        tcol = 4.f * tau_in[qcol];
        if (lane < 16) { CNT[lane] = 0; TAU[lane] = tcol; }
        lds_fence();
    }

    // Staging: thread t moves the 16-byte chunks t, t+256, t+512, t+768 of the 64x16-chunk tile.  Buffer loads: rows beyond
    // the bank read as zero in hardware (no clamping), the step's row offset is one scalar.  Every per-thread offset below
    // is loop-invariant: the fp32 MFMA shares issue with VALU work, so the step loop carries ~5 address VALU ops in all
    // (first version: 2.4 - 3.7 VALU per MFMA, 0.44 of the MFMA rate).
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(mk), 0, (unsigned)N * 256u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(msq), 0, (unsigned)N * 4u, 0x00020000);
    const unsigned voff_k = (unsigned)((t >> 4) * 256 + (t & 15) * 16), voff_m = (unsigned)((t & 63) * 4);
    const int st_off = (t >> 4) * 64 + (((t & 15) ^ ((t >> 4) & 15)) << 2);     // floats; chunk i adds 16 rows = 1024 floats
    int a_off[4];                                                               // A fragment of k block kb; row block rb adds 1024
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) a_off[kb] = col * 64 + (((g | (kb << 2)) ^ col) << 2);
    const int m_off = HROWS * 64 + 4 * g;                                       // accumulator init; row block rb adds 16
    const int l_off = col * CAP2;
    f32x4 st[4];
    float stm = 0.f;
    auto gload = [&](int h) {                                                   // step h (may lie beyond the bank: zeros)
        const unsigned vk = voff_k + (unsigned)h * (HROWS * 256u), vm = voff_m + (unsigned)h * (HROWS * 4u);
#pragma unroll
        for (int i = 0; i < 4; ++i)      // the chunk offset rides in the VECTOR offset: only that one is range-checked by the hardware
            st[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, vk + i * 4096u, 0, 0));
        stm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, vm, 0, 0));
    };
    auto sstore = [&](float *kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4 *>(kt + st_off + i * 1024) = st[i];
        if (t < HROWS) kt[HROWS * 64 + t] = -0.5f * stm;                        // the accumulators start from -|mk|^2 / 2
    };
    if (j0 < j1) {
        gload(j0 * ss);
        sstore(KT);
        gload((j0 + 1) * ss);
    }
    __syncthreads();

    auto step = [&](const int j, auto bufc) {
        constexpr int BUF = SINGLE ? 0 : decltype(bufc)::value;
        const float *kt = KT + BUF * KT_FLOATS;
        const int row0 = j * ss * HROWS;
        // ---- U tile: acc[rb][e] = mk[row] . qk[q] - |mk[row]|^2 / 2, row = row0 + 16 rb + 4 g + e, q = q0 + col
        // first fragments right behind the barrier; their LDS latency hides behind the staging work below
        f32x4 acc[4], fa[2][4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            fa[0][rb] = *reinterpret_cast<const f32x4 *>(kt + a_off[0] + rb * 1024);
            acc[rb] = *reinterpret_cast<const f32x4 *>(kt + m_off + rb * 16);
        }
        i32x4 cen[4];
        if constexpr (KM) {                                              // rows up to the end of the last step are inside the (padded) centre rows
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) cen[rb] = *reinterpret_cast<const i32x4 *>(cl + row0 + rb * 16);
        }
        __builtin_amdgcn_sched_barrier(0);
        // tile j+1 (loaded a step ago) -> the buffer whose readers finished before the previous barrier; tile j+2 -> registers
        // (unconditional: past the chunk they move zeros / an unused tile)
        if (!SINGLE) {
            sstore(KT + (BUF ^ 1) * KT_FLOATS);
            gload((j + 2) * ss);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int cur = kb & 1;
            if (kb < 3) {                                                // next fragments in flight under this block's 16 MFMAs
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    fa[cur ^ 1][rb] = *reinterpret_cast<const f32x4 *>(kt + a_off[kb + 1] + rb * 1024);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[cur][rb][e], bq[kb][e], acc[rb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (KM) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[rb][e] = __builtin_fmaf(nkb, (float)km_dist2(pq, cen[rb][e]), acc[rb][e]);
        }
        if (row0 + HROWS > N) {                                          // ragged last step: rows beyond the bank never win
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row0 + rb * 16 + 4 * g + e >= N) acc[rb][e] = -__builtin_inff();
        }
        if (!COLLECT) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int e = 0; e < 4; ++e) gm[rb][e] = fmaxf(gm[rb][e], acc[rb][e]);
        } else {
            // Optimistic appends, one accumulator register at a time and only where some lane of the wave passes its
            // threshold (a compare + a scalar branch otherwise): take a list position with an LDS atomic, store if it is
            // inside the list.  An append that finds its list full is remembered in `drop` and replayed after the list has
            // been cut back to its best K (which also raises that query's threshold): no overflow check on the way.
            unsigned drop = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = acc[i >> 2][i & 3];
                const bool h = v > tcol;
                if (__ballot(h)) {
                    if (h) {
                        const int p = atomicAdd(&CNT[col], 1);
                        if (p < CAP2) {
                            LV[l_off + p] = v;
                            LI[l_off + p] = row0 + (i >> 2) * 16 + 4 * g + (i & 3);
                        } else {
                            drop |= 1u << i;
                        }
                    }
                }
            }
            while (__ballot(drop != 0)) {                                // rare: adversarial orderings, massive ties
                const unsigned long long dl = __ballot(drop != 0);
                unsigned fq = (unsigned)((dl | (dl >> 16) | (dl >> 32) | (dl >> 48)) & 0xffffull);
                lds_fence();
                while (fq) {                                             // a list with drops holds exactly CAP2 entries
                    const int jj = __builtin_ctz(fq);
                    fq &= fq - 1;
                    const float tt = wave_select128(LV + jj * CAP2, LI + jj * CAP2, CAP2, lane, K);
                    if (lane == 0) { CNT[jj] = K; TAU[jj] = fmaxf(TAU[jj], tt); }
                    lds_fence();
                }
                tcol = TAU[col];
                unsigned again = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (((drop >> i) & 1u) && acc[i >> 2][i & 3] > tcol) {
                        const int p = atomicAdd(&CNT[col], 1);
                        if (p < CAP2) {
                            LV[l_off + p] = acc[i >> 2][i & 3];
                            LI[l_off + p] = row0 + (i >> 2) * 16 + 4 * g + (i & 3);
                        } else {
                            again |= 1u << i;
                        }
                    }
                drop = again;
            }
        }
        __syncthreads();
        if (SINGLE) {                                                    // every wave is done with the tile: overwrite it
            sstore(KT);
            gload((j + 2) * ss);
            __syncthreads();
        }
    };
    {
        using B0 = std::integral_constant<int, 0>;
        using B1 = std::integral_constant<int, 1>;
        int j = j0;
        for (; j + 1 < j1; j += 2) {
            step(j, B0{});
            step(j + 1, B1{});
        }
        if (j < j1) step(j, B0{});
    }
    if (q0 >= Q) return;
    if (!COLLECT) {
        // query-major [q][nc1 * 64]: threshold_kernel then reads one query's maxima as contiguous 256-byte runs (the first layout,
        // [group][q], cost it 64 cache lines per load: 32 us for a 5 us job at 8100 queries)
        if (q0 + col < Q) {
            float *dst = gmax + (long)(q0 + col) * ((long)gridDim.y * NGRP2) + chunk * NGRP2 + 16 * g;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) *reinterpret_cast<f32x4 *>(dst + 4 * rb) = gm[rb] * 0.25f;
        }
        return;
    }
    // chunk winners -> global: cand_n[chunk][q] (<= K) entries of cand_v / cand_i[chunk][q][TOPK]
    lds_fence();
    for (int jj = 0; jj < 16; ++jj) {
        float *lv = LV + jj * CAP2;
        int *li = LI + jj * CAP2;
        int cnt = __builtin_amdgcn_readfirstlane(CNT[jj]);
        if (cnt > K) { wave_select128(lv, li, cnt, lane, K); cnt = K; }
        lds_fence();
        const int q = q0 + jj;
        if (q < Q) {
            const long o = ((long)chunk * Q + q) * TOPK + lane;
            if (lane < cnt) { cand_v[o] = 0.25f * lv[lane]; cand_i[o] = li[lane]; }
            if (lane == 0) cand_n[(long)chunk * Q + q] = cnt;
        }
    }
}

// pass 1 of the fusion attention read (exact column maxima need every row): one wave = 16 queries, fragments straight
// from global/L2 (T = 1 memory: 1620 rows, a few microseconds)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void colmax_pass_kernel(
    const float *__restrict__ mk, const float *__restrict__ msq, const float *__restrict__ qk, int N, int Q,
    int steps_per_chunk, float *__restrict__ gmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = (blockIdx.x * WAVES + wave) * 16;
    if (q0 >= Q) return;
    const int chunk = blockIdx.y;
    const int nsteps = (N + HROWS - 1) / HROWS;
    const int h0 = chunk * steps_per_chunk;
    const int h1 = min(nsteps, h0 + steps_per_chunk);
    const int g = lane >> 4, col = lane & 15;
    f32x4 bq[4];
    load_bq(qk, Q, q0, lane, bq);
    const float ninf = -__builtin_inff();
    f32x4 gm = {ninf, ninf, ninf, ninf};
    for (int h = h0; h < h1; ++h) {
        const int row0 = h * HROWS;
        HalfFrag cur;
        load_half(mk, msq, N, row0, lane, cur);
        f32x4 acc[4];
        mfma_half(cur, bq, acc);
        const bool tail = row0 + HROWS > N;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = (tail && row0 + rb * 16 + 4 * g + j >= N) ? ninf : acc[rb][j];
                gm[rb] = fmaxf(gm[rb], v);
            }
    }
    if (q0 + col < Q) {
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) gmax[((long)chunk * NGRP + 4 * g + rb) * Q + q0 + col] = gm[rb];
    }
}

// Centres of the kernelized read: centre[f][n] = the query of frame f that bank row n matches best,
//   argmax over the frame's hw16 queries q of (mk[n] . qk[q] - |qk[q]|^2 / 2)
// (prop_net.py:94: affinity.max(2)[1]; the row-constant -|mk[n]|^2 drops out, the -|qk|^2 term does not: this argmax runs along a row), ties to
// the lowest query.  The tile walk of colmax_pass_kernel with the roles swapped: a wave keeps 16 * NB bank rows resident as B fragments and walks
// the frame's queries in 64-row steps as A fragments straight from global / L2, -|qk|^2 / 2 as the initial accumulator; every lane keeps a running
// (max, query) over the queries of its C rows - visited in rising order, so a strict compare keeps the lowest - and the four lane groups of a
// column combine at the end.  Written as (cy << 16 | cx) for the bias of the passes, and as the query index when centre_idx is given (tests).
template <int WAVES, int NB>
__global__ __launch_bounds__(64 * WAVES) void row_centre_kernel(
    const float *__restrict__ mk, int N, const float *__restrict__ qk, const float *__restrict__ qsq, long qsq_fs, int hw16, int w16,
    int32_t *__restrict__ centre, long cstride, int32_t *__restrict__ centre_idx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * WAVES + wave) * 16 * NB;
    if (n0 >= N) return;
    const int f = blockIdx.y;
    const float *qf = qk + (long)f * hw16 * 64, *sf = qsq + (long)f * qsq_fs;
    const int g = lane >> 4, col = lane & 15;
    f32x4 bm[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b) load_bq(mk, N, min(n0 + 16 * b, N - 1), lane, bm[b]);
    float best[NB];
    int bi[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { best[b] = -__builtin_inff(); bi[b] = 0; }
    for (int row0 = 0; row0 < hw16; row0 += HROWS) {
        HalfFrag cur;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            const float *ap = qf + (long)min(row0 + rb * 16 + col, hw16 - 1) * 64 + 4 * g;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) cur.a[rb][kb] = *reinterpret_cast<const f32x4 *>(ap + 16 * kb);
#pragma unroll
            for (int j = 0; j < 4; ++j) cur.c[rb][j] = sf[min(row0 + rb * 16 + 4 * g + j, hw16 - 1)];
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f32x4 acc[4];
            mfma_half(cur, bm[b], acc);                                  // (qk[q] . mk[n] - |qk[q]|^2 / 2) / 4, q = row0 + 16 rb + 4 g + j, n = n0 + 16 b + col
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = row0 + rb * 16 + 4 * g + j;
                    const bool take = q < hw16 && acc[rb][j] > best[b];
                    best[b] = take ? acc[rb][j] : best[b];
                    bi[b] = take ? q : bi[b];
                }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(best[b], o);
            const int oi = __shfl_xor(bi[b], o);
            const bool take = ov > best[b] || (ov == best[b] && oi < bi[b]);
            best[b] = take ? ov : best[b];
            bi[b] = take ? oi : bi[b];
        }
        const int n = n0 + 16 * b + col;
        if (g == 0 && n < N) {
            const int cy = bi[b] / w16;
            centre[(long)f * cstride + n] = (cy << 16) | (bi[b] - cy * w16);
            if (centre_idx) centre_idx[(long)f * N + n] = bi[b];
        }
    }
}

// tau[q] = K-th largest of the G group maxima of query q (-inf when fewer than K are finite); G <= 512
__global__ __launch_bounds__(256) void threshold_kernel(const float *__restrict__ gmax, int G, int Q,
                                                        float *__restrict__ tau, const int K) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    unsigned k[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int gi = lane + 64 * e;
        const float v = gi < G ? gmax[(long)q * G + gi] : -__builtin_inff();
        k[e] = v > -__builtin_inff() ? f2key(v) : 0u;
    }
    unsigned prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        int c = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) c += __popcll(__ballot(k[e] >= cand));
        if (c >= K) prefix = cand;
    }
    // prefix == 0: fewer than K finite maxima -> no usable bound.  The bound must stay BELOW the
    // K-th best (the filter keeps v > tau): step one key down.
    // ... and lowered by the re-score window: a row whose fp32 score lies a few ulps BELOW the K-th may beat it in exact arithmetic;
    // it has to reach the merge kernel's candidate list to be re-scored (merge_readout_kernel: RESCORE_W)
    if (lane == 0) tau[q] = prefix == 0u ? -__builtin_inff() : key2f(prefix - 1u) - 1.5f * RESCORE_W;
}

// one wave per query: merge the chunk lists (cand_n[c][q] entries each; cand_n == nullptr: K each, -inf = missing),
// softmax, sparse readout.  K = top_k; the lists keep their stride of TOPK, topk_idx / topk_w are [Q][K]
// Near-tie re-score (round 5): two fp32 implementations of the affinity differ by ~1e-5 (64-term dot products of |S| ~ 100: one ulp is
// 7.6e-6), so a query whose 50th and 51st scores lie closer than that gets another row set from every implementation - the reference's
// own thread counts included.  With `mk` / `qk` given, the candidates whose fp32 score lies within RESCORE_W of the
// provisional cut are scored again in fp64 from the key rows themselves (a handful of 256-byte rows for ~4 % of the queries) and the
// cut is taken in that order: the selection is then the top-50 of the EXACT scores wherever fp32 could not tell, i.e. one error source
// (ours) less in the comparison with any other implementation.  Softmax weights keep the fp32 scores (prop_net.py:53-60 in fp32).
// Scope of "exact" (advisor, round 5): every (chunk, query) list reaches this kernel cut to its best TOPK by fp32 score (chunk write-out of
// affinity_tile_kernel, and the rare overflow cut-back inside pass 2).  A row a few ulps below ITS CHUNK's 50th therefore never gets here; that
// only matters when one chunk alone holds >= 50 candidates at or above the global cut - a single-chunk read (small banks), or a top-50
// concentrated in one chunk.  There the selection is a valid fp32 top-50 and the re-score changes nothing; wherever the near-tie candidates
// survive the per-chunk cut (the usual case: the engine's reads span several chunks and the top-50 several frames) it is the exact order.
__device__ __forceinline__ double shfl_f64(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl((int)(b & 0xffffffffll), src), hi = __shfl((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// KM: the candidates carry biased scores; the fp64 re-score adds the same bias (the row's centre in the query's frame) to the exact affinity
template <bool KM = false>
__global__ __launch_bounds__(256) void merge_readout_kernel(const float *__restrict__ cand_v,
                                                            const int32_t *__restrict__ cand_i,
                                                            const int32_t *__restrict__ cand_n, int NC, int Q,
                                                            const float *__restrict__ mv, long mv_os, int k,
                                                            float *__restrict__ readout, long ro_os,
                                                            int32_t *__restrict__ topk_idx, float *__restrict__ topk_w,
                                                            const float *__restrict__ mk, const float *__restrict__ qk, const int K,
                                                            const KmArgs km) {
    __shared__ float s_v[4][MAXCHUNK2 * TOPK];
    __shared__ int s_i[4][MAXCHUNK2 * TOPK];
    __shared__ float s_w[4][64];
    __shared__ int s_x[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= Q) return;
    float *sv = s_v[wave];
    int *si = s_i[wave];
    // list sizes -> offsets (lane c owns chunk c; NC <= 64), then all entries with independent loads
    int nl = lane < NC ? (cand_n ? cand_n[(long)lane * Q + q] : K) : 0;
    int ol = nl;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(ol, o); if (lane >= o) ol += u; }
    const int n = __shfl(ol, 63);
    ol -= nl;
    for (int c = 0; c < NC; ++c) {
        const int nc = __shfl(nl, c), oc = __shfl(ol, c);
        if (lane < nc) {
            const long o = ((long)c * Q + q) * TOPK + lane;
            sv[oc + lane] = cand_v[o];
            si[oc + lane] = cand_i[o];
        }
    }
    lds_fence();
    // bitwise radix select of the K-th largest key over n entries
    unsigned prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = prefix | (1u << bit);
        int c = 0;
        for (int e = lane; e < n; e += 64) c += f2key(sv[e]) >= cand ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (c >= K) prefix = cand;
    }
    // compact winners (ties: first in list order) into s_w / s_x
    int base = 0;
    bool rescored = false;
    if (mk) {
        // window around the provisional cut: entries above it are in, entries below it are out, the `nnear` inside are ranked exactly
        const float cut = key2f(prefix), hi = cut + RESCORE_W, lo = cut - RESCORE_W;
        int nab = 0, nnear = 0;
        for (int e = lane; e < n; e += 64) { const float v = sv[e]; nab += v > hi ? 1 : 0; nnear += (v <= hi && v >= lo) ? 1 : 0; }
        for (int o = 32; o > 0; o >>= 1) { nab += __shfl_xor(nab, o); nnear += __shfl_xor(nnear, o); }
        if (nnear > 1 && nnear <= 64) {
            rescored = true;
            // positions of the near entries -> s_x[0 .. nnear) (read back into registers before the winners overwrite s_x)
            int nb = 0;
            for (int e0 = 0; e0 < n; e0 += 64) {
                const int e = e0 + lane;
                const float v = e < n ? sv[e] : 0.f;
                const unsigned long long mb = __ballot(e < n && v <= hi && v >= lo);
                if (e < n && v <= hi && v >= lo) s_x[wave][nb + lanes_below(mb, lane)] = e;
                nb += __popcll(mb);
            }
            lds_fence();
            const int me = lane < nnear ? s_x[wave][lane] : 0;
            const int row = lane < nnear ? si[me] : 0;
            double d = -1e300;
            if (lane < nnear) {                                       // S = (mk . qk - |mk|^2 / 2) / 4 in fp64 from the fp32 key rows
                const f32x4 *a4 = reinterpret_cast<const f32x4 *>(mk + (long)row * 64), *q4 = reinterpret_cast<const f32x4 *>(qk + (long)q * 64);
                double dot = 0.0, sq = 0.0;
#pragma unroll 4
                for (int c = 0; c < 16; ++c) {
                    const f32x4 a = a4[c], b = q4[c];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { dot += (double)a[u] * (double)b[u]; sq += (double)a[u] * (double)a[u]; }
                }
                d = (dot - 0.5 * sq) * 0.25;
                if constexpr (KM) {
                    const int fq = q / km.hw16, p = q - fq * km.hw16, y = p / km.w16;
                    d -= (double)km.inv2s * (double)km_dist2(s16x2{(short)(p - y * km.w16), (short)y}, km.centre[(long)fq * km.cstride + row]);
                }
            }
            int rank = 0;
            for (int j = 0; j < nnear; ++j) {
                const double dj = shfl_f64(d, j);
                rank += (dj > d || (dj == d && j < lane)) ? 1 : 0;
            }
            const float mv_ = lane < nnear ? sv[me] : 0.f;            // fp32 score (kept for the softmax)
            lds_fence();
            // sure winners first (list order), then the near entries that rank inside the remaining places
            for (int e0 = 0; e0 < n; e0 += 64) {
                const int e = e0 + lane;
                const bool keep = e < n && sv[e] > hi;
                const unsigned long long kb = __ballot(keep);
                if (keep) { const int pp = base + lanes_below(kb, lane); s_w[wave][pp] = sv[e]; s_x[wave][pp] = si[e]; }
                base += __popcll(kb);
            }
            const bool keepn = lane < nnear && rank < K - nab;
            const unsigned long long kn = __ballot(keepn);
            if (keepn) { const int pp = base + lanes_below(kn, lane); s_w[wave][pp] = mv_; s_x[wave][pp] = row; }
        }
    }
    if (!rescored) {
        int ngt = 0;
        for (int e = lane; e < n; e += 64) ngt += f2key(sv[e]) > prefix ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) ngt += __shfl_xor(ngt, o);
        int need = K - ngt;
        for (int e0 = 0; e0 < n; e0 += 64) {
            const int e = e0 + lane;
            const unsigned key = e < n ? f2key(sv[e]) : 0u;
            const unsigned long long eq = __ballot(e < n && key == prefix);
            const bool keep = e < n && (key > prefix || (key == prefix && lanes_below(eq, lane) < need));
            const unsigned long long kb = __ballot(keep);
            if (keep) {
                const int p = base + lanes_below(kb, lane);
                s_w[wave][p] = sv[e];
                s_x[wave][p] = si[e];
            }
            base += __popcll(kb);
            const int used = __popcll(eq) < need ? __popcll(eq) : need;
            need -= used;
        }
    }
    lds_fence();
    // softmax over the K (exp(v - max) / sum), wavefront reductions
    const float v = lane < K ? s_w[wave][lane] : -__builtin_inff();
    float mx = v;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float ex = lane < K ? expf(v - mx) : 0.f;
    float sum = ex;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float wgt = ex / sum;
    lds_fence();
    if (lane < K) {
        s_w[wave][lane] = wgt;
        if (topk_idx) topk_idx[(long)q * K + lane] = s_x[wave][lane];
        if (topk_w) topk_w[(long)q * K + lane] = wgt;
    }
    lds_fence();
    // gather: lane covers channels [4*lane, +4) and [256 + 4*lane, +4) of each 512-float value row
    for (int o = 0; o < k; ++o) {
        const float *mvo = mv + (long)o * mv_os;
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
        for (int j = 0; j < K; ++j) {
            const float wj = s_w[wave][j];
            const float *row = mvo + (long)s_x[wave][j] * 512 + 4 * lane;
            const f32x4 r0 = *reinterpret_cast<const f32x4 *>(row);
            const f32x4 r1 = *reinterpret_cast<const f32x4 *>(row + 256);
            a0 += r0 * wj;
            a1 += r1 * wj;
        }
        float *dst = readout + (long)o * ro_os + (long)q * 512 + 4 * lane;
        *reinterpret_cast<f32x4 *>(dst) = a0;
        *reinterpret_cast<f32x4 *>(dst + 256) = a1;
    }
}

// k > 1: the gather of merge_readout_kernel, one wave per (query, OBJECT) instead of one per query looping over the objects
// (5x the waves in flight for the K x 2 KB random rows per query and object; the merge kernel then only selects and
// softmaxes and leaves idx / weights [Q][K] in scratch).  4 rows (8 loads of 16 B) in flight per wave: on random rows of a 1.7 GB
// bank 10 in flight were 1.7 % slower (round 5: 0.6125 vs 0.6229 ms per read at T = 104, k = 5; an object-interleaved bank with the k
// object waves of a query side by side 0.631 - no better: the rows are 2 KB, a DRAM page either way)
__global__ __launch_bounds__(256) void gather_readout_kernel(const int32_t *__restrict__ idx, const float *__restrict__ w, int Q,
                                                             const float *__restrict__ mv, long mv_os, float *__restrict__ readout,
                                                             long ro_os, const int K) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const float *mvo = mv + (long)blockIdx.y * mv_os + 4 * lane;
    const int myi = lane < K ? idx[(long)q * K + lane] : 0;
    const float myw = lane < K ? w[(long)q * K + lane] : 0.f;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    // rows in selection order, blocks of 4 with all 8 loads requested before the first use, then the K % 4 last rows one by one (the cut is
    // a run-time value and the shuffles are convergent operations: the compiler does not unroll `for (j < K)` by itself)
    auto rows = [&](const int j, auto nc) {
        constexpr int n = decltype(nc)::value;
        f32x4 r0[n], r1[n];
        float wj[n];
#pragma unroll
        for (int u = 0; u < n; ++u) {
            wj[u] = __shfl(myw, j + u);
            const float *row = mvo + (long)__shfl(myi, j + u) * 512;
            r0[u] = *reinterpret_cast<const f32x4 *>(row);
            r1[u] = *reinterpret_cast<const f32x4 *>(row + 256);
        }
#pragma unroll
        for (int u = 0; u < n; ++u) {
            a0 += r0[u] * wj[u];
            a1 += r1[u] * wj[u];
        }
    };
    int j = 0;
    for (; j + 4 <= K; j += 4) rows(j, std::integral_constant<int, 4>{});
    for (; j < K; ++j) rows(j, std::integral_constant<int, 1>{});
    float *dst = readout + (long)blockIdx.y * ro_os + (long)q * 512 + 4 * lane;
    *reinterpret_cast<f32x4 *>(dst) = a0;
    *reinterpret_cast<f32x4 *>(dst + 256) = a1;
}

// Pass 2 runs with ONE key tile buffer (SINGLE): 50 KB of LDS per workgroup = 3 workgroups (12 waves) per CU instead of 2; the third
// workgroup hides the second barrier per step and the LDS-atomic latencies of the appends (+3..5 % on large banks, round 2).
// Workgroups one round of co-resident workgroups holds: pass 1 (33 KB of LDS) 4 per CU, pass 2 3 per CU, of 256 CUs
static constexpr int RESIDENT1 = 1024, RESIDENT2 = 768;

MemReadPlan memread_plan(int N, int Q) {
    MemReadPlan p;
    p.steps = (N + HROWS - 1) / HROWS;
    const int qblocks = (Q + 63) / 64;
    // pass 1 samples every ss-th step: at least ~48 sampled steps so that the 64 * nc1 row groups are all populated
    static const int ss_env = env_int("STCN_MEMREAD_SAMPLE", 0);
    p.ss = ss_env > 0 ? ss_env : (p.steps >= 768 ? 8 : (p.steps >= 192 ? 4 : (p.steps >= 96 ? 2 : 1)));
    p.ns = (p.steps + p.ss - 1) / p.ss;
    // chunks: as many as keep qblocks * nc within ONE round of co-resident workgroups (a few workgroups beyond the round
    // would run alone afterwards and double the time)
    auto chunks = [&](int steps, int resident, int hi, int *spc) {
        int nc = resident / qblocks;
        nc = nc < 1 ? 1 : (nc > hi ? hi : nc);
        nc = nc > steps ? steps : nc;
        *spc = (steps + nc - 1) / nc;
        return (steps + *spc - 1) / *spc;
    };
    p.nc1 = chunks(p.ns, RESIDENT1, MAXCHUNK1, &p.spc1);    // 64 maxima per chunk and query: <= 512 for threshold_kernel
    p.nc2 = chunks(p.steps, RESIDENT2, MAXCHUNK2, &p.spc2);
    return p;
}

// algorithmic work of one read.  FLOP: the N x Q x 64 affinity - walked once more by the kernelized read, for the row centres -
// and the top_k-sparse read-out.  Bytes: the key bank (+ |mk|^2) and the queries once, top_k value rows of 2 KB per query and object, the read-out once
MemReadCost memread_cost(int N, int Q, int k, int top_k, bool km) {
    const double n = N, q = Q;
    return {(km ? 4.0 : 2.0) * n * q * 64 + 2.0 * k * q * top_k * 512, 4.0 * (n * 65 + q * 64 + k * q * top_k * 512 + k * q * 512)};
}

// Bound of (chunks x queries) of either pass.  Q <= 64 qblocks, so nc1 <= max(1, min(MAXCHUNK1, RESIDENT1 / qblocks)) gives
// nc1 * Q <= max(Q, 64 * RESIDENT1) = max(Q, 65536), and nc2 <= max(1, min(MAXCHUNK2, RESIDENT2 / qblocks)) gives nc2 * Q <= max(Q, 49152)
static size_t memread_list_pairs(int Q) { return (size_t)64 * RESIDENT1 + (size_t)Q + 64; }
// THE scratch layout of a read of Q queries, P = memread_list_pairs(Q): cand_v / cand_i [nc2][Q][50] the chunk lists of pass 2 (<= P * 50),
// cand_n [nc2][Q] their lengths (<= P), tau [Q] the thresholds, gmax [Q][nc1 * 64] the group maxima of pass 1 (<= P * 64) that threshold_kernel
// reads - and, free from then on, the selection of the split read (k > 1, no topk outputs): indices [Q][50] at gmax, weights [Q][50] at
// gmax + Q * 50, written by merge_readout_kernel and read by gather_readout_kernel
MemReadScratchSizes memread_scratch_floats(int Q) {
    const size_t pairs = memread_list_pairs(Q);
    return {pairs * TOPK, pairs * TOPK, pairs, std::max(pairs * NGRP2, (size_t)2 * Q * TOPK), (size_t)Q};
}

long memread_centre_stride(int N) { return (long)((N + HROWS - 1) / HROWS) * HROWS; }

// the launches of one read; KM: the kernelized read - centres of every bank row per query frame first, then the same sequence on the biased score
template <bool KM>
static void memory_read_sequence(const MemRead &r, const MemReadScratch &scr, hipStream_t s) {
    const MemReadPlan pl = memread_plan(r.N, r.Q);
    const int N = r.N, Q = r.Q, top_k = r.top_k, qblocks = (Q + 63) / 64;
    static const bool rescore = env_on("STCN_MEMREAD_RESCORE");      // measurement aid: 0 = plain fp32 cut
    const size_t lds1 = (size_t)2 * KT_FLOATS * sizeof(float);                                    // pass 1: two key tile buffers
    const size_t lds2 = lds1 / 2 + (size_t)4 * LISTS_PER_WAVE * sizeof(float);                    // pass 2: one, and the lists of the 4 waves
    // several objects: merge once per query (indices / weights [Q][top_k] into the gmax alias of memread_scratch_floats), then gather
    // with one wave per (query, object)
    const bool split = !(r.k == 1 || r.topk_idx || r.topk_w);
    int32_t *gi = split ? reinterpret_cast<int32_t *>(scr.gmax) : r.topk_idx;
    float *gw = split ? scr.gmax + (size_t)Q * TOPK : r.topk_w;
    KmArgs km{};
    if constexpr (KM) {
        constexpr int CW = 4, CB = 2;
        km = KmArgs{r.km->centre, memread_centre_stride(N), r.km->h16 * r.km->w16, r.km->w16, 1.f / (2.f * r.km->sigma * r.km->sigma)};
        launch(row_centre_kernel<CW, CB>, dim3((N + 16 * CB * CW - 1) / (16 * CB * CW), Q / km.hw16), dim3(64 * CW), 0, s, nullptr, r.mk, N, r.qk, r.km->qsq,
               r.km->qsq_fs, km.hw16, km.w16, r.km->centre, km.cstride, r.km->centre_idx);
    }
    launch(affinity_tile_kernel<false, false, KM>, dim3(qblocks, pl.nc1), dim3(256), lds1, s, nullptr, r.mk, r.msq, r.qk, N, Q, pl.ns, pl.ss, pl.spc1,
           scr.gmax, (const float *)nullptr, (float *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, top_k, km);
    launch(threshold_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, nullptr, scr.gmax, pl.nc1 * NGRP2, Q, scr.tau, top_k);
    launch(affinity_tile_kernel<true, true, KM>, dim3(qblocks, pl.nc2), dim3(256), lds2, s, nullptr, r.mk, r.msq, r.qk, N, Q, pl.steps, 1, pl.spc2,
           (float *)nullptr, scr.tau, scr.cand_v, scr.cand_i, scr.cand_n, top_k, km);
    launch(merge_readout_kernel<KM>, dim3((Q + 3) / 4), dim3(256), 0, s, nullptr, scr.cand_v, scr.cand_i, scr.cand_n, pl.nc2, Q, r.mv, r.mv_os,
           split ? 0 : r.k, r.readout, r.ro_os, gi, gw, rescore ? r.mk : nullptr, r.qk, top_k, km);
    if (split) launch(gather_readout_kernel, dim3((Q + 3) / 4, r.k), dim3(256), 0, s, nullptr, gi, gw, Q, r.mv, r.mv_os, r.readout, r.ro_os, top_k);
}

void memory_read_launch(const MemRead &r, const MemReadScratch &scr, hipStream_t s) { r.km ? memory_read_sequence<true>(r, scr, s) : memory_read_sequence<false>(r, scr, s); }

// ------------------------------------------------------------------------------------------------
// Fusion attention read (prop_net.py:117-138,198-211): W = softmax over memory rows of the T=1
// affinity; amap[kk][ch][q] = sum_m pooled[kk][ch][m] W[m][q]; then bilinear x16.
// pooled_t [h*w cells][nchp]: channel c = 2 * row + (0: pos, 1: neg) of the kk mask rows, 16x16 block means (F.interpolate
// mode='area'), zero for c >= 2 kk; cell-major so that the pass kernel fetches a memory row's channels as contiguous 16-byte loads
__global__ void area_pool16_kernel(const float *__restrict__ pos, const float *__restrict__ neg, int kk, int h,
                                   int w, int nchp, float *__restrict__ pooled) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    const int hw = h * w;
    if (i >= (long)nchp * hw) return;
    const int cell = (int)(i % hw);
    const int c = (int)(i / hw);
    float acc = 0.f;
    if (c < 2 * kk) {
        const int ch = c & 1, r = c >> 1;
        const int cy = cell / w, cx = cell - cy * w;
        const int W = 16 * w;
        const float *src = (ch == 0 ? pos : neg) + (long)r * 256 * hw + (long)cy * 16 * W + cx * 16;
        for (int y = 0; y < 16; ++y) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(src + (long)y * W);
            const f32x4 a = p[0], b = p[1], cc = p[2], d = p[3];
            acc += (a.x + a.y + a.z + a.w) + (b.x + b.y + b.z + b.w) + (cc.x + cc.y + cc.z + cc.w) + (d.x + d.y + d.z + d.w);
        }
    }
    pooled[(long)cell * nchp + c] = acc * (1.f / 256.f);
}

// channels of the attention read padded to the instantiated widths (2 (k + 1) = 4 ... 18); with more than 8 objects to a multiple of 20:
// the pass kernel then runs once per slice of 20 channels (same column maxima, same row order: every channel's sum is what one wide pass gives)
int attention_nchp(int nch) { return nch <= 4 ? 4 : (nch <= 8 ? 8 : (nch <= 12 ? 12 : 20 * ((nch + 19) / 20))); }
// floats per (chunk, query) of the partial sums: the softmax denominator + one per channel (19 up to 8 objects, as sized since round 2)
static int attention_part_stride(int nch) { return 1 + (nch <= 18 ? 18 : nch); }
size_t attention_part_floats(int kk, int hw) { return (size_t)MAXCHUNK * hw * attention_part_stride(2 * kk); }
// pass 2 of the attention read: per (query block, row chunk) partial sums of e = exp(S - cm[q]), cm = the exact column maximum:
//   part[chunk][q][0] = sum_m e,  part[chunk][q][1 + c] = sum_m e * pooled[c][m]
template <int WAVES, int NCHP>
__global__ __launch_bounds__(64 * WAVES) void attention_pass_kernel(
    const float *__restrict__ mk, const float *__restrict__ msq, const float *__restrict__ qk, int N, int Q,
    int steps_per_chunk, const float *__restrict__ gmax, int G, const float *__restrict__ pooled, int nch,
    float *__restrict__ part, int prow, int pstr, int ch0) {      // pooled: first channel of this slice, row stride prow; nch: channels of this slice; part: [..][pstr], channel ch0 + c
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = (blockIdx.x * WAVES + wave) * 16;
    if (q0 >= Q) return;
    const int chunk = blockIdx.y;
    const int nsteps = (N + HROWS - 1) / HROWS;
    const int h0 = chunk * steps_per_chunk;
    const int h1 = min(nsteps, h0 + steps_per_chunk);
    const int g = lane >> 4, col = lane & 15;
    const int qcol = min(q0 + col, Q - 1);
    f32x4 bq[4];
    load_bq(qk, Q, q0, lane, bq);
    // exact column maximum of S = max over the G group maxima of pass 1 ([G][Q]): the four lane groups of a column take every
    // fourth group (independent loads in flight) and combine with two shuffles.  (A separate one-thread-per-query kernel walked
    // the 256 groups serially: 52 us for 1620 queries, 3 % of a round-2 frame.)
    float cm = -__builtin_inff();
    for (int gi = g; gi < G; gi += 4) cm = fmaxf(cm, gmax[(long)gi * Q + qcol]);
    cm = fmaxf(cm, __shfl_xor(cm, 16));
    cm = fmaxf(cm, __shfl_xor(cm, 32));
    float l = 0.f, a[NCHP];
#pragma unroll
    for (int c = 0; c < NCHP; ++c) a[c] = 0.f;
    for (int h = h0; h < h1; ++h) {
        const int row0 = h * HROWS;
        HalfFrag hf;
        load_half(mk, msq, N, row0, lane, hf);
        // the pooled channels of this lane's memory rows: NCHP / 4 16-byte loads per row; the 4 rows of row block 0 are requested
        // before the MFMAs of the step, those of block rb + 1 before the arithmetic of block rb (round 2: scalar loads behind
        // `if (c < nch)` - the compiler waited for each of the up to 72 per row block)
        f32x4 pl[2][4][NCHP / 4];
        auto pload = [&](int rb, f32x4 (&d)[4][NCHP / 4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rr = min(row0 + rb * 16 + 4 * g + j, N - 1);
#pragma unroll
                for (int c4 = 0; c4 < NCHP / 4; ++c4) d[j][c4] = *reinterpret_cast<const f32x4 *>(pooled + (long)rr * prow + 4 * c4);
            }
        };
        pload(0, pl[0]);
        f32x4 acc[4];
        mfma_half(hf, bq, acc);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            if (rb < 3) pload(rb + 1, pl[(rb + 1) & 1]);
            const int r = row0 + rb * 16 + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = r + j < N ? expf(acc[rb][j] - cm) : 0.f;
                l += e;
#pragma unroll
                for (int c = 0; c < NCHP; ++c) a[c] += e * pl[rb & 1][j][c >> 2][c & 3];
            }
        }
    }
    // sum the 4 lane groups that share a query column (fixed order -> deterministic)
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
#pragma unroll
    for (int c = 0; c < NCHP; ++c) { a[c] += __shfl_xor(a[c], 16); a[c] += __shfl_xor(a[c], 32); }
    if (g == 0 && q0 + col < Q) {
        float *dst = part + ((long)chunk * Q + q0 + col) * pstr;
        if (ch0 == 0) dst[0] = l;
#pragma unroll
        for (int c = 0; c < NCHP; ++c)
            if (c < nch) dst[1 + ch0 + c] = a[c];
    }
}

__global__ void attention_finalize_kernel(const float *__restrict__ part, int NC, int Q, int nch, int pstr,
                                          float *__restrict__ amap) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    float l = 0.f;
    for (int ch = 0; ch < NC; ++ch) l += part[((long)ch * Q + q) * pstr];
    for (int c = 0; c < nch; ++c) {
        float acc = 0.f;
        for (int ch = 0; ch < NC; ++ch) acc += part[((long)ch * Q + q) * pstr + 1 + c];
        amap[(long)c * Q + q] = acc / l;
    }
}

__global__ void bilinear_up16_kernel(const float *__restrict__ amap, int nch, int h, int w, float *__restrict__ out) {
    const int H = 16 * h, W = 16 * w;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)nch * H * W) return;
    const int c = (int)(i / ((long)H * W));
    const long r = i - (long)c * H * W;
    const int oy = (int)(r / W), ox = (int)(r - (long)oy * W);
    float sy = ((float)oy + 0.5f) * 0.0625f - 0.5f, sx = ((float)ox + 0.5f) * 0.0625f - 0.5f;
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
    int y0 = (int)sy, x0 = (int)sx;
    y0 = y0 > h - 1 ? h - 1 : y0;
    x0 = x0 > w - 1 ? w - 1 : x0;
    const int y1 = y0 < h - 1 ? y0 + 1 : y0, x1 = x0 < w - 1 ? x0 + 1 : x0;
    const float fy = sy - (float)y0, fx = sx - (float)x0;
    const float *a = amap + (long)c * h * w;
    out[i] = (1.f - fy) * ((1.f - fx) * a[y0 * w + x0] + fx * a[y0 * w + x1]) +
             fy * ((1.f - fx) * a[y1 * w + x0] + fx * a[y1 * w + x1]);
}

// pooled_t [h*w][nchp] = 16x16 block means of the +/- mask differences of the current interaction: the same for every frame
// of the round, so the engine computes it once per interaction (pos == nullptr below)
void attention_pool_launch(const float *pos, const float *neg, int kk, int h, int w, float *pooled, hipStream_t s) {
    const int nchp = attention_nchp(2 * kk);
    hipLaunchKernelGGL(area_pool16_kernel, dim3((unsigned)(((long)nchp * h * w + 255) / 256)), dim3(256), 0, s, pos, neg, kk, h, w, nchp, pooled);
}

static constexpr int ATTN_WAVES = 4;    // waves (of 16 queries) per workgroup of the two pass kernels
AttnPlan attention_plan(int hw) {
    AttnPlan p;
    p.steps = (hw + HROWS - 1) / HROWS;
    p.qblocks = (hw + 16 * ATTN_WAVES - 1) / (16 * ATTN_WAVES);
    p.NC = (512 + p.qblocks - 1) / p.qblocks;
    if (p.NC > MAXCHUNK) p.NC = MAXCHUNK;
    if (p.NC > p.steps) p.NC = p.steps;
    p.spc = (p.steps + p.NC - 1) / p.NC;
    p.NCeff = (p.steps + p.spc - 1) / p.spc;
    return p;
}

void attention_read_launch(const float *mk, const float *msq, const float *qk, const float *pos, const float *neg,
                           int kk, int h, int w, float *pooled, float *amap, float *attn, AttnScratch scr,
                           hipStream_t s) {
    const int hw = h * w, nch = kk * 2;
    if (pos) attention_pool_launch(pos, neg, kk, h, w, pooled, s);
    constexpr int WAVES = ATTN_WAVES;
    const AttnPlan pl = attention_plan(hw);
    const int spc = pl.spc, NCeff = pl.NCeff;
    const dim3 grid(pl.qblocks, NCeff);
    hipLaunchKernelGGL((colmax_pass_kernel<WAVES>), grid, dim3(64 * WAVES), 0, s, mk, msq, qk, hw, hw, spc, scr.gmax);
    const int nchp = attention_nchp(nch), pstr = attention_part_stride(nch);
    switch (nchp) {
#define STCN_AP(N_, C0_, NCH_) hipLaunchKernelGGL((attention_pass_kernel<WAVES, N_>), grid, dim3(64 * WAVES), 0, s, mk, msq, qk, hw, hw, spc, scr.gmax, NCeff * NGRP, pooled + (C0_), NCH_, scr.part, nchp, pstr, C0_)
        case 4: STCN_AP(4, 0, nch); break;
        case 8: STCN_AP(8, 0, nch); break;
        case 12: STCN_AP(12, 0, nch); break;
        default:
            for (int c0 = 0; c0 < nch; c0 += 20) STCN_AP(20, c0, nch - c0 < 20 ? nch - c0 : 20);
            break;
#undef STCN_AP
    }
    hipLaunchKernelGGL(attention_finalize_kernel, dim3((hw + 255) / 256), dim3(256), 0, s, scr.part, NCeff, hw, nch, pstr,
                       amap);
    const long tot = (long)nch * 256 * hw;
    hipLaunchKernelGGL(bilinear_up16_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, amap, nch, h, w,
                       attn);
}

}  // namespace stcn
