// frame_select.hip - squared L2 distances between T feature vectors of K fp32 values each (the cached f16 maps of a clip: the l2_mask frame selector).
// D[i][j] = |x_i|^2 + |x_j|^2 - 2 x_i . x_j cancels for neighbouring frames, so the Gram matrix is accumulated in fp64: the product of two
// fp32 values is exact there, and v_mfma_f64_16x16x4_f64 leaves fp64 summation as the only error.  A tall-skinny product (T <= 106, K ~ 1.7 M):
// K is cut into slices, one workgroup each; a workgroup holds the whole upper triangle of 16 x 16 frame tiles in its accumulators and writes it
// to scratch; a second kernel sums the slices in a fixed order and forms the distances.
#include <hip/hip_ext.h>

#include <utility>

#include "kernels.h"

namespace stcn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// waves of a workgroup: the tile pairs are dealt round-robin to them (at most 7 tiles of 16 frames: 28 pairs, 7 per wave = 56 accumulator VGPRs)
constexpr int FG_WAVES = 4;

// pair p of the upper triangle of nt x nt tiles, rows first: (0,0) (0,1) .. (0,nt-1) (1,1) ..
constexpr int fg_pair_a(int nt, int p) { int a = 0; while (p >= nt - a) { p -= nt - a; ++a; } return a; }
constexpr int fg_pair_b(int nt, int p) { int a = 0; while (p >= nt - a) { p -= nt - a; ++a; } return a + p; }
__host__ __device__ constexpr int fg_pair_index(int nt, int a, int b) { return a * nt - a * (a - 1) / 2 + (b - a); }

// what wave W of a workgroup holds when the clip has NT tiles: pairs W, W + 4, ... and the tiles they touch
template <int NT, int W>
struct FgWave {
    static constexpr int NP = NT * (NT + 1) / 2;
    static constexpr int N = W < NP ? (NP - W + FG_WAVES - 1) / FG_WAVES : 0;
    static constexpr int pair(int j) { return W + FG_WAVES * j; }
    static constexpr int a(int j) { return fg_pair_a(NT, pair(j)); }
    static constexpr int b(int j) { return fg_pair_b(NT, pair(j)); }
    static constexpr bool need(int t) {
        for (int j = 0; j < N; ++j)
            if (a(j) == t || b(j) == t) return true;
        return false;
    }
};
template <int... I, typename F>
__device__ __forceinline__ void fg_for(std::integer_sequence<int, I...>, F &&f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void fg_for(F &&f) { fg_for(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f)); }

constexpr int FG_U = FRAME_GRAM_KSTEP / 16;             // 16-byte loads per lane, tile and step: 4 k-groups x 4 floats = 16 k each

// Lane l serves frame l & 15 of every tile and k-group g = l >> 4: per step and tile it loads FG_U x 16 bytes (k = k0 + 16 u + 4 g .. + 3) and
// converts once; component c of those loads is the operand of one MFMA (its 4 k: k0 + 16 u + 4 g + c, g = 0..3 - A and B agree, which is all
// the instruction asks).  A diagonal pair takes the same register as A and B.  No LDS, no atomics.  Addresses are clamped into [0, K - 4] and
// what lies behind the slice's end is zeroed AFTER the load: no load is conditional.  A step loads, converts and multiplies; the latency of
// its loads is covered by the second workgroup of the compute unit.  (Written with the next step's loads in front of this step's MFMAs, hipcc
// sinks them to their first use - this loop; pinned there by an empty asm use behind a scheduling barrier, the kernel took 0.91 / 0.97 / 1.02
// of its time at T = 40 / 66 / 104 with 20 % more registers: not kept.)
template <int NT, int W>
__device__ __forceinline__ void fg_wave(const float *__restrict__ x, const FrameIndex &index, long stride, int T, long K, long k0, long k1,
                                        double *__restrict__ part) {
    using Wv = FgWave<NT, W>;
    if constexpr (Wv::N > 0) {
        const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
        const float *row[NT];
        fg_for<NT>([&](auto t) {
            if constexpr (Wv::need(t)) {
                const int f = min(t * 16 + r, T - 1);       // rows >= T of the last tile read a valid frame; they are never stored
                row[t] = x + (long)index.v[f] * stride;
            }
        });
        f64x4 acc[Wv::N];
        fg_for<Wv::N>([&](auto j) { acc[j] = f64x4{0., 0., 0., 0.}; });
        for (long k = k0; k < k1; k += FRAME_GRAM_KSTEP) {
            f32x4 cur[FG_U][NT];
            fg_for<FG_U>([&](auto u) {
                const long kk = k + 16 * decltype(u)::value + 4 * g, kl = kk < K - 4 ? kk : K - 4;
                fg_for<NT>([&](auto t) {
                    if constexpr (Wv::need(t)) cur[u][t] = *reinterpret_cast<const f32x4 *>(row[t] + kl);
                });
            });
            fg_for<FG_U>([&](auto u) {
                const bool valid = k + 16 * decltype(u)::value + 4 * g < k1;
                fg_for<4>([&](auto c) {
                    double d[NT];
                    fg_for<NT>([&](auto t) {
                        if constexpr (Wv::need(t)) d[t] = (double)(valid ? cur[u][t][decltype(c)::value] : 0.f);      // one select per value, on the fp32
                    });
                    fg_for<Wv::N>([&](auto j) {
                        constexpr int a = Wv::a(decltype(j)::value), b = Wv::b(decltype(j)::value);      // constants, or d[] lands in scratch
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(d[a], d[b], acc[j], 0, 0, 0);
                    });
                });
            });
        }
        // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg (NOT the f32 map)
        fg_for<Wv::N>([&](auto j) {
            constexpr int jj = decltype(j)::value, a = Wv::a(jj), b = Wv::b(jj), p = Wv::pair(jj);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int ri = g + 4 * reg;
                if (a * 16 + ri < T && b * 16 + r < T) part[(p * 16 + ri) * 16 + r] = acc[jj][reg];
            }
        });
    }
}

// x: vector t starts at x + index.v[t] * stride; slice blockIdx.x covers k in [blockIdx.x * len, min(K, (blockIdx.x + 1) * len)); part [S][pairs][16][16]
template <int NT>
__global__ __launch_bounds__(64 * FG_WAVES) void frame_gram_kernel(const float *__restrict__ x, const FrameIndex index, long stride, int T, long K, long len,
                                                                   double *__restrict__ part) {
    const long k0 = (long)blockIdx.x * len, k1 = min(K, k0 + len);
    part += (size_t)blockIdx.x * (NT * (NT + 1) / 2) * 256;
    switch (threadIdx.x >> 6) {             // wave-uniform: each wave runs the loop compiled for its own pairs
        case 0: fg_wave<NT, 0>(x, index, stride, T, K, k0, k1, part); break;
        case 1: fg_wave<NT, 1>(x, index, stride, T, K, k0, k1, part); break;
        case 2: fg_wave<NT, 2>(x, index, stride, T, K, k0, k1, part); break;
        default: fg_wave<NT, 3>(x, index, stride, T, K, k0, k1, part); break;
    }
}

// One workgroup per tile pair (a, b), one thread per element: G_ij, G_ii and G_jj summed over the S slices in ascending order - a fixed order,
// the same for every thread that needs a diagonal element, so two runs (and the two triangles) give the same bits - then
// D[i][j] = D[j][i] = G_ii + G_jj - 2 G_ij for i < j and D[i][i] = 0.
__global__ __launch_bounds__(256) void frame_gram_reduce_kernel(const double *__restrict__ part, int S, int nt, int T, double *__restrict__ dist) {
    int a = 0, p = blockIdx.x;
    while (p >= nt - a) { p -= nt - a; ++a; }
    const int b = a + p, pairs = nt * (nt + 1) / 2;
    const int ri = threadIdx.x >> 4, cj = threadIdx.x & 15, i = a * 16 + ri, j = b * 16 + cj;
    if (i >= T || j >= T || i > j) return;
    if (i == j) { dist[(size_t)i * T + i] = 0.; return; }
    const double *pij = part + ((size_t)blockIdx.x * 16 + ri) * 16 + cj;
    const double *pii = part + ((size_t)fg_pair_index(nt, a, a) * 16 + ri) * 16 + ri;
    const double *pjj = part + ((size_t)fg_pair_index(nt, b, b) * 16 + cj) * 16 + cj;
    const size_t ss = (size_t)pairs * 256;
    double gij = 0., gii = 0., gjj = 0.;
#pragma unroll 8
    for (int s = 0; s < S; ++s) {
        gij += pij[s * ss];
        gii += pii[s * ss];
        gjj += pjj[s * ss];
    }
    const double d = gii + gjj - 2. * gij;
    dist[(size_t)i * T + j] = d;
    dist[(size_t)j * T + i] = d;
}

// ---------------------------------------------------------------- host side
FrameGramPlan frame_gram_plan(int T, long K) {
    FrameGramPlan pl{};
    pl.nt = (T + 15) / 16;
    pl.pairs = pl.nt * (pl.nt + 1) / 2;
    const long steps = (K + FRAME_GRAM_KSTEP - 1) / FRAME_GRAM_KSTEP;
    const long want = steps < FRAME_GRAM_MAX_SLICES ? steps : FRAME_GRAM_MAX_SLICES;
    const long per = (steps + want - 1) / want;              // k-steps per slice
    pl.len = per * FRAME_GRAM_KSTEP;
    pl.slices = (int)((steps + per - 1) / per);             // (slices - 1) * len < K: the last slice is never empty
    return pl;
}
size_t frame_gram_scratch_bytes(int T, long K) {
    const FrameGramPlan pl = frame_gram_plan(T, K);
    return (size_t)pl.slices * pl.pairs * 256 * sizeof(double);
}

void frame_gram_launch(const float *x, const FrameIndex &index, long stride, int T, long K, double *scratch, double *dist, hipStream_t s,
                       hipEvent_t *ev_gram, hipEvent_t *ev_red) {
    const FrameGramPlan pl = frame_gram_plan(T, K);
    const dim3 grid(pl.slices), block(64 * (pl.pairs < FG_WAVES ? pl.pairs : FG_WAVES));
    switch (pl.nt) {
        case 1: launch(frame_gram_kernel<1>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
        case 2: launch(frame_gram_kernel<2>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
        case 3: launch(frame_gram_kernel<3>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
        case 4: launch(frame_gram_kernel<4>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
        case 5: launch(frame_gram_kernel<5>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
        case 6: launch(frame_gram_kernel<6>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
        default: launch(frame_gram_kernel<7>, grid, block, 0, s, ev_gram, x, index, stride, T, K, pl.len, scratch); break;
    }
    launch(frame_gram_reduce_kernel, dim3(pl.pairs), dim3(256), 0, s, ev_red, (const double *)scratch, pl.slices, pl.nt, T, dist);
}

}  // namespace stcn
