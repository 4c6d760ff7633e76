// metrics.hip - J (region IoU) and F (boundary measure) counts on the GPU, integer-exact.
// Reference: interactions/metrics.py:24-34 (get_j_and_f), :38-97 (_seg2bmap at equal size), :100-160 (f_measure:
// disk(ceil(0.008*|shape|)) dilation of each boundary map, matches = boundary & dilated other boundary).
// HBM-bound stencil work: one pass builds both 1-pixel boundary maps, a second pass visits the pixels and, ONLY
// at boundary pixels (a few thousand per frame), scans the disk window of the other map; six integer counters per
// frame are accumulated with integer atomics (exact, order-independent).
#include <algorithm>

#include "kernels.h"

namespace stcn {

// Counting: a thread visits PPT pixels (a wave 64 consecutive pixels per step: coalesced byte loads), keeps its counters in registers
// and the wave adds them up ONCE at the end - one integer atomic per wave and counter when the wave's 64 x PPT pixels lie inside one
// frame (all but the ~T waves that straddle a frame boundary, which fall back to one atomic per pixel).  Round 3 issued one atomic per
// wave and counter per 64 PIXELS: 1.7 M atomics on 6 T addresses made the two kernels 4.4 ms per 66-frame 480p clip - 15 % of an
// annotation round of the eval driver; a per-pixel atomicAdd before that 49 ms.
static constexpr int PPT = 16;

// The walk of the four counting kernels: wave w of workgroup b owns the 64 x PPT pixels from first_pixel(w) on, of the n = T x H x W of
// the clip.  A pixel is handed to the kernel body with its index i in the clip and its frame t; its row and column cost an integer
// division, so they are computed where the body asks for them (the match kernels do only at boundary pixels), not for every pixel.
struct Pixel {
    long i;
    int t, rem, W;         // rem: index inside frame t
    __device__ __forceinline__ int y() const { return rem / W; }
    __device__ __forceinline__ int x() const { return rem - y() * W; }
};

struct WaveWalk {
    long hw, n, base;      // pixels per frame, pixels in all, first pixel of this wave
    int W, lane, t0;       // t0: the frame of `base`
    bool one_frame;        // wave-uniform: every pixel of the wave lies in frame t0 (false for a wave past the end, which visits nothing)
    static __device__ __forceinline__ long first_pixel(int wave) { return ((long)blockIdx.x * 4 + wave) * (64L * PPT); }
    __device__ __forceinline__ WaveWalk(int T, int H, int W_) : hw((long)H * W_), n(T * hw), base(first_pixel(threadIdx.x >> 6)), W(W_), lane(threadIdx.x & 63) {
        t0 = (int)(base / hw);
        one_frame = base < n && (int)((min(base + 64L * PPT, n) - 1) / hw) == t0;
    }
    template <typename Body> __device__ __forceinline__ void for_each(Body &&body) const {
        for (int j = 0; j < PPT; ++j) {
            const long i = base + j * 64L + lane;
            if (i >= n) break;
            const int t = one_frame ? t0 : (int)(i / hw);
            body(Pixel{i, t, (int)(i - t * hw), W});
        }
    }
};

// The disk of radius r around (y, x), clipped to the H x W frame: visit(index inside the frame) for its elements, rows from the centre
// outwards (0, -1, +1, -2, ...), until done() says - before a row - that everything wanted was found: the two boundaries usually run
// close to each other, the scan ends early.
template <typename Visit, typename Done>
__device__ __forceinline__ void disk_scan(int y, int x, int H, int W, int r, Visit &&visit, Done &&done) {
    for (int d = 0; d <= 2 * r && !done(); ++d) {
        const int dy = (d & 1) ? -((d + 1) >> 1) : (d >> 1);
        const int yy = y + dy;
        if ((unsigned)yy >= (unsigned)H) continue;
        int hx = 0;                                           // half width of the disk at this row: largest dx with dx^2 + dy^2 <= r^2
        while ((hx + 1) * (hx + 1) + dy * dy <= r * r) ++hx;
        const int x0 = max(x - hx, 0), x1 = min(x + hx, W - 1);
        const long row = (long)yy * W;
        for (int xx = x0; xx <= x1; ++xx) visit(row + xx);
    }
}

// ---- counters: two policies, on purpose -----------------------------------------------------------------------------------------------
// Binary masks: all pixels of a frame add to the same six counters, so a thread counts in REGISTERS, the wave adds its lanes up once
// (wave_sum) and lane 0 issues one global atomic per counter.  Label maps: a pixel adds to the counters of the few objects it touches,
// in a [k][6] table per wave in LDS (LabelCounters, flush_tables) - registers would be k x 6 per lane.  The binary entry points are NOT
// routed through the label kernels with k = 1: every lane of a wave would then add to the same LDS word, and what those same-address
// LDS atomics cost beside one register add per lane has never been measured.  In both, the ~T waves that lie across a frame boundary
// add per pixel to global memory.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// n register counters of a wave inside one frame -> the frame's counters from `c` on (lane 0, the non-zero ones)
template <int N> __device__ __forceinline__ void wave_flush(const WaveWalk &w, const int (&v)[N], int *__restrict__ c) {
    if (!w.one_frame) return;
    int sum[N];
#pragma unroll
    for (int e = 0; e < N; ++e) sum[e] = wave_sum(v[e]);
    if (w.lane != 0) return;
#pragma unroll
    for (int e = 0; e < N; ++e)
        if (sum[e]) atomicAdd(&c[e], sum[e]);
}

// bit0 = gt boundary, bit1 = pred boundary.  j_only: intersection / union only (bmap untouched)
__global__ __launch_bounds__(256) void jf_boundary_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ pr, int T, int H, int W,
                                                          uint8_t *__restrict__ bmap, int *__restrict__ counts, int j_only) {
    const WaveWalk walk(T, H, W);
    int c[4] = {0, 0, 0, 0};               // inter, union, n_gt_b, n_fg_b
    walk.for_each([&](const Pixel &px) {
        const long i = px.i;
        const int g = gt[i] != 0, p = pr[i] != 0;
        int bg = 0, bp = 0;
        if (!j_only) {
            const int y = px.y(), x = px.x();
            auto bnd = [&](const uint8_t *seg, int s) -> int {
                const uint8_t *q = seg + i;
                if (y < H - 1 && x < W - 1) {
                    const int e = q[1] != 0, so = q[W] != 0, se = q[W + 1] != 0;
                    return (s ^ e) | (s ^ so) | (s ^ se);
                }
                if (y == H - 1 && x < W - 1) return s ^ (q[1] != 0);
                if (x == W - 1 && y < H - 1) return s ^ (q[W] != 0);
                return 0;
            };
            bg = bnd(gt, g);
            bp = bnd(pr, p);
            bmap[i] = (uint8_t)(bg | (bp << 1));
        }
        if (walk.one_frame) { c[0] += g & p; c[1] += g | p; c[2] += bg; c[3] += bp; }
        else {                                                                           // a wave across a frame boundary: per pixel
            int *ct = counts + px.t * 6;
            if (g & p) atomicAdd(&ct[0], 1);
            if (g | p) atomicAdd(&ct[1], 1);
            if (bg) atomicAdd(&ct[2], 1);
            if (bp) atomicAdd(&ct[3], 1);
        }
    });
    wave_flush(walk, c, counts + walk.t0 * 6);
}

__global__ __launch_bounds__(256) void jf_match_kernel(const uint8_t *__restrict__ bmap, int T, int H, int W, int r, int *__restrict__ counts) {
    const WaveWalk walk(T, H, W);
    int c[2] = {0, 0};                     // gt_match, fg_match
    walk.for_each([&](const Pixel &px) {
        const int me = bmap[px.i];
        if (!me) return;                                      // only boundary pixels (a few thousand per frame) scan the disk
        const uint8_t *b = bmap + (long)px.t * walk.hw;
        const int want = ((me & 1) ? 2 : 0) | ((me & 2) ? 1 : 0);
        int other = 0;                                        // bits of the OTHER map found inside the disk
        disk_scan(px.y(), px.x(), H, W, r, [&](long e) { other |= b[e]; }, [&] { return (other & want) == want; });
        const int m4 = (me & 1) && (other & 2), m5 = (me & 2) && (other & 1);
        if (walk.one_frame) { c[0] += m4; c[1] += m5; }
        else {
            if (m4) atomicAdd(&counts[px.t * 6 + 4], 1);      // gt boundary pixel inside dilated pred boundary
            if (m5) atomicAdd(&counts[px.t * 6 + 5], 1);      // pred boundary pixel inside dilated gt boundary
        }
    });
    wave_flush(walk, c, counts + walk.t0 * 6 + 4);
}

void jf_counts_launch(const uint8_t *gt, const uint8_t *pred, int T, int H, int W, int radius, uint8_t *bmap,
                      int *counts, hipStream_t s) {
    const long n = (long)T * H * W;
    const unsigned blocks = (unsigned)((n + 256L * PPT - 1) / (256L * PPT));
    (void)hipMemsetAsync(counts, 0, (size_t)T * 6 * sizeof(int), s);
    // radius < 0: J only (intersection / union; bmap may be null)
    hipLaunchKernelGGL(jf_boundary_kernel, dim3(blocks), dim3(256), 0, s, gt, pred, T, H, W, bmap, counts, radius < 0 ? 1 : 0);
    if (radius >= 0) hipLaunchKernelGGL(jf_match_kernel, dim3(blocks), dim3(256), 0, s, bmap, T, H, W, radius, counts);
}

// ---- label maps of k objects: one pass over the pixels serves every object ------------------------------------------------------------
// A pixel carries ONE label per map, so it touches the region counters of at most two objects (its gt label, its pred label) and is a
// boundary pixel of at most four per map (its own label and those of its east / south / south-east neighbours, wherever they differ:
// object o's binary mask changes between two pixels exactly when one of them is o and the other is not).  The boundary pass stores, per
// pixel and map, the SET of those objects (BSet: bit o - 1 = object o; background takes part only as "not o"); the match pass scans the
// disk once per boundary pixel and ORs the sets it finds - object o's gt boundary is matched iff bit o - 1 is in the OR of the pred sets,
// so a neighbouring object's boundary inside the disk never counts.  Per object this is the arithmetic of the binary kernels above.
// Counters: a wave that lies inside one frame adds into its own [k][6] table in LDS (integer LDS atomics) and the workgroup flushes the
// non-zero entries with one global integer atomic each; a wave across a frame boundary adds per pixel to global memory, as above.
static constexpr int LT = STCN_MAX_OBJECTS * 6;          // the C entry points refuse more objects
static_assert(STCN_MAX_OBJECTS <= 32, "a pixel's object set is at most one 32-bit word");

template <typename Wd> struct alignas(2 * sizeof(Wd)) BSet { Wd g, p; };

__device__ __forceinline__ int label_of(uint8_t v, int k) { return v > k ? 0 : v; }       // an object that appears later: background
__device__ __forceinline__ unsigned bit_of(int l) { return l ? 1u << (l - 1) : 0u; }

struct LabelCounters {
    int *lds;              // this wave's [k][6] table, used when the wave lies in one frame
    int *counts;           // [k][T_all][6], at the first counted frame
    int T_all;
    bool one_frame;
    __device__ __forceinline__ void add(int o, int t, int c) const {
        if (one_frame) atomicAdd(&lds[o * 6 + c], 1);
        else atomicAdd(&counts[((long)o * T_all + t) * 6 + c], 1);
    }
    __device__ __forceinline__ void add_set(unsigned set, int t, int c) const {
        for (unsigned m = set; m; m &= m - 1) add(__ffs((int)m) - 1, t, c);
    }
};

// every thread of the workgroup: the tables of its four waves -> global counters (a non-zero entry belongs to a wave inside one frame)
__device__ __forceinline__ void flush_tables(const int (*tab)[LT], int k, long hw, int *__restrict__ counts, int T_all) {
    for (int e = threadIdx.x; e < 4 * k * 6; e += 256) {
        const int w = e / (k * 6), r = e - w * (k * 6);
        const int v = tab[w][r];
        if (!v) continue;
        const int t = (int)(WaveWalk::first_pixel(w) / hw);
        atomicAdd(&counts[((long)(r / 6) * T_all + t) * 6 + r % 6], v);
    }
}

template <typename Wd>
__global__ __launch_bounds__(256) void label_boundary_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ pr, int k, int T, int H, int W,
                                                             BSet<Wd> *__restrict__ bsets, int *__restrict__ counts, int T_all, int j_only) {
    __shared__ int tab[4][LT];
    for (int e = threadIdx.x; e < 4 * LT; e += 256) (&tab[0][0])[e] = 0;
    __syncthreads();
    const WaveWalk walk(T, H, W);
    const LabelCounters cn{tab[threadIdx.x >> 6], counts, T_all, walk.one_frame};
    walk.for_each([&](const Pixel &px) {
        const long i = px.i;
        const int t = px.t;
        const int g = label_of(gt[i], k), p = label_of(pr[i], k);
        if (!j_only) {
            const int y = px.y(), x = px.x();
            auto bnd = [&](const uint8_t *seg, int s) -> unsigned {                      // _seg2bmap for every object at once
                const uint8_t *q = seg + i;
                unsigned b = 0;
                auto differ = [&](uint8_t v) { const int nb = label_of(v, k); if (nb != s) b |= bit_of(s) | bit_of(nb); };
                if (y < H - 1 && x < W - 1) { differ(q[1]); differ(q[W]); differ(q[W + 1]); }
                else if (y == H - 1 && x < W - 1) differ(q[1]);
                else if (x == W - 1 && y < H - 1) differ(q[W]);
                return b;
            };
            const unsigned bg = bnd(gt, g), bp = bnd(pr, p);
            bsets[i] = BSet<Wd>{(Wd)bg, (Wd)bp};
            cn.add_set(bg, t, 2);
            cn.add_set(bp, t, 3);
        }
        if (g) { if (g == p) cn.add(g - 1, t, 0); cn.add(g - 1, t, 1); }                // union of o: every pixel that is o in either map
        if (p && p != g) cn.add(p - 1, t, 1);
    });
    __syncthreads();
    flush_tables(tab, k, walk.hw, counts, T_all);
}

template <typename Wd>
__global__ __launch_bounds__(256) void label_match_kernel(const BSet<Wd> *__restrict__ bsets, int k, int T, int H, int W, int r,
                                                          int *__restrict__ counts, int T_all) {
    __shared__ int tab[4][LT];
    for (int e = threadIdx.x; e < 4 * LT; e += 256) (&tab[0][0])[e] = 0;
    __syncthreads();
    const WaveWalk walk(T, H, W);
    const LabelCounters cn{tab[threadIdx.x >> 6], counts, T_all, walk.one_frame};
    walk.for_each([&](const Pixel &px) {
        const BSet<Wd> me = bsets[px.i];
        if (!(me.g | me.p)) return;                           // only boundary pixels scan the disk
        const BSet<Wd> *b = bsets + (long)px.t * walk.hw;
        unsigned og = 0, op = 0;                              // objects whose gt / pred boundary lies inside the disk
        disk_scan(px.y(), px.x(), H, W, r, [&](long e) { const BSet<Wd> v = b[e]; og |= v.g; op |= v.p; },
                  [&] { return (op & me.g) == me.g && (og & me.p) == me.p; });
        cn.add_set(me.g & op, px.t, 4);                       // object o's gt boundary pixel inside ITS dilated pred boundary
        cn.add_set(me.p & og, px.t, 5);
    });
    __syncthreads();
    flush_tables(tab, k, walk.hw, counts, T_all);
}

size_t label_scratch_bytes(int k, int T, int H, int W) { return (size_t)T * H * W * (k <= 8 ? sizeof(BSet<uint8_t>) : sizeof(BSet<uint32_t>)); }

template <typename Wd>
static void label_counts_kernels(const uint8_t *gt, const uint8_t *pred, int k, int Tn, int H, int W, int radius, void *bsets, int *counts, int T_all,
                                 unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(label_boundary_kernel<Wd>, dim3(blocks), dim3(256), 0, s, gt, pred, k, Tn, H, W, (BSet<Wd> *)bsets, counts, T_all, radius < 0 ? 1 : 0);
    if (radius >= 0) hipLaunchKernelGGL(label_match_kernel<Wd>, dim3(blocks), dim3(256), 0, s, (const BSet<Wd> *)bsets, k, Tn, H, W, radius, counts, T_all);
}

void label_counts_launch(const uint8_t *gt, const uint8_t *pred, int k, int Tn, int H, int W, int radius, void *bsets, int *counts, int T_all,
                         hipStream_t s) {
    const long n = (long)Tn * H * W;
    const unsigned blocks = (unsigned)((n + 256L * PPT - 1) / (256L * PPT));
    // the Tn counted frames of every object: k rows of Tn * 6 ints, T_all * 6 ints apart
    (void)hipMemset2DAsync(counts, (size_t)T_all * 6 * sizeof(int), 0, (size_t)Tn * 6 * sizeof(int), (size_t)k, s);
    if (k <= 8) label_counts_kernels<uint8_t>(gt, pred, k, Tn, H, W, radius, bsets, counts, T_all, blocks, s);
    else label_counts_kernels<uint32_t>(gt, pred, k, Tn, H, W, radius, bsets, counts, T_all, blocks, s);
}

// ---- one annotation round on the device (round 6): compose -> counts -> quality + selection ------------------------------------------
// gen[t] = the engine's mask of frame t (cropped out of the padded [T][nh][nw] tensor), or the ground truth where the frame is annotated
// (interactions/eval.py:57-60: annotated frames count with their GT mask).  gen is what util/fq_dataset.py:64-84 saves as a state.
// Binary masks: non-zero = object; LABELS: label maps of k objects.  `also`: one more frame (of the T composed) that counts as annotated
// whatever its flag says - the candidate of a trial round, whose flags are the caller's and stay untouched; -1: none.
// `annot` (typed rounds, else null): the flags are annotation TYPES and a frame of type 2 - annotated with clicks or a box - counts with
// the annotator's mask annot[t] (interactions/eval.py:61-64); every other non-zero flag is the ground truth as before.
template <bool LABELS>
__global__ __launch_bounds__(256) void round_compose_kernel(const uint8_t *__restrict__ masks, int nh, int nw, int lh, int lw,
                                                            const uint8_t *__restrict__ gt, const uint8_t *__restrict__ annotated, int k, int T, int H,
                                                            int W, uint8_t *__restrict__ gen, int also, const uint8_t *__restrict__ annot) {
    const long hw = (long)H * W, n = T * hw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int t = (int)(i / hw);
        const int rem = (int)(i - t * hw);
        const int y = rem / W, x = rem - y * W;
        const int flag = annotated[t];
        const uint8_t v = annot && flag == 2 ? annot[i] : flag || t == also ? gt[i] : masks[((long)t * nh + y + lh) * nw + x + lw];
        gen[i] = LABELS ? (uint8_t)label_of(v, k) : (uint8_t)(v != 0);
    }
}

// quality[t] in fp64 with the operations, and their order, of the host path (eva_vos_amd/metrics.py::_scores_from_counts, itself the
// reference's interactions/metrics.py:141-158 / eval.py:62-79): J = inter / union (0 when the union is empty), F = 2 p r / (p + r) with the
// reference's special cases, J&F = 0.5 (J + F); frames whose ground truth is empty get the NO_OBJECT token.  IEEE division / multiplication /
// addition are correctly rounded on the device as on the host, so the values - and therefore the arg-min (first index of the minimum, as
// numpy.argmin) - are bit-identical to the host path's.  One workgroup; T <= a few hundred.
__device__ __forceinline__ double quality_of(const int *__restrict__ c, int j_only) {
    const double j = c[1] == 0 ? 0.0 : __ddiv_rn((double)c[0], (double)c[1]);
    if (j_only) return j;
    const int n_gt = c[2], n_fg = c[3];
    double p, r;
    if (n_fg == 0 && n_gt > 0) { p = 1.0; r = 0.0; }
    else if (n_fg > 0 && n_gt == 0) { p = 0.0; r = 1.0; }
    else if (n_fg == 0 && n_gt == 0) { p = 1.0; r = 1.0; }
    else { p = __ddiv_rn((double)c[5], (double)n_fg); r = __ddiv_rn((double)c[4], (double)n_gt); }
    const double s = __dadd_rn(p, r);
    const double f = s == 0.0 ? 0.0 : __ddiv_rn(__dmul_rn(__dmul_rn(2.0, p), r), s);
    return __dmul_rn(0.5, __dadd_rn(j, f));
}

// first index of the minimum over the workgroup's 256 (best, besti) pairs, each the first minimum of its thread's ascending subsequence
__device__ __forceinline__ void block_argmin(double best, int besti, int *__restrict__ select) {
    __shared__ double sv[256];
    __shared__ int si[256];
    sv[threadIdx.x] = best; si[threadIdx.x] = besti;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double v = sv[threadIdx.x + o]; const int i2 = si[threadIdx.x + o];
            if (v < sv[threadIdx.x] || (v == sv[threadIdx.x] && i2 < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) select[0] = si[0];
}

// object_quality[o][t] = quality_of the counts of object o in frame t, NO_OBJECT where the object is not in the frame's ground truth;
// quality[t] = the mean over the objects that are - added in ascending o, correctly rounded, then one division by their number - or
// NO_OBJECT when there is none; select = first index of the minimum of quality (block_argmin).  The host restatement is
// metrics.label_round_quality.  flags [k][T]: object o is in frame t iff (flags[o][t] != 0) != absent - the label form passes `present`,
// the binary form k = 1, its `noobj` flags with absent = 1, and no object_quality.  With one object the mean is the object's quality to
// the bit: quality_of returns non-negative values (quotients, sums and products of non-negative numbers, never -0.0), for which
// 0.0 + q and q / 1.0 are exact.  One workgroup; T <= a few hundred.
__global__ __launch_bounds__(256) void round_quality_kernel(const int *__restrict__ counts, const uint8_t *__restrict__ flags, int absent, int k, int T,
                                                            int j_only, double no_object, double *__restrict__ object_quality,
                                                            double *__restrict__ quality, int *__restrict__ select) {
    double best = __builtin_inf();
    int besti = 0x7fffffff;
    for (int t = threadIdx.x; t < T; t += 256) {
        double sum = 0.0;
        int cnt = 0;
        for (int o = 0; o < k; ++o) {
            double q = no_object;
            if ((flags[o * T + t] != 0) != (absent != 0)) {
                q = quality_of(counts + ((long)o * T + t) * 6, j_only);
                sum = __dadd_rn(sum, q);
                ++cnt;
            }
            if (object_quality) object_quality[o * T + t] = q;
        }
        const double q = cnt ? __ddiv_rn(sum, (double)cnt) : no_object;
        quality[t] = q;
        if (q < best) { best = q; besti = t; }                               // ascending t per thread: the first minimum of its subsequence
    }
    block_argmin(best, besti, select);
}

// One round, three enqueues.  masks / gt / annotated / gen / scratch / counts point at the FIRST of the Tn frames to (re)compose and count,
// frame t0 of the clip; the quality and the arg-min cover all T_all frames, whose counts start t0 frames earlier: the caller passes the
// counts of frame t0, and flags, object_quality and quality as whole-clip arrays.  k = 0: binary masks (flags = noobj [T_all], scratch =
// the boundary map, no object_quality); k >= 1: label maps of k objects (flags = present [k][T_all], scratch = the object sets, counts
// [k][T_all][6]).
void round_score_launch(const uint8_t *masks, int nh, int nw, int lh, int lw, const uint8_t *gt, const uint8_t *annotated, const uint8_t *flags, int k,
                        int Tn, int H, int W, int radius, double no_object, uint8_t *gen, void *scratch, int *counts, int T_all,
                        double *object_quality, double *quality, int *select, hipStream_t s, int t0, const uint8_t *annot) {
    const long n = (long)Tn * H * W;
    const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k ? round_compose_kernel<true> : round_compose_kernel<false>, dim3(blocks), dim3(256), 0, s, masks, nh, nw, lh, lw, gt, annotated, k,
                       Tn, H, W, gen, -1, annot);
    if (k) label_counts_launch(gt, gen, k, Tn, H, W, radius, scratch, counts, T_all, s);
    else jf_counts_launch(gt, gen, Tn, H, W, radius, (uint8_t *)scratch, counts, s);
    hipLaunchKernelGGL(round_quality_kernel, dim3(1), dim3(256), 0, s, counts - (long)t0 * 6, flags, k ? 0 : 1, k ? k : 1, T_all, radius < 0 ? 1 : 0,
                       no_object, k ? object_quality : nullptr, quality, select);
}

// ---- a trial round: the quality row of "annotate `candidate` next", beside the caller's rounds ------------------------------------------
// quality[t] for all T frames from TWO count arrays: span [(t1 - t0)][6] - counted just now over the frames the trial can have changed -
// for t in [t0, t1), base [T][6] - the caller's last round, read only - for every other frame; NO_OBJECT for flagged frames.  The value is
// quality_of, which is what round_quality_kernel writes for one object (its mean over one object is exact, see there).
__global__ __launch_bounds__(256) void trial_quality_kernel(const int *__restrict__ base, const int *__restrict__ span, int t0, int t1,
                                                            const uint8_t *__restrict__ noobj, int T, int j_only, double no_object,
                                                            double *__restrict__ quality) {
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += gridDim.x * 256) {
        const int *c = t >= t0 && t < t1 ? span + (long)(t - t0) * 6 : base + (long)t * 6;
        quality[t] = noobj[t] ? no_object : quality_of(c, j_only);
    }
}

// Compose + count frames [t0, t1) into the caller's scratch (masks / gt / annotated point at frame t0, as in round_score_launch; noobj and
// base are whole-clip arrays), then one quality row.  `also`: the candidate's index inside the span, -1 when it lies outside.  Writes
// span_gen, bmap, span_counts and quality, nothing else.
void trial_score_launch(const uint8_t *masks, int nh, int nw, int lh, int lw, const uint8_t *gt, const uint8_t *annotated, const uint8_t *noobj, int also,
                        int T_all, int H, int W, int t0, int t1, int radius, double no_object, const int *base, uint8_t *span_gen, uint8_t *bmap,
                        int *span_counts, double *quality, hipStream_t s) {
    const int Tn = t1 - t0;
    if (Tn > 0) {
        const long n = (long)Tn * H * W;
        const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(round_compose_kernel<false>, dim3(blocks), dim3(256), 0, s, masks, nh, nw, lh, lw, gt, annotated, 0, Tn, H, W, span_gen, also,
                           (const uint8_t *)nullptr);
        jf_counts_launch(gt, span_gen, Tn, H, W, radius, bmap, span_counts, s);
    }
    hipLaunchKernelGGL(trial_quality_kernel, dim3((T_all + 255) / 256), dim3(256), 0, s, base, span_counts, t0, t1, noobj, T_all, radius < 0 ? 1 : 0,
                       no_object, quality);
}

}  // namespace stcn
