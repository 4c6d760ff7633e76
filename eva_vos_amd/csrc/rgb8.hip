// rgb8.hip - normalised fp32 frames as the 8-bit RGB images the annotation dataset stores: clip fp32 [T,3,H,W] -> out uint8 [n,H,W,3], per frame
// (x - min) / max(max - min, 1e-8) * 255, truncated (datasets/helpers.py:4-17 `im_normalize(tens2image(.))`, generate_annotation_dataset.py:
// 170-174), min and max over the whole [3,H,W] frame, every operation a correctly rounded fp32 one - what NumPy computes on the host.
//
// Three launches, all on a (blocks, n) grid so that one call serves every row of a session:
//   init   : scratch [n][2] = { key(+inf), key(-inf) }
//   pass 1 : per-frame min / max.  16-byte loads over the aligned body of the frame (a frame starts wherever 3 * H * W floats put it: up to
//            three scalar head elements, up to three scalar tail elements), a wave reduction, LDS across the waves, then ONE integer atomicMin
//            and ONE atomicMax per workgroup on an order-preserving 32-bit key of the float.
//   pass 2 : four pixels per thread: three planes x four floats in, 12 bytes out as three 4-byte stores where the frame's first output byte is
//            4-byte aligned and the run is whole, byte stores otherwise.
// Inputs are finite (the min / max of a frame with a NaN is not NumPy's).  -0.0 and +0.0 order as -0.0 < +0.0 in the key; which of the two a
// frame's minimum is changes no output byte (x - min differs in the sign of a zero only, which truncates to 0).
#include <cmath>

#include "kernels.h"

namespace stcn {

namespace {

constexpr int RGB8_THREADS = 256;
constexpr int RGB8_LOADS = 4;                                   // pass 1: float4 loads per thread
constexpr int RGB8_BLOCK_VECS = RGB8_THREADS * RGB8_LOADS;      // pass 1: float4s of the aligned body per workgroup (4096 floats)
constexpr int RGB8_RUN = 4;                                     // pass 2: pixels per thread

// unsigned keys that order as the floats do: negative floats with all bits flipped, the others with the sign bit set
__device__ __forceinline__ unsigned rgb8_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rgb8_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ void rgb8_init_kernel(unsigned *__restrict__ keys, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        keys[2 * i] = 0xFFFFFFFFu;                                // above every key: the minimum
        keys[2 * i + 1] = 0u;                                     // below every key: the maximum
    }
}

// grid (workgroups of RGB8_BLOCK_VECS float4s of the body, n).  head: floats before the frame's first 16-byte boundary; workgroup 0 also takes
// them and the tail behind the last whole float4.
__global__ __launch_bounds__(RGB8_THREADS) void rgb8_minmax_kernel(const float *__restrict__ clip, int T, int N, const int *__restrict__ frames,
                                                                   unsigned *__restrict__ keys) {
    const int i = blockIdx.y;
    const int f = frames ? frames[i] : i;
    if ((unsigned)f >= (unsigned)T) return;                        // nothing of such a frame is read
    const float *frame = clip + (size_t)f * N;
    int head = (int)((16 - ((uintptr_t)frame & 15)) & 15) / 4;
    if (head > N) head = N;
    const int nvec = (N - head) / 4;
    const float4 *body = reinterpret_cast<const float4 *>(frame + head);
    float lo = INFINITY, hi = -INFINITY;
    const int v0 = blockIdx.x * RGB8_BLOCK_VECS + threadIdx.x;
#pragma unroll
    for (int j = 0; j < RGB8_LOADS; ++j) {
        const int v = v0 + j * RGB8_THREADS;
        if (v < nvec) {
            const float4 x = body[v];
            lo = fminf(fminf(lo, x.x), fminf(x.y, fminf(x.z, x.w)));
            hi = fmaxf(fmaxf(hi, x.x), fmaxf(x.y, fmaxf(x.z, x.w)));
        }
    }
    if (blockIdx.x == 0) {
        const int tail0 = head + 4 * nvec;
        const int t = threadIdx.x;
        int e = -1;
        if (t < head) e = t;                                      // at most three each
        else if (t >= 64 && t - 64 < N - tail0) e = tail0 + t - 64;
        if (e >= 0) {
            const float x = frame[e];
            lo = fminf(lo, x);
            hi = fmaxf(hi, x);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    __shared__ float wave_lo[RGB8_THREADS / 64], wave_hi[RGB8_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        wave_lo[threadIdx.x >> 6] = lo;
        wave_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < RGB8_THREADS / 64; ++w) {
            lo = fminf(lo, wave_lo[w]);
            hi = fmaxf(hi, wave_hi[w]);
        }
        atomicMin(&keys[2 * i], rgb8_key(lo));
        atomicMax(&keys[2 * i + 1], rgb8_key(hi));
    }
}

__device__ __forceinline__ unsigned rgb8_byte(float x, float lo, float d) {
#pragma clang fp contract(off)
    return (unsigned)(int)__fmul_rn(__fdiv_rn(__fsub_rn(x, lo), d), 255.f);        // 0..255: no contraction, IEEE division, truncation
}

// grid (runs of RGB8_RUN pixels, n).  out_vec: every frame's first output byte is 4-byte aligned (out is, and 3 * H * W is a multiple of 4, or
// n is 1), so the 12 bytes of a whole run are three aligned words.
__global__ __launch_bounds__(RGB8_THREADS) void rgb8_store_kernel(const float *__restrict__ clip, int T, int HW, const int *__restrict__ frames,
                                                                  const unsigned *__restrict__ keys, int out_vec, uint8_t *__restrict__ out) {
    const int p0 = (blockIdx.x * RGB8_THREADS + threadIdx.x) * RGB8_RUN;
    if (p0 >= HW) return;
    const int i = blockIdx.y;
    const int f = frames ? frames[i] : i;
    const bool ok = (unsigned)f < (unsigned)T;
    const bool whole = p0 + RGB8_RUN <= HW;
    unsigned b[3][RGB8_RUN];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < RGB8_RUN; ++j) b[c][j] = 0u;
    if (ok) {                                                       // a frame outside the clip is not read: its image is zeros
        const float lo = rgb8_unkey(keys[2 * i]);
        const float d = fmaxf(__fsub_rn(rgb8_unkey(keys[2 * i + 1]), lo), 1e-8f);
        const float *frame = clip + (size_t)f * 3 * HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *src = frame + (size_t)c * HW + p0;
            float x[RGB8_RUN] = {0.f, 0.f, 0.f, 0.f};
            if (whole && ((uintptr_t)src & 15) == 0) {
                const float4 v = *reinterpret_cast<const float4 *>(src);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < RGB8_RUN; ++j)
                    if (p0 + j < HW) x[j] = src[j];
            }
#pragma unroll
            for (int j = 0; j < RGB8_RUN; ++j) b[c][j] = rgb8_byte(x[j], lo, d);
        }
    }
    uint8_t *o = out + ((size_t)i * HW + p0) * 3;
    if (whole && out_vec) {                                         // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3, little-endian words
        unsigned *w = reinterpret_cast<unsigned *>(o);
        w[0] = b[0][0] | b[1][0] << 8 | b[2][0] << 16 | b[0][1] << 24;
        w[1] = b[1][1] | b[2][1] << 8 | b[0][2] << 16 | b[1][2] << 24;
        w[2] = b[2][2] | b[0][3] << 8 | b[1][3] << 16 | b[2][3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < RGB8_RUN; ++j)
            if (p0 + j < HW) {
                o[3 * j] = (uint8_t)b[0][j];
                o[3 * j + 1] = (uint8_t)b[1][j];
                o[3 * j + 2] = (uint8_t)b[2][j];
            }
    }
}

}  // namespace

void frames_to_rgb8_launch(const float *clip, int T, int H, int W, const int *frames, int n, void *scratch, uint8_t *out, hipStream_t s) {
    const int HW = H * W, N = 3 * HW;
    unsigned *keys = static_cast<unsigned *>(scratch);
    rgb8_init_kernel<<<(n + RGB8_THREADS - 1) / RGB8_THREADS, RGB8_THREADS, 0, s>>>(keys, n);
    // the body of a frame has at most N / 4 float4s whatever its head: one workgroup at least, for the head and the tail
    const int groups = (N / 4 + RGB8_BLOCK_VECS - 1) / RGB8_BLOCK_VECS;
    const dim3 grid1((unsigned)(groups > 0 ? groups : 1), (unsigned)n);
    rgb8_minmax_kernel<<<grid1, RGB8_THREADS, 0, s>>>(clip, T, N, frames, keys);
    const int runs = (HW + RGB8_RUN - 1) / RGB8_RUN;
    const int out_vec = (uintptr_t)out % 4 == 0 && (n == 1 || N % 4 == 0);
    const dim3 grid2((unsigned)((runs + RGB8_THREADS - 1) / RGB8_THREADS), (unsigned)n);
    rgb8_store_kernel<<<grid2, RGB8_THREADS, 0, s>>>(clip, T, HW, frames, keys, out_vec, out);
}

}  // namespace stcn
