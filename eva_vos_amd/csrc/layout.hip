// layout.hip - the reference's NCHW tensors <-> the engine's [rows][channels], on the device.
// The stage API (stages.cpp) takes and returns every tensor as the reference's modules do (prop_net.py:153-211: [1,C,h,w] features, a
// [1,CK,T,h,w] key bank); the convolutions and the memory read work on rows.  Both directions are one batched 2-D transpose.
#include "kernels.h"

namespace stcn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// src [B][M][src_ld] (element (m, n) at m * src_ld + n, n < N) -> dst [B][N][dst_ld] (element (n, m) at n * dst_ld + m).
// One workgroup moves a 64 x 64 tile through LDS in 4-byte LDS accesses.  Row pitch 65 dwords: the column-wise stores of the load phase
// (lane = 16 quads of one source row, 4 rows per wave; bank = (4 * quad + i + row) mod 32) are 2-way, which a 4-byte LDS store does not
// pay for; the row-wise reads of the store phase (bank = (row + 4 * quad + i) mod 32) are 2-way as well and pay double.  Without the
// padding both would be 16-way.  HBM-bound all the same: 32 KB cross the CU per tile (~3000 cycles at ~10 B/clk/CU) against ~500 LDS cycles.
// VS / VD: the rows of src / dst start on 16-byte boundaries (base, leading dimension and batch stride multiples of 4 floats): whole
// quads move as one 16-byte access, a quad cut by a ragged edge element by element.  Otherwise (a T-slice of a bank whose planes are
// h16 * w16 * Tm floats apart, 350 for a 7 x 10 key frame) that side moves in 4-byte accesses, still over whole cache lines per wave.
constexpr int TR_TILE = 64, TR_PITCH = TR_TILE + 1;
template <bool VS, bool VD>
__global__ __launch_bounds__(256) void transpose_kernel(const float *__restrict__ src, float *__restrict__ dst, int M, int N, long src_ld,
                                                        long dst_ld, long src_bs, long dst_bs) {
    __shared__ float tile[TR_TILE * TR_PITCH];           // tile[n][m]
    const int n0 = blockIdx.x * TR_TILE, m0 = blockIdx.y * TR_TILE;
    src += (long)blockIdx.z * src_bs;
    dst += (long)blockIdx.z * dst_bs;
    const int q = threadIdx.x & 15, r = threadIdx.x >> 4;      // quad within a tile row, tile row (16 per pass)
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int m = m0 + r + 16 * pass, n = n0 + 4 * q;
        if (m >= M || n >= N) continue;
        const float *p = src + (long)m * src_ld + n;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (VS && n + 3 < N) {
            const f32x4 x = *reinterpret_cast<const f32x4 *>(p);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (n + i < N) v[i] = p[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(4 * q + i) * TR_PITCH + r + 16 * pass] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int n = n0 + r + 16 * pass, m = m0 + 4 * q;
        if (n >= N || m >= M) continue;
        const float *t = tile + (r + 16 * pass) * TR_PITCH + 4 * q;
        float *p = dst + (long)n * dst_ld + m;
        if (VD && m + 3 < M) {
            const f32x4 x = {t[0], t[1], t[2], t[3]};
            *reinterpret_cast<f32x4 *>(p) = x;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (m + i < M) p[i] = t[i];
        }
    }
}

static bool quad_aligned(const void *p, long ld, long bs) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0 && bs % 4 == 0; }

static void transpose_launch(const float *src, float *dst, int B, int M, int N, long src_ld, long dst_ld, long src_bs, long dst_bs, hipStream_t s) {
    const dim3 grid((N + TR_TILE - 1) / TR_TILE, (M + TR_TILE - 1) / TR_TILE, B);
    const bool vs = quad_aligned(src, src_ld, src_bs), vd = quad_aligned(dst, dst_ld, dst_bs);
    auto *k = vs ? (vd ? transpose_kernel<true, true> : transpose_kernel<true, false>) : (vd ? transpose_kernel<false, true> : transpose_kernel<false, false>);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, src, dst, M, N, src_ld, dst_ld, src_bs, dst_bs);
}

void planes_to_rows_launch(const float *planes, long ld, long planes_bs, float *rows, long rows_bs, int B, int R, int C, hipStream_t s) {
    transpose_launch(planes, rows, B, C, R, ld, C, planes_bs, rows_bs, s);
}
void rows_to_planes_launch(const float *rows, long rows_bs, float *planes, long ld, long planes_bs, int B, int R, int C, hipStream_t s) {
    transpose_launch(rows, planes, B, R, C, C, ld, rows_bs, planes_bs, s);
}

}  // namespace stcn
