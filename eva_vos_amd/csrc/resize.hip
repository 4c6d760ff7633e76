// resize.hip - the evaluated masks of a round as network input: uint8 [T,H,W] -> fp32 [n,channels,out_h,out_w], nearest-resized, the value of
// the byte as a float (what `.float()` gives, so label maps pass too), every channel plane the same (interactions/policies.py:12-18,44-45,
// mulitple_annotations.py:287-297: torchvision Resize NEAREST + repeat 'b h w -> b 3 h w').  One launch: only the sampled bytes are read, all
// channel planes are written from that one read, four adjacent outputs of a plane per thread as one 16-byte store.
//
// The source index is torch's `nearest` rule, per axis and in fp32: min((int)floorf(dst * ((float)in / out)), in - 1); the scale is computed
// once on the host, in fp32, and travels as a kernel argument.
#include <cmath>

#include "kernels.h"

namespace stcn {

namespace {

constexpr int RESIZE_THREADS = 256;
constexpr int RESIZE_RUN = 4;               // outputs per thread: one float4

__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

// grid (groups of RESIZE_RUN outputs of a plane, n).  `vec`: out is 16-byte aligned and the plane is a multiple of 4 floats, so every group of
// every plane is an aligned float4; else scalar stores with the plane's end checked.  A frame index outside [0,T) is never read: its planes
// are filled with NaN.
__global__ __launch_bounds__(RESIZE_THREADS) void masks_resize_nearest_kernel(const uint8_t *__restrict__ src, int T, int H, int W,
                                                                              const int *__restrict__ frames, int out_h, int out_w, int channels,
                                                                              float scale_y, float scale_x, int vec, float *__restrict__ out) {
    const int plane = out_h * out_w;
    const int p0 = (blockIdx.x * RESIZE_THREADS + threadIdx.x) * RESIZE_RUN;
    if (p0 >= plane) return;
    const int i = blockIdx.y;
    const int f = frames ? frames[i] : i;
    const bool ok = (unsigned)f < (unsigned)T;
    const uint8_t *frame = src + (size_t)(ok ? f : 0) * H * W;
    float v[RESIZE_RUN];
#pragma unroll
    for (int j = 0; j < RESIZE_RUN; ++j) {
        const int p = p0 + j;
        v[j] = 0.f;
        if (p < plane) {
            const int y = p / out_w, x = p - y * out_w;
            v[j] = ok ? (float)frame[(size_t)nearest_src(y, scale_y, H) * W + nearest_src(x, scale_x, W)] : NAN;
        }
    }
    float *o = out + (size_t)i * channels * plane + p0;
    for (int c = 0; c < channels; ++c, o += plane) {
        if (vec) {
            *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < RESIZE_RUN; ++j)
                if (p0 + j < plane) o[j] = v[j];
        }
    }
}

}  // namespace

void masks_resize_nearest_launch(const uint8_t *src, int T, int H, int W, const int *frames, int n, int out_h, int out_w, int channels, float *out,
                                 hipStream_t s) {
    const int plane = out_h * out_w;
    const int groups = (plane + RESIZE_RUN - 1) / RESIZE_RUN;
    const int vec = plane % RESIZE_RUN == 0 && (uintptr_t)out % 16 == 0;
    const dim3 grid((unsigned)((groups + RESIZE_THREADS - 1) / RESIZE_THREADS), (unsigned)n);
    masks_resize_nearest_kernel<<<grid, RESIZE_THREADS, 0, s>>>(src, T, H, W, frames, out_h, out_w, channels, (float)H / (float)out_h,
                                                                (float)W / (float)out_w, vec, out);
}

}  // namespace stcn
