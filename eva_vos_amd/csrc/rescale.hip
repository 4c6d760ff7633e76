// rescale.hip - a clip at a working resolution: frames down before the engine sees them, masks up after it has spoken.
//
// prob_upsample_argmax : prob fp32 [k1,T,1,nh,nw] (the engine's padded probabilities) -> out uint8 [T,H,W].  Per frame t in [t0,t1) the
//   unpadded h x w window at (lh, lw) of every channel is interpolated bilinearly (align_corners=False: src = (dst + 0.5) * in / out - 0.5,
//   clamped below at 0, i1 = min(i0 + 1, in - 1), in fp32 as torch evaluates it) to H x W and the arg-max over the channels is written as one
//   byte, the lowest index winning a tie (a strict `>` against the running best).  The k1 * T * H * W interpolated floats never exist.  The
//   padded rows and columns are never read; frames outside [t0,t1) are never written.  One launch: a thread makes 4 adjacent bytes of a row -
//   per-axis source indices and weights once, then a loop over the channels whose taps are cache hits of its neighbours' - and stores them as
//   one 32-bit word where the address allows it (rows of an odd W start at any byte), else byte by byte.
//
// frames_downsample_aa : src fp32 [planes,H,W] -> dst fp32 [planes,h,w], h <= H, w <= W: antialiased bicubic (A = -0.5, align_corners=False),
//   separable - a horizontal and a vertical 1-D pass.  The taps of an axis (first source index, count, weights normalised over the part of
//   the support that lies inside the image) are a function of (in, out) alone: built on the host in fp64, uploaded once per pair and device
//   and kept; the kernel computes no cubic.  A workgroup makes a 64 x 32 output tile of one plane: it walks the source rows the tile reads in
//   chunks of 16, filters each chunk horizontally into an LDS tile [16][64] and adds the chunk's share to the vertical sums held in
//   registers, so neither LDS nor registers depend on the scale - every loop over taps is a loop.  Products and sums are fp64 (weights too)
//   and a value is rounded to fp32 once, at the store: a constant image stays constant.
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "kernels.h"

namespace stcn {

namespace {

constexpr int UP_THREADS = 256;
constexpr int UP_RUN = 4;                   // outputs per thread: one 32-bit word
constexpr int UP_ROWS = UP_THREADS / 64;    // output rows per workgroup, one per wave
constexpr int UP_COLS = 64 * UP_RUN;        // output columns per workgroup

// grid (tiles of UP_ROWS x UP_COLS outputs, row-major, frames).  sy / sx: (float)in / out, computed once on the host.
__global__ __launch_bounds__(UP_THREADS) void prob_upsample_argmax_kernel(const float *__restrict__ prob, int k1, int T, int nh, int nw, int lh, int lw,
                                                                          int h, int w, int H, int W, float sy, float sx, int t0, int tiles_x,
                                                                          uint8_t *__restrict__ out) {
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int y = tile_y * UP_ROWS + (threadIdx.x >> 6);
    const int x0 = tile_x * UP_COLS + (threadIdx.x & 63) * UP_RUN;
    if (y >= H || x0 >= W) return;
    const int t = t0 + blockIdx.y;
    const float fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f);
    int y0 = (int)fy;
    y0 = y0 < h - 1 ? y0 : h - 1;
    const int y1 = y0 < h - 1 ? y0 + 1 : h - 1;
    const float ly = fy - (float)y0, hy = 1.f - ly;
    int xa[UP_RUN], xb[UP_RUN];
    float lx[UP_RUN];
#pragma unroll
    for (int j = 0; j < UP_RUN; ++j) {
        const int x = x0 + j < W ? x0 + j : W - 1;                 // a row's tail: computed like the last pixel, not stored
        const float fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
        int a = (int)fx;
        a = a < w - 1 ? a : w - 1;
        xa[j] = a;
        xb[j] = a < w - 1 ? a + 1 : w - 1;
        lx[j] = fx - (float)a;
    }
    const size_t plane = (size_t)nh * nw, chan = (size_t)T * plane;
    const float *r0 = prob + (size_t)t * plane + (size_t)(lh + y0) * nw + lw;
    const float *r1 = prob + (size_t)t * plane + (size_t)(lh + y1) * nw + lw;
    float best[UP_RUN];
    unsigned arg[UP_RUN];
    for (int c = 0; c < k1; ++c, r0 += chan, r1 += chan) {
#pragma unroll
        for (int j = 0; j < UP_RUN; ++j) {
            const float hx = 1.f - lx[j];
            const float v = hy * (hx * r0[xa[j]] + lx[j] * r0[xb[j]]) + ly * (hx * r1[xa[j]] + lx[j] * r1[xb[j]]);
            if (c == 0 || v > best[j]) {
                best[j] = v;
                arg[j] = (unsigned)c;
            }
        }
    }
    uint8_t *o = out + ((size_t)t * H + y) * W + x0;
    if (x0 + UP_RUN <= W && ((uintptr_t)o & 3) == 0) {
        *reinterpret_cast<unsigned *>(o) = arg[0] | arg[1] << 8 | arg[2] << 16 | arg[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < UP_RUN; ++j)
            if (x0 + j < W) o[j] = (uint8_t)arg[j];
    }
}

// ---- the taps of one axis -------------------------------------------------------------------------------------------------------------
struct AxisTaps {
    const int *first = nullptr;             // [out] first source index
    const int *count = nullptr;             // [out] taps, 1 .. taps
    const double *weight = nullptr;         // [out][taps] normalised; entries behind `count` are not read
    int taps = 0;                           // 2 * ceil(support) + 1: a bound on count that grows with the scale
};

double cubic(double x) {                    // Keys' kernel, A = -0.5
    constexpr double a = -0.5;
    x = std::fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

struct TapsKey {
    int device, in, out;
    bool operator<(const TapsKey &o) const { return std::tie(device, in, out) < std::tie(o.device, o.in, o.out); }
};
std::mutex taps_lock;
std::map<TapsKey, AxisTaps> taps_cache;     // lives as long as the process: 4 * in + 3 * out doubles per pair at most

// The table of (in -> out) on the current device, from the cache or built and uploaded now (a blocking copy, once per pair).
hipError_t axis_taps(int in, int out, AxisTaps *res) {
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(taps_lock);
    const TapsKey key{device, in, out};
    auto hit = taps_cache.find(key);
    if (hit != taps_cache.end()) {
        *res = hit->second;
        return hipSuccess;
    }
    const double scale = (double)in / out;
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0, inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    const int taps = (int)std::ceil(support) * 2 + 1;
    std::vector<int> first(out), count(out);
    std::vector<double> weight((size_t)out * taps, 0.0);
    for (int i = 0; i < out; ++i) {
        const double center = scale * (i + 0.5);
        const long lo = std::max((long)(center - support + 0.5), 0L);
        long n = std::min((long)(center + support + 0.5), (long)in) - lo;
        n = std::min(std::max(n, 1L), (long)taps);
        double *wt = &weight[(size_t)i * taps], total = 0.0;
        for (long j = 0; j < n; ++j) total += wt[j] = cubic((j + lo - center + 0.5) * inv);
        for (long j = 0; j < n; ++j) wt[j] /= total;
        first[i] = (int)lo;
        count[i] = (int)n;
    }
    const size_t wbytes = weight.size() * sizeof(double), ibytes = (size_t)out * sizeof(int);
    char *dev = nullptr;
    if ((e = hipMalloc((void **)&dev, wbytes + 2 * ibytes)) != hipSuccess) return e;
    if ((e = hipMemcpy(dev, weight.data(), wbytes, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(dev + wbytes, first.data(), ibytes, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(dev + wbytes + ibytes, count.data(), ibytes, hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipFree(dev);
        return e;
    }
    AxisTaps t;
    t.weight = reinterpret_cast<const double *>(dev);
    t.first = reinterpret_cast<const int *>(dev + wbytes);
    t.count = reinterpret_cast<const int *>(dev + wbytes + ibytes);
    t.taps = taps;
    taps_cache[key] = t;
    *res = t;
    return hipSuccess;
}

constexpr int DOWN_THREADS = 256;
constexpr int DOWN_TW = 64;                 // output columns per workgroup: one per lane
constexpr int DOWN_GROUPS = DOWN_THREADS / 64;
constexpr int DOWN_TH = 32;                 // output rows per workgroup
constexpr int DOWN_OWN = DOWN_TH / DOWN_GROUPS;     // output rows per thread: oy0 + wave + DOWN_GROUPS * i
constexpr int DOWN_CHUNK = 16;              // source rows filtered horizontally per step
constexpr int DOWN_HROWS = DOWN_CHUNK / DOWN_GROUPS; // of which a thread filters these many: r0 + wave + DOWN_GROUPS * m

// grid (tiles of DOWN_TH x DOWN_TW outputs, row-major, planes)
__global__ __launch_bounds__(DOWN_THREADS) void frames_downsample_aa_kernel(const float *__restrict__ src, int H, int W, int h, int w, AxisTaps tx, AxisTaps ty,
                                                                            int tiles_x, float *__restrict__ dst) {
    __shared__ double rows[DOWN_CHUNK][DOWN_TW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int ox = tile_x * DOWN_TW + lane, oy0 = tile_y * DOWN_TH;
    const float *plane = src + (size_t)blockIdx.y * H * W;
    const bool col = ox < w;
    const int xfirst = col ? tx.first[ox] : 0, xcount = col ? tx.count[ox] : 0;
    const double *wx = tx.weight + (size_t)(col ? ox : 0) * tx.taps;
    int yfirst[DOWN_OWN], ycount[DOWN_OWN];
    double acc[DOWN_OWN];
#pragma unroll
    for (int i = 0; i < DOWN_OWN; ++i) {
        const int oy = oy0 + wave + DOWN_GROUPS * i;
        yfirst[i] = oy < h ? ty.first[oy] : 0;
        ycount[i] = oy < h ? ty.count[oy] : 0;
        acc[i] = 0.0;
    }
    // first and first + count do not decrease along an axis: the tile reads the source rows [r_begin, r_end)
    const int oy_last = (oy0 + DOWN_TH < h ? oy0 + DOWN_TH : h) - 1;
    const int r_begin = ty.first[oy0], r_end = ty.first[oy_last] + ty.count[oy_last];
    for (int r0 = r_begin; r0 < r_end; r0 += DOWN_CHUNK) {
        const float *in[DOWN_HROWS];
        double sum[DOWN_HROWS];
#pragma unroll
        for (int m = 0; m < DOWN_HROWS; ++m) {
            const int r = r0 + wave + DOWN_GROUPS * m;
            in[m] = plane + (size_t)(r < r_end ? r : r_end - 1) * W + xfirst;       // behind the last row: a row that exists, a sum nobody reads
            sum[m] = 0.0;
        }
        for (int j = 0; j < xcount; ++j) {
            const double wj = wx[j];
#pragma unroll
            for (int m = 0; m < DOWN_HROWS; ++m) sum[m] = fma(wj, (double)in[m][j], sum[m]);
        }
#pragma unroll
        for (int m = 0; m < DOWN_HROWS; ++m) rows[wave + DOWN_GROUPS * m][lane] = sum[m];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < DOWN_OWN; ++i) {
            const int lo = yfirst[i] > r0 ? yfirst[i] : r0;
            const int end = yfirst[i] + ycount[i], hi = end < r0 + DOWN_CHUNK ? end : r0 + DOWN_CHUNK;
            const int oy = oy0 + wave + DOWN_GROUPS * i;
            const double *wy = ty.weight + (size_t)(oy < h ? oy : 0) * ty.taps;
            for (int r = lo; r < hi; ++r) acc[i] = fma(wy[r - yfirst[i]], rows[r - r0][lane], acc[i]);
        }
        __syncthreads();
    }
    float *o = dst + (size_t)blockIdx.y * h * w;
#pragma unroll
    for (int i = 0; i < DOWN_OWN; ++i) {
        const int oy = oy0 + wave + DOWN_GROUPS * i;
        if (col && oy < h) o[(size_t)oy * w + ox] = (float)acc[i];
    }
}

constexpr int GRID_Y_MAX = 65535;

}  // namespace

void prob_upsample_argmax_launch(const float *prob, int k1, int T, int nh, int nw, int lh, int lw, int h, int w, int H, int W, int t0, int t1,
                                 uint8_t *out, hipStream_t s) {
    const int tiles_x = (W + UP_COLS - 1) / UP_COLS, tiles_y = (H + UP_ROWS - 1) / UP_ROWS;
    for (int t = t0; t < t1; t += GRID_Y_MAX) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(t1 - t < GRID_Y_MAX ? t1 - t : GRID_Y_MAX));
        prob_upsample_argmax_kernel<<<grid, UP_THREADS, 0, s>>>(prob, k1, T, nh, nw, lh, lw, h, w, H, W, (float)h / (float)H, (float)w / (float)W, t,
                                                                tiles_x, out);
    }
}

hipError_t frames_downsample_aa_launch(const float *src, int planes, int H, int W, int h, int w, float *dst, hipStream_t s) {
    AxisTaps tx, ty;
    hipError_t e = axis_taps(W, w, &tx);
    if (e == hipSuccess) e = axis_taps(H, h, &ty);
    if (e != hipSuccess) return e;
    const int tiles_x = (w + DOWN_TW - 1) / DOWN_TW, tiles_y = (h + DOWN_TH - 1) / DOWN_TH;
    for (int p = 0; p < planes; p += GRID_Y_MAX) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(planes - p < GRID_Y_MAX ? planes - p : GRID_Y_MAX));
        frames_downsample_aa_kernel<<<grid, DOWN_THREADS, 0, s>>>(src + (size_t)p * H * W, H, W, h, w, tx, ty, tiles_x, dst + (size_t)p * h * w);
    }
    return hipSuccess;
}

}  // namespace stcn
