// robot.hip - the simulated user of the mixed-annotation sessions on the GPU: where would a person click to correct `pred` towards `gt`
// (robots/click_robot.py:14-99), the box of a mask (robots/bbox_robot.py:11-16), and which of a segmenter's candidates is closest to a target
// (annotator/annotator.py:38-57 with interactions/metrics.py:9-19).  Integer-exact; every call enqueues only, and the number of launches of
// a call depends on (H, W) and the mode alone.
//
// Connected components (8-connectivity) of the three-valued error map 0 = agree, 1 = false positive, 2 = false negative; neighbours join
// only inside a class, so one labelling serves both regions.  Union-find with "the parent's index is never above the child's": a root is the
// smallest linear index of its set, which is the label the selection needs (the raster-first pixel of the component).
//   ccl_tile_kernel    : union-find of a 32 x 32 tile in LDS, then parent[i] = the global index of the tile-local root
//   ccl_merge_kernel   : the pixel pairs across tile borders, in global memory (find + atomicMin)
//   ccl_flatten_kernel : parent[i] = root, size[root] += 1
// No workgroup waits for another: a union is a loop of find + atomicMin in which max(a, b) falls with every step, a find walks strictly
// decreasing indices - both end after at most H * W steps whatever the other threads do, and the loops carry that bound.
#include <algorithm>
#include <climits>

#include "kernels.h"

namespace stcn {

namespace {

constexpr int TILE_W = 32, TILE_H = 32, TILE_PX = TILE_W * TILE_H;
constexpr int RUN = 16;                 // consecutive pixels of one thread in the flatten pass: one size atomic per run and root

using u64 = unsigned long long;

// what the kernels of one call hand to each other, at the head of the scratch (zeroed by the call's memset)
struct RobotHdr {
    u64 best[2];        // per class (0 = false positive, 1 = false negative): size << 24 | (2^24 - 1 - root) of the largest component; atomicMax
    u64 sum[4];         // sum of y, sum of x over the pixels of the false positive's best component, then the false negative's
    u64 min_d2;         // nearest-object-pixel search: smallest squared distance to (tx, ty) ...
    unsigned min_idx;   // ... and the first pixel in raster order that has it
    int ncomp[2];       // components per class
    int gt_count;       // object pixels (middle click)
    int need;           // 1: the click at (tx, ty) is not on the object, search the nearest object pixel
    int tx, ty;
    int fp_x, fp_y, fn_x, fn_y, mid_x, mid_y, mid_valid;
};
constexpr size_t HDR_BYTES = 256;
static_assert(sizeof(RobotHdr) <= HDR_BYTES, "the header has its 256 bytes");

struct RobotScratch {
    RobotHdr *hdr;
    int *hist_y, *hist_x;       // [H], [W]: object pixels per row / column (middle click)
    int *parent, *size;         // [H*W] each
    size_t zero_bytes;          // header + histograms, zeroed per call
};

inline size_t hist_bytes(int H, int W) { return ((size_t)(H + W) * sizeof(int) + 15) / 16 * 16; }

inline RobotScratch carve(void *scratch, int H, int W) {
    char *p = static_cast<char *>(scratch);
    const size_t n = (size_t)H * W;
    RobotScratch s;
    s.hdr = reinterpret_cast<RobotHdr *>(p);
    s.hist_y = reinterpret_cast<int *>(p + HDR_BYTES);
    s.hist_x = s.hist_y + H;
    s.zero_bytes = HDR_BYTES + hist_bytes(H, W);
    s.parent = reinterpret_cast<int *>(p + s.zero_bytes);
    s.size = s.parent + n;
    return s;
}

__device__ __forceinline__ int error_class(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, long i) {
    const int p = pred[i] != 0, g = gt[i] != 0;
    return p == g ? 0 : (p ? 1 : 2);
}

// ---- union-find.  SCOPE: workgroup for the LDS table of a tile, agent for the table in global memory (loads that bypass the CU's L1) ----
template <int SCOPE> __device__ __forceinline__ int uf_find(int *tab, int a, int bound) {
    for (int step = 0; step < bound; ++step) {                  // parent <= child: at most `bound` strictly decreasing steps
        const int p = __hip_atomic_load(tab + a, __ATOMIC_RELAXED, SCOPE);
        if (p == a) break;
        a = p;
    }
    return a;
}

template <int SCOPE> __device__ __forceinline__ void uf_union(int *tab, int a, int b, int bound) {
    for (int step = 0; step < bound; ++step) {                  // max(a, b) falls with every step
        a = uf_find<SCOPE>(tab, a, bound);
        b = uf_find<SCOPE>(tab, b, bound);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(tab + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;                                   // a was a root and now hangs under b
        a = old;                                                // somebody moved a meanwhile: its former parent still has to meet b
    }
}

__global__ __launch_bounds__(256) void ccl_tile_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, int H, int W, int tiles_x,
                                                       int *__restrict__ parent, int *__restrict__ size) {
    __shared__ int lab[TILE_PX];
    __shared__ uint8_t cls[TILE_PX];
    const int ty0 = (int)(blockIdx.x / tiles_x) * TILE_H, tx0 = (int)(blockIdx.x % tiles_x) * TILE_W;
    for (int p = threadIdx.x; p < TILE_PX; p += 256) {
        const int y = ty0 + p / TILE_W, x = tx0 + p % TILE_W;
        cls[p] = y < H && x < W ? (uint8_t)error_class(pred, gt, (long)y * W + x) : 0;
        lab[p] = p;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < TILE_PX; p += 256) {
        const int c = cls[p];
        if (!c) continue;
        const int ly = p / TILE_W, lx = p % TILE_W;
        if (lx > 0 && cls[p - 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, p, p - 1, TILE_PX);
        if (ly > 0) {
            if (cls[p - TILE_W] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, p, p - TILE_W, TILE_PX);      // N joins NW and NE itself
            else {
                if (lx > 0 && cls[p - TILE_W - 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, p, p - TILE_W - 1, TILE_PX);
                if (lx < TILE_W - 1 && cls[p - TILE_W + 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, p, p - TILE_W + 1, TILE_PX);
            }
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < TILE_PX; p += 256) {
        const int y = ty0 + p / TILE_W, x = tx0 + p % TILE_W;
        if (y >= H || x >= W) continue;
        const long i = (long)y * W + x;
        int root = -1;                                          // pixels without an error belong to no set
        if (cls[p]) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, p, TILE_PX);       // raster order inside the tile = raster order in the frame
            root = (ty0 + r / TILE_W) * W + tx0 + r % TILE_W;
        }
        parent[i] = root;
        size[i] = 0;
    }
}

// the pairs the tiles could not see: a pixel and its W / NW / N / NE neighbour in another tile
__global__ __launch_bounds__(256) void ccl_merge_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, int H, int W, int *parent) {
    const int n = H * W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = error_class(pred, gt, i);
    if (!c) return;
    const int y = i / W, x = i - y * W;
    const int lx = x % TILE_W, ly = y % TILE_H;
    auto same = [&](int j) { return error_class(pred, gt, j) == c; };
    auto join = [&](int j) { uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, i, j, n); };
    if (lx == 0 && x > 0 && same(i - 1)) join(i - 1);
    if (y == 0) return;
    const bool north = same(i - W);                             // in this tile or not: N joins NW and NE (its own W / E neighbours) itself
    if (north) { if (ly == 0) join(i - W); return; }
    if ((lx == 0 || ly == 0) && x > 0 && same(i - W - 1)) join(i - W - 1);
    if ((lx == TILE_W - 1 || ly == 0) && x < W - 1 && same(i - W + 1)) join(i - W + 1);
}

// parent[i] = the root; size[root] = pixels of the component (a thread adds once per run of pixels with one root)
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int n, int *parent, int *__restrict__ size) {
    const long first = ((long)blockIdx.x * 256 + threadIdx.x) * RUN;
    int cur = -1, cnt = 0;
    for (int j = 0; j < RUN; ++j) {
        const long i = first + j;
        if (i >= n) break;
        int r = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (r >= 0) {
            r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(parent, r, n);
            __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // an ancestor of i either way: finds of others stay right
        }
        if (r != cur) {
            if (cur >= 0) atomicAdd(&size[cur], cnt);
            cur = r; cnt = 0;
        }
        ++cnt;
    }
    if (cur >= 0) atomicAdd(&size[cur], cnt);
}

// the largest component per class; on equal sizes the smaller root, i.e. the component whose first pixel comes first in raster order
// (click_robot.py:27-28: np.argmax of the bincount takes the smallest label, labels are numbered by first pixels)
__global__ __launch_bounds__(256) void robot_best_kernel(const uint8_t *__restrict__ pred, const int *__restrict__ parent, const int *__restrict__ size, int n,
                                                         RobotHdr *hdr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || parent[i] != i) return;
    const int c = pred[i] != 0 ? 0 : 1;                         // a root has an error: predicted = false positive
    atomicMax(&hdr->best[c], ((u64)size[i] << 24) | (u64)((1 << 24) - 1 - i));
    atomicAdd(&hdr->ncomp[c], 1);
}

struct Best { int root[2], size[2], chosen; };                 // chosen: -1 none, 0 false positive, 1 false negative
__device__ __forceinline__ Best best_of(const RobotHdr *hdr) {
    Best b;
    for (int c = 0; c < 2; ++c) {
        const bool has = hdr->ncomp[c] > 0;
        b.size[c] = has ? (int)(hdr->best[c] >> 24) : 0;
        b.root[c] = has ? (1 << 24) - 1 - (int)(hdr->best[c] & ((1 << 24) - 1)) : -2;
    }
    // click_robot.py:63: np.argmax(components_len) - the false positive comes first in that list and wins a tie
    b.chosen = b.size[0] == 0 && b.size[1] == 0 ? -1 : (b.size[0] >= b.size[1] ? 0 : 1);
    return b;
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}

// One pixel pass after the selection: the coordinate sums of both best components, the pixels of the clicked one (component, optional),
// and - only when there is no error at all (parent == nullptr: a middle click was asked for) - the row / column histograms of the object.
__global__ __launch_bounds__(256) void robot_sums_kernel(const uint8_t *__restrict__ gt, const int *__restrict__ parent, int H, int W, RobotHdr *hdr,
                                                         int *__restrict__ hist_y, int *__restrict__ hist_x, uint8_t *__restrict__ component) {
    const int n = H * W;
    Best b;
    b.root[0] = b.root[1] = -2; b.chosen = -1;
    if (parent) b = best_of(hdr);
    const int chosen_root = b.chosen < 0 ? -2 : b.root[b.chosen];
    u64 s[4] = {0, 0, 0, 0};
    int objects = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int l = parent ? parent[i] : -1;
        if (component) component[i] = (uint8_t)(l == chosen_root);
        const bool fp = l == b.root[0], fn = l == b.root[1];
        const bool middle = b.chosen < 0 && gt[i] != 0;
        if (!(fp || fn || middle)) continue;
        const int y = i / W, x = i - y * W;
        if (fp) { s[0] += y; s[1] += x; }
        if (fn) { s[2] += y; s[3] += x; }
        if (middle) { atomicAdd(&hist_y[y], 1); atomicAdd(&hist_x[x], 1); ++objects; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const u64 v = wave_sum64(s[e]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&hdr->sum[e], v);
    }
    const int o = (int)wave_sum64((u64)objects);
    if ((threadIdx.x & 63) == 0 && o) atomicAdd(&hdr->gt_count, o);
}

// the k1-th and k2-th smallest (k1 <= k2) of the multiset that hist [len] counts, by the whole workgroup; the results in out[0], out[1]
__device__ void block_order_stats(const int *__restrict__ hist, int len, int k1, int k2, int *out) {
    __shared__ int part[256];
    const int chunk = (len + 255) / 256;
    const int lo = min((int)threadIdx.x * chunk, len), hi = min(lo + chunk, len);
    int acc = 0;
    for (int e = lo; e < hi; ++e) acc += hist[e];
    __syncthreads();                                            // (the previous call's readers of part[] are done)
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ks[2] = {k1, k2};
        for (int q = 0; q < 2; ++q) {
            int before = 0, t = 0;
            while (t < 255 && before + part[t] <= ks[q]) before += part[t++];
            int e = min(t * chunk, len - 1);
            const int end = min(e + chunk, len);
            for (; e < end - 1; ++e) {
                if (before + hist[e] > ks[q]) break;
                before += hist[e];
            }
            out[q] = e;
        }
    }
    __syncthreads();
}

// One workgroup: the clicks before the fallback.  centroid = (int(sum x / n), int(sum y / n)) in fp64 (click_robot.py:32-33,48-49: np.mean of
// integers below 2^53 is exact whatever its order, then one correctly rounded division); the middle click from the medians of the object's
// rows and columns (:83-87: np.median = the mean of the two middle values, then int()).
__global__ __launch_bounds__(256) void robot_click_kernel(const uint8_t *__restrict__ gt, int H, int W, int middle_only, RobotHdr *hdr,
                                                          const int *__restrict__ hist_y, const int *__restrict__ hist_x) {
    __shared__ int med[4];
    Best b;
    b.chosen = -1; b.size[0] = b.size[1] = 0;
    if (!middle_only) b = best_of(hdr);
    if (b.chosen < 0) {
        const int cnt = hdr->gt_count;                          // (read by every thread before thread 0 writes the header below)
        if (cnt > 0) {
            block_order_stats(hist_y, H, (cnt - 1) / 2, cnt / 2, med);
            block_order_stats(hist_x, W, (cnt - 1) / 2, cnt / 2, med + 2);
        }
        if (threadIdx.x != 0) return;
        hdr->min_d2 = ~0ull; hdr->min_idx = 0xffffffffu;
        if (cnt == 0) return;                                   // no object: no click (the reference fails on the median of nothing)
        const int my = (med[0] + med[1]) >> 1, mx = (med[2] + med[3]) >> 1;
        hdr->mid_valid = 1; hdr->mid_y = my; hdr->mid_x = mx;
        if (gt[(long)my * W + mx] == 0) { hdr->need = 1; hdr->ty = my; hdr->tx = mx; }
        return;
    }
    if (threadIdx.x != 0) return;
    hdr->min_d2 = ~0ull; hdr->min_idx = 0xffffffffu;
    if (b.size[0]) {
        hdr->fp_y = (int)__ddiv_rn((double)hdr->sum[0], (double)b.size[0]);
        hdr->fp_x = (int)__ddiv_rn((double)hdr->sum[1], (double)b.size[0]);
    }
    if (b.size[1]) {
        const int cy = (int)__ddiv_rn((double)hdr->sum[2], (double)b.size[1]), cx = (int)__ddiv_rn((double)hdr->sum[3], (double)b.size[1]);
        hdr->fn_y = cy; hdr->fn_x = cx;
        if (gt[(long)cy * W + cx] == 0) { hdr->need = 1; hdr->ty = cy; hdr->tx = cx; }     // :51-55
    }
}

// The fallback (click_robot.py:51-55,88-93): the object pixel nearest to (tx, ty); np.argmin of the fp64 sqrt of integers = the smallest
// integer squared distance, the first such pixel in raster order.  Distance and index do not fit one 64-bit key together at 2^24 pixels
// (a 1 x 2^24 frame: 48 + 24 bits), so two passes: the distance, then the index among the pixels that have it.
__global__ __launch_bounds__(256) void robot_nearest_kernel(const uint8_t *__restrict__ gt, int H, int W, RobotHdr *hdr, int pass) {
    if (!hdr->need) return;
    const int n = H * W;
    const long ty = hdr->ty, tx = hdr->tx;
    const u64 want = hdr->min_d2;                               // pass 1: the result of pass 0
    u64 best = ~0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (gt[i] == 0) continue;
        const int y = i / W, x = i - y * W;
        const u64 d2 = (u64)((y - ty) * (y - ty) + (x - tx) * (x - tx));
        if (pass == 0) best = d2 < best ? d2 : best;
        else if (d2 == want && (u64)i < best) best = (u64)i;
    }
    best = wave_min64(best);
    if ((threadIdx.x & 63) != 0 || best == ~0ull) return;
    if (pass == 0) atomicMin(&hdr->min_d2, best);
    else atomicMin(&hdr->min_idx, (unsigned)best);
}

// the record (include/stcn_hip.h: STCN_ROBOT_*)
__global__ void robot_record_kernel(int W, int middle_only, int two_clicks, const RobotHdr *__restrict__ hdr, int *__restrict__ rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int r[STCN_ROBOT_RECORD_INTS];
    for (int e = 0; e < STCN_ROBOT_RECORD_INTS; ++e) r[e] = 0;
    Best b;
    b.chosen = -1; b.size[0] = b.size[1] = 0;
    if (!middle_only) {
        b = best_of(hdr);
        r[STCN_ROBOT_FP_SIZE] = b.size[0]; r[STCN_ROBOT_FN_SIZE] = b.size[1];
        r[STCN_ROBOT_FP_COUNT] = hdr->ncomp[0]; r[STCN_ROBOT_FN_COUNT] = hdr->ncomp[1];
    }
    int px = hdr->need ? (int)(hdr->min_idx % (unsigned)W) : 0, py = hdr->need ? (int)(hdr->min_idx / (unsigned)W) : 0;      // the moved click
    if (b.chosen < 0) {
        if (hdr->mid_valid) {
            r[STCN_ROBOT_N_CLICKS] = 1;
            r[STCN_ROBOT_X0] = hdr->need ? px : hdr->mid_x; r[STCN_ROBOT_Y0] = hdr->need ? py : hdr->mid_y; r[STCN_ROBOT_LABEL0] = 1;
            r[STCN_ROBOT_MOVED] = hdr->need;
        }
    } else {
        const int fnx = hdr->need ? px : hdr->fn_x, fny = hdr->need ? py : hdr->fn_y;
        r[STCN_ROBOT_CLASS] = b.chosen + 1;
        r[STCN_ROBOT_N_CLICKS] = 1;
        if (b.chosen == 0) {
            r[STCN_ROBOT_X0] = hdr->fp_x; r[STCN_ROBOT_Y0] = hdr->fp_y; r[STCN_ROBOT_LABEL0] = 0;
            if (two_clicks && b.size[1]) {                      // :71-74: a mask on another object - the positive click goes along
                r[STCN_ROBOT_N_CLICKS] = 2;
                r[STCN_ROBOT_X1] = fnx; r[STCN_ROBOT_Y1] = fny; r[STCN_ROBOT_LABEL1] = 1;
                r[STCN_ROBOT_MOVED] = hdr->need;
            }
        } else {
            r[STCN_ROBOT_X0] = fnx; r[STCN_ROBOT_Y0] = fny; r[STCN_ROBOT_LABEL0] = 1;
            r[STCN_ROBOT_MOVED] = hdr->need;
        }
    }
    for (int e = 0; e < STCN_ROBOT_RECORD_INTS; ++e) rec[e] = r[e];
}

// ---- box of a mask (torchvision.ops.masks_to_boxes of one mask: min / max of the coordinates of its non-zero pixels) -------------------
__global__ void bbox_init_kernel(int *rec) {
    if (threadIdx.x == 0) { rec[0] = 0; rec[1] = INT_MAX; rec[2] = INT_MAX; rec[3] = -1; rec[4] = -1; }
}
__global__ __launch_bounds__(256) void bbox_kernel(const uint8_t *__restrict__ mask, int H, int W, int *rec) {
    const int n = H * W;
    int x1 = INT_MAX, y1 = INT_MAX, x2 = -1, y2 = -1;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (mask[i] == 0) continue;
        const int y = i / W, x = i - y * W;
        x1 = min(x1, x); y1 = min(y1, y); x2 = max(x2, x); y2 = max(y2, y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x1 = min(x1, __shfl_xor(x1, o)); y1 = min(y1, __shfl_xor(y1, o));
        x2 = max(x2, __shfl_xor(x2, o)); y2 = max(y2, __shfl_xor(y2, o));
    }
    if ((threadIdx.x & 63) != 0 || x2 < 0) return;
    atomicMax(&rec[0], 1);
    atomicMin(&rec[1], x1); atomicMin(&rec[2], y1); atomicMax(&rec[3], x2); atomicMax(&rec[4], y2);
}
// an empty mask: "no box", and the coordinates zero
__global__ void bbox_close_kernel(int *rec) {
    if (threadIdx.x == 0 && rec[0] == 0) { rec[1] = rec[2] = rec[3] = rec[4] = 0; }
}

// ---- best of M candidates against a target ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void best_mask_counts_kernel(const uint8_t *__restrict__ cand, const uint8_t *__restrict__ target, int M, int n,
                                                               int *__restrict__ out) {
    int inter[STCN_ROBOT_MAX_CANDIDATES], uni[STCN_ROBOT_MAX_CANDIDATES];
#pragma unroll
    for (int m = 0; m < STCN_ROBOT_MAX_CANDIDATES; ++m) inter[m] = uni[m] = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int t = target[i] != 0;
#pragma unroll
        for (int m = 0; m < STCN_ROBOT_MAX_CANDIDATES; ++m) {
            if (m >= M) break;
            const int c = cand[(long)m * n + i] != 0;
            inter[m] += c & t; uni[m] += c | t;
        }
    }
#pragma unroll
    for (int m = 0; m < STCN_ROBOT_MAX_CANDIDATES; ++m) {
        if (m >= M) break;
        int a = inter[m], u = uni[m];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); u += __shfl_xor(u, o); }
        if ((threadIdx.x & 63) == 0) {
            if (a) atomicAdd(&out[2 + 2 * m], a);
            if (u) atomicAdd(&out[3 + 2 * m], u);
        }
    }
}
// interactions/metrics.py:12-15 in fp32: float(count) + 1e-6f, one division (the mean over the one mask of the batch is the value itself);
// annotator.py:49-55: the first candidate strictly above the running maximum, which starts at 0; none: -1 and 0
__global__ void best_mask_select_kernel(int M, int *out) {
    if (threadIdx.x != 0) return;
    int sel = -1;
    float best = 0.0f;
    for (int m = 0; m < M; ++m) {
        const float iou = __fdiv_rn(__fadd_rn((float)out[2 + 2 * m], 1e-6f), __fadd_rn((float)out[3 + 2 * m], 1e-6f));
        if (iou > best) { best = iou; sel = m; }
    }
    out[0] = sel;
    out[1] = __float_as_int(best);
}

unsigned pixel_blocks(int n, int per_thread = 1) {
    return (unsigned)(((long)n + 256L * per_thread - 1) / (256L * per_thread));
}
unsigned stride_blocks(int n) { return (unsigned)std::min<long>(((long)n + 255) / 256, 2048); }

}  // namespace

size_t robot_scratch_bytes(int H, int W) { return HDR_BYTES + hist_bytes(H, W) + (size_t)H * W * 2 * sizeof(int); }

void robot_click_launch(const uint8_t *pred, const uint8_t *gt, int H, int W, int middle_only, int two_clicks, void *scratch, int *record,
                        uint8_t *component, hipStream_t s) {
    const int n = H * W;
    const RobotScratch sc = carve(scratch, H, W);
    (void)hipMemsetAsync(scratch, 0, sc.zero_bytes, s);
    if (!middle_only) {
        const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H;
        hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)tiles_x * tiles_y), dim3(256), 0, s, pred, gt, H, W, tiles_x, sc.parent, sc.size);
        hipLaunchKernelGGL(ccl_merge_kernel, dim3(pixel_blocks(n)), dim3(256), 0, s, pred, gt, H, W, sc.parent);
        hipLaunchKernelGGL(ccl_flatten_kernel, dim3(pixel_blocks(n, RUN)), dim3(256), 0, s, n, sc.parent, sc.size);
        hipLaunchKernelGGL(robot_best_kernel, dim3(pixel_blocks(n)), dim3(256), 0, s, pred, sc.parent, sc.size, n, sc.hdr);
    }
    hipLaunchKernelGGL(robot_sums_kernel, dim3(stride_blocks(n)), dim3(256), 0, s, gt, middle_only ? nullptr : sc.parent, H, W, sc.hdr, sc.hist_y,
                       sc.hist_x, component);
    hipLaunchKernelGGL(robot_click_kernel, dim3(1), dim3(256), 0, s, gt, H, W, middle_only, sc.hdr, sc.hist_y, sc.hist_x);
    hipLaunchKernelGGL(robot_nearest_kernel, dim3(stride_blocks(n)), dim3(256), 0, s, gt, H, W, sc.hdr, 0);
    hipLaunchKernelGGL(robot_nearest_kernel, dim3(stride_blocks(n)), dim3(256), 0, s, gt, H, W, sc.hdr, 1);
    hipLaunchKernelGGL(robot_record_kernel, dim3(1), dim3(64), 0, s, W, middle_only, two_clicks, sc.hdr, record);
}

void robot_bbox_launch(const uint8_t *mask, int H, int W, int *record, hipStream_t s) {
    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, s, record);
    hipLaunchKernelGGL(bbox_kernel, dim3(stride_blocks(H * W)), dim3(256), 0, s, mask, H, W, record);
    hipLaunchKernelGGL(bbox_close_kernel, dim3(1), dim3(64), 0, s, record);
}

void robot_best_mask_launch(const uint8_t *cand, const uint8_t *target, int M, int H, int W, int *out, hipStream_t s) {
    (void)hipMemsetAsync(out, 0, (size_t)STCN_ROBOT_BEST_INTS * sizeof(int), s);
    hipLaunchKernelGGL(best_mask_counts_kernel, dim3(stride_blocks(H * W)), dim3(256), 0, s, cand, target, M, H * W, out);
    hipLaunchKernelGGL(best_mask_select_kernel, dim3(1), dim3(64), 0, s, M, out);
}

}  // namespace stcn
