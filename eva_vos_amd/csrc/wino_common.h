// wino_common.h - host side that the two Winograd families (winograd.hip F(2x2,3x3), winograd4.hip F(4x4,3x3)) share: the tile geometry,
// the 32-bit extent guards, the K-piece arithmetic, the input-transform grid, the common part of the GEMM descriptors and the weight
// transform.  Everything here is computed while PLANNING (wino_plan / wino4_plan); the launch functions read the plan.
#pragma once
#include "kernels.h"

namespace stcn {

// output tiles of edge x edge pixels (2 or 4), the tile count padded to whole workgroup tiles of pad_unit tiles
static inline WinoGeom wino_geom(const ConvP &p, int edge, int pad_unit) {
    WinoGeom g;
    g.TH = (p.OH + edge - 1) / edge; g.TW = (p.OW + edge - 1) / edge;
    g.Mt = p.B * g.TH * g.TW;
    g.Mt_pad = (g.Mt + pad_unit - 1) / pad_unit * pad_unit;
    g.KB = p.Cin / 8;
    return g;
}

// V, the output and the residual are addressed with 32-bit byte offsets (buffer resources): every extent below 4 GiB
static inline bool wino_extents_ok(const ConvP &p, int positions, long Mt_pad) {
    if ((long)positions * p.Cin * Mt_pad * 4 >= (1L << 32)) return false;
    if ((long)p.B * (p.y_bs ? p.y_bs : (long)p.OH * p.OW * p.N) * 4 >= (1L << 32)) return false;
    if (p.res && (long)(p.res_bmod ? p.res_bmod : p.B) * p.res_bs * 4 >= (1L << 32)) return false;
    return true;
}

// KB k-blocks cut into about `want` ranges: at most max_pieces of them, each at least min_kb k-blocks (or the whole K); `per` k-blocks
// per piece, and the piece count that leaves none empty
struct KPieces { int pieces, per; };
static inline KPieces k_pieces(int want, int KB, int min_kb, int max_pieces) {
    int sp = want > max_pieces ? max_pieces : want;
    while (sp > 1 && KB / sp < min_kb) --sp;
    const int per = (KB + sp - 1) / sp;
    return {(KB + per - 1) / per, per};
}

// grid of the input transforms: 8 threads per tile in x; the 32-channel blocks cut into `chunks` (y) of `per` so that the grid fills the chip
struct WinoInGrid { unsigned gx; int chunks, per; };
static inline WinoInGrid wino_input_grid(long tiles, int Cin) {
    const unsigned gx = (unsigned)((8L * tiles + 255) / 256);
    const int NCB = Cin / 32;
    int chunks = (int)((2048 + gx - 1) / gx);
    chunks = chunks < 1 ? 1 : (chunks > NCB ? NCB : chunks);
    const int per = (NCB + chunks - 1) / chunks;
    return {gx, (NCB + per - 1) / per, per};
}

// the fields WinoG and Wino4G have in common, by name (the structs are kernel arguments: their layouts stay their own)
template <typename G>
static inline void wino_fill_desc(G &g, const ConvP &p, const WinoGeom &ge, int positions, const float *V, const float *U, int tiles_n) {
    g.V = V; g.U = U;
    g.v_bytes = (unsigned)((size_t)positions * p.Cin * ge.Mt_pad * 4);
    g.u_bytes = (unsigned)((size_t)positions * p.Cin * p.N * 4);
    g.Mt = ge.Mt; g.Mt_pad = ge.Mt_pad; g.KB = ge.KB; g.N = p.N;
    g.TH = ge.TH; g.TW = ge.TW; g.OH = p.OH; g.OW = p.OW; g.B = p.B; g.M = p.M;
    g.bias = p.bias; g.res = p.res; g.res_bs = p.res_bs; g.res_bmod = p.res_bmod; g.y = p.y; g.y_bs = p.y_bs; g.relu_out = p.relu_out;
    g.fd_tpi = fastdiv_make((unsigned)(ge.TH * ge.TW)); g.fd_tw = fastdiv_make((unsigned)ge.TW); g.fd_tiles_n = fastdiv_make((unsigned)tiles_n);
}

// U = G g G^T, laid out [P * P][Cin/8][N][8], from the BN-folded direct weights w [N][Kp] (k = (ky*3 + kx) * Cin + c), on the host in double
template <int P>
static inline void wino_transform_weights_with(const double (&G)[P][3], const float *w, int N, int Cin, int Kp, float *U) {
    const int KB = Cin / 8;
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < Cin; ++c) {
            double g[3][3], tmp[P][3];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) g[ky][kx] = w[(size_t)n * Kp + (size_t)(ky * 3 + kx) * Cin + c];
            for (int i = 0; i < P; ++i)
                for (int kx = 0; kx < 3; ++kx) tmp[i][kx] = G[i][0] * g[0][kx] + G[i][1] * g[1][kx] + G[i][2] * g[2][kx];
            for (int i = 0; i < P; ++i)
                for (int j = 0; j < P; ++j) {
                    const double u = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
                    U[((((size_t)(i * P + j) * KB + c / 8) * N + n) << 3) + (c & 7)] = (float)u;
                }
        }
}

}  // namespace stcn
