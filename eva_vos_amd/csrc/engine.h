// engine.h - host-side model / workspace / per-video engine of libstcn_hip.so (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <deque>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/stcn_hip.h"
#include "kernels.h"

namespace stcn {

void set_error(const char *fmt, ...);
struct Model;
struct ConvW;
// engine buffers come from a per-device pool (engine.cpp: a hipFree per buffer synchronises the device and stalls the other lanes)
hipError_t pool_malloc(void **p, size_t bytes);
void pool_free(void *p);
void pool_release();
// does a conv of this shape get Winograd weights (make_wino / make_wino4 / make_wino_fusion12 below)?
bool wants_wino(const ConvW &cw);
bool wants_wino4(const ConvW &cw);
bool wants_wino_fusion12(const ConvW &cw);
// builds the Winograd weights of a stride-1-capable 3x3 conv from its repacked fp32 host weights (no-op when not eligible)
int make_wino(Model &m, ConvW &cw, const std::vector<float> &w_host);
// F(4x4,3x3) weights of a decoder-side 3x3 conv (no-op when not eligible)
int make_wino4(Model &m, ConvW &cw, const std::vector<float> &w_host);
int make_wino_fusion12(Model &m, ConvW &cw, const std::vector<float> &w_host);   // FusionNet conv1: U over 16 zero-padded channels
#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));    \
            return STCN_E_HIP;                                                             \
        }                                                                                  \
    } while (0)
#define RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// ---- owners of device resources: move-only, creation returns the hipError_t, the destructor gives the resource back, and each converts
// to its raw pointer / handle so that a use site reads as with the raw one.  Whoever destroys an owner has drained the streams that may
// still use the resource (~stcn_engine, ~stcn_stage) - or hands the buffer to a RetireQueue instead.
template <class T = void>
struct PoolBuf {                           // a buffer of the device pool
    T *p = nullptr;
    PoolBuf() = default;
    PoolBuf(PoolBuf &&o) noexcept : p(o.release()) {}
    template <class U> PoolBuf(PoolBuf<U> &&o) noexcept : p(o.release()) {}       // typed -> untyped, on the way into a RetireQueue
    PoolBuf &operator=(PoolBuf &&o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
    ~PoolBuf() { reset(); }
    hipError_t alloc(size_t bytes) { reset(); return pool_malloc((void **)&p, bytes); }
    void reset() { pool_free(p); p = nullptr; }
    T *release() { T *q = p; p = nullptr; return q; }
    operator T *() const { return p; }
};
struct Event {                             // timing disabled
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    operator hipEvent_t() const { return ev; }
};
struct Stream {                            // non-blocking
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&) = delete;
    ~Stream() { reset(); }
    void reset() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};
// Buffers that work already enqueued on a stream may still use: they go back to the pool once ONE event, recorded on that stream behind
// the latest retirement, has fired.  When to collect, whether to wait and what to do without an event stay with the caller.
struct RetireQueue {
    std::vector<std::pair<PoolBuf<>, size_t>> bufs;      // (buffer, bytes it has room for)
    Event ev;
    // records the event on s, creating it at the first use; on failure *what names the step and nothing has changed
    hipError_t mark(hipStream_t s, const char **what) {
        *what = "event create";
        if (!ev) { const hipError_t er = ev.create(); if (er != hipSuccess) return er; }
        *what = "event record";
        return hipEventRecord(ev, s);
    }
    void push(PoolBuf<> b, size_t bytes = 0) { bufs.emplace_back(std::move(b), bytes); }      // after mark()
    void collect(bool wait) {              // frees everything once the event has fired: waits for it, or leaves it for later (never blocks)
        if (bufs.empty()) return;
        if (wait) (void)hipEventSynchronize(ev);
        else if (hipEventQuery(ev) != hipSuccess) return;
        bufs.clear();
    }
    // the smallest retired buffer with room for `bytes`, taken out of the queue (for reuse on the SAME stream: ordered behind its last use)
    bool take_fitting(size_t bytes, PoolBuf<> *b, size_t *cap) {
        size_t best = bufs.size();
        for (size_t i = 0; i < bufs.size(); ++i)
            if (bufs[i].second >= bytes && (best == bufs.size() || bufs[i].second < bufs[best].second)) best = i;
        if (best == bufs.size()) return false;
        *b = std::move(bufs[best].first); *cap = bufs[best].second;
        bufs.erase(bufs.begin() + (long)best);
        return true;
    }
};

struct ConvW {
    float *w = nullptr, *bias = nullptr;   // device: [Cout][Kp], [Cout]
    float *wino_u = nullptr;               // device: Winograd F(2x2,3x3) weights [16][Cin/8][Cout][8] (eligible 3x3 convs)
    float *wino4_u = nullptr;              // device: Winograd F(4x4,3x3) weights [36][Cin/8][Cout][8] (decoder layers)
    float bias0 = 0.f;                     // host copy of bias[0] (Cout == 1 convs)
    int cout = 0, cin = 0, cin_p = 0, kh = 0, kw = 0, K = 0, Kp = 0;
};

struct Model {
    int device = 0;
    std::map<std::string, ConvW> conv;
    CbamW cbam{};
    bool has_prop = false;                 // the propagation network's layers are there (false: stcn_fusion_model_create, FusionNet only)
    bool has_fuse = false;
    int top_k = MEMREAD_MAX_TOPK;          // rows per query of the memory read (PropagationNetwork(top_k=...), prop_net.py:141)
    float km = 0.f;                        // > 0: the kernelized read, standard deviation of its Gaussian (EvalMemoryReader(top_k, km), prop_net.py:75-99); 0: the plain read
    int wino4_min_wg = 100;                // fewest 32 x 32 workgroups for which a flagged layer takes the F(4x4) kernel (tests: 0)
    std::vector<void *> allocs;
    const ConvW &c(const std::string &name) const;
};

struct Dims {
    int nh, nw, h2, w2, h4, w4, h8, w8, h16, w16;
    long npix;
    int hw2, hw4, hw8, hw16;
    void set(int nh_, int nw_) {
        nh = nh_; nw = nw_;
        h2 = nh / 2; w2 = nw / 2; h4 = nh / 4; w4 = nw / 4; h8 = nh / 8; w8 = nw / 8; h16 = nh / 16; w16 = nw / 16;
        npix = (long)nh * nw; hw2 = h2 * w2; hw4 = h4 * w4; hw8 = h8 * w8; hw16 = h16 * w16;
    }
};
// A key-cache slot: ten fields of one frame, in this order, each starting at a multiple of 4 floats (off) - the one statement of it
enum { SLOT_K16, SLOT_MSQ, SLOT_F16_THIN, SLOT_F16, SLOT_S8, SLOT_S4, SLOT_DTHIN, SLOT_CTHIN, SLOT_VD, SLOT_VC, SLOT_FIELDS };
struct SlotLayout { size_t off[SLOT_FIELDS], ext[SLOT_FIELDS], total; };      // floats
inline SlotLayout slot_layout(const Dims &d) {
    const size_t q = (size_t)d.hw16;
    SlotLayout l{{}, {q * 64, (q + 3) / 4 * 4, q * 512, q * 1024, (size_t)d.hw8 * 512, (size_t)d.hw4 * 256, q * 512, q * 512, q * 512, q * 512}, 0};
    for (int f = 0; f < SLOT_FIELDS; ++f) { l.off[f] = l.total; l.total += l.ext[f]; }
    return l;
}

// per-kernel-class accounting (flops always; device time when profiling is on)
struct Prof {
    bool on = false;
    double flops[STCN_K_COUNT] = {0};
    double bytes[STCN_K_COUNT] = {0};     // algorithmic HBM bytes (each operand once)
    double exec_flops[STCN_K_COUNT] = {0};   // FLOP the matrix cores executed (Winograd convs: 2.25x fewer than algorithmic)
    int launches[STCN_K_COUNT] = {0};
    struct Ev { int cls; bool hbm; hipEvent_t a, b; };    // a, b contiguous: attach() hands out &a as hipEvent_t[2]
    std::deque<Ev> events;                      // deque: attach() returns pointers into it
    std::vector<hipEvent_t> pool;
    void reset();
    void begin(int cls, hipStream_t s);
    // register an event pair that the launch itself will fill (launch() in kernels.h); null when off
    hipEvent_t *attach(int cls, bool hbm_bound_conv = false);
    // conv launches below the machine balance (HBM-bound), also counted in the STCN_K_CONV totals
    double hbm_conv_flops = 0, hbm_conv_bytes = 0, hbm_conv_ms = 0; int hbm_conv_launches = 0;
    double wino2_flops = 0, wino4_flops = 0;    // algorithmic FLOP of the convs that ran as Winograd F(2x2,3x3) / F(4x4,3x3)
    void end(hipStream_t s);
    int collect(float *ms);
    ~Prof();
private:
    Ev &push_pair(int cls, bool hbm);           // appends an event pair (from the pool, else created) to events
};

size_t wino_v_capacity(const Dims &d, int maxb);     // Work::wino_v_floats of a workspace whose largest conv batch is maxb
// What the V workspace holds: set by run_conv after the input transform of an unchunked F(4x4) launch, cleared by every other launch that
// writes the workspace (F(2x2), a chunked F(4x4) launch).  It names the tensor as the transform read it - not its contents: only a conv
// whose caller states that the tensor has not been written since (ConvArgs::reuse_v) compares it.
struct VToken {
    const float *x = nullptr;           // null: nothing to reuse
    long bs = 0; unsigned bytes = 0;    // batch stride, extent of the descriptor
    int B = 0, H = 0, W = 0, C = 0;
    int relu = 0;                       // ReLU on the input AS IT TAKES EFFECT (0 for a tensor stated non-negative)
    int Mt_pad = 0;                     // padded tile count: with B, H, W the layout of V
    bool operator==(const VToken &o) const {
        return x == o.x && bs == o.bs && bytes == o.bytes && B == o.B && H == o.H && W == o.W && C == o.C && relu == o.relu && Mt_pad == o.Mt_pad;
    }
};
// scratch for one in-flight frame computation (sized for nh x nw and k objects)
struct Work {
    Dims d{};
    int k = 0;
    size_t S = 0;                       // floats per big buffer
    float *A = nullptr, *B = nullptr, *C = nullptr, *D = nullptr;
    float *splitk = nullptr; size_t splitk_floats = 0;
    float *wino_v = nullptr; size_t wino_v_floats = 0;   // Winograd-transformed input of the conv in flight
    VToken v_token;                     // what wino_v holds after the last launch through this workspace
    float *cbam = nullptr;
    float *readout = nullptr;           // [k][hw16][512]
    float *logit4 = nullptr;            // [k][hw4]
    float *flogit = nullptr;            // [k][npix]  fusion logits
    float *agg = nullptr;               // [k+1][npix] aggregated output of the current frame
    float *agg_alt = nullptr;           // second buffer: decode groups alternate while the side stream fuses the previous group
    float *pooled = nullptr, *amap = nullptr, *attn = nullptr;   // attention read
    float *cand_v = nullptr; int32_t *cand_i = nullptr, *cand_n = nullptr;   // memory-read chunk winners
    float *gmax = nullptr, *tau = nullptr;                       // memory-read group maxima / thresholds
    int32_t *centre = nullptr;          // kernelized read: [group][memread_centre_stride(bank rows)] row centres; grows with the bank (bank_reserve), not owned
    float *qk = nullptr;                // [group][hw16][64] queries of a decode group
    float *vin = nullptr;               // value-encoder packed input [k][npix][8]
    Prof *prof = nullptr;
    Knobs kn = Knobs::from_env();       // launch-level tunables, read once when the workspace is made
    int conv_cls = STCN_K_CONV;         // accounting class of the conv GEMMs launched through this workspace (fusion_logit switches it)
    std::vector<PoolBuf<>> owned;       // what init() allocated; the pointers above are views (the test rigs of hooks.cpp lend wino_v / splitk of their own)
    Work() = default;
    Work(const Work &) = delete;        // every buffer has one owner
    int init(int nh, int nw, int k, int key_batch = 1, int group = 1);   // group: frames decoded per pass (k == 1)
};

// ---- stages (enqueue only) -----------------------------------------------------------------
struct KeyOut { float *k16, *msq, *f16_thin, *f16, *s8, *s4, *f8_copy, *f4_copy, *dthin = nullptr, *cthin = nullptr; };
void inject_failure_after(int n);        // tests: the n-th launch_status() of this thread fails
int launch_status(const char *what);     // STCN_OK, or STCN_E_HIP with the failing launch class in the error string
const char *last_conv_path();            // kernel family of this thread's last run_conv ("wino4 chunks=2", "direct_pointwise splitk=1", ...)
void set_conv_path(const char *s);
void conv_trace(int on);                 // tests: log "name=path" of every conv this thread enqueues
const char *conv_trace_get();
// ---- one convolution: what a call sets, by name
// Batch strides are in elements.  CONV_DENSE: densely packed ([B][H][W][C] input, [B][OH][OW][Cout] residual), worked out by plan_conv.
// A zero stride means a BROADCAST over the batch for an input or the residual, and a dense tensor for the output.
constexpr long CONV_DENSE = -1;
struct ConvArgs {
    const float *x0 = nullptr, *x1 = nullptr;       // input = channel concat of up to two sources
    int c0 = 0, c1 = 0;
    long bs0 = CONV_DENSE, bs1 = 0;
    int B = 1, H = 0, W = 0, stride = 1;
    float *y = nullptr; long y_bs = 0;
    const float *res = nullptr; long res_bs = CONV_DENSE; int res_bmod = 0;   // res_bmod: see ConvP
    int relu_in = 0, relu_out = 0, force_splitk = 0;
    int x_nonneg = 0;       // the caller states: no input value is negative (relu_in has no effect on it)
    int reuse_v = 0;        // the caller states: the previous conv of this workspace read this very tensor and nothing wrote it since -
                            // when Work::v_token agrees, the launch takes V from the workspace instead of transforming again
    ConvArgs &nonneg_input() { x_nonneg = 1; return *this; }
    ConvArgs &same_input_as_last(bool yes = true) { reuse_v = yes; return *this; }
    ConvArgs(const float *x, int c, int B_, int H_, int W_, long bs = CONV_DENSE) : x0(x), c0(c), bs0(bs), B(B_), H(H_), W(W_) {}
    ConvArgs &concat(const float *x, int c, long bs) { x1 = x; c1 = c; bs1 = bs; return *this; }
    ConvArgs &strided(int s) { stride = s; return *this; }
    ConvArgs &out(float *y_, long bs = 0) { y = y_; y_bs = bs; return *this; }
    ConvArgs &residual(const float *r, long bs = CONV_DENSE, int bmod = 0) { res = r; res_bs = bs; res_bmod = bmod; return *this; }
    ConvArgs &relu(int in, int out_) { relu_in = in; relu_out = out_; return *this; }
    ConvArgs &splitk(int k) { force_splitk = k; return *this; }
};
// the planning half of run_conv (pure host code): ConvP of layer `name` over a, and the plan of the family that takes it
int plan_conv(const Model &m, const Work &w, const std::string &name, const ConvArgs &a, ConvP &p, ConvPlan &pl);
const char *format_conv_path(const ConvPlan &pl, char *out, size_t n);
int run_conv(const Model &m, Work &w, hipStream_t s, const std::string &name, const ConvArgs &a);
// ---- one sweep of do_pass: its schedule, as data
// The frames strictly between idx and closest, visited away from idx (direction = sign of closest - idx), cut into decode groups.  A frame is
// inserted into the memory bank when it is not the sweep's last and lies >= mem_freq frames from the last inserted one (from idx before the
// first insertion); a group ends at an inserting frame, at `cap` frames, or with the sweep.  Pure host code: no engine state, no HIP call.
struct SweepGroup {
    int first;        // first frame in sweep order
    int t_lo;         // lowest frame (== first in a forward sweep)
    int G;            // frames
    bool inserts;     // the group's last frame in sweep order goes into the bank (no other frame of a group ever does)
};
std::vector<SweepGroup> plan_sweep(int idx, int closest, int mem_freq, int cap);
constexpr int MAX_DECODE_GROUP = 8;      // the largest cap an engine uses
// ---- one engine: what it is built with and how its bank is sized, as data
// The five engine variables, read once (absent: the default) - the environment half of "explicit option, else environment, else default"
struct EngineEnv {
    int lookahead = 2, decode_batch = 8, key_batch = 0, fuse_side = 1, dual_sweep = 1;
    static EngineEnv from_env();         // STCN_LOOKAHEAD, STCN_DECODE_BATCH, STCN_KEY_BATCH, STCN_FUSE_SIDE, STCN_DUAL_SWEEP
};
constexpr int KEY_CACHE_SLOTS = 106;     // key_buf holds at most 106 frames (inference_core.py:46,118)
struct WorkShape { int key_batch, group; };      // what Work::init is given
struct EnginePlan {
    int mem_freq = 5;                    // as given to stcn_engine_create: the bank is sized for it
    int n_slots = 0;                     // key-cache slots: min(T, KEY_CACHE_SLOTS)
    int lookahead_req = 0;               // look-ahead as asked for: > 0 = one video in flight - the side stream, fuse_side and the dual sweep key on it
    int lookahead = 0;                   // ... and as it runs: 0 for a clip longer than the key cache (its slots are recycled)
    int group = 1;                       // frames per memory-read + decoder pass: <= mem_freq (a group ends at the next bank insertion),
                                         // <= MAX_DECODE_GROUP, objects x frames <= 16 (workspace ~ 0.1 GB each)
    int key_batch = 1;                   // frames per key-encoder pass: as asked, else max(4, group) - a decode group is key-encoded in one pass; <= 8
    bool fuse_side = false;              // FusionNet of rounds >= 2 on the side stream: one video in flight and a fusion network
    bool dual_sweep = false;             // the backward sweep beside the forward one, on stream2 / work2: one video in flight, no cache recycling, T >= 3
    int bank_lo = 0;                     // bank slots in front of the certain slots: the longest backward sweep's temporaries + 1 spare (0: serial sweeps)
    int bank_initial = 0;                // slots reserved at create: room for the first 8 interactions (later ones grow the bank)
    WorkShape main{1, 1}, side{1, 1}, second{1, 1};      // work, work_side, work2 (second exists iff dual_sweep)
    bool has_side = false;               // the side stream and its workspace exist: look-ahead or fuse_side
};
// Pure host code: no HIP call, no getenv, no engine state.  T, k, mem_freq >= 1 as stcn_engine_create checks them.
EnginePlan plan_engine(int T, int k, int mem_freq, bool has_fuse, const stcn_engine_opts &opts, const EngineEnv &env);
// the bank slots an engine needs for a sweep over `span` frames beside `certain` certain slots - the one statement of it
int bank_slots_needed(const EnginePlan &p, int span, int certain);
// B consecutive frames at once; outputs of frame b at o.<ptr> + b * out_bs
int encode_key(const Model &m, Work &w, hipStream_t s, const float *img4, const KeyOut &o, int B = 1, long out_bs = 0);
// vd / vc: cached frame-only halves of fuser.block1 (nullptr: compute the full two-source convs)
int encode_value(const Model &m, Work &w, hipStream_t s, const float *img4, const float *f16,
                 const float *masks, long mask_stride, float *out, long out_bs, const float *vd = nullptr,
                 const float *vc = nullptr);
int value_frame_parts(const Model &m, Work &w, hipStream_t s, const float *f16, float *vd, float *vc);
// dthin / cthin: cached frame-only halves of decoder.compress (nullptr: full two-source convs)
// G > 1: G frames at once, batch laid out [object][frame] - readout [k][G][hw16][512] (what one memory read of G * hw16
// queries writes), agg [G][k+1][npix], the per-frame inputs of frame g at <ptr> + g * slot_bs (consecutive key-cache slots)
int decode(const Model &m, Work &w, hipStream_t s, const float *readout, const float *f16_thin,
           const float *s8, const float *s4, float *agg, long agg_stride, const float *dthin = nullptr,
           const float *cthin = nullptr, int G = 1, long slot_bs = 0, long agg_gs = 0);      // agg_gs: floats between the agg blocks of consecutive frames (0: (k + 1) * agg_stride)
// the decoder alone, up to decoder.pred: w.logit4 [B][hw4] (decode = this + the sigmoid / aggregate tail)
int decode_logit4(const Model &m, Work &w, hipStream_t s, const float *readout, const float *f16_thin, const float *s8, const float *s4,
                  const float *dthin = nullptr, const float *cthin = nullptr, int G = 1, long slot_bs = 0);
int fusion_logit(const Model &m, Work &w, hipStream_t s, const float *img4, const float *prev,
                 const float *curr, const float *attn2, float nc, float nr, float *logit);

// capacity of the stage contexts' bank staging (stages.cpp) after growing `cap` to hold `need`: geometric, pure host code
long stage_grow(long cap, long need);

}  // namespace stcn

struct stcn_model { stcn::Model m; };

struct stcn_engine {
    const stcn::Model *model = nullptr;
    hipStream_t stream = nullptr;
    int T = 0, H = 0, W = 0, k = 0;
    stcn::EnginePlan plan;             // what the tunables resolved to when the engine was created (plan_engine); a clone copies its source's
    int lw = 0, uw = 0, lh = 0, uh = 0;
    stcn::Dims d{};
    float *images4 = nullptr;          // [T][nh][nw][4]; immutable after create, shared with clones
    std::shared_ptr<stcn::PoolBuf<float>> images_owner;  // frees images4 with the last engine that uses it
    float *prob = nullptr;             // caller-owned [k+1][T][npix]
    uint8_t *masks = nullptr;          // caller-owned [T][npix]
    // key-feature cache (plan.n_slots slots)
    std::vector<int> slot_of;          // frame -> slot or -1
    std::vector<char> vparts_ready;    // frame -> value-encoder frame parts (vd, vc) are in its slot
    int n_cached = 0;
    stcn::PoolBuf<float> cache;
    stcn::SlotLayout slot{}; size_t slot_floats = 0;   // slot_floats = slot.total
    stcn::PoolBuf<double> gram_scratch;    // stcn_engine_frame_distances: partial Gram tiles (frame_gram_scratch_bytes), taken from the pool at the first call
    // memory bank: rows = slots * hw16
    int bank_cap = 0, n_certain = 0;
    stcn::PoolBuf<float> bank_k, bank_msq, bank_v;
    stcn::PoolBuf<int32_t> bank_centre;    // kernelized read (model km > 0): the row-centre scratch of work / work2, one block each, sized for bank_cap
    stcn::RetireQueue retired;         // bank buffers replaced by a larger generation
    std::set<int> interacted;
    stcn::PoolBuf<float> mask_pad, pos, neg;   // [k+1][npix] each
    stcn::Work work;
    // key-encoder look-ahead: frames ahead of the decode chain are encoded on a side stream
    stcn::Stream side;
    stcn::Work work_side;
    // round 6: the BACKWARD sweep of an interaction on its own stream and workspace, concurrently with the forward sweep (the two sweeps
    // of do_pass share nothing but the certain memory, which neither writes: inference_core.py:250-253 runs them one after the other).
    // Its temporary bank slots grow DOWNWARD from plan.bank_lo, in front of the certain slots, the forward sweep's upward behind them: each
    // sweep reads one contiguous row range [its temporaries | certain] / [certain | its temporaries].  One video in flight only (same
    // switch as the key-encoder look-ahead); clips longer than the key cache (flush-all policy) keep the serial order.
    stcn::Stream stream2;
    stcn::Work work2;
    stcn::Event ev_fork, ev_join;
    std::vector<stcn::Event> key_ready;   // per frame: recorded on `side` after its encode_key
    std::vector<char> key_pending;       // per frame: main stream has not yet waited on key_ready
    // FusionNet of a decoded group on the side stream (rounds >= 2: the side stream has no keys to encode), two agg buffers
    stcn::Event ev_dec[2], ev_fuse[2];
    char fuse_pending[2] = {0, 0};       // ev_fuse[b] is recorded and the main stream has not waited for it yet
    int agg_buf = 0;
    stcn::Prof prof;
    stcn_stats stats{};
    int64_t key_frames = 0;              // frames that went through the key encoder since creation / the last reset (stcn_get_key_frames)
    std::string failed;                  // non-empty: a failed interaction left prob / masks half-written (see stcn_interact)
    // undo journal (stcn_engine_set_undo): the last undo_depth interactions, oldest first.  An entry holds what its interaction was about
    // to overwrite - frames [f0, f0 + n) of the k + 1 prob rows, then the same frames of masks, in ONE pool buffer sized to that span - and the
    // host bookkeeping to put back.  A dropped entry's buffer is RETIRED: copies out of / into it may still be in flight on the engine's
    // stream, so it is reused by this engine's next save (same stream: ordered) or handed to the pool once the event of undo_retired,
    // recorded behind the latest retirement, has fired.  Depth 0: all of this stays empty and nothing is allocated, recorded or enqueued.
    struct UndoEntry { int idx, f0, n, n_certain0; bool was_interacted; stcn::PoolBuf<> buf; size_t bytes; };
    int undo_depth = 0;
    std::deque<UndoEntry> journal;
    stcn::RetireQueue undo_retired;
    // drains the caller's stream (the device when it is null), then side, then stream2: only then do the members above give anything back
    ~stcn_engine();
};
