/*
 * stcn_hip.h - C ABI of libstcn_hip.so, the MI355X (gfx950) STCN mask-propagation engine.
 *
 * The reference (thanosDelatolas/eva-vos) has no FFI: its boundary for this path is the Python
 * class mivos.inference_core.InferenceCore.  Every entry point below cites the reference
 * interface it replaces (paths under /root/reference).  The only caller is the ctypes shim
 * eva_vos_amd/inference_core.py (re-exported as mivos/inference_core.py); see INTEGRATION.md.
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, sizes; no torch / C++ types cross the boundary.
 *   - every function returns 0 on success or a negative STCN_E_* code; stcn_last_error() gives a
 *     thread-local message.  No exception crosses the ABI.
 *   - "dev" pointers are HIP device pointers on the engine's device; the caller owns them and
 *     keeps them alive for the lifetime stated per function.
 *   - an engine is NOT thread-safe; one engine <-> one HIP stream <-> one video.  Distinct engines
 *     may be driven concurrently from distinct host threads.
 *   - all activations are fp32 (the reference computes in fp32 throughout).
 */
#ifndef STCN_HIP_H
#define STCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STCN_OK            0
#define STCN_E_INVALID    -1   /* bad argument / shape */
#define STCN_E_MISSING    -2   /* a required weight tensor is absent */
#define STCN_E_HIP        -3   /* HIP runtime error */
#define STCN_E_STATE      -4   /* call not valid in the current engine state */

/* Objects per engine (`num_objects` of InferenceCore.__init__, mivos/inference_core.py:34): the reference class has no limit (its own
 * pipelines pass 1: datasets/annotation_dataset.py:55-67); this library is built and tested for 1 .. STCN_MAX_OBJECTS. */
#define STCN_MAX_OBJECTS  32

typedef struct stcn_model  stcn_model;   /* folded + repacked weights, read-only, shareable */
typedef struct stcn_engine stcn_engine;  /* per-video state */

/* One named fp32 tensor of a state_dict (host memory, C-contiguous).
 * Replaces: torch `state_dict()` of PropagationNetwork / FusionNet handed to
 * InferenceCore.__init__ as live nn.Modules (mivos/inference_core.py:34-38;
 * eval_annotation_method.py:58-64). */
typedef struct {
    const char  *name;      /* e.g. "key_encoder.layer3.0.conv2.weight" */
    const float *data;      /* host pointer, fp32 */
    int32_t      ndim;      /* 1..4 */
    int64_t      shape[4];
} stcn_weight_desc;

const char *stcn_last_error(void);
const char *stcn_version(void);

/* Build a model on HIP device `device`: folds every eval-mode BatchNorm into its convolution,
 * repacks weights to the engine's [Cout][kh][kw][Cin] layout and uploads them.
 * `prop` must hold the 405-tensor PropagationNetwork dict (int64 num_batches_tracked entries may be
 * omitted); `fuse` the 12-tensor FusionNet dict or NULL/0 (then fusion rounds fail with STCN_E_STATE).
 * Replaces: prop_net.to(device) / fuse_net.to(device) (inference_core.py:36-38). */
int stcn_model_create(int device,
                      const stcn_weight_desc *prop, int n_prop,
                      const stcn_weight_desc *fuse, int n_fuse,
                      stcn_model **out);
int stcn_model_destroy(stcn_model *m);

/* Model hyper-parameters that CHANGE RESULTS (unlike stcn_engine_opts below).  A NON-POSITIVE field means "not given".
 *   top_k   rows of the memory bank each query reads: softmax over the top_k best affinities, 1 .. STCN_MAX_TOP_K, default 50
 *           (`top_k` of PropagationNetwork.__init__, model/propagation/prop_net.py:141, handed to MemoryReader and applied by
 *           softmax_w_top, prop_net.py:53-60).  Every capacity of the read is sized for 50; a larger value, and the reference's
 *           top_k=None (a dense softmax over the whole bank, another kernel family), return STCN_E_INVALID / are not expressible.
 *   km      the kernelized memory read (`km` of EvalMemoryReader, prop_net.py:74-99; the reference's PropagationNetwork passes None and a
 *           caller switches it on with `prop_model.memory.km = 5.6`): every memory row takes the position of the query it matches best in
 *           the frame being read (prop_net.py:94-95), and exp(affinity - max) is multiplied by a Gaussian of standard deviation km (in
 *           1/16-scale positions) around it BEFORE the top_k cut (make_gaussian :33-44, softmax_w_g_top :46-51).  A finite value > 0;
 *           0 or negative = not given = the plain read, bit for bit; NaN / infinity return STCN_E_INVALID.  The fusion attention read
 *           (AttentionMemory, prop_net.py:117-138) has no Gaussian in the reference and none here.
 * stcn_model_create(...) = stcn_model_create_ex(..., NULL, out).  Arguments are validated before the first device call.  Engines,
 * their clones and resets read the values from the model they share. */
#define STCN_MAX_TOP_K  50
typedef struct { int32_t top_k; float km; } stcn_model_opts;
int stcn_model_create_ex(int device,
                         const stcn_weight_desc *prop, int n_prop,
                         const stcn_weight_desc *fuse, int n_fuse,
                         const stcn_model_opts *opts, stcn_model **out);
/* The top_k the model runs with (PropagationNetwork.memory.top_k, prop_net.py:149). */
int stcn_model_get_top_k(const stcn_model *m, int32_t *top_k);
/* The km the model runs with (PropagationNetwork.memory.km); 0 = the plain read. */
int stcn_model_get_km(const stcn_model *m, float *km);

/* Create the per-video engine.
 *   images_dev : fp32 [1,T,3,H,W] (NCHW, normalized, unpadded), read once during this call.
 *   prob_dev   : fp32 [k+1,T,1,nh,nw] owned by the caller (a torch tensor in the shim); the engine
 *                initialises it (bg row 1e-7, others 0) and writes into it on every interact().
 *   masks_dev  : uint8 [T,1,nh,nw] owned by the caller; per-frame argmax written by interact().
 *   nh, nw     : H, W rounded up to multiples of 16 (symmetric zero pad, tensor_util.py:62-80).
 *   stream     : hipStream_t (as void*) all engine work is enqueued on; NULL = default stream.
 * Replaces: InferenceCore.__init__ (inference_core.py:34-99) with mem_profile=0. */
int stcn_engine_create(const stcn_model *m, int T, int H, int W, int k, int mem_freq,
                       void *stream, const float *images_dev, float *prob_dev, uint8_t *masks_dev,
                       stcn_engine **out);
int stcn_engine_destroy(stcn_engine *e);

/* Engine tunables given explicitly instead of through the environment.  A NEGATIVE field means "not given": the engine then
 * takes the environment variable (read once, while the engine is created) or its default.  Results never depend on them.
 *   lookahead     STCN_LOOKAHEAD     (default 2)  0 = no side stream at all (drivers that keep several videos in flight per GPU)
 *   decode_batch  STCN_DECODE_BATCH  (default 8)  frames per memory-read + decoder pass, clipped to mem_freq and 16 / k
 *   key_batch     STCN_KEY_BATCH     (default 0 = max(4, decode group))  frames per key-encoder pass
 *   fuse_side     STCN_FUSE_SIDE     (default 1)  FusionNet of rounds >= 2 on the side stream
 * stcn_engine_create(...) = stcn_engine_create_ex(..., NULL, out).  A clone inherits its source's resolved values.
 * (No reference counterpart: InferenceCore has no tuning surface; eva_vos_amd.InferenceCore(..., engine_options={...}).) */
typedef struct { int32_t lookahead, decode_batch, key_batch, fuse_side; } stcn_engine_opts;
int stcn_engine_create_ex(const stcn_model *m, int T, int H, int W, int k, int mem_freq,
                          void *stream, const float *images_dev, float *prob_dev, uint8_t *masks_dev,
                          const stcn_engine_opts *opts, stcn_engine **out);
/* The values the engine actually runs with (after the environment / defaults were resolved and clipped: look-ahead is 0 when the
 * clip is longer than the key cache, the decode group never exceeds mem_freq or 16 / k objects, fuse_side needs a fusion network). */
int stcn_engine_get_opts(const stcn_engine *e, stcn_engine_opts *out);
/* Everything an engine is configured with, resolved once when it is created (a clone carries its source's, whatever the environment
 * says by then), as STCN_ENGINE_PLAN_INTS int32 in this order:
 *   n_slots        key-cache slots: min(T, 106)
 *   lookahead      as it runs: 0 for a clip longer than the key cache
 *   lookahead_req  as asked for (option / STCN_LOOKAHEAD / 2): > 0 = one video in flight, what the next three rest on
 *   group          decode group: option / STCN_DECODE_BATCH / 8, at most mem_freq, 8 and 16 / k objects, at least 1
 *   key_batch      option / STCN_KEY_BATCH / 0, where <= 0 means max(4, group); at most 8
 *   fuse_side      lookahead_req > 0, a fusion network, and option / STCN_FUSE_SIDE / 1
 *   dual_sweep     the backward sweep of an interaction beside the forward one: lookahead_req > 0, 3 <= T <= n_slots, STCN_DUAL_SWEEP (1) != 0
 *   bank_lo        bank slots in front of the certain slots: (T - 1) / mem_freq + 2 with the dual sweep, else 0
 *   bank_initial   bank slots reserved at create: bank_lo + (T - 1) / mem_freq + 1 + 8
 *   main key_batch, main group, has_side, side key_batch, side group, second key_batch, second group
 *                  what the engine's workspaces are built for; the side one exists when has_side, the second one when dual_sweep
 * stcn_engine_get_plan writes them for a live engine and one more: the capacity of its memory bank in slots, now (n > STCN_ENGINE_PLAN_INTS).
 * Test hook stcn_test_engine_plan: the plan an engine of this shape would get under opts (NULL: none given) and the environment as it is
 * now; has_fuse: the model has a fusion network.  No device call, no GPU needed. */
#define STCN_ENGINE_PLAN_INTS 16
int stcn_engine_get_plan(const stcn_engine *e, int32_t *out, int n);
int stcn_test_engine_plan(int T, int k, int mem_freq, int has_fuse, const stcn_engine_opts *opts, int32_t *out, int n);

/* Back to the state right after stcn_engine_create (same clip): forgets interactions, certain memory and the
 * key-feature cache, re-initialises prob / masks.  Lets a driver reuse one engine's device memory for the
 * next sample of the same shape instead of re-allocating ~4.6 GB.  (No reference counterpart: the reference
 * constructs a new InferenceCore per sample, interactions/eval.py:99.) */
int stcn_engine_reset(stcn_engine *e);

/* stcn_engine_reset with flags; stcn_engine_reset(e) = stcn_engine_reset_ex(e, 0, NULL).
 *   STCN_RESET_KEEP_FRAMES  the next session is for ANOTHER OBJECT OF THE SAME CLIP: interactions, certain memory, bank contents, statistics
 *       and a failed state are forgotten and prob / masks re-initialised as above, but the packed clip and the occupied key-cache slots
 *       stay.  What a slot holds (key, |key|^2, the 1/16, 1/8 and 1/4-scale encoder features, the frame-only parts of the value encoder) is
 *       a function of the frame and the model only, so the next session encodes no key for a kept frame (stcn_stats.key_miss counts only
 *       frames that were not kept).  Its results are bit-identical to a fresh engine's wherever that engine would have key-encoded the
 *       frames in the same batches - every session starting with the same frame is such a case; otherwise the slot order and the batch
 *       shapes of the key encoder and the decoder differ, and results agree up to the rounding of differently shaped launches.
 *       The features are dropped (the call then behaves as with flags = 0) when the engine was in a failed state - the failed interaction may
 *       have left slots half-written - and when the clip is longer than the key cache (T > 106 frames: recycled slots have no stable content).
 *   kept_frames (may be NULL) receives the number of frames whose features were kept, 0 when none were.
 * Both forms drain the engine's side streams first.  Unknown flag bits and a null engine return STCN_E_INVALID before any device call. */
#define STCN_RESET_KEEP_FRAMES 1u
int stcn_engine_reset_ex(stcn_engine *e, uint32_t flags, int32_t *kept_frames);

/* Deep copy of all engine state (certain memory, key cache, interaction set).  The clone writes to
 * the caller-provided prob/masks buffers, which the caller must have filled with a copy of the
 * source's.  Replaces: copy.deepcopy(processor) (interactions/policies.py:103-104). */
int stcn_engine_clone(const stcn_engine *src, float *prob_dev, uint8_t *masks_dev, void *stream,
                      stcn_engine **out);

/* Interact -> propagate both ways -> fuse -> per-frame argmax.
 *   mask_dev      : fp32 [mask_channels,1,H,W] (unpadded).  mask_channels is k (no bg row; only
 *                   valid for k==1, scribble==0) or k+1 (bg first; requires scribble!=0), exactly as
 *                   the reference accepts (inference_core.py:220-233).
 *   Enqueues on the engine stream and returns without synchronising; prob_dev / masks_dev are
 *   complete once the stream has drained.
 *   Errors: bad arguments (STCN_E_INVALID) and a failing up-front reservation of bank memory (STCN_E_HIP: out of memory) are
 *   detected before anything is touched - the engine stays usable, the call may be repeated.  A failure INSIDE the
 *   interaction (failed launch, out of memory while the bank grows) rolls the host bookkeeping back (set of
 *   interacted frames, certain-memory count) and puts the engine into a failed state: prob_dev / masks_dev hold
 *   a partially propagated round, further stcn_interact calls return STCN_E_STATE until stcn_engine_reset().
 * Replaces: InferenceCore.interact (inference_core.py:209-259) incl. do_pass (:126-191) and
 * fuse_one_frame (:193-207). */
int stcn_interact(stcn_engine *e, const float *mask_dev, int mask_channels, int idx, int scribble);

/* Counters of the last interact(): frames visited by the propagation loops, key-encoder misses,
 * value encodes, fused frames, final bank sizes of the forward / backward pass. */
typedef struct {
    int32_t frames, key_miss, value_enc, fused, bank_fwd, bank_bwd;
} stcn_stats;
int stcn_get_stats(const stcn_engine *e, stcn_stats *out);
/* key_miss summed over the interactions since stcn_engine_create / the last reset (either form): the frames the session so far sent
 * through the key encoder - 0 for a session that ran on kept frame features alone.  A clone starts at its source's count. */
int stcn_get_key_frames(const stcn_engine *e, int64_t *out);

/* ---- undo: take the last interaction(s) back in place -----------------------------------------------------------------------
 * For callers that TRY an annotation and take it back: the upper-bound policy tries every remaining frame in every round
 * (get_frame_upper_bound, interactions/policies.py:90-117, on a copy.deepcopy of the processor per candidate), an interactive front end
 * (the GUI the reference's InferenceCore docstring names) lets its user step back.  Neither needs a second engine: an interaction at idx
 * rewrites prob / masks only in the frames strictly between the interacted neighbours of idx, appends one certain-memory slot and may
 * add idx to the set of interacted frames.
 *
 * stcn_engine_set_undo keeps the last `depth` interactions undoable; 0 - the default - switches the journal off: the engine then allocates
 * nothing, enqueues nothing and records nothing for it, every other call is what it is without this section, bit for bit.  Lowering the
 * depth drops the oldest entries.  A negative depth or a null engine returns STCN_E_INVALID before any device call.
 * With depth >= 1 stcn_interact first saves the frames it is about to overwrite - the k + 1 rows of prob and the masks of those frames -
 * into a buffer from the engine-buffer pool sized to that span (stcn_engine_get_undo reports the bytes), after its up-front reservation
 * has succeeded and before its first mutation; the copies are enqueued on the engine's stream, with no synchronisation.  A call that
 * fails in that reservation (or for lack of memory for the journal itself) adds no entry; a failure INSIDE an interaction empties the
 * journal with the rest of the failed state.  The buffer of a dropped entry (depth overflow, reset, a consumed undo) returns to the pool
 * once the stream is past its last use; the engine's next save may take it before that.
 *
 * stcn_engine_undo takes the newest entry back (enqueue only): restores the saved frames, pops the certain slot, and removes the frame
 * from the interacted set unless it was in it before.  idx_out / still_interacted_out (each may be NULL) receive the frame of the undone
 * interaction and whether it is still interacted (1: the undone call was a re-annotation).  An empty journal and an engine in a failed
 * state return STCN_E_STATE and touch nothing: the rule "stcn_engine_reset() after a failure" stands, undo does not recover from one.
 *
 * NOT restored, on purpose:
 *   - key-cache slots filled by the undone interaction: plain caches, a function of the frame and the model only (the lazily written
 *     frame parts of the value encoder included: they are computed one frame at a time, the same bytes whoever writes them);
 *   - the engine's pos / neg / padded-mask scratch: every interaction rewrites it before reading it;
 *   - stcn_stats, stcn_get_key_frames, the profiling counters: they keep describing the work that was done.
 * GUARANTEE.  After stcn_engine_undo the engine's prob, masks, certain memory and interacted set are byte-identical to what they were
 * before the undone call.  If the undone interaction encoded no key (stcn_stats.key_miss == 0 - from the second interaction of a clip of
 * at most 106 frames on, every key is cached), every later result is byte-identical to that of an engine that never ran it.  Otherwise the
 * cache holds other slots than it would, later key-encoder and decoder passes may run in other batches, and later results agree up to
 * the rounding of differently shaped launches - the rule STCN_RESET_KEEP_FRAMES states above.
 * stcn_engine_reset[_ex] empties the journal and keeps the depth; stcn_engine_clone gives the clone its source's depth and an EMPTY journal
 * (the source's entries describe the source's tensors).  (No reference counterpart: InferenceCore has no undo.) */
int stcn_engine_set_undo(stcn_engine *e, int depth);
int stcn_engine_undo(stcn_engine *e, int32_t *idx_out, int32_t *still_interacted_out);
/* depth as set, entries held now, device bytes their buffers hold; each pointer may be NULL.  A null engine returns STCN_E_INVALID. */
int stcn_engine_get_undo(const stcn_engine *e, int32_t *depth, int32_t *entries, int64_t *bytes);

/* ---- cached frame features and the distances between them -----------------------------------------------------------------
 * For frame selectors that need neither ground truth nor a trained network: the reference's l2_mask policy (interactions/mask.py:159-193)
 * annotates next the frame whose features lie farthest, in L2, from every annotated frame (get_frame_l2 / get_min_l2_dist,
 * interactions/policies.py:21-36,69-88) and runs a second pretrained encoder over the clip for them.  Here the features exist already: after
 * the first interaction of a clip of at most STCN_FRAME_GRAM_MAX_T frames every frame's ResNet-50 f16 map [hw16][1024] sits in its
 * key-cache slot, a function of the frame and the model only.
 *
 * Squared L2 distances between T vectors of K fp32 values: dist[i][j] = |x_i - x_j|^2 as fp64 [T,T], symmetric to the bit, zero diagonal,
 * the same bits on every run.  |a|^2 + |b|^2 - 2 a.b cancels between near-equal frames, so the Gram matrix is accumulated in fp64
 * (v_mfma_f64_16x16x4_f64: the product of two fp32 values is exact in fp64, what remains is fp64 summation error,
 * <= K * 2^-53 * (|x_i|^2 + |x_j|^2)).  K is cut into slices whose partial sums pass through a scratch buffer:
 * stcn_frame_gram_scratch gives its size in bytes and the slice count (each pointer may be NULL) from the host-side plan alone - no GPU is
 * needed.  1 <= T <= STCN_FRAME_GRAM_MAX_T, K >= 4 and K % 4 == 0, else STCN_E_INVALID. */
#define STCN_FRAME_GRAM_MAX_T 106
int stcn_frame_gram_scratch(int T, int64_t K, int64_t *bytes, int32_t *slices);
/* The generic entry (enqueue only): vector t starts at x_dev + t * stride.  A null pointer, T outside 1..106, K < 4 or K % 4 != 0,
 * stride < K or stride % 4 != 0, and an x_dev that is not 16-byte aligned return STCN_E_INVALID with a message that names the value,
 * before any device call.  Floats between K and stride are never read. */
int stcn_frame_sq_distances(void *stream, const float *x_dev, int T, int64_t K, int64_t stride, void *scratch_dev, double *dist_dev /*[T,T]*/);
/* The same for the engine's clip, on the engine's stream (enqueue only): vector t is the cached f16 map of frame t, read in place from its
 * key-cache slot; the scratch comes from the engine-buffer pool at the first call.  STCN_E_STATE, with a message that says which: the engine
 * is in a failed state; the clip is longer than the key cache (T > 106); some frame holds no slot - before the first interaction and
 * after a plain reset (STCN_RESET_KEEP_FRAMES keeps them: the next object's session may call at once).
 * Ordering: every slot write is on the engine's stream or joined into it before stcn_interact returns - a sweep's stream waits for the key
 * encoder's event of every frame it visits (no such wait is left pending when an interaction ends: keys are only enqueued for frames of the
 * sweep in progress), the stream of a concurrent backward sweep is joined before the argmax, and a failed interaction is refused here. */
int stcn_engine_frame_distances(stcn_engine *e, double *dist_dev /*[T,T]*/);
/* One cached map: an asynchronous device-to-device copy of frame `frame`'s f16 [hw16,1024] (rows = 1/16-scale positions, the engine's
 * layout) on the engine's stream.  Same state rules (only `frame` has to hold a slot); a frame outside [0,T) returns STCN_E_INVALID.
 * (No reference counterpart: the reference's callers would call prop_net.encode_key themselves.) */
int stcn_engine_frame_features(stcn_engine *e, int frame, float *f16_dev /*[hw16,1024]*/);

/* Algorithmic work of the last interact() in FLOP (2 x MAC of every conv / GEMM issued). */
int stcn_get_flops(const stcn_engine *e, double *flops);

/* ---- the reference's stage interface --------------------------------------------------------------------------
 * What the reference's layer below InferenceCore offers: PropagationNetwork.encode_key / encode_value / segment_with_query / get_attention
 * (model/propagation/prop_net.py:153-211), FusionNet.forward (model/fusion_net.py:32-50) and aggregate_wbg (model/aggregate.py:22-37), for
 * callers that run their own propagation loop.  Every tensor is a device fp32 tensor in the REFERENCE's layout (NCHW, batch 1, C-contiguous
 * unless a stride is given); the conversion to and from the engine's [rows][channels] happens on the device (csrc/layout.hip).
 * A stage context holds the workspace of one frame size on one stream.  Stage calls enqueue on that stream and return; they never synchronise
 * the device.  After the first call that reaches a given memory size (T, k) they do not allocate: the bank staging of stcn_stage_segment grows
 * geometrically, and a growing call waits for the context's own stream once.  A context is NOT thread-safe; two streams take two contexts.
 * Limits: batch 1, no autograd, 1 <= k <= STCN_MAX_OBJECTS, frames padded to multiples of 16 (tensor_util.py:62-80 - InferenceCore pads,
 * inference_core.py:50-53), top_k / km as the model holds them. */
typedef struct stcn_stage stcn_stage;
/* nh, nw: the padded frame size, multiples of 16; max_objects: the largest k (and, + 1, the largest b of stcn_stage_attention) a call will
 * pass, 1 .. STCN_MAX_OBJECTS; stream: hipStream_t (as void*), NULL = default stream.  The model outlives the context.
 * Replaces: nothing the reference spells out - its modules allocate per call through torch's caching allocator. */
int stcn_stage_create(const stcn_model *m, int nh, int nw, int max_objects, void *stream, stcn_stage **out);
/* Waits for the context's stream, then hands its buffers back to the library's pool. */
int stcn_stage_destroy(stcn_stage *s);
/* PropagationNetwork.encode_key (prop_net.py:172-177).  frame [1,3,nh,nw] -> k16 [1,64,h16,w16], f16_thin [1,512,h16,w16],
 * f16 [1,1024,h16,w16], f8 [1,512,h8,w8], f4 [1,256,h4,w4]; an output that is NULL is not written. */
int stcn_stage_encode_key(stcn_stage *s, const float *frame, float *k16, float *f16_thin, float *f16, float *f8, float *f4);
/* PropagationNetwork.encode_value (prop_net.py:153-170).  frame [1,3,nh,nw], kf16 [1,1024,h16,w16] (encode_key's f16), masks [k,1,nh,nw]
 * (the "others" masks of :160-167 are formed inside) -> out [k,512,1,h16,w16]. */
int stcn_stage_encode_value(stcn_stage *s, const float *frame, const float *kf16, const float *masks, int k, float *out);
/* PropagationNetwork.segment_with_query (prop_net.py:179-192): memory read (EvalMemoryReader.get_affinity + readout, :80-115, with the
 * model's top_k and km) + decoder + sigmoid -> prob [k,1,nh,nw], the per-object probabilities, NOT aggregated.
 *   mk16 [1,64,T,h16,w16] with mk_plane_stride elements between its channel planes, mv16 [k,512,T,h16,w16] with mv_plane_stride between
 *   channel planes and mv_object_stride between objects: the T-slices keys[:, :, :m_front] / values[:, :, :m_front] of preallocated banks
 *   that do_pass hands over (inference_core.py:150-170) are read IN PLACE (plane strides Tm * h16 * w16 >= T * h16 * w16).
 *   qf8 [1,512,h8,w8], qf4 [1,256,h4,w4], qk16 [1,64,h16,w16], qv16 [1,512,h16,w16] (encode_key's f16_thin).
 * T * h16 * w16 < top_k returns STCN_E_INVALID (torch.topk raises there, prop_net.py:51-53). */
int stcn_stage_segment(stcn_stage *s, const float *mk16, long mk_plane_stride, const float *mv16, long mv_plane_stride, long mv_object_stride,
                       int T, int k, const float *qf8, const float *qf4, const float *qk16, const float *qv16, float *prob);
/* PropagationNetwork.get_attention (prop_net.py:198-211; AttentionMemory :117-138 - a dense softmax, no top_k, no km).
 * mk16 [1,64,1,h16,w16], pos / neg [b,1,nh,nw], qk16 [1,64,h16,w16] -> attn [b,2,nh,nw]; 1 <= b <= max_objects + 1. */
int stcn_stage_attention(stcn_stage *s, const float *mk16, const float *pos, const float *neg, const float *qk16, int b, float *attn);
/* FusionNet.forward (fusion_net.py:32-50) for one object.  im [1,3,nh,nw], seg1 / seg2 [1,1,nh,nw], attn [1,2,nh,nw], (nc, nr) = the two
 * entries of `time` [1,2] (inference_core.py:199-201) -> logit [1,1,nh,nw].  STCN_E_STATE when the model has no fusion network. */
int stcn_stage_fusion(stcn_stage *s, const float *im, const float *seg1, const float *seg2, const float *attn, float nc, float nr, float *logit);
/* aggregate_wbg (model/aggregate.py:22-37).  prob [k,1,h,w] = [k][npix] -> out [k+1][npix] (keep_bg != 0) or [k][npix]; hard != 0: logits
 * x 1000 (:30-32).  Needs no context: one launch on `stream`. */
int stcn_aggregate_wbg(void *stream, const float *prob, int k, long npix, int keep_bg, int hard, float *out);
/* A model of the FusionNet alone (fuse_net.to(device), inference_core.py:37, without a PropagationNetwork): it serves stcn_stage_fusion;
 * every other stage call on a context of it, and stcn_engine_create, return STCN_E_STATE. */
int stcn_fusion_model_create(int device, const stcn_weight_desc *fuse, int n_fuse, stcn_model **out);
/* Test hook: the layout conversion of the stage calls alone.  to_rows != 0: src = B tensors [C][ld] (planes_bs apart), of which R <= ld
 * elements per channel plane are read -> dst [B][R][C]; to_rows == 0: src [B][R][C] -> dst = B tensors [C][ld].  C % 4 == 0. */
int stcn_test_transpose(void *stream, const float *src, float *dst, int B, int R, int C, long ld, long planes_bs, int to_rows);

/* ---- stage-level hooks (used by tests/ and bench.py only; all pointers are device fp32) --------
 * Layouts are the engine's internal ones: activations NHWC, i.e. [rows = h*w][channels]. */

/* Generic convolution through the implicit-GEMM kernel (what every nn.Conv2d of the path lowers to:
 * modules.py / mod_resnet.py / prop_net.py convs).  x: [B,H,W,Cin] (Cin multiple of 4),
 * w: [Cout,KH,KW,Cin], bias: [Cout], res: [B,OH,OW,Cout] or NULL, y: [B,OH,OW,Cout].
 * flags: bit0 relu on input, bit1 relu on output.  splitk<=0 lets the engine choose.  Cout == 1 (the dot-product kernel of decoder.pred)
 * is stride 1 and takes no residual: res must be NULL there (STCN_E_INVALID otherwise; it used to be ignored). */
int stcn_test_conv(void *stream, const float *x, const float *w, const float *bias, const float *res,
                   float *y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                   int pad, int flags, int splitk);

/* The same convolution with its operands in every form the engine passes (stcn_test_conv is this call with the dense defaults).  Cin: channels
 * of x; x1 / c1: a second source whose channels follow those of x (NULL / 0: one source) - w stays [Cout][KH*KW*(Cin + c1)], ordered (kh, kw,
 * cin) with the channels of x first.  Batch strides in elements: -1 = dense, 0 = broadcast (one image serves every batch element; y_bs has no
 * broadcast: 0 is dense too).  bs0, bs1: of x and x1; res_bs: of res; res_bmod > 0: batch element b adds res + (b % res_bmod) * res_bs (a
 * per-frame residual under a batch laid out [object][frame]); y_bs: of y.  The caller allocates every buffer to the extent its stride implies:
 * B * stride floats, or one image when the stride is 0.  What the planner refuses (a two-source input whose Cin is no multiple of 32, an
 * operand beyond 2 GiB) returns STCN_E_INVALID with its message before anything is launched. */
int stcn_test_conv_ex(void *stream, const float *x, const float *w, const float *bias, const float *res,
                      float *y, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                      int pad, int flags, int splitk, const float *x1, int c1, long bs0, long bs1, long res_bs, int res_bmod, long y_bs);

/* Test hook: the kernel family and plan stcn_test_conv would run this shape as (the string stcn_last_conv_path() gives after it), from
 * the host-side planners alone: nothing is allocated on a device, nothing is launched, no GPU is needed.  out: n bytes. */
int stcn_test_conv_path(int B, int H, int W, int Cin, int Cout, int K, int stride, int flags, int splitk, char *out, int n);
/* Test hook: the same plan in numbers, under the same conditions (no GPU is needed).  iv (n >= STCN_CONV_PLAN_INTS int32):
 *   family (0 literal, 1 fusion, 2 F(4x4), 3 F(2x2), 4 direct), splitk, ppw, tail, n_in, n_gemm, reduce;
 *   Winograd tile geometry TH, TW, Mt, Mt_pad, KB, and F(2x2)'s kb_per_split;
 *   F(4x4): mb, tiles_m, tiles_n, grid, full_wg, pieces, per, chunks, tm_per_chunk;
 *   direct: tile_big, rem_full, rem_split, rem_per, chain
 * - fields of other families than the plan's are zero - and, only when n > STCN_CONV_PLAN_INTS, one more: affine_out (direct: the dense
 * [M][N] epilogue through buffer descriptors, (M + 128) * N * 4 < 2^32).  dv (2 doubles): v_floats, fl_exec. */
#define STCN_CONV_PLAN_INTS 27
int stcn_test_conv_plan(int B, int H, int W, int Cin, int Cout, int K, int stride, int flags, int splitk, int32_t *iv, int n, double *dv);
/* Which kernel family the calling thread's last convolution (stcn_test_conv, or the last conv an interact() enqueued) ran as:
 * "direct splitk=1", "direct_pointwise splitk=1", "direct_narrow ...", "direct_smallc ...", "direct_big ...", "... +tail ...",
 * "wino2 ppw=1 splitk=2" (Winograd F(2x2,3x3)), "wino4 chunks=2 +tail" (F(4x4,3x3)), "fusion_wino", "fusion_direct", "n1".
 * Tests assert the path per shape: a silent fall-back to another instance would still pass a numerical comparison. */
const char *stcn_last_conv_path(void);
/* Test hook: the schedule of one sweep of an interaction, from the host-side planner alone (no GPU is needed).  The sweep visits the frames
 * strictly between idx and closest, away from idx (closest < idx: backward), in decode groups of at most cap frames; mem_freq as given to
 * stcn_engine_create.  Writes the first n groups in sweep order as 4 int32 each - { first frame in sweep order, lowest frame, frames,
 * 1 if the group's last frame in sweep order is inserted into the memory bank } - and the number of groups of the sweep to *count. */
int stcn_test_sweep_plan(int idx, int closest, int mem_freq, int cap, int32_t *out, int n, int32_t *count);
/* Test hook: stcn_test_conv_trace(1) starts (and clears) a log of the CALLING THREAD's convolutions, one "layer=path\n" line per conv
 * enqueued (stage hooks and stcn_interact alike: engine launches happen on the caller's thread); (0) stops it; _get returns the log.
 * Lets a sequence test assert that e.g. every decoder layer of a 853x480 clip really ran as "wino4 ...". */
int stcn_test_conv_trace(int on);
const char *stcn_test_conv_trace_get(void);

/* Test hook: ONE launch of a small kernel (elementwise / pooling / CBAM, csrc/kernels.h) by name, then a synchronisation.  ptrs: nptr device
 * pointers, iv: ni non-negative integers (sizes, strides in elements), fv: nf doubles, per kernel in this order (layouts as kernels.h states):
 *   maxpool3x3s2          ptrs x, y                           iv B, H, W, C
 *   upsample2x_add        ptrs x, skip, u                     iv B, h, w, C, skip_bs, skip_bmod
 *   up4_sigmoid_aggregate ptrs logit4, agg                    iv k, h4, w4, agg_stride, obj_stride, G, logit_gs, agg_gs
 *   up4_sigmoid           ptrs logit4, prob                   iv k, h4, w4
 *   sigmoid_aggregate     ptrs logit, agg                     iv k, npix, agg_stride
 *   argmax                ptrs prob, masks (uint8)            iv kk, T, npix
 *   rowsumsq              ptrs x, out                         iv n, C, B, x_bs, out_bs
 *   pack_image            ptrs img_chw, out                   iv H, W, nh, nw, lw, lh
 *   pack_value_input      ptrs img4, masks, out               iv mask_stride, k, npix
 *   pack_fusion_input     ptrs img4, prev, curr, attn2, out   iv npix                                  fv nc, nr
 *   interact_mask         ptrs mask, prob_idx, padded, pos, neg   iv mc, H, W, nh, nw, lw, lh, prob_row_stride, kk
 *   cbam                  ptrs x, out, w1, b1, w2, b2, wsp    iv B, h, w                               fv bsp   (the hook allocates the scratch)
 *   copy_rows             ptrs src, dst                       iv src_stride, dst_stride, rows, n
 *   copy2                 ptrs a, da, b, db                   iv na, nb
 *   fill                  ptrs p                              iv n                                     fv v
 * Strides and element counts (skip_bs, agg_stride, obj_stride, logit_gs, agg_gs, x_bs, out_bs, mask_stride, prob_row_stride, src_stride,
 * dst_stride, the npix of sigmoid_aggregate / argmax / pack_fusion_input, n of copy_rows / fill, na, nb) may reach 2^40, every other integer INT_MAX.
 * An unknown name, other counts than these, a null pointer, a negative integer or one beyond its range return STCN_E_INVALID - the message names the kernel and
 * the counts it takes - before any device call. */
int stcn_test_kernel(const char *name, void *stream, void *const *ptrs, int nptr, const int64_t *iv, int ni, const double *fv, int nf);

/* encode_key of one frame (prop_net.py:172-177).  img: [1,3,nh,nw] NCHW padded.  Outputs (NHWC):
 * k16 [hw16,64], f16_thin [hw16,512], f16 [hw16,1024], f8 [hw8,512], f4 [hw4,256]; any may be NULL. */
int stcn_test_encode_key(const stcn_model *m, void *stream, const float *img, int nh, int nw,
                         float *k16, float *f16_thin, float *f16, float *f8, float *f4);

/* encode_value (prop_net.py:153-170).  masks: [k,nh*nw] planes; f16 NHWC; out [k,hw16,512]. */
int stcn_test_encode_value(const stcn_model *m, void *stream, const float *img, const float *f16,
                           const float *masks, int k, int nh, int nw, float *out);

/* Space-time memory read (prop_net.py:80-115 with the top-50 softmax of :53-60).
 * mk [N,64], mv [k,N,512], qk [Q,64] -> topk_idx [Q,50] (int32), topk_w [Q,50], readout [k,Q,512].  N < 2^24 rows (the kernels' key descriptor
 * counts bytes in 32 bits): a larger bank is refused with STCN_E_INVALID here, in stcn_stage_segment and where the engine's bank grows. */
int stcn_test_memory_read(void *stream, const float *mk, const float *mv, const float *qk,
                          int N, int Q, int k, int32_t *topk_idx, float *topk_w, float *readout);
/* The same read with the cut given (softmax_w_top(x, top=top_k), prop_net.py:53-60): 1 <= top_k <= STCN_MAX_TOP_K, N >= top_k;
 * topk_idx / topk_w are [Q,top_k].  stcn_test_memory_read(...) is the top_k = 50 case. */
int stcn_test_memory_read_k(void *stream, const float *mk, const float *mv, const float *qk,
                            int N, int Q, int k, int top_k, int32_t *topk_idx, float *topk_w, float *readout);
/* The kernelized read (EvalMemoryReader(top_k, km).get_affinity + readout, prop_net.py:80-115): the Q queries are Q / (h16 * w16) whole
 * frames of h16 x w16 positions (a decode group; Q must be a multiple of h16 * w16), each frame read as the reference reads one frame.
 * centres (may be NULL) [Q / (h16 * w16)][N] int32: per frame, the query of that frame every memory row matches best (argmax_idx,
 * prop_net.py:94).  km > 0 finite; otherwise the limits of stcn_test_memory_read_k.  h16 = w16 = 0, km = 0, centres = NULL is that call. */
int stcn_test_memory_read_km(void *stream, const float *mk, const float *mv, const float *qk,
                             int N, int Q, int k, int top_k, int h16, int w16, float km, int32_t *centres,
                             int32_t *topk_idx, float *topk_w, float *readout);

/* Measurement hook of the same read: `iters` whole reads on caller-provided device data between two HIP events on
 * `stream` (scratch allocated outside the timed region); *ms = average per read; plan7 (may be NULL) receives the launch
 * plan {steps, pass-1 sample stride, sampled steps, pass-1 chunks, steps per chunk, pass-2 chunks, steps per chunk}. */
int stcn_bench_memory_read(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k,
                           int iters, float *readout, float *ms, int32_t *plan7);
/* ... at another cut (prop_net.py:53-60 with top = top_k; same limits as stcn_test_memory_read_k); the call above is top_k = 50. */
int stcn_bench_memory_read_k(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k,
                             int iters, float *readout, float *ms, int32_t *plan7);
/* ... of the kernelized read (arguments as stcn_test_memory_read_km): the row-centre pass is inside the timed region. */
int stcn_bench_memory_read_km(void *stream, const float *mk, const float *mv, const float *qk, int N, int Q, int k, int top_k,
                              int h16, int w16, float km, int iters, float *readout, float *ms, int32_t *plan7);

/* Decoder + sigmoid + soft aggregation (prop_net.py:13-30,189-192; aggregate.py:22-37).
 * readout [k,hw16,512], f16_thin/f8/f4 NHWC -> logit4 [k,hw4] (may be NULL), agg [k+1,nh*nw]. */
int stcn_test_decode(const stcn_model *m, void *stream, const float *readout, const float *f16_thin,
                     const float *f8, const float *f4, int k, int nh, int nw, float *logit4, float *agg);

/* Attention read of fusion (prop_net.py:117-138,198-211).  mk,qk [hw16,64]; pos,neg [kk,nh*nw]
 * -> attn [kk,2,nh*nw]. */
int stcn_test_attention(void *stream, const float *mk, const float *qk, const float *pos,
                        const float *neg, int kk, int nh, int nw, float *attn);
/* The same read with its stages in view; stcn_test_attention(...) = stcn_test_attention_ex(..., NULL, NULL, NULL, NULL, attn).  All optional:
 *   msq        [hw16 + 64] |mk|^2 per memory row and 64 more floats that are read and never used; NULL: computed here
 *   pooled_in  [hw16][nchp] the pooled masks an earlier call returned in pooled_out: the read then runs without pooling (pos = neg = NULL),
 *              as the engine does on every frame of an interaction after the first.  Exactly one of (pos, neg) and pooled_in is given.
 *   pooled_out [hw16][nchp] 16x16 block means, channel 2 r = pos[r], 2 r + 1 = neg[r], zero from 2 kk up to
 *              nchp = 4, 8, 12 for 2 kk <= 4, 8, 12, else 2 kk rounded up to a multiple of 20
 *   amap_out   [2 kk][hw16] pooled channels carried through the softmax, before the bilinear x16
 * nh, nw: multiples of 16.  Arguments are checked before the first device call. */
int stcn_test_attention_ex(void *stream, const float *mk, const float *qk, const float *pos, const float *neg, int kk, int nh, int nw,
                           const float *msq, const float *pooled_in, float *pooled_out, float *amap_out, float *attn);

/* FusionNet logit for one object (fusion_net.py:32-50).  img [1,3,nh,nw] NCHW; prev,curr [nh*nw];
 * attn [2,nh*nw] -> logit [nh*nw]. */
int stcn_test_fusion(const stcn_model *m, void *stream, const float *img, const float *prev,
                     const float *curr, const float *attn, float nc, float nr, int nh, int nw,
                     float *logit);

/* Launch plan of the top-k memory read for N bank rows and Q queries (what stcn_test_memory_read[_k] / the engine will run; it does
 * not depend on top_k):
 * plan7 = { 64-row steps, pass-1 sample stride, sampled steps, pass-1 chunks, steps per pass-1 chunk, pass-2 chunks,
 * steps per pass-2 chunk }.  Lets tests assert WHICH plan (sample stride 1/2/4/8) a comparison exercised. */
int stcn_memread_plan(int N, int Q, int32_t *plan7);
/* Launch plan of the fusion attention read of a frame of hw = h16 * w16 positions (what stcn_test_attention[_ex], stcn_stage_attention and
 * the engine will run; it does not depend on the number of mask rows):
 * plan5 = { 64-row steps of the memory, workgroups of 64 queries, chunks asked for, steps per chunk, chunks launched }.  The column maxima
 * take 16 floats per chunk and query of a scratch of 256 per query: chunks launched <= 16.  Works without a GPU. */
int stcn_attention_plan(int hw, int32_t *plan5);
/* Scratch of that read for Q queries, in elements (what the engine and the hooks allocate; it depends on Q alone):
 * sizes5 = { cand_v, cand_i, cand_n, gmax, tau }.  Every (N, Q) plan fits: nc2 * Q * 50 <= cand_v = cand_i, nc2 * Q <= cand_n,
 * nc1 * Q * 64 <= gmax, 2 * Q * 50 <= gmax (the selection of a read of several objects reuses it), Q <= tau.  Works without a GPU. */
int stcn_memread_scratch(int Q, int64_t *sizes5);

/* Engine buffers (workspaces, key cache, memory bank, packed clip) come from a per-device pool: a destroyed engine's buffers
 * wait there for the next engine of the same sizes (the reference's drivers build one InferenceCore per sample; a hipFree
 * per buffer would synchronise the device under the other videos in flight).  STCN_POOL_GB bounds the pool (default 64, 0 = off);
 * this call returns everything it holds to the driver. */
int stcn_pool_release(void);
/* What the pool has handed out and not got back (buffers, bytes of their size classes) and what it keeps parked, over all devices;
 * null pointers are skipped.  With STCN_POOL_GB=0 nothing is tracked: all zero.  Lets tests show that destroyed engines left nothing behind. */
int stcn_pool_stats(int64_t *live_buffers, int64_t *live_bytes, int64_t *cached_bytes);

/* Test hook (fault injection): the n-th kernel-launch status check made by the CALLING THREAD from now on reports a
 * failure (n = 0 disarms).  Used to show that a failing stcn_interact leaves the engine in a defined state.
 * n = -1: the next stcn_interact of the calling thread fails in its up-front memory reservation - before anything is touched:
 * that call returns STCN_E_HIP and the engine stays USABLE (no failed state). */
int stcn_test_fail_at(int n);

/* Test hook (stream ordering): every FusionNet group handed to the engine's side stream starts `us` microseconds late (0: off;
 * process-wide).  Orderings between the two streams that rest on events alone become observable: a missing wait is a wrong result. */
int stcn_test_side_delay_us(int us);

/* Time `iters` launches of the dominant kernel (implicit-GEMM conv) on `stream` with HIP events;
 * returns average milliseconds per launch.  Used by bench.py for the roofline object. */
int stcn_bench_conv(void *stream, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                    int pad, int splitk, int iters, float *avg_ms, double *flops_per_launch);

/* Matrix rate the chip sustains under a pure fp32-MFMA load (v_mfma_f32_32x32x2_f32 on register operands, no memory
 * traffic) for about ms_target milliseconds: TFLOP/s.  bench.py reports it beside the datasheet peak (the clock under
 * matrix load is lower than the datasheet's). */
int stcn_bench_mfma_rate(void *stream, int ms_target, float *tflops, float *ms_out);

/* Per-kernel-class time of the last interact() measured with HIP events on the engine stream
 * (enabled by stcn_engine_set_profiling(e,1); adds a few % overhead).  ms[] indexed by STCN_K_*. */
enum { STCN_K_CONV = 0, STCN_K_CONV_REDUCE, STCN_K_MEMREAD, STCN_K_ELEMWISE, STCN_K_CONV_N1,
       STCN_K_OTHER, STCN_K_WINO_INPUT /* Winograd input transform of the 3x3 convs */,
       STCN_K_FUSION_CONV /* the FusionNet conv GEMMs (rounds >= 2) */, STCN_K_ATTENTION /* fusion attention read */, STCN_K_COUNT };
int stcn_engine_set_profiling(stcn_engine *e, int on);
int stcn_get_kernel_ms(const stcn_engine *e, float *ms /*[STCN_K_COUNT]*/, int32_t *launches /*[STCN_K_COUNT]*/);
/* Algorithmic FLOP (2 x MAC) issued per kernel class by the last interact(). */
int stcn_get_kernel_flops(const stcn_engine *e, double *flops /*[STCN_K_COUNT]*/);
/* Algorithmic HBM bytes (every operand of every launch once; conv class only) of the last interact(). */
int stcn_get_kernel_bytes(const stcn_engine *e, double *bytes /*[STCN_K_COUNT]*/);
/* FLOP the matrix cores actually EXECUTED per class (= the algorithmic FLOP except for the convs that ran as Winograd
 * F(2x2,3x3): 2.25x fewer multiplies than the 2*M*N*K of stcn_get_kernel_flops). */
int stcn_get_kernel_exec_flops(const stcn_engine *e, double *flops /*[STCN_K_COUNT]*/);
/* Conv launches of the last interact() whose arithmetic intensity (algorithmic FLOP / algorithmic bytes) lies below the
 * machine balance 157.3 TFLOP/s / 8 TB/s = 19.7 FLOP/B - HBM-bound, e.g. the 1x1 channel expansions of the key encoder.
 * They are part of the STCN_K_CONV totals; out[6] = { FLOP, bytes, device ms (profiling on), launches of those launches,
 * algorithmic FLOP of the convs that ran as Winograd F(2x2,3x3), ... as Winograd F(4x4,3x3) }. */
int stcn_get_conv_regimes(stcn_engine *e, double *out /*[6]*/);

/* ---- caller-side metric -------------------------------------------------------
 * Integer counts behind J (region IoU) and F (boundary measure) for T frames, on the device.
 *   gt_dev, pred_dev : uint8 [T,H,W], non-zero = object (unpadded masks)
 *   counts_dev       : int32 [T,6] = intersection, union, gt boundary px, pred boundary px,
 *                      gt boundary px matched within the disk, pred boundary px matched within the disk
 *   scratch_dev      : uint8 [T*H*W]
 * The disk radius is ceil(0.008 * ||(H,W)||) as in the reference.  Enqueues on `stream`, no sync.
 * RADIUS LIMIT of every call that builds boundary maps - this one, stcn_metrics_objects_scratch, stcn_metrics_objects_jf_counts, and
 * stcn_metrics_round / _round_typed / _objects_round / _trial with j_only == 0: a shape whose radius exceeds 46339 (the disk scan squares
 * up to radius + 1 in 32 bits; 2 x 5 792 375 is the first such thin frame) returns STCN_E_INVALID before any device call, the error text
 * naming H, W, the radius and the limit.  The J-only forms have no disk and take any shape.
 * Replaces: get_j_and_f / f_measure / _seg2bmap (interactions/metrics.py:24-34,38-97,100-160) as called per
 * frame per round by eval_processor_metric (interactions/eval.py:50-79). */
int stcn_metrics_jf_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int T, int H, int W,
                           int32_t *counts_dev, uint8_t *scratch_dev);
/* The region measure alone: counts_dev int32 [T,6] with columns 0 (intersection) and 1 (union) filled, the others zero; no scratch.
 * What the oracle annotation policy needs per round (interactions/mask.py:113-146 selects the frame with the worst J; eval_processor_metric
 * with metric='j', interactions/eval.py:27-81). */
int stcn_metrics_j_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int T, int H, int W, int32_t *counts_dev);
/* One annotation round scored ON THE DEVICE (enqueue only): what the reference's loops do on the host after every interact() -
 * eval_processor_metric (interactions/eval.py:27-81: annotated frames count with their ground truth :57-60, per-frame J or J&F :62-79, the
 * NO_OBJECT token for frames without the object :67) followed by the oracle policy's arg-min (interactions/mask.py:130-133; policies.py:62-72).
 *   masks_dev     : the engine's uint8 [T][nh][nw] mask tensor (InferenceCore.masks), cropped at (lh, lw) to H x W
 *   gt_dev        : uint8 [T,H,W] ground truth, non-zero = object;  annotated_dev / noobj_dev : uint8 [T] flags
 *   gen_dev       : uint8 [T,H,W] OUT - the evaluated masks (engine mask, GT on annotated frames): the state util/fq_dataset.py:64-84 saves
 *   scratch_dev   : uint8 [T*H*W] (unused when j_only);  counts_dev : int32 [T,6] OUT as stcn_metrics_jf_counts
 *   j_only == 0   : the radius limit of stcn_metrics_jf_counts applies
 *   quality_dev   : double [T] OUT - per-frame J (j_only) or J&F, no_object for flagged frames; fp64 with the host path's operations in the
 *                   host path's order, i.e. bit-identical to it;  select_dev : int32 [1] OUT - first index of the minimum (numpy.argmin)
 * Only select (4 bytes) has to cross PCIe per round; the quality rows of a session can be fetched together at its end.
 * [t0, t1): the frames whose masks the round just propagated can have changed (the spans on both sides of the new annotation, and the annotated
 *   frame itself): only they are composed and counted; gen / counts of the other frames are kept from the caller's earlier rounds (the first
 *   round passes 0, T).  quality / select always cover all T frames. */
int stcn_metrics_round(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev, const uint8_t *annotated_dev,
                       const uint8_t *noobj_dev, int T, int H, int W, int t0, int t1, int j_only, double no_object, uint8_t *gen_dev, uint8_t *scratch_dev,
                       int32_t *counts_dev, double *quality_dev, int32_t *select_dev);

/* A TRIAL round scored beside the caller's rounds (enqueue only): the quality a round would have if `candidate` were annotated next, after
 * the caller has tried that interaction on the engine (and before it takes it back with stcn_engine_undo) - what the upper-bound policy
 * evaluates for every remaining frame (interactions/policies.py:98-113).  Binary masks; arguments as stcn_metrics_round, except:
 *   annotated_dev  : the flags of the caller's last round, read only; the trial counts frame `candidate` (0 <= candidate < T) as annotated too
 *   [t0, t1)       : the frames the trial can have changed - those strictly between the annotated neighbours of candidate; t0 == t1: none
 *   counts_dev     : const int32 [T,6] - the counts of the caller's last round, the source for every frame outside [t0, t1)
 *   span_gen_dev   : uint8 [(t1 - t0) * H * W] scratch - the evaluated masks of the span
 *   scratch_dev    : uint8 [(t1 - t0) * H * W] scratch - its boundary map (unused when j_only);  span_counts_dev : int32 [(t1 - t0), 6] scratch
 *   quality_dev    : double [T] OUT - per frame the value stcn_metrics_round would write after a real round with this annotation, to the bit:
 *                    from the span's counts inside [t0, t1), from counts_dev outside, no_object for flagged frames
 * Nothing else is written: no gen, no counts, no selection - the caller's round state is what it was.  Null pointers, t0 > t1, a span or a
 * candidate outside [0, T) and, with j_only == 0, a radius above the limit of stcn_metrics_jf_counts return STCN_E_INVALID before any
 * device call. */
int stcn_metrics_trial(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev, const uint8_t *annotated_dev,
                       const uint8_t *noobj_dev, int candidate, int T, int H, int W, int t0, int t1, int j_only, double no_object,
                       const int32_t *counts_dev, uint8_t *span_gen_dev, uint8_t *scratch_dev, int32_t *span_counts_dev, double *quality_dev);

/* ---- the same for LABEL MAPS of k objects (multi-object annotation sessions) -------------------------------------------------
 * A label map is uint8, 0 = background, o in 1..k = object o (the engine's mask tensor for num_objects = k; the palette-index ground truth);
 * a label above k - an object that first appears later - counts as background for every object.  1 <= k <= STCN_MAX_OBJECTS.
 * All objects are served by ONE pass over the pixels: the number of launches does not depend on k.
 *
 * Boundary scratch of the calls below for k objects and T frames of H x W, in BYTES (the one statement of its size: a per-pixel set of
 * objects per map - bytes for k <= 8, 32-bit words above).  Works without a GPU.  Refuses a shape above the radius limit of
 * stcn_metrics_jf_counts, as the calls that take the scratch do. */
int stcn_metrics_objects_scratch(int k, int T, int H, int W, int64_t *bytes);
/* Per object the counts of stcn_metrics_jf_counts for the binary masks (gt == o), (pred == o), integer-exact:
 *   gt_dev, pred_dev : uint8 [T,H,W] label maps;  counts_dev : int32 [k,T,6] OUT;  scratch_dev : stcn_metrics_objects_scratch bytes.
 * Enqueues on `stream`, no sync.  The radius limit of stcn_metrics_jf_counts applies. */
int stcn_metrics_objects_jf_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int k, int T, int H, int W,
                                   int32_t *counts_dev, void *scratch_dev);
/* The region measure alone, as stcn_metrics_j_counts: columns 0 and 1 of counts_dev [k,T,6] filled, the others zero; no scratch. */
int stcn_metrics_objects_j_counts(void *stream, const uint8_t *gt_dev, const uint8_t *pred_dev, int k, int T, int H, int W, int32_t *counts_dev);
/* One annotation round of a k-object session scored on the device (enqueue only), the counterpart of stcn_metrics_round:
 *   masks_dev          : the engine's uint8 [T][nh][nw] label tensor, cropped at (lh, lw) to H x W
 *   gt_dev             : uint8 [T,H,W] ground-truth label map;  annotated_dev : uint8 [T] flags
 *   present_dev        : uint8 [k,T], non-zero where (gt == o) is not empty in frame t
 *   gen_dev            : uint8 [T,H,W] OUT - the evaluated label map (engine labels, ground truth on annotated frames; labels above k as 0)
 *   scratch_dev        : stcn_metrics_objects_scratch bytes (unused when j_only);  counts_dev : int32 [k,T,6] OUT
 *   object_quality_dev : double [k,T] OUT - J (j_only) or J&F of object o in frame t as stcn_metrics_round computes it from the counts,
 *                        no_object where the object is not present
 *   quality_dev        : double [T] OUT - the mean of object_quality over the objects present in the frame: added in ascending o, then divided
 *                        by their number (correctly rounded fp64, bit-identical to eva_vos_amd.metrics.label_round_quality); no_object for a
 *                        frame without any object;  select_dev : int32 [1] OUT - first index of the minimum of quality_dev (numpy.argmin)
 * [t0, t1) as in stcn_metrics_round: only those frames are composed and counted, quality / select cover all T frames; with j_only == 0 the
 * radius limit of stcn_metrics_jf_counts applies. */
int stcn_metrics_objects_round(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev,
                               const uint8_t *annotated_dev, const uint8_t *present_dev, int k, int T, int H, int W, int t0, int t1, int j_only,
                               double no_object, uint8_t *gen_dev, void *scratch_dev, int32_t *counts_dev, double *object_quality_dev,
                               double *quality_dev, int32_t *select_dev);

/* ---- typed rounds: sessions that mix masks with cheaper annotations (clicks, a box) ------------------------------------------
 * stcn_metrics_round with an annotation TYPE per frame in the place of the annotated flag (interactions/eval.py:57-64: a frame annotated
 * with a mask, type 1, is evaluated with its ground truth; one annotated with clicks or a box, type 2, with the annotator's imperfect mask):
 *   type_dev  : uint8 [T] - 0 = the engine's mask, 1 = ground truth, 2 = annotator mask (any other non-zero value counts as 1)
 *   annot_dev : uint8 [T,H,W], non-zero = object - the current annotator mask of every type-2 frame; other frames are not read
 * Binary masks only (the reference's typed policies are one-object).  Counts, quality, arg-min and the [t0, t1) contract are those of
 * stcn_metrics_round, and so is the radius limit when j_only == 0; without a type-2 frame the outputs are its outputs, bit for bit. */
int stcn_metrics_round_typed(void *stream, const uint8_t *masks_dev, int nh, int nw, int lh, int lw, const uint8_t *gt_dev, const uint8_t *type_dev,
                             const uint8_t *annot_dev, const uint8_t *noobj_dev, int T, int H, int W, int t0, int t1, int j_only, double no_object,
                             uint8_t *gen_dev, uint8_t *scratch_dev, int32_t *counts_dev, double *quality_dev, int32_t *select_dev);

/* ---- the simulated user on the device (robots/click_robot.py, robots/bbox_robot.py, annotator/annotator.py:38-57) ---------------
 * Masks are uint8 [H,W], non-zero = object, 1 <= H * W <= 2^24 (the engine's largest padded frame).  Every call enqueues on `stream`
 * without a sync; null pointers (other than those marked optional) and H * W outside that range return STCN_E_INVALID before any device call.
 *
 * The click record, int32 [STCN_ROBOT_RECORD_INTS]: */
#define STCN_ROBOT_N_CLICKS   0    /* 0 (no object to click on), 1 or 2 */
#define STCN_ROBOT_X0         1    /* first click (x, y, label): label 0 = negative click, 1 = positive click */
#define STCN_ROBOT_Y0         2
#define STCN_ROBOT_LABEL0     3
#define STCN_ROBOT_X1         4    /* second click: only the iou < 0.1 branch gives one */
#define STCN_ROBOT_Y1         5
#define STCN_ROBOT_LABEL1     6
#define STCN_ROBOT_CLASS      7    /* the clicked region: 0 = none (middle click), 1 = false positive, 2 = false negative */
#define STCN_ROBOT_FP_SIZE    8    /* pixels of the largest false-positive / false-negative component (0: there is none) */
#define STCN_ROBOT_FN_SIZE    9
#define STCN_ROBOT_FP_COUNT   10   /* false-positive / false-negative components */
#define STCN_ROBOT_FN_COUNT   11
#define STCN_ROBOT_MOVED      12   /* 1: a positive click of the record fell outside the object and was moved to its nearest pixel */
#define STCN_ROBOT_RECORD_INTS 16  /* the rest is zero */
#define STCN_ROBOT_INTERACT   0    /* mode */
#define STCN_ROBOT_MIDDLE     1
/* Bytes of scratch_dev for an H x W frame (the one statement of its size).  Works without a GPU. */
int stcn_robot_scratch(int H, int W, int64_t *bytes);
/* ClickRobot.interact (robots/click_robot.py:14-75) / ClickRobot.middle_click (:78-99) of one mask pair:
 *   mode STCN_ROBOT_INTERACT: 8-connected components of the false-positive (pred && !gt) and of the false-negative (!pred && gt) region
 *     (:22-23,39-40, skimage.measure.label connectivity=2); per region the largest component, on equal sizes the one whose first pixel comes
 *     first in raster order (:27-28,43-44); its centroid (int(mean x), int(mean y)), the means in correctly rounded fp64 (:31-33,47-49); the
 *     positive click moves to the nearest object pixel - smallest squared distance, first in raster order - when it is not on the object
 *     (:51-55); the larger of the two components is clicked, the false positive on a tie (:63-70); use_iou != 0 and iou < 0.1 with a negative
 *     click chosen and a false negative present: both clicks, labels (0, 1) (:71-74); no error at all: the middle click (:64-65).
 *   mode STCN_ROBOT_MIDDLE: pred_dev may be NULL; the medians of the rows and of the columns of the object pixels (an even count: the mean of
 *     the two middle values), int(), with the same nearest-pixel fallback (:83-93).  An empty gt gives a record with 0 clicks (the reference
 *     raises there).
 *   record_dev    : int32 [STCN_ROBOT_RECORD_INTS] OUT
 *   component_dev : optional uint8 [H,W] OUT - 1 on the pixels of the clicked component (STCN_ROBOT_CLASS), all zero for a middle click
 * The object is `gt != 0` everywhere (the reference tests `gt == 1` in the fallback; its masks are 0 / 1). */
int stcn_robot_click(void *stream, const uint8_t *pred_dev, const uint8_t *gt_dev, int H, int W, int mode, int use_iou, double iou,
                     void *scratch_dev, int32_t *record_dev, uint8_t *component_dev);
/* BboxRobot.interact (robots/bbox_robot.py:11-16: torchvision.ops.masks_to_boxes of one mask): record_dev int32 [STCN_ROBOT_BBOX_INTS] OUT =
 * { 1, x1, y1, x2, y2 } - the smallest and largest x and y of the non-zero pixels - or { 0, 0, 0, 0, 0 } for an empty mask ("no box"). */
#define STCN_ROBOT_BBOX_INTS  5
int stcn_robot_bbox(void *stream, const uint8_t *mask_dev, int H, int W, int32_t *record_dev);
/* Annotator.best_sam_mask (annotator/annotator.py:38-57) with compute_iou (interactions/metrics.py:9-19): M candidates (1 <= M <=
 * STCN_ROBOT_MAX_CANDIDATES) cand_dev uint8 [M,H,W] against target_dev uint8 [H,W]:
 *   out_dev int32 [STCN_ROBOT_BEST_INTS] OUT = { selection, the bits of its fp32 IoU, then M pairs (intersection, union) }
 * IoU = (float(intersection) + 1e-6f) / (float(union) + 1e-6f) in fp32; the selection is the first candidate whose IoU is strictly above
 * the running maximum, which starts at 0 (-1 and 0.0 when there is none).  The caller downloads the first 8 bytes. */
#define STCN_ROBOT_MAX_CANDIDATES 8
#define STCN_ROBOT_BEST_INTS  (2 + 2 * STCN_ROBOT_MAX_CANDIDATES)
int stcn_robot_best_mask(void *stream, const uint8_t *cand_dev, const uint8_t *target_dev, int M, int H, int W, int32_t *out_dev);

/* ---- masks as network input (interactions/policies.py:12-18,44-45, mulitple_annotations.py:287-297) --------------------------------
 * src uint8 [T,H,W] on the device (the masks a round evaluated, or a label map) -> out fp32 [n,channels,out_h,out_w]: resized with torch's
 * `nearest` rule, per axis in fp32: source index = min((int)floorf(dst * ((float)in / out)), in - 1); the value of the byte as a float; all
 * `channels` planes equal.  frames_dev: int32 [n] on the device, the frames to take, in that order, or NULL = the first n frames (n = T: all).
 * A frame index outside [0,T) is not read: its planes are filled with NaN.  One launch on `stream`, no sync; only the sampled bytes are read.
 * Null src / out, a size below 1, out_h * out_w above 2^24, frames_dev with n <= 0, n <= 0 or n > T without frames_dev, and n > 65535 return
 * STCN_E_INVALID with a message before any device call. */
int stcn_masks_resize_nearest(void *stream, const uint8_t *src, int T, int H, int W, const int32_t *frames_dev, int n, int out_h, int out_w,
                              int channels, float *out);

/* ---- frames as stored images (datasets/helpers.py:4-17, generate_annotation_dataset.py:170-174) -------------------------------------
 * clip_dev fp32 [T,3,H,W] on the device (normalised frames) -> out_dev uint8 [n,H,W,3]: per frame the minimum and the maximum over all
 * 3 * H * W values, then (x - min) / max(max - min, 1e-8f) * 255, every operation a correctly rounded fp32 one (no contraction, no fast
 * division), truncated to a byte: what `(im_normalize(tens2image(frame)) * 255).astype(uint8)` gives on the host, byte for byte.
 * INPUTS ARE FINITE: with a NaN or an infinity in a frame its image is unspecified.  frames_dev: int32 [n] on the device, the frames to take,
 * in that order (repeats allowed), or NULL = frames 0 .. n - 1.  A frame index outside [0,T) reads nothing and gives an image of zeros.
 * scratch_dev: n * 2 * 4 bytes, 4-byte aligned; the call initialises it on `stream`.  Three launches on `stream`, no sync.
 * Null clip_dev / scratch_dev / out_dev, n < 0, n > 65535, T, H or W below 1, H * W above 2^24 and a clip_dev or scratch_dev that is not
 * 4-byte aligned return STCN_E_INVALID with a message before any device call; n == 0 is a successful no-op. */
int stcn_frames_to_rgb8(void *stream, const float *clip_dev, int T, int H, int W, const int32_t *frames_dev, int n, void *scratch_dev,
                        uint8_t *out_dev);

/* ---- a clip at a working resolution: frames down before the engine, masks up after it --------------------------------------------------
 * stcn_prob_upsample_argmax: prob fp32 [k1,T,1,nh,nw] on the device (an engine's padded probabilities, k1 = objects + 1) -> masks_out uint8
 * [T,H,W].  For every frame t in [t0,t1) the unpadded window of h x w values at row lh, column lw of each channel is interpolated bilinearly
 * to H x W - align_corners=False: src = (dst + 0.5) * in / out - 0.5, clamped below at 0, i1 = min(i0 + 1, in - 1), evaluated in fp32 - and
 * the arg-max over the channels is written as one byte; the lowest index wins a tie.  The interpolated probabilities are never stored.  The
 * padded rows and columns of prob are not read (edges clamp at the window); frames outside [t0,t1) are not written; masks_out may start at
 * any byte.  One launch on `stream` (per 65535 frames), no sync; t0 == t1 is a successful no-op.
 * Null prob / masks_out, k1 outside 2..STCN_MAX_OBJECTS + 1, a size below 1, a window outside the padded plane (lh + h > nh, lw + w > nw, a
 * negative lh or lw), H * W above 2^24 and t0 > t1 or a range outside [0,T] return STCN_E_INVALID with a message before any device call. */
int stcn_prob_upsample_argmax(void *stream, const float *prob, int k1, int T, int nh, int nw, int lh, int lw, int h, int w, int H, int W,
                              int t0, int t1, uint8_t *masks_out);
/* stcn_frames_downsample_aa: src fp32 [planes,H,W] on the device -> dst fp32 [planes,h,w], h <= H and w <= W: antialiased bicubic resampling
 * (A = -0.5, align_corners=False: what F.interpolate(mode="bicubic", antialias=True) defines), a horizontal and a vertical pass with fp64
 * products and sums, rounded to fp32 once.  Per axis the support is 2 * in / out source pixels to either side of the output's centre and the
 * weights are normalised over the part of it inside the image; the tables of an (in, out) pair are built on the host and uploaded at the
 * first call that needs them (a blocking copy; kept per device for the life of the process), every later call only enqueues: one launch on
 * `stream` (per 65535 planes), no sync.  Null src / dst, a size below 1, H * W above 2^24 and h > H or w > W (frames are never enlarged)
 * return STCN_E_INVALID with a message before any device call. */
int stcn_frames_downsample_aa(void *stream, const float *src, int planes, int H, int W, int h, int w, float *dst);

#ifdef __cplusplus
}
#endif
#endif /* STCN_HIP_H */
