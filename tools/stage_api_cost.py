"""GPU box: what do the public stage calls (PropagationNetwork.encode_key / encode_value / segment_with_query / get_attention, FusionNet(),
aggregate_wbg) cost at 480x864, beside the engine's own kernel time for the same work, and what do the NCHW <-> rows transposes reach?

  1. every public call: device ms (events around `iters` calls on one stream, after warm-up) and host ms per call (the enqueue);
     the engine: kernel_profile() of InferenceCore rounds that isolate the same work (a 1-frame clip = encode_key + encode_value, a 2-frame
     clip adds one encode_key + memory read + decode, a fused frame adds attention + FusionNet);
  2. the transposes alone on the f4 (256 x 25 920) and f16 (1024 x 1620) shapes, both directions, in bytes/s, beside tools/micro/hbm_stream
     on the same box (built with STCN_BUILD_LABS=1; "not measured" when the program is not there);
  3. the bank re-transpose of segment_with_query at T = 20 beside the memory read it feeds;
  4. frames/s of the stage loop of tests/test_gpu_stage_api.py (T = 20, mem_freq = 5, k = 1) beside InferenceCore on the same clip.

python tools/stage_api_cost.py [--out FILE] [--iters 20]"""
import ctypes as C
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from eva_vos_amd import _lib, synth  # noqa: E402
from eva_vos_amd.inference_core import InferenceCore  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402
from mivos.model.aggregate import aggregate_wbg  # noqa: E402
from oracle import stcn_oracle as O  # noqa: E402

ITERS = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
H, W, T = 480, 854, 20
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, iters=ITERS, warm=3):
    """(device ms, host ms) per call: events around `iters` calls, a host clock around their enqueue."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters, 1e3 * host / iters


def engine_round_ms(prop, fuse, img, msk, script):
    """Kernel ms per class of the LAST interact of `script` on a fresh core (profiling on)."""
    core = InferenceCore(prop, fuse, img, 1, mem_freq=5)
    core.set_profiling(True)
    for idx in script:
        core.interact(msk[:, idx], idx, download=False)
    torch.cuda.synchronize()
    prof = core.kernel_profile()
    return {c: prof[c]["ms"] for c in _lib.K_CLASSES if prof[c]["ms"] > 0}, core.stats()


def main():
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    torch.set_grad_enabled(False)
    prop, fuse = PropagationNetwork().eval(), FusionNet().eval()
    prop.load_state_dict(synth.recipe_state_dict(prop))
    fuse.load_state_dict(synth.recipe_state_dict(fuse))
    img, msk = synth.synthetic_clip(T, H, W), synth.synthetic_mask(T, H, W, 1)
    imgs = O.pad16(img)[0].cuda()
    m0 = O.pad16(msk[:, 0])[0].cuda()
    nh, nw = imgs.shape[-2:]
    h, w = nh // 16, nw // 16
    say(f"Stage API cost on one {torch.cuda.get_device_name(0)}, library src {_lib.src_hash()}; {nh}x{nw} (padded {H}x{W}), k = 1, {ITERS} calls per figure after 3 warm-up calls.")
    say("device ms = HIP events around the calls on one stream; host ms = the enqueue (Python + fingerprint lookup + C call), no synchronise inside.")
    say()
    # ---- 1. the public calls
    kf = prop.encode_key(imgs[:, 0])
    kf2 = prop.encode_key(imgs[:, 2])
    v0 = prop.encode_value(imgs[:, 0], kf[2], m0)
    seg1 = lambda: prop.segment_with_query(kf[0].unsqueeze(2), v0, kf2[3], kf2[4], kf2[0], kf2[1])      # noqa: E731
    prob = seg1()
    pos, neg = torch.cat([m0 * 0.1, m0]), torch.cat([m0 * 0.2, 1 - m0])
    attn = prop.get_attention(kf[0].unsqueeze(2), pos, neg, kf2[0])
    dist = torch.FloatTensor([0.25, 0.75]).unsqueeze(0)
    calls = {
        "encode_key": lambda: prop.encode_key(imgs[:, 0]),
        "encode_value (k=1)": lambda: prop.encode_value(imgs[:, 0], kf[2], m0),
        "segment_with_query (T=1 memory)": seg1,
        "get_attention (b=2)": lambda: prop.get_attention(kf[0].unsqueeze(2), pos, neg, kf2[0]),
        "FusionNet() (time on the CPU)": lambda: fuse(imgs[:, 2], prob, prob, attn[1:2], dist),
        "aggregate_wbg (keep_bg)": lambda: aggregate_wbg(prob, keep_bg=True),
    }
    say("1. public calls                              device ms   host ms")
    res = {}
    for name, fn in calls.items():
        res[name] = timed(fn)
        say(f"   {name:40s} {res[name][0]:9.3f} {res[name][1]:9.3f}")
    # the same segment with the bank tensors prepared once (what a loop does: the slices of its preallocated bank)
    big_k, big_v = kf[0].unsqueeze(2).expand(-1, -1, T, -1, -1).contiguous(), v0.expand(-1, -1, T, -1, -1).contiguous()
    seg20 = timed(lambda: prop.segment_with_query(big_k, big_v, kf2[3], kf2[4], kf2[0], kf2[1]))
    say(f"   {'segment_with_query (T=20 memory)':40s} {seg20[0]:9.3f} {seg20[1]:9.3f}")
    say()
    say("   the engine's kernel time for the same work (InferenceCore.kernel_profile(), ms per class of one interact()):")
    e1, _ = engine_round_ms(prop, fuse, img[:, :1], msk[:, :1], [0])
    e2, _ = engine_round_ms(prop, fuse, img[:, :2], msk[:, :2], [0])
    e3, st3 = engine_round_ms(prop, fuse, img[:, :3], msk[:, :3], [0, 2])
    fmt = lambda d: ", ".join(f"{c} {v:.3f}" for c, v in d.items()) + f"; total {sum(d.values()):.3f}"      # noqa: E731
    say(f"   1-frame clip, interact(0)  = encode_key + encode_value:                       {fmt(e1)}")
    say(f"   2-frame clip, interact(0)  = the above + encode_key + memory read + decode:   {fmt(e2)}")
    say(f"   3-frame clip, interact(2) after interact(0) = encode_key + encode_value + one frame read, decoded and FUSED ({st3['fused']} fused): {fmt(e3)}")
    key_val = res["encode_key"][0] + res["encode_value (k=1)"][0]
    key_seg = res["encode_key"][0] + res["segment_with_query (T=1 memory)"][0]
    say(f"   stage calls for the same work: encode_key + encode_value {key_val:.3f} ms (engine {sum(e1.values()):.3f}); encode_key + segment_with_query "
        f"{key_seg:.3f} ms (engine, difference of the two clips, {sum(e2.values()) - sum(e1.values()):.3f}); memory read class alone in the engine {e2.get('memread', 0):.3f} ms;")
    say(f"   get_attention {res['get_attention (b=2)'][0]:.3f} ms (engine attention class {e3.get('attention', 0):.3f}); FusionNet() {res['FusionNet() (time on the CPU)'][0]:.3f} ms "
        f"(engine fusion_conv class {e3.get('fusion_conv', 0):.3f})")
    say()
    # ---- 2. the transposes alone
    lib, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    say("2. transposes alone (stcn_test_transpose; bytes = one read + one write of the tensor)")
    rates = {}
    for name, Cc, R in (("f4  256 x 25920", 256, 16 * h * w), ("f16 1024 x 1620", 1024, h * w)):
        a, b = torch.randn(Cc * R, device="cuda"), torch.empty(Cc * R, device="cuda")
        for to_rows in (1, 0):
            ms, _ = timed(lambda: _lib.check(lib.stcn_test_transpose(stream, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), 1, R, Cc, R, 0, to_rows)), iters=200, warm=10)
            rates[(name, to_rows)] = 8.0 * Cc * R / (ms * 1e-3) / 1e12
            say(f"   {name} {'NCHW -> rows' if to_rows else 'rows -> NCHW'}: {1e3 * ms:8.1f} us = {rates[(name, to_rows)]:.2f} TB/s ({8.0 * Cc * R / 1e6:.1f} MB moved)")
    exe = os.path.join(ROOT, "tools", "micro", "hbm_stream")
    stream_tbs = None
    if os.path.exists(exe):
        out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True).stdout
        copies = [float(ln.split("=")[-1].split()[0]) for ln in out.splitlines() if ln.startswith("copy")]
        stream_tbs = max(copies) if copies else None
    say(f"   yardstick tools/micro/hbm_stream, copy 1 : 1 of 133 MB: " + (f"{stream_tbs:.2f} TB/s (best of 3)" if stream_tbs else "not measured (program not built)"))
    if stream_tbs:
        for k_, v in rates.items():
            say(f"   {k_[0]} {'NCHW -> rows' if k_[1] else 'rows -> NCHW'}: {100 * v / stream_tbs:.0f} % of the yardstick" + ("  (BELOW HALF)" if v < 0.5 * stream_tbs else ""))
    say("   (the 133 MB yardstick streams from HBM; the 53 MB / 13 MB tensors here fit the 256 MB memory-side cache, and a call's launch overhead of a few us is inside the figure)")
    say()
    # ---- 3. the bank re-transpose at T = 20
    N = T * h * w
    kb, vb = torch.randn(64 * N, device="cuda"), torch.randn(512 * N, device="cuda")
    ko, vo = torch.empty_like(kb), torch.empty_like(vb)
    tk, _ = timed(lambda: _lib.check(lib.stcn_test_transpose(stream, C.c_void_p(kb.data_ptr()), C.c_void_p(ko.data_ptr()), 1, N, 64, N, 0, 1)), iters=100, warm=5)
    tv, _ = timed(lambda: _lib.check(lib.stcn_test_transpose(stream, C.c_void_p(vb.data_ptr()), C.c_void_p(vo.data_ptr()), 1, N, 512, N, 0, 1)), iters=100, warm=5)
    qk = torch.randn(h * w, 64, device="cuda") * 0.8
    ro, msr = torch.empty(h * w * 512, device="cuda"), C.c_float()
    _lib.check(lib.stcn_bench_memory_read(stream, C.c_void_p(ko.data_ptr()), C.c_void_p(vo.data_ptr()), C.c_void_p(qk.data_ptr()), N, h * w, 1, 20, C.c_void_p(ro.data_ptr()), C.byref(msr), None))
    say(f"3. segment_with_query at T = {T} (N = {N} bank rows, k = 1): bank re-transpose keys {1e3 * tk:.1f} us + values {1e3 * tv:.1f} us = {1e3 * (tk + tv):.1f} us per call; "
        f"the memory read itself (stcn_bench_memory_read, random keys) {1e3 * msr.value:.1f} us" + ("  -> THE RE-TRANSPOSE EXCEEDS THE READ" if tk + tv > msr.value else ""))
    say()
    # ---- 4. the loop
    from test_gpu_stage_api import StageLoopCore
    def fps(make):
        best = 0.0
        for _ in range(3):
            core = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            core.interact(msk[:, 0], 0)
            torch.cuda.synchronize()
            best = max(best, (T - 1) / (time.perf_counter() - t0))
        return best
    f_loop = fps(lambda: StageLoopCore(prop, fuse, img, 1, mem_freq=5))
    f_core = fps(lambda: InferenceCore(prop, fuse, img, 1, mem_freq=5))
    say(f"4. one interact(0) over a {T}-frame clip, mem_freq = 5, k = 1 (wall clock incl. the mask download, best of 3 fresh cores): stage loop {f_loop:.1f} frames/s, InferenceCore {f_core:.1f} frames/s")
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        open(OUT, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
