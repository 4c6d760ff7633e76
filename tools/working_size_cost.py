"""GPU box: what does the working-resolution switch cost and save - and does the down kernel earn its place?

On one MI355X at 1080 x 1920 -> 480 x 853 (the window of a 480 x 864 padded plane), repetitions interleaved over what is compared, in one process:

  upsample_argmax   : the kernel (stcn_prob_upsample_argmax, one launch) for T = 40 and k = 1 and 5 beside the torch route on the same
                      probabilities - ``interpolate(bilinear)`` of the window, ``argmax`` over the channels, ``.to(uint8)`` - ms per call from HIP
                      events over calls back to back, and the peak device memory each route adds while it runs;
  downsample_frames : the kernel (stcn_frames_downsample_aa, one launch, tap tables cached) for an 8-frame chunk beside the torch op
                      ``interpolate(bicubic, antialias=True)``, the same way; and, at the sizes the tests use, how far each is from the torch CPU
                      operator in float64 (the definition) - the ratio the GPU test bounds by 4;
  sessions          : rounds/s of ``eval_driver.run --policy rand_mask`` on a synthetic 1080p tree at the clips' own size beside
                      ``--working-size 480`` (recipe weights, one lane, clip decoding included).

KEEP-OR-DROP RULE (stated before measuring; printed as the verdict, no margin): the down kernel stays only if it is not slower than the torch op
in EVERY repetition.  The up kernel stays regardless, for its memory footprint; its time is reported.

NOT measured here: real videos and weights (what the switch does to J&F), several lanes, several ranks.

python tools/working_size_cost.py [--out profiles/working_size.txt] [--reps 3] [--no-session]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from eva_vos_amd import _lib, eval_driver, fq_driver, synth, working_size  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "working_size.txt")
H, W, SIZE, T, CHUNK = 1080, 1920, 480, 40, 8
UP_CALLS, DOWN_CALLS = 20, 50
VIDEOS, SESSION_T, ROUNDS = 2, 20, 5
ACCURACY = [((203, 231), (96, 109)), ((231, 203), (109, 96)), ((100, 131), (96, 125)), ((800, 1000), (96, 120)), ((1080, 1920), (480, 853))]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return f"{np.median(v):8.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def peak_mb(fn):
    """Device memory the call adds at its peak, outputs included (PyTorch's allocator: the kernels allocate nothing themselves)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    h, w = working_size.working_shape(H, W, SIZE)
    lw, uw = (-w) % 16 // 2, (-w) % 16 - (-w) % 16 // 2
    pad = (lw, uw, 0, 0)
    say(f"working resolution {H} x {W} -> {h} x {w} (padded plane {h} x {w + lw + uw}), library source {_lib.src_hash()}, {torch.cuda.get_device_name(0)}; "
        f"{REPS} repetitions interleaved")
    g = torch.Generator().manual_seed(0)
    for k in (1, 5):
        logits = F.interpolate(torch.randn(T, k + 1, h // 8 + 2, (w + lw + uw) // 8 + 2, generator=g) * 4, size=(h, w + lw + uw), mode="bicubic")
        prob = torch.softmax(logits, 1).clamp(1e-7, 1 - 1e-7).permute(1, 0, 2, 3)[:, :, None].contiguous().to(dev)      # [k+1,T,1,nh,nw]
        out = torch.empty((T, 1, H, W), dtype=torch.uint8, device=dev)

        def kernel():
            return working_size.upsample_argmax(prob, pad, (h, w), (H, W), 0, T, out)

        def route():
            up = F.interpolate(prob[:, :, 0, :, lw:lw + w], size=(H, W), mode="bilinear", align_corners=False)
            return up.argmax(0).to(torch.uint8)

        differ = int((kernel()[:, 0] != route()).sum())               # warm-up; near-ties may fall either way
        kt, tt = [], []
        for rep in range(REPS):
            kt.append(events_ms(kernel, UP_CALLS))
            tt.append(events_ms(route, UP_CALLS))
        km, tm = peak_mb(lambda: working_size.upsample_argmax(prob, pad, (h, w), (H, W), 0, T, torch.empty_like(out))), peak_mb(route)
        say(f"upsample_argmax, T = {T}, k = {k}: fp32 [{k + 1},{T},1,{h},{w + lw + uw}] -> uint8 [{T},1,{H},{W}]; {differ} of {T * H * W} pixels differ between the routes")
        say(f"   kernel (one launch)                         {spread(kt)}   peak device memory added {km:9.1f} MiB")
        say(f"   torch (interpolate, argmax, .to(uint8))     {spread(tt)}   peak device memory added {tm:9.1f} MiB")
        say(f"   kernel / torch = {np.median(kt) / np.median(tt):.3f} in time, {km / tm:.4f} in memory; per repetition: " + ", ".join(f"{a / b:.3f}" for a, b in zip(kt, tt)))
        del prob, out
    say()
    x = torch.randn(CHUNK, 3, H, W, generator=g).to(dev)
    dst = torch.empty((CHUNK, 3, h, w), dtype=torch.float32, device=dev)
    fn = _lib.lib().stcn_frames_downsample_aa
    import ctypes as C

    def kernel():
        _lib.check(fn(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(x.data_ptr()), CHUNK * 3, H, W, h, w, C.c_void_p(dst.data_ptr())))
        return dst

    def route():
        return F.interpolate(x, size=(h, w), mode="bicubic", antialias=True, align_corners=False)

    gap = float((kernel() - route()).abs().max())                     # warm-up: tap tables uploaded, code objects loaded
    kt, tt = [], []
    for rep in range(REPS):
        kt.append(events_ms(kernel, DOWN_CALLS))
        tt.append(events_ms(route, DOWN_CALLS))
    say(f"downsample_frames, one chunk: fp32 [{CHUNK},3,{H},{W}] -> [{CHUNK},3,{h},{w}]; max |kernel - torch on the device| = {gap:.2e}")
    say(f"   kernel (one launch, cached tap tables)      {spread(kt)}")
    say(f"   torch (interpolate bicubic, antialias)      {spread(tt)}")
    say(f"   kernel / torch = {np.median(kt) / np.median(tt):.3f}; per repetition: " + ", ".join(f"{a / b:.3f}" for a, b in zip(kt, tt)))
    ok = all(a <= b for a, b in zip(kt, tt))
    del x, dst
    say("   distance from the torch CPU operator in float64 on N(0,1) data, 3 planes: kernel, torch CPU fp32, ratio (the GPU test bounds it by 4)")
    for (Hs, Ws), (hs, ws) in ACCURACY:
        xs = torch.randn(3, Hs, Ws, generator=g)
        ref = F.interpolate(xs[None].double(), size=(hs, ws), mode="bicubic", antialias=True, align_corners=False)[0]
        t32 = F.interpolate(xs[None], size=(hs, ws), mode="bicubic", antialias=True, align_corners=False)[0]
        got = working_size.downsample_frames(xs[None, None], min(hs, ws))[0, 0].cpu()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        ek, et = float((got.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
        say(f"      {Hs:4d} x {Ws:4d} -> {hs:3d} x {ws:3d}: {ek:.3e}  {et:.3e}  {ek / et:.3f}")
    say()
    say("VERDICT (keep-or-drop rule): the down kernel is " + ("not slower than the torch op in every repetition: it STAYS" if ok
        else "SLOWER than the torch op in a repetition: it is to be TAKEN OUT (downsample_frames calls the torch op)") + "; the up kernel stays for its memory footprint")
    if "--no-session" not in sys.argv:
        say()
        prop, fuse = PropagationNetwork(), FusionNet()
        prop.load_state_dict(synth.recipe_state_dict(prop))
        fuse.load_state_dict(synth.recipe_state_dict(fuse))
        prop, fuse = prop.eval(), fuse.eval()
        with tempfile.TemporaryDirectory() as tmp:
            root = os.path.join(tmp, "db")
            imset = fq_driver.make_synthetic_tree(root, {f"v{i}": (SESSION_T, H, W, 1) for i in range(VIDEOS)})
            runs = {"own size": None, f"--working-size {SIZE}": SIZE}
            rates, rounds_run = {n: [] for n in runs}, {}
            for rep in range(REPS):
                for name, size in runs.items():
                    stats = {}
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    eval_driver.run(root, imset, "", prop, fuse, "rand_mask", rounds=ROUNDS, lanes=1, stats=stats, seed=rep, working_size=size)
                    torch.cuda.synchronize()
                    rates[name].append(stats["interactions"] / (time.perf_counter() - t))
                    rounds_run[name] = stats["interactions"]
            say(f"sessions (rand_mask, recipe weights), {VIDEOS} videos x {SESSION_T} frames at {H} x {W}, {ROUNDS} rounds each, one lane, clip decoding included:")
            for name in runs:
                say(f"   {name:20s} {np.median(rates[name]):7.2f} rounds/s (min {min(rates[name]):.2f}, max {max(rates[name]):.2f}), {rounds_run[name]} rounds run")
            a, b = (np.median(rates[n]) for n in runs)
            say(f"   --working-size {SIZE} / own size = {b / a:.3f} in rounds/s")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
