"""GPU box: what does InferenceCore.frame_distances() cost - the T x T squared L2 distances between the cached f16 maps of a clip
(stcn_engine_frame_distances: csrc/frame_select.hip, an fp64 Gram matrix on v_mfma_f64_16x16x4_f64) - and is the kernel worth having?

At 480 x 854 and T = 40, 66, 104, three repetitions interleaved over the clip lengths and the routes, HIP events on the engine's stream:

  1. ms of stcn_engine_frame_distances (enqueue to completion, no download), and the bytes/s it reads the T maps at beside
     tools/micro/hbm_stream on the same box (built with STCN_BUILD_LABS=1; "not measured" when the program is not there);
  2. ms of the route that needs no new HIP: the cached maps gathered into one [T, K] tensor (stcn_engine_frame_features straight into its
     rows - the gather counts), x.double() once, x @ x.T in torch's fp64 GEMM, distances from the Gram matrix;
  3. the call as a fraction of the first interaction of the same clip.

ACCEPTANCE (printed as the verdict): at T = 66 the HIP call is no slower than the torch route of the same run, medians, no margin.

python tools/frame_distances_cost.py [--out profiles/frame_distances.txt] [--reps 3]"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from eva_vos_amd import _lib, synth  # noqa: E402
from eva_vos_amd.inference_core import InferenceCore  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "frame_distances.txt")
H, W, LENGTHS, CALLS = 480, 854, (40, 66, 104), 5
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def events_ms(fn, calls=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def spread(v):
    return f"{np.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def main():
    torch.set_grad_enabled(False)
    lib = _lib.lib()
    prop, fuse = PropagationNetwork(), FusionNet()
    prop.load_state_dict(synth.recipe_state_dict(prop))
    fuse.load_state_dict(synth.recipe_state_dict(fuse))
    clip = synth.synthetic_clip(max(LENGTHS), H, W).cuda()
    mask = synth.synthetic_mask(max(LENGTHS), H, W, 1)[:, 0].cuda()
    say(f"frame distances at {H} x {W}, library source {_lib.src_hash()}, {torch.cuda.get_device_name(0)}; {REPS} repetitions interleaved over T and routes")
    first, hip, route, gather = ({T: [] for T in LENGTHS} for _ in range(4))
    worst = 0.0
    for rep in range(REPS):
        for T in LENGTHS:
            core = InferenceCore(prop.eval(), fuse.eval(), clip[:, :T], 1)
            torch.cuda.synchronize()
            first[T].append(events_ms(lambda: core.interact(mask, 0, download=False)))
            K = core.kh * core.kw * 1024
            dist = torch.empty((T, T), dtype=torch.float64, device="cuda")
            call = lambda: _lib.check(lib.stcn_engine_frame_distances(core._engine, C.c_void_p(dist.data_ptr())))      # noqa: E731
            call()                                                  # takes the scratch from the pool
            torch.cuda.synchronize()
            hip[T].append(events_ms(call, CALLS))
            x = torch.empty((T, K), device="cuda")

            def gather_rows():
                for t in range(T):
                    _lib.check(lib.stcn_engine_frame_features(core._engine, t, C.c_void_p(x[t].data_ptr())))

            def torch_route():
                gather_rows()
                xd = x.double()
                g = xd @ xd.T
                n = g.diagonal()
                return n[:, None] + n[None] - 2 * g, n

            ref, n = torch_route()                                  # warm-up: rocBLAS picks its kernel, the allocator its blocks
            torch.cuda.synchronize()
            gather[T].append(events_ms(gather_rows, CALLS))
            route[T].append(events_ms(torch_route, CALLS))
            worst = max(worst, float(((dist - ref).abs() / (n[:, None] + n[None])).max()))
            del core, x, ref, n
    exe = os.path.join(ROOT, "tools", "micro", "hbm_stream")
    stream_tbs = None
    if os.path.exists(exe):
        out = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True).stdout
        copies = [float(ln.split("=")[-1].split()[0]) for ln in out.splitlines() if ln.startswith("copy")]
        stream_tbs = max(copies) if copies else None
    say("yardstick tools/micro/hbm_stream, copy 1 : 1 of 133 MB: " + (f"{stream_tbs:.2f} TB/s (best of 3)" if stream_tbs else "not measured (program not built)"))
    say()
    for T in LENGTHS:
        K = (H + 15) // 16 * ((W + 15) // 16) * 1024
        nbytes, slices = C.c_int64(), C.c_int32()
        _lib.check(lib.stcn_frame_gram_scratch(T, K, C.byref(nbytes), C.byref(slices)))
        m_hip, m_route = float(np.median(hip[T])), float(np.median(route[T]))
        tbs = 4.0 * T * K / (m_hip * 1e-3) / 1e12
        say(f"T = {T}: K = {K}, {4.0 * T * K / 1e6:.0f} MB of maps, {slices.value} slices, {nbytes.value / 1e6:.1f} MB scratch")
        say(f"   stcn_engine_frame_distances   {spread(hip[T])} = {tbs:.2f} TB/s of maps read" + (f" = {100 * tbs / stream_tbs:.0f} % of the yardstick" if stream_tbs else ""))
        say(f"   torch route, gather included  {spread(route[T])}   (the gather alone {spread(gather[T])})")
        say(f"   first interaction of the clip {spread(first[T])}: the call is {100 * m_hip / np.median(first[T]):.2f} % of it")
        say(f"   HIP / torch = {m_hip / m_route:.3f}; per repetition: " + ", ".join(f"{a / b:.3f}" for a, b in zip(hip[T], route[T])))
    say()
    say(f"agreement of the two routes, worst |D_hip - D_torch| / (G_ii + G_jj) over all runs: {worst:.2e}")
    ok = float(np.median(hip[66])) <= float(np.median(route[66]))
    say(f"VERDICT at T = 66: the HIP call takes {np.median(hip[66]):.3f} ms, the torch route {np.median(route[66]):.3f} ms: " +
        ("ACCEPTED (no slower)" if ok else "REJECTED (the kernel loses to the torch route)"))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
