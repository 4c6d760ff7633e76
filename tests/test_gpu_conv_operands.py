"""GPU: the operand forms of a convolution that stcn_test_conv cannot express, per conv family, against F.conv2d in fp64 - an input with a
batch stride larger than dense, a two-source channel concat (second source dense or broadcast), a residual with a batch stride / broadcast /
per frame of a batch laid out [object][frame] (res_bmod), an output with a batch stride.  Every case pins the kernel family it is listed
for, fills the output buffer with NaN and requires the gaps between batch elements and a guard behind the last one to stay NaN."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from eva_vos_amd import _lib
from gpu_util import dev, nhwc, stream

pytestmark = pytest.mark.gpu

GUARD = 64
JUNK = 1.0e30        # what lies between the batch elements of a strided input / residual: finite, and ruinous if a kernel adds it in
KG = [(3, 2), (2, 3), (1, 4)]       # batches B = k * G laid out [object][frame]


def plan(B, H, W, Cin, Cout, K, s, flags, splitk=0):
    """(path string, plan numbers) of the device-free planner for the dense single-source conv of this shape."""
    names = ("family splitk ppw tail n_in n_gemm reduce TH TW Mt Mt_pad KB kbps mb tiles_m tiles_n grid full_wg pieces per chunks tm_per_chunk "
             "tile_big rem_full rem_split rem_per chain").split()
    buf, iv, dv = C.create_string_buffer(128), (C.c_int32 * 27)(), (C.c_double * 2)()
    _lib.check(_lib.lib().stcn_test_conv_path(B, H, W, Cin, Cout, K, s, flags, splitk, buf, 128))
    _lib.check(_lib.lib().stcn_test_conv_plan(B, H, W, Cin, Cout, K, s, flags, splitk, iv, 27, dv))
    return buf.value.decode(), dict(zip(names, iv))


def last_path():
    return _lib.lib().stcn_last_conv_path().decode()


def strided(t, bs, fill=JUNK):
    """[B, ...] (cpu, one batch element contiguous) -> device buffer of B * bs floats, element b at b * bs, `fill` in the gaps."""
    B, n = t.shape[0], t[0].numel()
    buf = torch.full((B, bs), fill, dtype=torch.float32)
    buf[:, :n] = t.reshape(B, n)
    return buf.reshape(-1).cuda()


def conv_ex(x, w, b, y, B, H, W, c0, Cout, K, s, flags, splitk=0, res=None, x1=None, c1=0, bs0=-1, bs1=-1, res_bs=-1, res_bmod=0, y_bs=-1):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.lib().stcn_test_conv_ex(stream(), p(x), p(w), p(b), p(res), p(y), B, H, W, c0, Cout, K, K, s, K // 2, flags, splitk,
                                      p(x1), c1, bs0, bs1, res_bs, res_bmod, y_bs)
    torch.cuda.synchronize()
    return rc


def run_and_check(ref, x, w, b, B, H, W, c0, Cout, K, s, flags, y_pad=0, **kw):
    """Runs the conv into a NaN-filled buffer with y_bs = dense + y_pad (0: dense) and a guard; ref: [B, Cout, OH, OW] fp64."""
    OH, OW = ref.shape[2], ref.shape[3]
    dense = OH * OW * Cout
    ybs = dense + y_pad
    y = torch.full((B * ybs + GUARD,), float("nan"), device="cuda")
    rc = conv_ex(x, w, b, y, B, H, W, c0, Cout, K, s, flags, y_bs=ybs if y_pad else -1, **kw)
    assert rc == 0, _lib.lib().stcn_last_error().decode()
    yc = y.cpu()
    assert torch.isnan(yc[B * ybs:]).all(), "the guard behind the output was written"
    body = yc[:B * ybs].reshape(B, ybs)
    assert torch.isnan(body[:, dense:]).all(), "a gap between two batch elements of the output was written"
    got = body[:, :dense].reshape(B, OH, OW, Cout).permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all(), "an addressed output element was not written"
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"{last_path()}: max-norm relative error {err:.2e}")
    assert err < 2e-5, err
    return got


@functools.lru_cache(maxsize=None)
def conv_data(B, H, W, Cin, Cout, K, s, relu_in):
    """Seeded input, weights, bias and the fp64 conv (no residual, no output ReLU) - computed once, shared by the cases of one shape."""
    g = torch.Generator().manual_seed(B * 1000003 + H * 10007 + W * 101 + Cin * 7 + Cout + K)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (2.0 / (Cin * K * K)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d((F.relu(x) if relu_in else x).double(), w.double(), b.double(), stride=s, padding=K // 2)
    return x, w, b, ref


# ------------------------------------------------------------------------------------------------ strided input (and output)
#            name         Cin  Cout K flags ppw   path prefix
STRIDED = [("direct3x3", 64, 96, 3, 0, None, "direct splitk"),
           ("general1x1", 64, 64, 1, 2, None, "direct splitk"),          # a strided 1x1 is NOT the pointwise instance
           ("wino2-ppw1", 128, 64, 3, 1, "1", "wino2 ppw=1"),
           ("wino2-ppw2", 128, 64, 3, 2, "2", "wino2 ppw=2"),
           ("wino4", 128, 64, 3, 7, None, "wino4")]


@pytest.mark.parametrize("y_pad", [0, 64], ids=["y-dense", "y-strided"])
@pytest.mark.parametrize("B", [6, 4])
@pytest.mark.parametrize("name,Cin,Cout,K,flags,ppw,path", STRIDED, ids=[c[0] for c in STRIDED])
def test_input_with_a_batch_stride_larger_than_dense(name, Cin, Cout, K, flags, ppw, path, B, y_pad, monkeypatch):
    H, W = 9, 11
    if ppw:
        monkeypatch.setenv("STCN_WINO_PPW", ppw)
    if K == 1:
        assert plan(B, H, W, Cin, Cout, K, 1, flags)[0].startswith("direct_pointwise "), "the dense twin of this case is the pointwise instance"
    x, w, b, ref = conv_data(B, H, W, Cin, Cout, K, 1, flags & 1)
    if flags & 2:
        ref = F.relu(ref)
    bs0 = H * W * Cin + 192
    run_and_check(ref, strided(x.permute(0, 2, 3, 1), bs0), dev(w.permute(0, 2, 3, 1)), dev(b), B, H, W, Cin, Cout, K, 1, flags, y_pad=y_pad, bs0=bs0)
    assert last_path().startswith(path), (last_path(), path)


# ------------------------------------------------------------------------------------------------ two sources
def two_source(B, H, W, c0, c1, Cout, K, relu_in, bs1_dense, splitk=0, path="direct"):
    x, w, b, ref = conv_data(B, H, W, c0 + c1, Cout, K, 1, relu_in)
    if not bs1_dense:                      # the second source is one frame tensor, broadcast over the batch
        x = x.clone()
        x[:, c0:] = x[:1, c0:]
        ref = F.conv2d((F.relu(x) if relu_in else x).double(), w.double(), b.double(), padding=K // 2)
    x0 = nhwc(x[:, :c0])
    x1 = nhwc(x[:, c0:]) if bs1_dense else nhwc(x[:1, c0:])
    run_and_check(ref, x0, dev(w.permute(0, 2, 3, 1)), dev(b), B, H, W, c0, Cout, K, 1, relu_in, splitk=splitk, x1=x1, c1=c1,
                  bs1=-1 if bs1_dense else 0)
    assert last_path().startswith(path), (last_path(), path)


@pytest.mark.parametrize("relu_in", [0, 1])
@pytest.mark.parametrize("bs1_dense", [True, False], ids=["x1-dense", "x1-broadcast"])
@pytest.mark.parametrize("c0,c1", [(32, 32), (64, 160), (256, 1024)])
@pytest.mark.parametrize("K", [3, 1])
def test_two_source_concat_switches_source_at_c0(K, c0, c1, bs1_dense, relu_in):
    """The tap walk of the direct kernel switches from x to x1 at channel c0 of every tap; M = B * 63 rows is ragged against the 64-row tile."""
    B = 6 if (c0 + relu_in) % 64 else 4
    two_source(B, 7, 9, c0, c1, 96, K, relu_in, bs1_dense, path="direct ")


def test_two_source_concat_under_a_forced_split_k():
    two_source(6, 7, 9, 64, 160, 96, 3, 1, False, splitk=3, path="direct splitk=3")


def test_two_source_concat_on_the_128x128_tile_instance():
    """Kp = 2304 and Cout = 256: the deep-K instance with 2x2 accumulator blocks per wave."""
    two_source(6, 39, 41, 64, 192, 256, 3, 0, False, splitk=3, path="direct_big splitk=3")


def test_two_source_concat_with_a_ragged_first_source_is_refused_without_a_launch():
    B, H, W, c0, c1, Cout = 2, 5, 5, 48, 16, 64
    for K in (1, 3):
        y = torch.full((B * H * W * Cout + GUARD,), float("nan"), device="cuda")
        x0, x1 = torch.zeros(B, H, W, c0, device="cuda"), torch.zeros(B, H, W, c1, device="cuda")
        w, b = torch.zeros(Cout, K, K, c0 + c1, device="cuda"), torch.zeros(Cout, device="cuda")
        assert conv_ex(x0, w, b, y, B, H, W, c0, Cout, K, 1, 0, x1=x1, c1=c1) == -1
        assert "32-aligned" in _lib.lib().stcn_last_error().decode()
        assert torch.isnan(y).all(), "a refused conv wrote to its output"


def test_an_operand_beyond_2_gib_is_refused_without_a_launch():
    """plan_conv's limit (the kernels address with 32-bit byte offsets) comes back as STCN_E_INVALID with its message; nothing runs, so the
    buffers need not have the extent the stride claims."""
    B, H, W, Cin, Cout = 2, 5, 5, 64, 64
    y = torch.full((B * H * W * Cout + GUARD,), float("nan"), device="cuda")
    x, w, b = torch.zeros(B, H, W, Cin, device="cuda"), torch.zeros(Cout, 1, 1, Cin, device="cuda"), torch.zeros(Cout, device="cuda")
    assert conv_ex(x, w, b, y, B, H, W, Cin, Cout, 1, 1, 0, bs0=1 << 28) == -1
    assert "2 GiB" in _lib.lib().stcn_last_error().decode()
    assert torch.isnan(y).all(), "a refused conv wrote to its output"


# ------------------------------------------------------------------------------------------------ residual forms
# per path: channels, kernel, flags bit 2, the frame size per batch size, and what the device-free plan must say.
# How the sizes were found (to be repeated when a planner change makes the assertion on the plan below fail): for the path's channel counts and
# each batch size, walk odd H = 3, 5, ... with W = H + 2 or H + 4 (ragged against every tile) through plan() - stcn_test_conv_path /
# stcn_test_conv_plan, no GPU needed - and take the first size whose plan satisfies the predicate; where that size is a single workgroup
# (direct_splitk, wino2_split, wino4_small) the next one up with batch boundaries inside a tile was taken.  The fp64 reference of the largest
# (wino4_tail, 10 GFLOP) takes half a second.
RES_PATHS = {
    "direct":        (64, 96, 3, 0, {6: (27, 31), 4: (31, 35)}, lambda p, d: p.startswith("direct splitk=1")),
    "direct_narrow": (64, 32, 1, 0, {6: (9, 11), 4: (9, 11)}, lambda p, d: p.startswith("direct_narrow splitk=1")),
    "direct_splitk": (64, 96, 3, 0, {6: (7, 9), 4: (7, 9)}, lambda p, d: p.startswith("direct splitk=") and d["splitk"] > 1),
    "direct_tail":   (64, 96, 3, 0, {6: (37, 39), 4: (45, 47)}, lambda p, d: p.startswith("direct +tail")),
    "wino2":         (128, 512, 3, 0, {6: (25, 31), 4: (33, 35)}, lambda p, d: p.startswith("wino2") and d["splitk"] == 1),
    "wino2_split":   (128, 64, 3, 0, {6: (7, 9), 4: (7, 9)}, lambda p, d: p.startswith("wino2") and d["splitk"] > 1),
    "wino4_whole":   (64, 512, 3, 4, {6: (23, 30), 4: (27, 34)}, lambda p, d: p.startswith("wino4") and d["pieces"] == 1 and d["grid"] > 1),
    "wino4_tail":    (128, 512, 3, 4, {6: (35, 39), 4: (43, 47)}, lambda p, d: p.startswith("wino4") and "+tail" in p and d["pieces"] > 1 and d["full_wg"] > 0),
    "wino4_small":   (128, 64, 3, 4, {6: (7, 9), 4: (7, 9)}, lambda p, d: p.startswith("wino4") and "+tail" in p and d["pieces"] > 1 and d["full_wg"] == 0),
}
FORMS = ["broadcast", "slots", "frames"]       # res_bs = 0 | slot stride, res_bmod = 0 | slot stride, res_bmod = G


def residual_operand(form, k, G, Cout, OH, OW, seed):
    """(device buffer, res_bs, res_bmod, the residual of every batch element [B, Cout, OH, OW]).  The slots are dense + 96 floats apart, so a
    kernel that ignores the stride and one that ignores the modulo read different wrong data; the buffer always holds B slots (those a
    per-frame residual does not use are junk), so neither of the two reads outside it."""
    B, dense = k * G, OH * OW * Cout
    g = torch.Generator().manual_seed(seed)
    if form == "broadcast":
        r = torch.randn(1, Cout, OH, OW, generator=g)
        return nhwc(r).reshape(-1), 0, 0, r.expand(B, -1, -1, -1)
    rs = dense + 96
    if form == "slots":
        r = torch.randn(B, Cout, OH, OW, generator=g)
        return strided(r.permute(0, 2, 3, 1), rs), rs, 0, r
    r = torch.randn(G, Cout, OH, OW, generator=g)
    buf = torch.full((B, rs), JUNK)
    buf[:G, :dense] = r.permute(0, 2, 3, 1).reshape(G, dense)
    return buf.reshape(-1).cuda(), rs, G, r[[b % G for b in range(B)]]


@pytest.mark.parametrize("k,G", KG, ids=[f"k{k}G{G}" for k, G in KG])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(RES_PATHS))
def test_residual_forms_on_every_epilogue(name, form, k, G):
    """Batch element b = object * G + frame adds the residual of ITS form; both ReLUs in the batches of 6, ReLU on the output alone in
    the batch of 4 (ReLU on the input changes the conv, not the epilogue)."""
    Cin, Cout, K, f4, sizes, want = RES_PATHS[name]
    B = k * G
    H, W = sizes[B]
    flags = (3 if B == 6 else 2) | f4
    p, d = plan(B, H, W, Cin, Cout, K, 1, flags)
    assert want(p, d), (p, d)                                    # the plan does not depend on the residual's form
    x, w, b, conv = conv_data(B, H, W, Cin, Cout, K, 1, flags & 1)
    rbuf, res_bs, res_bmod, r = residual_operand(form, k, G, Cout, H, W, B * 31 + G)
    ref = F.relu(conv + r.double())
    run_and_check(ref, nhwc(x), dev(w.permute(0, 2, 3, 1)), dev(b), B, H, W, Cin, Cout, K, 1, flags, res=rbuf, res_bs=res_bs, res_bmod=res_bmod,
                  y_pad=64 if form == "slots" else 0)
    assert last_path() == p, (last_path(), p)


def test_a_per_frame_residual_keeps_a_large_pointwise_conv_off_the_chain_kernel():
    """affine_out: the chain kernel addresses y and the residual as one dense [M][N] matrix; its dense twin must take it."""
    k, G, H, W, Cin, Cout = 3, 2, 96, 100, 64, 128
    B = k * G
    assert plan(B, H, W, Cin, Cout, 1, 1, 2)[0].startswith("direct_pointwise_chain")
    x, w, b, conv = conv_data(B, H, W, Cin, Cout, 1, 1, 0)
    xd, wd, bd = nhwc(x), dev(w.permute(0, 2, 3, 1)), dev(b)
    g = torch.Generator().manual_seed(5)
    r = torch.randn(B, Cout, H, W, generator=g)
    run_and_check(F.relu(conv + r.double()), xd, wd, bd, B, H, W, Cin, Cout, 1, 1, 2, res=nhwc(r))
    assert last_path().startswith("direct_pointwise_chain"), last_path()
    rbuf, res_bs, res_bmod, rf = residual_operand("frames", k, G, Cout, H, W, 6)
    run_and_check(F.relu(conv + rf.double()), xd, wd, bd, B, H, W, Cin, Cout, 1, 1, 2, res=rbuf, res_bs=res_bs, res_bmod=res_bmod)
    assert last_path().startswith("direct_pointwise ") and "chain" not in last_path(), last_path()
