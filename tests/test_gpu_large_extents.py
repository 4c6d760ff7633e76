"""GPU: operand extents of 1 to 8 GiB - the 32-bit byte offsets of the conv kernels, the guards around them (2 GiB inputs, 4 GiB dense
outputs, the chain kernel's 2 GiB output, 4 GiB Winograd workspaces) and the 64-bit strides of the elementwise, layout and gather kernels.

Convs (large_extents.py): a batch of thousands of ragged 17x23 images is B copies of 3 base images, a residual has period 2, so F.conv2d in
fp64 on the CPU of the 3 base images is the reference of EVERY output element; the comparison runs on the device in fp64, chunk by chunk,
against the suite's 2e-5 max-norm bound for convs.  The output is NaN before the call and must be finite after it, a 64-float NaN guard
behind it must survive, and every case pins its kernel family.  Elementwise kernels: the same formula in fp64 with torch on the device, at
the tolerance of the op's test in test_gpu_small_kernels.py; what a launch must not touch is NaN and is counted afterwards.

Every case states its peak device memory (none above 16 GB), frees its buffers, and none skips on free memory."""
import ctypes as C
import gc
import threading

import pytest
import torch
import torch.nn.functional as F

from eva_vos_amd import _lib
from gpu_util import EPS, aggregate_bound, guard_intact, guarded, kernel, model_handle, stream, tap_max, torch_aggregate_wbg, up4_prob
from large_extents import ENGINE_CONVS, LARGE_CONVS, P, REFUSED_CONV, RES_P, periodic_check

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
BOUND = 2e-5          # test_conv_matches_fp64_reference


class DeviceMemorySampler(threading.Thread):
    """The most device memory in use while a case runs, sampled every half millisecond: torch's own statistics do not see what the library
    allocates for the length of a call (the conv hook's Winograd workspace and slabs)."""

    def __init__(self):
        super().__init__(daemon=True)
        self.base = self.used()
        self.peak, self.done = self.base, threading.Event()

    @staticmethod
    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free

    def run(self):
        while not self.done.wait(0.0005):
            self.peak = max(self.peak, self.used())


@pytest.fixture(autouse=True)
def free_device_memory():
    """Buffers of gigabytes are freed between the cases; after a device fault (every later call reports it) nothing more is started.  Prints
    the peak of the case: torch's own buffers, and the sampled growth of the device's memory in use (the library's allocations included)."""
    torch.cuda.reset_peak_memory_stats()
    sampler = DeviceMemorySampler()
    sampler.start()
    yield
    sampler.done.set()
    sampler.join()
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:
        pytest.exit(f"the device reports a fault, no further case is started: {ex}", returncode=3)
    print(f"peak of torch's own buffers {torch.cuda.max_memory_allocated() / 1e9:.1f} GB, sampled peak of the device's memory in use "
          f"{(sampler.peak - sampler.base) / 1e9:.1f} GB")
    gc.collect()
    torch.cuda.empty_cache()


def err():
    return _lib.lib().stcn_last_error().decode()


def last_path():
    return _lib.lib().stcn_last_conv_path().decode()


def conv_ex(x, w, b, y, B, H, W, c0, Cout, K, s, flags, splitk=0, res=None, x1=None, c1=0, bs0=-1):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.lib().stcn_test_conv_ex(stream(), p(x), p(w), p(b), p(res), p(y), B, H, W, c0, Cout, K, K, s, K // 2, flags, splitk,
                                      p(x1), c1, bs0, -1, -1, 0, -1)
    torch.cuda.synchronize()
    return rc


def conv_operands(case, n_img=P):
    """Seeded base images [n_img, Cin, H, W], weights and bias on the CPU."""
    B, H, W, Cin, Cout, K, s, flags, splitk = case
    g = torch.Generator().manual_seed(B * 1000003 + H * 10007 + W * 101 + Cin * 7 + Cout + K)
    xb = torch.randn(n_img, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (2.0 / (Cin * K * K)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    return g, xb, w, b


def periodic_batch(base, B):
    """base [p, ...] on the device -> [B, ...], element b = base[b % p]."""
    return base.index_select(0, torch.arange(B, device="cuda") % base.shape[0])


def run_periodic_conv(case, residual, path):
    B, H, W, Cin, Cout, K, s, flags, splitk = case
    g, xb, w, b = conv_operands(case)
    ref = F.conv2d((F.relu(xb) if flags & 1 else xb).double(), w.double(), b.double(), stride=s, padding=K // 2)      # [3, Cout, OH, OW]
    OH, OW = ref.shape[2:]
    dense = OH * OW * Cout
    expected = ref.permute(0, 2, 3, 1).reshape(P, dense).cuda()
    res = None
    if residual:                            # element b adds res[b % 2]: the expected values have period 6
        rb = torch.randn(RES_P, Cout, OH, OW, generator=g).permute(0, 2, 3, 1).reshape(RES_P, dense).cuda()
        j = torch.arange(P * RES_P, device="cuda")
        expected = expected[j % P] + rb[j % RES_P].double()
        res = periodic_batch(rb, B)
    if flags & 2:
        expected = F.relu(expected)
    x = periodic_batch(xb.permute(0, 2, 3, 1).contiguous().cuda(), B)
    n = B * dense
    y = guarded(n, guard=GUARD)
    rc = conv_ex(x, w.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda(), y, B, H, W, Cin, Cout, K, s, flags, splitk, res=res)
    assert rc == 0, err()
    assert last_path().startswith(path), (last_path(), path)
    assert guard_intact(y, n), "the guard behind the output was written"
    worst, unwritten = periodic_check(y[:n], expected)
    rel = worst / float(expected.abs().max())
    print(f"{last_path()}: x {x.numel() * 4 / 2**30:.2f} GiB, y {n * 4 / 2**30:.2f} GiB, max-norm relative error {rel:.2e}, {unwritten} values not finite")
    assert unwritten == 0, f"{unwritten} addressed output values are not finite"
    assert rel < BOUND, rel


@pytest.mark.parametrize("name,case,residual,path,peak_gb", LARGE_CONVS, ids=[f"{c[0]}-peak{c[4]}GB" for c in LARGE_CONVS])
def test_conv_with_operands_of_gigabytes(name, case, residual, path, peak_gb):
    """The windows of the planner table (large_extents.py); x / y / V extents are in the ids, the peak device memory behind `peak`."""
    run_periodic_conv(case, residual, path)


def test_cout_1_conv_with_an_input_just_under_2_gib():
    """decoder.pred's kernel (64-bit pointers, no descriptor): 5300 images, x = 1.98 GiB, y 8 MB.  Peak 11.6 GB: the hook allocates the Winograd
    workspace of every stride-1 3x3 shape, 8.7 GiB here, used or not."""
    run_periodic_conv((5300, 17, 23, 256, 1, 3, 1, 1, 0), False, "n1")


def test_forced_split_k_on_the_largest_output_its_slabs_hold():
    """The issue's row 'forced split-K reduce on a > 2 GiB output' cannot run: the conv hook's slab workspace is 16 Mi floats and conv_plan
    drops a split whose splitk * M * N floats do not fit (test_conv_plan.py pins that), so conv_reduce_kernel never sees more than 8 Mi output
    floats under splitk = 2.  This is the largest 64 -> 256 3x3 batch of 17x23 images below that: B = 83, y = 33 MB, with the residual.
    Peak 0.3 GB."""
    run_periodic_conv((83, 17, 23, 64, 256, 3, 1, 3, 2), True, "direct splitk=2")


# ------------------------------------------------------------------------------------------------ engine-shaped frames
def band_reference(xb, w, b, r0, rows, flags):
    """fp64 conv (3x3, stride 1, pad 1) of output rows [r0, r0 + rows) of the image xb [Cin, H, W]: only its rows + 2 input rows are read."""
    H = xb.shape[1]
    lo, hi = r0 - 1, r0 + rows + 1
    xin = xb[:, max(lo, 0):min(hi, H)].double()
    xin = F.pad(xin, (0, 0, max(0, -lo), max(0, hi - H)))                       # zero rows where the band touches the image border
    if flags & 1:
        xin = F.relu(xin)
    out = F.conv2d(xin[None], w.double(), b.double(), padding=(0, 1))[0]         # [Cout, rows, W]
    return F.relu(out) if flags & 2 else out


@pytest.mark.parametrize("name,case,residual,path,peak_gb", ENGINE_CONVS, ids=[f"{c[0]}-peak{c[4]}GB" for c in ENGINE_CONVS])
def test_conv_of_whole_frames_at_engine_batch_sizes(name, case, residual, path, peak_gb):
    """1080p at B = 16 (x and y 1.99 GiB, direct_big with tail split) and 720p at k = 32 (V = 3.96 GiB in one F(4x4) launch): b * batch_stride
    dominates every offset.  An fp64 conv of whole frames of this size is too slow on the CPU, so: fp64 bands of 6 output rows - the first
    rows of element 0, rows in the middle of the middle element, the last rows of the last element (both outputs end 8 MB and 250 MB short
    of 2^31 bytes, so no band holds that offset itself; the last band is the one next to it) - and, on the device, every element b against
    element b % 3 of the same output, both at 2e-5 of the largest band value."""
    B, H, W, Cin, Cout, K, s, flags, splitk = case
    g, xb, w, b = conv_operands(case)
    dense = H * W * Cout
    x = periodic_batch(xb.permute(0, 2, 3, 1).contiguous().cuda(), B)
    n = B * dense
    y = guarded(n, guard=GUARD)
    rc = conv_ex(x, w.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda(), y, B, H, W, Cin, Cout, K, s, flags, splitk)
    assert rc == 0, err()
    assert last_path().startswith(path), (last_path(), path)
    assert guard_intact(y, n), "the guard behind the output was written"
    yv = y[:n].reshape(B, H, W, Cout)
    scale, worst = 0.0, 0.0
    for bi, r0 in ((0, 0), (B // 2, H // 2 - 3), (B - 1, H - 6)):
        ref = band_reference(xb[bi % P], w, b, r0, 6, flags)                     # [Cout, 6, W]
        got = yv[bi, r0:r0 + 6].permute(2, 0, 1).cpu().double()
        assert torch.isfinite(got).all(), (bi, r0)
        scale, worst = max(scale, float(ref.abs().max())), max(worst, float((got - ref).abs().max()))
    print(f"{last_path()}: bands max-norm relative error {worst / scale:.2e}")
    assert worst / scale < BOUND, worst / scale
    worst, unwritten = periodic_check(y[:n], yv[:P].reshape(P, dense).double())
    print(f"every element against element b % 3: {worst / scale:.2e}, {unwritten} values not finite")
    assert unwritten == 0 and worst / scale < BOUND, (unwritten, worst / scale)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("K", [1, 3])
def test_an_input_of_2_gib_is_refused_without_a_launch(K):
    """plan_conv's limit, one source and two; nothing runs, so the buffers need not have the extents the shape claims (K = 3: the hook
    allocates the 9.5 GB Winograd workspace of the shape before it plans)."""
    B, H, W, Cin, Cout = REFUSED_CONV[:5]
    y = torch.full((1024,), NAN, device="cuda")
    x, b = torch.zeros(1024, device="cuda"), torch.zeros(Cout, device="cuda")
    assert conv_ex(x, torch.zeros(Cout, K, K, Cin, device="cuda"), b, y, B, H, W, Cin, Cout, K, 1, 2) == -1 and "2 GiB" in err(), err()
    # a second source of 256 channels behind a first of 64 (0.54 GB, allowed)
    assert conv_ex(x, torch.zeros(Cout, K, K, 64 + Cin, device="cuda"), b, y, B, H, W, 64, Cout, K, 1, 2, x1=x, c1=Cin) == -1 and "2 GiB" in err(), err()
    # a strided input: B * bs0 * 4 = 2^31 exactly
    assert conv_ex(x, torch.zeros(Cout, K, K, 64, device="cuda"), b, y, 4, 5, 5, 64, Cout, K, 1, 2, bs0=1 << 27) == -1 and "2 GiB" in err(), err()
    assert torch.isnan(y).all(), "a refused conv wrote to its output"


def test_a_memory_of_2_pow_24_rows_is_refused_by_the_stage_call_without_a_launch(nets):
    """The read kernels build the key descriptor as (unsigned)N * 256 bytes.  T * h16 * w16 = 2^24 exactly; refused before the bank is touched,
    so the tensors need not have that extent."""
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.stcn_stage_create(model_handle(nets), 128, 128, 1, stream(), C.byref(h)), "stcn_stage_create")
    try:
        t = torch.zeros(1024, device="cuda")
        p = C.c_void_p(t.data_ptr())
        T = (1 << 24) // 64
        assert lib.stcn_stage_segment(h, p, 1 << 24, p, 1 << 24, 0, T, 1, p, p, p, p, p) == -1 and "2^24" in err(), err()
    finally:
        lib.stcn_stage_destroy(h)


# ------------------------------------------------------------------------------------------------ elementwise kernels
NPIX = 480 * 864            # 414 720: the project's headline frame
T_ROW = 100 * NPIX          # a row of prob / agg [k + 1][T = 100][npix]


def count_nan(t, chunk=1 << 28):
    """NaNs of a 1-D tensor, in chunks (a sum over the whole mask makes an int64 copy of it: 11 GB for a 5.5 GB buffer; per chunk 2 GB)."""
    return sum(int(torch.count_nonzero(torch.isnan(t[i:i + chunk]))) for i in range(0, t.numel(), chunk))


def test_argmax_over_a_prob_of_4_4_gb():
    """kk = 33 rows of T = 34 frames of 1024 x 960 pixels: row strides of 134 MB, the last row starts 4.3 GB in.  Continuous random values:
    no ties.  Peak 5.2 GB."""
    kk, T, npix = 33, 34, 1024 * 960
    prob = torch.rand(kk, T * npix, device="cuda")
    masks = guarded(T * npix, torch.uint8)
    kernel("argmax", [prob, masks], [kk, T, npix])
    assert guard_intact(masks, T * npix)
    ref = torch.argmax(prob, dim=0).to(torch.uint8)
    assert len(torch.unique(ref)) == kk
    assert torch.equal(masks[:T * npix], ref)


def test_argmax_over_more_pixels_than_one_pass_of_its_grid_covers():
    """The elementwise launches are capped at 2^20 blocks of 256 and walk their items with the stride of the grid: T * npix = 2^28 + 1000 (648
    frames of 480p are 2^28 + 303 104) needs a second pass, in which only 4 blocks still have work.  kk = 2.  Peak 5.0 GB."""
    kk, T, npix = 2, 4, (1 << 26) + 250
    prob = torch.rand(kk, T * npix, device="cuda")
    masks = guarded(T * npix, torch.uint8)
    kernel("argmax", [prob, masks], [kk, T, npix])
    assert guard_intact(masks, T * npix)
    assert torch.equal(masks[:T * npix], (prob[1] > prob[0]).to(torch.uint8))


def test_sigmoid_aggregate_into_the_last_frame_of_a_5_5_gb_agg():
    """k = 32, agg rows 100 frames apart: row 32 of frame 99 ends at the end of the 5.5 GB buffer.  Bound as in
    test_sigmoid_aggregate_matches_the_fp64_formula: max(1e-6, 4 x the error of the formula in torch fp32 against fp64 on these logits).
    Peak 8.1 GB."""
    k = 32
    logit = torch.rand(k, NPIX, device="cuda") * 16 - 8
    ref = torch_aggregate_wbg(torch.sigmoid(logit.double()), keep_bg=True)
    err32 = float((torch_aggregate_wbg(torch.sigmoid(logit), keep_bg=True).double() - ref).abs().max())
    n = (k + 1) * T_ROW
    agg = guarded(n)
    kernel("sigmoid_aggregate", [logit, agg[99 * NPIX:]], [k, NPIX, T_ROW])
    assert guard_intact(agg, n)
    assert count_nan(agg[:n]) == n - (k + 1) * NPIX, "a frame other than the last was written, or a value of the last was not"
    got = agg[:n].reshape(k + 1, 100, NPIX)[:, 99].double()
    worst = float((got - ref).abs().max())
    print(f"kernel {worst:.2e}, torch fp32 {err32:.2e}, bound {aggregate_bound(err32):.2e}")
    assert worst < aggregate_bound(err32), (worst, err32)


def test_up4_sigmoid_aggregate_into_the_last_two_frames_of_wide_rows():
    """G = 2 frames of k = 8 objects, agg rows 100 frames apart and the frames one frame apart (agg_gs = npix), written as frames 98 and 99:
    row 8 of frame 99 ends at the end of the 1.5 GB buffer.  Bound as in test_up4_sigmoid_aggregate_matches_the_fp64_formula.  Peak 4.0 GB."""
    k, G, h4, w4 = 8, 2, 120, 216
    hw4 = h4 * w4
    logit = torch.rand(k, G, h4, w4, device="cuda") * 16 - 8
    ref = torch.stack([torch_aggregate_wbg(up4_prob(logit[:, g].double()), keep_bg=True) for g in range(G)])      # [G, k + 1, H, W]
    f32 = torch.stack([torch_aggregate_wbg(up4_prob(logit[:, g]), keep_bg=True) for g in range(G)])
    err32 = float((f32.double() - ref).abs().max())
    n = (k + 1) * T_ROW
    agg = guarded(n)
    kernel("up4_sigmoid_aggregate", [logit, agg[98 * NPIX:]], [k, h4, w4, T_ROW, G * hw4, G, hw4, NPIX])
    assert guard_intact(agg, n)
    assert count_nan(agg[:n]) == n - G * (k + 1) * NPIX
    got = agg[:n].reshape(k + 1, 100, NPIX)[:, 98:].permute(1, 0, 2).reshape(G, k + 1, 4 * h4, 4 * w4).double()
    worst = float((got - ref).abs().max())
    print(f"kernel {worst:.2e}, torch fp32 {err32:.2e}, bound {aggregate_bound(err32):.2e}")
    assert worst < aggregate_bound(err32), (worst, err32)


def test_interact_mask_on_the_last_frame_of_a_5_5_gb_prob():
    """kk = 33 rows 100 frames apart, the interaction on frame 99; exact, and the other 99 frames of every row stay NaN.  Peak 8.3 GB."""
    kk, nh, nw, H, W, lh, lw = 33, 480, 864, 470, 850, 5, 7
    mask = torch.rand(kk, H, W, device="cuda")
    n = kk * T_ROW
    prob = guarded(n)
    rows = prob[:n].reshape(kk, 100, NPIX)
    before = torch.rand(kk, NPIX, device="cuda")
    rows[:, 99] = before
    pad = torch.zeros(kk, nh, nw, device="cuda")
    pad[:, lh:lh + H, lw:lw + W] = mask
    m = pad.reshape(kk, NPIX)
    d = m - before
    padded, pos, neg = guarded(kk * NPIX), guarded(kk * NPIX), guarded(kk * NPIX)
    kernel("interact_mask", [mask, prob[99 * NPIX:], padded, pos, neg], [kk, H, W, nh, nw, lw, lh, T_ROW, kk])
    assert guard_intact(prob, n) and guard_intact(padded, kk * NPIX) and guard_intact(pos, kk * NPIX) and guard_intact(neg, kk * NPIX)
    assert count_nan(prob[:n]) == n - kk * NPIX
    assert torch.equal(rows[:, 99], m) and torch.equal(padded[:kk * NPIX].reshape(kk, NPIX), m)
    assert torch.equal(pos[:kk * NPIX].reshape(kk, NPIX), d.clamp(0, 1)) and torch.equal(neg[:kk * NPIX].reshape(kk, NPIX), (-d).clamp(0, 1))


@pytest.mark.parametrize("B,G", [(16, 0), (32, 4), (33, 3)],
                         ids=["B16-out2.1GB-peak8.4GB", "B32-out4.3GB-skip-per-frame-peak9.5GB", "B33-second-pass-of-the-grid-peak9.7GB"])
def test_upsample2x_add_with_outputs_beyond_2_and_4_gb(B, G):
    """h = 136, w = 240, C = 256.  B = 16: a dense skip of the output's size; B = 32: the skip per frame of an [object][frame] batch (skip_bmod = G).
    B = 33: 2^28 + 7.3 M work items of 4 floats, more than one pass of the capped grid covers - the frames of the last element come from the second.
    Per element against F.interpolate in fp64 on the device, at the bound of test_upsample2x_add_matches_interpolate_plus_skip."""
    h, w, Cc = 136, 240, 256
    dense = 4 * h * w * Cc
    x = torch.randn(B, h, w, Cc, device="cuda")
    skip = torch.randn(G or B, 2 * h, 2 * w, Cc, device="cuda")
    n = B * dense
    u = guarded(n)
    kernel("upsample2x_add", [x, skip, u], [B, h, w, Cc, dense, G])
    assert guard_intact(u, n)
    worst_excess, worst = -1.0, 0.0
    for b in range(B):
        xb = x[b].permute(2, 0, 1)[None].double()
        sk = skip[b % G if G else b].permute(2, 0, 1)[None].double()
        ref = F.interpolate(xb, scale_factor=2, mode="bilinear", align_corners=False) + sk
        got = u[b * dense:(b + 1) * dense].reshape(1, 2 * h, 2 * w, Cc).permute(0, 3, 1, 2).double()
        assert torch.isfinite(got).all(), b
        e = (got - ref).abs()
        worst, worst_excess = max(worst, float(e.max())), max(worst_excess, float((e - 16 * EPS * (sk.abs() + tap_max(xb, 0.5))).max()))
    print(f"B={B}: max |error| {worst:.2e}, max (error - bound) {worst_excess:.2e}")
    assert worst_excess <= 0, worst_excess


def test_maxpool_of_a_4_3_gb_input():
    """B = 32 frames of 544 x 960 x 64, all negative; exact against F.max_pool2d per frame.  Peak 5.6 GB."""
    B, H, W, Cc = 32, 544, 960, 64
    x = torch.rand(B, H, W, Cc, device="cuda").neg_().sub_(0.01)
    dense = (H // 2) * (W // 2) * Cc
    y = guarded(B * dense)
    kernel("maxpool3x3s2", [x, y], [B, H, W, Cc])
    assert guard_intact(y, B * dense)
    for b in range(B):
        ref = F.max_pool2d(x[b].permute(2, 0, 1)[None], 3, 2, 1)[0].permute(1, 2, 0)
        assert torch.equal(y[b * dense:(b + 1) * dense].reshape(ref.shape), ref), b


def test_copy_rows_with_row_strides_beyond_2_pow_31_elements():
    """Two rows 2^31 + 24 floats apart on the source side, then on the destination side (one 8.6 GB buffer serves both); exact, and all the
    buffer but the two rows stays NaN.  Peak 11.0 GB."""
    rows, n, wide, near = 2, 1000, (1 << 31) + 24, 1100
    big = guarded(wide + n)
    src = torch.rand(rows, n, device="cuda")
    big[:n], big[wide:wide + n] = src[0], src[1]
    dst = guarded(rows * near)
    kernel("copy_rows", [big, dst], [wide, near, rows, n])
    assert guard_intact(dst, rows * near)
    body = dst[:rows * near].reshape(rows, near)
    assert torch.equal(body[:, :n], src) and torch.isnan(body[:, n:]).all()
    big.fill_(NAN)
    src2 = torch.rand(rows, near, device="cuda")
    kernel("copy_rows", [src2, big], [near, wide, rows, n])
    assert guard_intact(big, wide + n)
    assert torch.equal(big[:n], src2[0, :n]) and torch.equal(big[wide:wide + n], src2[1, :n])
    assert count_nan(big[:wide + n]) == wide + n - rows * n


def test_transposes_with_planes_1_1e9_elements_apart():
    """B = 2 tensors of C = 512 planes of R = 140 rows, the tensors 1.1e9 floats (4.4 GB) apart; both directions exact, and the 4.4 GB between
    and around the planes stay NaN.  Peak 6.8 GB."""
    B, R, Cc, bs = 2, 140, 512, 1100000000
    lib = _lib.lib()
    n = bs + Cc * R
    planes = guarded(n)
    vals = torch.rand(B, Cc, R, device="cuda")
    planes[:Cc * R], planes[bs:bs + Cc * R] = vals[0].reshape(-1), vals[1].reshape(-1)
    rows = guarded(B * R * Cc)
    _lib.check(lib.stcn_test_transpose(stream(), C.c_void_p(planes.data_ptr()), C.c_void_p(rows.data_ptr()), B, R, Cc, R, bs, 1), "stcn_test_transpose")
    torch.cuda.synchronize()
    assert guard_intact(rows, B * R * Cc)
    assert torch.equal(rows[:B * R * Cc].reshape(B, R, Cc), vals.permute(0, 2, 1))
    planes.fill_(NAN)
    src = torch.rand(B, R, Cc, device="cuda")
    _lib.check(lib.stcn_test_transpose(stream(), C.c_void_p(src.data_ptr()), C.c_void_p(planes.data_ptr()), B, R, Cc, R, bs, 0), "stcn_test_transpose")
    torch.cuda.synchronize()
    assert guard_intact(planes, n)
    assert torch.equal(planes[:Cc * R].reshape(Cc, R), src[0].t()) and torch.equal(planes[bs:bs + Cc * R].reshape(Cc, R), src[1].t())
    assert count_nan(planes[:n]) == n - B * Cc * R


def test_memory_read_gathers_from_value_planes_beyond_4_gib():
    """N = 168 480 rows (104 frames at 480p), Q = 97, k = 16: mv is 5.5 GB and the planes of objects 13 to 15 start beyond 4 GiB.  The selection
    (idx, w) must equal the k = 1 read of the same keys, and every object's read-out the fp64 gather of ITS rows with those weights, at 2e-5
    of the largest read-out value - through both gathers: merge_readout_kernel's own loop over the objects (idx / w requested) and
    gather_readout_kernel (not requested).  Peak 5.6 GB."""
    N, Q, k, TK = 168480, 97, 16, 50
    mk, qk = torch.randn(N, 64, device="cuda"), torch.randn(Q, 64, device="cuda")
    mv = torch.randn(k, N, 512, device="cuda")
    lib = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def read(k_, with_idx):
        idx, w = torch.full((Q, TK), -1, dtype=torch.int32, device="cuda"), torch.full((Q, TK), NAN, device="cuda")
        ro = guarded(k_ * Q * 512)
        _lib.check(lib.stcn_test_memory_read(stream(), p(mk), p(mv), p(qk), N, Q, k_, p(idx) if with_idx else None, p(w) if with_idx else None, p(ro)),
                   "stcn_test_memory_read")
        torch.cuda.synchronize()
        assert guard_intact(ro, k_ * Q * 512)
        return idx.long(), w, ro[:k_ * Q * 512].reshape(k_, Q, 512)

    i1, w1, _ = read(1, True)
    assert (i1 >= 0).all() and (i1 < N).all() and torch.isfinite(w1).all()
    ik, wk, ro_merge = read(k, True)
    assert torch.equal(ik, i1) and torch.equal(wk, w1)
    _, _, ro_gather = read(k, False)
    ref = torch.stack([(mv[o][i1].double() * w1.double()[:, :, None]).sum(1) for o in range(k)])       # [k, Q, 512]
    scale = float(ref.abs().max())
    for name, ro in (("merge", ro_merge), ("gather", ro_gather)):
        assert torch.isfinite(ro).all(), name
        rel = float((ro.double() - ref).abs().max()) / scale
        print(f"{name}: max-norm relative error {rel:.2e}")
        assert rel < BOUND, (name, rel)
