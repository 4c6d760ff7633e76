"""Shared by test_gpu_large_extents.py (GPU) and test_conv_plan.py (CPU): the conv cases whose operands are 1 to 8 GiB, the paths the planner
must give them, and the checker of a periodic batch.

The method: a batch of thousands of small images is B copies of P = 3 base images (element b = base[b % 3]), a residual has period 2, so the
expected output of element b is one of 3 (or, with a residual, 6) small fp64 results.  3 never divides 2^31 or 2^32 bytes: a write whose
32-bit offset wrapped or changed sign lands in an element of another phase and shows as a wrong value there and as an unwritten (NaN)
element where it belonged."""
import torch

P = 3                # base images of a batch
RES_P = 2            # period of a residual

# (id, (B, H, W, Cin, Cout, K, stride, flags, splitk), residual, the path the planner must give (prefix), peak device memory in GB)
# flags: 1 ReLU on the input, 2 ReLU on the output, 4 as a decoder layer (F(4x4) eligible).  The peak is the larger of two phases: the launch
# (x, y, the dense residual, and the V workspace the conv hook allocates for every stride-1 3x3 conv - the larger of both Winograd forms, used
# or not - which it frees on return) and the check (x, y, the residual and 1.7 GB of fp64 chunks).
LARGE_CONVS = [
    ("chain-y2.09G", (5600, 17, 23, 64, 256, 1, 1, 2, 0), False, "direct_pointwise_chain", 4.5),
    ("chain-guard-y2.10G", (9000, 17, 23, 64, 160, 1, 1, 2, 0), False, "direct_pointwise ", 4.9),
    ("chain-N160-y1.17G", (5000, 17, 23, 64, 160, 1, 1, 2, 0), False, "direct_pointwise_chain", 3.5),
    ("chain-y4.00G-last-dense", (5363, 17, 23, 64, 512, 1, 1, 2, 0), False, "direct_pointwise_chain", 6.6),
    ("pointwise-y4.18G-res", (5600, 17, 23, 64, 512, 1, 1, 2, 0), True, "direct_pointwise ", 11.2),
    ("direct3x3-y2.09G-res", (5600, 17, 23, 64, 256, 3, 1, 3, 0), True, "direct ", 7.6),
    ("big-s2-x1.98G", (5300, 17, 23, 256, 512, 3, 2, 2, 0), False, "direct_big", 5.0),
    ("narrow-15.6Mrows", (40000, 17, 23, 32, 32, 1, 1, 2, 0), False, "direct_narrow", 5.7),
    ("stem-y2.63G", (300, 368, 400, 8, 64, 7, 2, 2, 0), False, "direct_smallc", 5.9),
    ("wino2-V3.96G", (2400, 17, 23, 256, 64, 3, 1, 2, 0), False, "wino2", 5.6),
    ("wino2-y3.04G-V3.13G-res", (3800, 17, 23, 128, 512, 3, 1, 3, 0), True, "wino2", 10.3),
    ("wino2-declines-V7.25G", (4400, 17, 23, 256, 64, 3, 1, 2, 0), False, "direct +tail", 10.1),
    ("wino4-chunked-y2.09G", (5600, 17, 23, 64, 256, 3, 1, 6, 0), False, "wino4 chunks=10", 5.4),
    ("wino4-chunked-V3.09G", (3000, 17, 23, 256, 64, 3, 1, 6, 0), False, "wino4 chunks=11", 6.9),
    ("wino4-declines-V5.46G", (5300, 17, 23, 256, 64, 3, 1, 6, 0), False, "direct +tail", 12.1),
]
# the two engine-shaped cases: whole frames, b * batch_stride dominates every offset
ENGINE_CONVS = [
    ("1080p-B16-xy1.99G", (16, 272, 480, 256, 256, 3, 1, 7, 0), False, "direct_big +tail", 13.0),
    ("720p-k32-V3.96G-one-launch", (32, 180, 320, 256, 256, 3, 1, 7, 0), False, "wino4 chunks=1", 11.4),
]
REFUSED_CONV = (5400, 17, 23, 256, 64, 3, 1, 2, 0)          # x = 2.16e9 bytes


def conv_peak_gb(case, residual, chunk_elems=1 << 26):
    """Peak device memory of a periodic conv case in GB (1e9 bytes), worked out from its shape: the larger of the launch phase - x, y, the dense
    residual, the V workspace the conv hook allocates for a stride-1 3x3 conv (the larger of both Winograd forms) and its 64 MB of slabs - and
    of the check phase - x, y, the residual, the expected values and the three fp64 temporaries and the mask of one chunk of periodic_check."""
    B, H, W, Cin, Cout, K, s, flags, splitk = case
    OH, OW = (H + 2 * (K // 2) - K) // s + 1, (W + 2 * (K // 2) - K) // s + 1
    dense, period = OH * OW * Cout, P * RES_P if residual else P
    operands = (B * H * W * Cin + B * dense * (2 if residual else 1)) * 4
    v = 0
    if K == 3 and s == 1:
        pad = lambda n, u: -(-n // u) * u
        v = 4 * max(16 * Cin * pad(B * -(-OH // 2) * -(-OW // 2), 64), 36 * Cin * pad(B * -(-OH // 4) * -(-OW // 4), 128))
    chunk = max(1, chunk_elems // (period * dense)) * period * dense
    return max(operands + v + (64 << 20), operands + chunk * 25 + period * dense * 8) / 1e9


def periodic_check(y, expected, chunk_elems=1 << 26):
    """y: 1-D tensor of B * dense values, batch element b at b * dense; expected: [period, dense] fp64, element b must equal expected[b % period].
    Returns (the largest |y - expected| over the finite values of y, the count of values of y that are not finite), every value looked at,
    in chunks of whole periods of about chunk_elems values."""
    period, dense = expected.shape
    B = y.numel() // dense
    assert y.numel() == B * dense
    per = max(1, chunk_elems // (period * dense)) * period
    err, bad = 0.0, 0
    for b0 in range(0, B, per):
        part = y[b0 * dense:min(B, b0 + per) * dense].reshape(-1, dense)
        n = part.shape[0]
        whole = n // period
        for lo, hi, exp in ((0, whole * period, expected), (whole * period, n, expected[:n - whole * period])):
            if hi == lo:
                continue
            d = (part[lo:hi].reshape(-1, exp.shape[0], dense).double() - exp).abs_()
            finite = torch.isfinite(d)
            bad += int((~finite).sum())
            err = max(err, float(torch.where(finite, d, torch.zeros((), dtype=d.dtype, device=d.device)).max()))
    return err, bad
