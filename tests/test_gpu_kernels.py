"""GPU: each hand-written HIP kernel family against a CPU reference of the same op (through the C ABI)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import call, dev, nhwc, stream
from oracle import stcn_oracle as O

pytestmark = pytest.mark.gpu

#        B   H    W   Cin  Cout K  s  flags splitk
CONVS = [
    (1, 30, 54, 1024, 256, 1, 1, 0, 0),     # key encoder 1x1
    (1, 30, 54, 256, 256, 3, 1, 2, 0),      # 3x3 + relu out
    (1, 28, 44, 128, 128, 3, 2, 0, 1),      # stride 2, no split
    (1, 30, 54, 512, 64, 3, 1, 0, 4),       # forced split-K 4
    (2, 17, 23, 64, 128, 3, 1, 3, 0),       # ragged M, batch 2, relu in+out, residual
    (1, 64, 80, 4, 64, 7, 2, 2, 0),         # key stem (Cin padded 3->4)
    (2, 48, 64, 8, 64, 7, 2, 2, 0),         # value stem (Cin padded 5->8), batch 2
    (1, 40, 56, 12, 32, 3, 1, 2, 0),        # fusion conv1 (9->12 channels), narrow tile
    (1, 40, 56, 32, 32, 3, 1, 0, 0),        # fusion 32->32 + residual
    (1, 21, 37, 32, 32, 3, 1, 2, 0),        # FusionNet kernel: rows not a multiple of the 8-row patch, ragged second column tile
    (1, 9, 70, 12, 32, 3, 1, 2, 0),         # ... its 12-channel instance, three column tiles
    (1, 480, 864, 32, 32, 3, 1, 2, 0),      # ... at the size it runs at (1620 patches: more than one round of workgroups)
    (1, 9, 7, 64, 64, 1, 1, 0, 0),          # tiny
    (1, 15, 27, 1280, 512, 3, 1, 1, 0),     # fuser-like big K, relu in, auto split
    (1, 30, 54, 256, 1, 3, 1, 1, 0),        # decoder.pred (Cout 1), relu in
    (1, 40, 56, 32, 1, 3, 1, 0, 0),         # fusion final_conv (Cout 1)
    (1, 21, 150, 32, 1, 3, 1, 1, 0),        # ... three 64-pixel strips, ragged rows and columns, ReLU on the input
    # more than one round of tiles: the plan balances the tail (whole rounds unsplit + K pieces of the last tiles)
    (2, 67, 65, 64, 256, 3, 1, 3, 0),       # 548 tiles = 512 + 36 x 4 pieces; ragged last tile, batch 2, residual, relus
    (1, 184, 192, 64, 32, 3, 1, 2, 0),      # narrow tiles: 276 = 256 + 20 x 4 pieces
    (1, 368, 400, 8, 64, 7, 2, 2, 0),       # generic-path stem: 575 = 512 + 63 x 3 pieces
    # Winograd F(2x2,3x3) path (stride-1 3x3, Cin >= 128, Cout % 64 == 0): odd sizes (ragged last tile row / column, padded
    # tile count), batch 2 with residual and both ReLUs, split over input channels when few tiles
    (2, 17, 23, 128, 128, 3, 1, 3, 0),
    (1, 31, 45, 256, 64, 3, 1, 0, 0),
    (3, 16, 20, 512, 192, 3, 1, 2, 0),
    (1, 6, 5, 128, 64, 3, 1, 1, 0),         # 9 tiles in one padded workgroup tile, split over input channels
    (5, 120, 216, 64, 64, 3, 1, 3, 0),      # 64 channels run F(2x2) only in large launches: layer1 of the key encoder over a 5-frame group
    # Cin = 1024: the 8-wave instance (2 positions per wave) by default; few tiles -> split over input channels (key_proj: N = 64,
    # key_comp: N = 512), batch 2 -> residual + modulo-free batch stride in the Winograd epilogue and in the split-K reduce
    (1, 14, 18, 1024, 64, 3, 1, 0, 0),
    (2, 10, 12, 1024, 512, 3, 1, 3, 0),
    (2, 30, 54, 1024, 128, 3, 1, 2, 0),     # enough tiles for an unsplit launch of the 8-wave instance
    # F(4x4,3x3) (flags bit 2 = "decoder layer"): ragged tiles (sizes not multiples of 4), batch with residual and ReLUs, a
    # partially filled workgroup tile, Cout = 32 (one n-tile) and 192, and the shapes it runs at (1/4 and 1/8 scale)
    (2, 17, 23, 128, 128, 3, 1, 7, 0),
    (1, 31, 45, 256, 64, 3, 1, 4, 0),
    (3, 16, 20, 512, 192, 3, 1, 6, 0),
    (1, 6, 5, 128, 32, 3, 1, 5, 0),
    (1, 120, 216, 256, 256, 3, 1, 5, 0),
    (2, 60, 108, 512, 256, 3, 1, 6, 0),
    # ... and its tail split: 288 workgroups of 32 tiles x 32 channels = one round of 256 + 32 tiles cut into 8 K pieces each
    (5, 30, 54, 512, 512, 3, 1, 6, 0),      # the 1/16-scale decoder layers over a 5-frame group
    (2, 52, 78, 256, 512, 3, 1, 7, 0),      # with a residual, both ReLUs, ragged tiles (13 x 20 per image)
    # ... and its chunked launches (transform / GEMM alternate over slices of whole rounds): 408 workgroups of 64 tiles, run a
    # second time under STCN_WINO4_CHUNK_MB=1 = two slices (32 + 19 tile blocks)
    (2, 120, 216, 128, 256, 3, 1, 7, 0),
    # ... and its SMALL launches: fewer workgroups than half a round of CUs - EVERY tile is cut into K pieces (the value encoder's fuser and
    # frame parts at batch 1: 1620 pixels x 512 channels = 64 workgroups x 4 pieces; one decoder frame at 1/8 scale: 104 x 2)
    (1, 30, 54, 1024, 512, 3, 1, 4, 0),
    (1, 30, 54, 256, 512, 3, 1, 7, 0),
    (2, 30, 54, 512, 512, 3, 1, 6, 0),      # batch 2 with a residual: 128 workgroups x 2 pieces
    (1, 60, 108, 512, 256, 3, 1, 5, 0),
    # ... and at Cin = 64 (W4_MIN_CIN since round 5: KB = 8, one K piece): the key trunk's res2 convs over a 5-frame batch, a ragged batch-1
    # shape (every tile cut into K pieces) and the value encoder's layer1 over the objects of a multi-object engine (advisor, round 5)
    (5, 120, 216, 64, 64, 3, 1, 7, 0),
    (1, 37, 51, 64, 96, 3, 1, 5, 0),
    (3, 61, 45, 64, 64, 3, 1, 6, 0),
    # pointwise instance (1x1, stride 1): ragged M, residual + ReLU, split-K, and the stride-2 1x1 that must NOT take it
    (2, 19, 21, 256, 192, 1, 1, 2, 0),
    (1, 30, 54, 512, 128, 1, 1, 0, 3),
    (2, 30, 54, 256, 512, 1, 2, 2, 0),
    # Cout 1 over a batch (the decoder runs decoder.pred at B = frames x objects): strips that cross image boundaries
    (6, 9, 70, 256, 1, 3, 1, 1, 0),
    (3, 21, 150, 32, 1, 3, 1, 0, 0),
]


# the kernel family every CONVS case must run as (prefix of stcn_last_conv_path() in the default variant): a shape that silently
# falls back to another instance would still pass the numerical comparison below
PATHS = [
    "direct_pointwise", "wino2", "direct splitk=1", "direct splitk=4", "direct splitk", "direct_smallc", "direct_smallc",
    "fusion_wino", "fusion_wino", "fusion_wino", "fusion_wino", "fusion_wino", "direct_pointwise", "wino2", "n1", "n1", "n1",
    "direct +tail", "direct_narrow +tail", "direct_smallc +tail",
    "wino2", "wino2", "wino2", "wino2", "wino2",
    "wino2", "wino2", "wino2",
    "wino4", "wino4", "wino4", "wino4", "wino4", "wino4",
    "wino4 chunks=1 +tail", "wino4",
    "wino4",
    "wino4 chunks=1 +tail", "wino4 chunks=1 +tail", "wino4 chunks=1 +tail", "wino4 chunks=1 +tail",
    "wino4", "wino4", "wino4",
    "direct_pointwise", "direct_pointwise splitk=3", "direct splitk",
    "n1", "n1",
]


def last_path():
    from eva_vos_amd import _lib
    return _lib.lib().stcn_last_conv_path().decode()


def _is_wino(Cin, Cout, K, s, splitk, tiles=0):
    return K == 3 and s == 1 and (Cin >= 128 or (Cin == 64 and tiles >= 16384)) and Cin % 32 == 0 and Cout % 64 == 0 and splitk == 0


def test_the_path_table_covers_every_case():
    assert len(PATHS) == len(CONVS)


def conv_fp64_case(B, H, W, Cin, Cout, K, s, flags):
    """The seeded operands of one CONVS-style case - bias always, a residual for batch 2 and the FusionNet shape - and F.conv2d of them in
    fp64 (ReLUs as flags bits 0 / 1 say): x, w, b, res (or None), ref, OH, OW.  Shared with tests/switch_arm_cases.py."""
    g = torch.Generator().manual_seed(Cin * 131 + Cout * 7 + K)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (2.0 / (Cin * K * K)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    OH, OW = (H + 2 * (K // 2) - K) // s + 1, (W + 2 * (K // 2) - K) // s + 1
    use_res = Cout > 1 and (B == 2 or (Cin == 32 and Cout == 32))
    res = torch.randn(B, Cout, OH, OW, generator=g) if use_res else None
    xin = F.relu(x) if flags & 1 else x
    ref = F.conv2d(xin.double(), w.double(), b.double(), stride=s, padding=K // 2)
    if res is not None:
        ref = ref + res.double()
    if flags & 2:
        ref = F.relu(ref)
    return x, w, b, res, ref, OH, OW


@pytest.mark.parametrize("B,H,W,Cin,Cout,K,s,flags,splitk,path", [c + (p,) for c, p in zip(CONVS, PATHS)])
def test_conv_matches_fp64_reference(B, H, W, Cin, Cout, K, s, flags, splitk, path, monkeypatch):
    x, w, b, res, ref, OH, OW = conv_fp64_case(B, H, W, Cin, Cout, K, s, flags)
    # Winograd-eligible shapes run under BOTH GEMM instances (16 waves x 1 position, 8 waves x 2 positions), whatever the
    # default choice for their channel count is
    monkeypatch.setenv("STCN_WINO_MIN_CIN", "64")          # the opt-in F(2x2) path of 64-channel layers stays tested
    monkeypatch.setenv("STCN_FUSION_CONV12", "1")          # the 12-channel instance of the FusionNet kernel is off by default
    variants = ("1", "2") if _is_wino(Cin, Cout, K, s, splitk, B * ((OH + 1) // 2) * ((OW + 1) // 2)) else (None,)
    if flags & 4:
        variants = (None, "chunk")
    if Cin in (12, 32) and Cout == 32 and K == 3:
        variants = (None, "direct")           # FusionNet layers: the in-workgroup Winograd kernel (default) and the direct one
    for ppw in variants:
        if ppw == "chunk":
            monkeypatch.setenv("STCN_WINO4_CHUNK_MB", "1")
        elif ppw == "direct":
            monkeypatch.setenv("STCN_FUSION_WINO", "0")
        elif ppw:
            monkeypatch.setenv("STCN_WINO_PPW", ppw)
        y = torch.empty(B, OH, OW, Cout, device="cuda")
        call("stcn_test_conv", stream(), nhwc(x), dev(w.permute(0, 2, 3, 1)), dev(b),
             None if res is None else nhwc(res), y, B, H, W, Cin, Cout, K, K, s, K // 2, flags, splitk)
        got = y.permute(0, 3, 1, 2).cpu().double()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err < 2e-5, (err, ppw)          # fp32 accumulation vs fp64
        # ... and it ran as the kernel this case is in the list for
        ran = last_path()
        want = {"direct": "fusion_direct", "1": "wino2 ppw=1", "2": "wino2 ppw=2", "chunk": "wino4"}.get(ppw, path)
        assert ran.startswith(want), (ran, want)
        if ppw == "chunk" and (B, H, W, Cin, Cout) == (2, 120, 216, 128, 256):
            assert "chunks=2" in ran, ran


#                B  H    W    Cin  Cout flags  (1x1 convs large enough for the chain kernel: >= 1536 tiles of 64x64)
CHAIN_CASES = [(5, 120, 216, 64, 256, 2),      # res2 conv3: 2 K tiles per tile, 8100 tiles, residual + ReLU
               (5, 120, 216, 256, 64, 2),      # res2 conv1: one n-tile per row block - consecutive tiles walk down M
               (5, 60, 108, 128, 512, 2),      # layer2 conv3
               (3, 97, 131, 96, 192, 3),       # odd K-tile count (3), 3 n-tiles (no panels), ragged M, ReLU on the input
               (3, 111, 120, 32, 320, 0),      # ONE K tile per tile, 5 n-tiles
               (1, 200, 333, 160, 100, 2)]     # N not a multiple of 64 (ragged last n-tile), 5 K tiles


@pytest.mark.parametrize("B,H,W,Cin,Cout,flags", CHAIN_CASES)
def test_pointwise_chain_kernel_equals_the_one_tile_instance(B, H, W, Cin, Cout, flags, monkeypatch):
    """pw_chain_kernel (several consecutive 64x64 tiles per workgroup as ONE software pipeline, STCN_PW_CHAIN=1) against fp64 and -
    same staging, MFMA and accumulation order - BIT-identical to the one-tile pointwise instance; with and without a residual."""
    g = torch.Generator().manual_seed(B * 7 + H * 13 + Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) * (2.0 / Cin) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, Cout, H, W, generator=g)
    for use_res in (True, False):
        ref = F.conv2d((F.relu(x) if flags & 1 else x).double(), w.double(), b.double())
        if use_res:
            ref = ref + res.double()
        if flags & 2:
            ref = F.relu(ref)
        outs = []
        for chain in ("0", "1", "2"):          # one tile per workgroup / consecutive tiles / tiles strided over the grid (default)
            monkeypatch.setenv("STCN_PW_CHAIN", chain)
            y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
            call("stcn_test_conv", stream(), nhwc(x), dev(w.permute(0, 2, 3, 1)), dev(b), nhwc(res) if use_res else None, y,
                 B, H, W, Cin, Cout, 1, 1, 1, 0, flags, 0)
            assert last_path().startswith("direct_pointwise_chain" if chain != "0" else "direct_pointwise "), last_path()
            outs.append(y.cpu())
            if chain == "0":
                tail = "+tail" in last_path()        # the one-tile plan cut its last tiles into K pieces: another summation order there
        assert torch.equal(outs[1], outs[2]), "the two tile walks of the chain kernel compute the same tiles in the same order of arithmetic"
        got = outs[1].permute(0, 3, 1, 2).double()
        assert torch.isfinite(got).all()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err < 2e-5, err
        if tail:
            assert (outs[0] - outs[1]).abs().max().item() <= 2e-6 * ref.abs().max().item()
        else:
            assert torch.equal(outs[0], outs[1]), "the chain kernel must reproduce the one-tile instance bit for bit"


def _random_conv_cases():
    """Seeded sweep over the shapes the fixed list cannot enumerate: every Winograd / FusionNet / direct instance under random
    sizes (ragged tile rows and columns, padded workgroup tiles), batch, residual and ReLU combinations."""
    soak, seed = int(os.environ.get("STCN_SOAK_CONV", 0)), int(os.environ.get("STCN_SOAK_SEED", 1))
    if soak:                       # one-off soak run (tools/parity_long.sh): N other cases, larger frames / batches / channel counts, any path
        rng = np.random.RandomState(7000 + seed)
        cases = []
        for i in range(soak):
            K, s = [(3, 1), (3, 1), (1, 1), (3, 2), (1, 2), (7, 2)][int(rng.randint(0, 6))]
            B = int(rng.randint(1, 7))
            H, W = int(rng.randint(3, 131)), int(rng.randint(3, 131))
            Cin = int(rng.choice([4, 8])) if K == 7 else int(rng.choice([12, 32, 64, 96, 128, 160, 256, 288, 512, 1024]))
            Cout = 64 if K == 7 else int(rng.choice([32, 64, 96, 128, 160, 256, 512]))
            if Cin * Cout * H * W * B > 3e10 // (K * K):          # keep the fp64 reference of a case within seconds
                H, W = H // 3 + 3, W // 3 + 3
            flags = int(rng.randint(0, 4)) | (4 if rng.rand() < 0.5 else 0)
            if Cin in (12, 32) and Cout == 32:
                flags &= 2
            cases.append((B, H, W, Cin, Cout, K, s, flags, bool(rng.randint(0, 2)), None))
        return cases
    rng = np.random.RandomState(20260303)
    cases = []
    for i in range(36):
        kind = ("f2", "f4", "fusion", "direct1x1", "direct3x3s2", "f4")[i % 6]
        B = int(rng.randint(1, 4))
        H, W = int(rng.randint(3, 41)), int(rng.randint(3, 49))
        flags = int(rng.randint(0, 4))                      # bit 0: ReLU on the input, bit 1: ReLU on the output
        res = bool(rng.randint(0, 2))
        if kind == "f2":
            Cin, Cout, K, s = int(rng.choice([128, 160, 256])), int(rng.choice([64, 128, 192])), 3, 1
        elif kind == "f4":
            Cin, Cout, K, s = int(rng.choice([64, 128, 256, 288])), int(rng.choice([32, 64, 96, 160])), 3, 1
            flags |= 4
        elif kind == "fusion":
            Cin, Cout, K, s, B = int(rng.choice([12, 32])), 32, 3, 1, 1
            flags &= 2                                      # the FusionNet kernels take no ReLU on the input
        elif kind == "direct1x1":
            Cin, Cout, K, s = int(rng.choice([64, 96, 256])), int(rng.choice([32, 64, 160, 256])), 1, 1
        else:
            Cin, Cout, K, s = int(rng.choice([64, 128])), int(rng.choice([64, 128])), 3, 2
        path = {"f2": "wino2", "f4": "wino4", "fusion": "fusion_wino", "direct1x1": "direct_pointwise", "direct3x3s2": "direct s"}[kind]
        if kind == "direct1x1" and Cout <= 32:
            path = "direct_narrow s"                        # Cout <= 32: the 128x32-tile instance (no pointwise form of it)
        cases.append((B, H, W, Cin, Cout, K, s, flags, res, path))
    return cases


@pytest.mark.parametrize("B,H,W,Cin,Cout,K,s,flags,use_res,path", _random_conv_cases())
def test_conv_random_shapes_match_fp64_reference(B, H, W, Cin, Cout, K, s, flags, use_res, path):
    g = torch.Generator().manual_seed(B * 1000003 + H * 10007 + W * 101 + Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, K, K, generator=g) * (2.0 / (Cin * K * K)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    OH, OW = (H + 2 * (K // 2) - K) // s + 1, (W + 2 * (K // 2) - K) // s + 1
    res = torch.randn(B, Cout, OH, OW, generator=g) if use_res else None
    ref = F.conv2d((F.relu(x) if flags & 1 else x).double(), w.double(), b.double(), stride=s, padding=K // 2)
    if res is not None:
        ref = ref + res.double()
    if flags & 2:
        ref = F.relu(ref)
    y = torch.full((B, OH, OW, Cout), float("nan"), device="cuda")     # every output must be written
    call("stcn_test_conv", stream(), nhwc(x), dev(w.permute(0, 2, 3, 1)), dev(b),
         None if res is None else nhwc(res), y, B, H, W, Cin, Cout, K, K, s, K // 2, flags, 0)
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    assert err < 2e-5, err
    assert path is None or last_path().startswith(path), (last_path(), path)       # the kernel family the case was drawn for (soak: any)


def _memread(mk, mv, qk):
    N, Q, k = mk.shape[0], qk.shape[0], mv.shape[0]
    idx = torch.empty(Q, 50, dtype=torch.int32, device="cuda")
    w = torch.empty(Q, 50, device="cuda")
    ro = torch.empty(k, Q, 512, device="cuda")
    call("stcn_test_memory_read", stream(), dev(mk), dev(mv), dev(qk), N, Q, k, idx, w, ro)
    return idx.cpu().long(), w.cpu(), ro.cpu()


def _dense(idx, w, N):
    d = torch.zeros(idx.shape[0], N)
    d.scatter_(1, idx, w)
    return d


def _memread_cases():
    fixed = [(160, 80, 1, 1.0), (1620, 333, 2, 1.0), (5000, 200, 3, 0.5), (20 * 1620, 97, 1, 1.0), (50, 16, 1, 1.0)]
    soak, seed = int(os.environ.get("STCN_SOAK_MEMREAD", 0)), int(os.environ.get("STCN_SOAK_SEED", 1))
    if not soak:
        return fixed
    rng = np.random.RandomState(9000 + seed)       # soak: any bank size from the minimum (50 rows) to 40 frames, ragged query counts, k up to 8
    return [(int(np.exp(rng.uniform(np.log(50), np.log(65000)))), int(rng.randint(1, 700)), int(rng.randint(1, 9)) if rng.rand() < 0.5 else 1,
             float(rng.choice([0.3, 0.5, 1.0, 1.5]))) for _ in range(soak)]


@pytest.mark.parametrize("N,Q,k,scale", _memread_cases())
def test_memory_read_matches_oracle(N, Q, k, scale):
    g = torch.Generator().manual_seed(N + Q)
    mk = torch.randn(N, 64, generator=g) * scale
    qk = torch.randn(Q, 64, generator=g) * scale
    mv = torch.randn(k, N, 512, generator=g)
    oi, ow, oro, gap = O.memory_read(mk, mv, qk, return_gap=True)
    gi, gw, gro = _memread(mk, mv, qk)
    assert (gi >= 0).all() and (gi < N).all()
    assert all(len(set(r.tolist())) == 50 for r in gi), "duplicate rows selected"
    assert torch.allclose(gw.sum(1), torch.ones(Q), atol=1e-5)
    # the fixed cases have no query whose 50th / 51st scores are closer than fp32 rounding: identical selection everywhere; a soak run
    # meets such queries (any member of the tie is a valid choice: test_near_tie_queries_are_the_only_ones_that_differ) and exempts them
    ok = torch.ones(Q, dtype=torch.bool) if not os.environ.get("STCN_SOAK_MEMREAD") else gap >= 1e-4
    assert ok.float().mean() > 0.5 or Q < 20              # small key scales over large banks: ~14 % of the queries are near-ties
    if ok.any():
        assert (_dense(gi, gw, N) - _dense(oi, ow, N)).abs().max(1).values[ok].max() < 2e-5
        assert ((gro - oro).abs().amax((0, 2)) / oro.abs().max())[ok].max() < 2e-5


def _plan(N, Q):
    import ctypes as C
    from eva_vos_amd import _lib
    pl = (C.c_int32 * 7)()
    _lib.check(_lib.lib().stcn_memread_plan(N, Q, pl))
    return dict(zip(("steps", "ss", "ns", "nc1", "spc1", "nc2", "spc2"), pl))


@pytest.mark.parametrize("T,Q,k", [(52, 1620, 1), (104, 1620, 5), (104, 1531, 1)])
def test_memory_read_at_config3_bank_sizes_matches_oracle(T, Q, k):
    """The plan the full-bank runs take - pass 1 samples every 8th 64-row step, 29 pass-2 chunks - against the dense CPU
    oracle (S is 0.5 - 1.1 GB on the host) at N = 84 240 and 168 480 rows, Q = one frame of queries and a ragged Q, k = 1
    and 5.  With ~1e5 rows per query a few queries have a 50th/51st score gap below fp32 rounding of the scores: those must
    still get a VALID top-50 of the fp64 scores with its own weights; every other query the identical selection."""
    N = T * 1620
    pl = _plan(N, Q)
    assert pl["ss"] == 8 and pl["steps"] == (N + 63) // 64, pl
    g = torch.Generator().manual_seed(N + Q + k)
    mk = torch.randn(N, 64, generator=g) * 0.8
    qk = torch.randn(Q, 64, generator=g) * 0.8
    mv = torch.randn(k, N, 512, generator=g)
    oi, ow, oro, gap = O.memory_read(mk, mv, qk, return_gap=True)
    gi, gw, gro = _memread(mk, mv, qk)
    assert (gi >= 0).all() and (gi < N).all()
    assert (torch.sort(gi, 1).values.diff(dim=1) > 0).all(), "duplicate rows selected"
    near = gap < 1e-4
    assert near.float().mean() < 0.02, float(near.float().mean())
    same = (torch.sort(gi, 1).values == torch.sort(oi, 1).values).all(1)
    assert same[~near].all(), "a clear-cut query selected other rows than the oracle"
    # weights of the identical selections (compared row-aligned), read-out
    o_sorted, g_sorted = torch.sort(oi, 1), torch.sort(gi, 1)
    dw = (torch.gather(gw, 1, g_sorted.indices) - torch.gather(ow, 1, o_sorted.indices)).abs().max(1).values
    assert dw[same].max() < 2e-5, float(dw[same].max())
    err = (gro - oro).abs().amax((0, 2)) / oro.abs().max()
    assert err[same].max() < 2e-5, float(err[same].max())
    assert torch.allclose(gw.sum(1), torch.ones(Q), atol=1e-5)
    # near-tie queries that chose differently: a valid top-50 of the true scores, own weights, own read-out
    for q in torch.nonzero(~same).flatten().tolist():
        sq = O.affinity_logits(mk.double(), qk[q:q + 1].double())[:, 0]            # [N] fp64 scores of this query
        sel = torch.zeros(N, dtype=torch.bool)
        sel[gi[q]] = True
        assert sq[sel].min() >= sq[~sel].max() - 1e-4, q
        assert (torch.softmax(sq[gi[q]], 0).float() - gw[q]).abs().max() < 2e-5
        own = torch.einsum("j,kjc->kc", gw[q], mv[:, gi[q]])
        assert (gro[:, q] - own).abs().max() / own.abs().max() < 2e-5
    print(f"N={N} Q={Q} k={k}: plan {pl}; {int(near.sum())} near-tie queries, {int((~same).sum())} selected differently")


def test_memory_read_rising_scores_forces_many_selects():
    """Scores increase with the row index.  Written for the one-pass streaming read, where every tile beat the running threshold and
    forced a select.  Under the two-pass read pass 1's threshold lands about 50 rows from the end of the bank: all candidates sit in
    one short chunk, its list is 32 entries long (CAP2 = 64), and neither the cut-back inside pass 2 nor the write-out select runs.
    Lists that overflow: test_gpu_memread_lists.py; the lengths on this bank: test_memread_lists.py."""
    N, Q = 4000, 48
    u = torch.randn(64, generator=torch.Generator().manual_seed(3))
    u = u / u.norm() * 3.0
    a = torch.linspace(0.0, 0.9, N)[:, None]
    mk = a * u[None, :] + 1e-3 * torch.randn(N, 64, generator=torch.Generator().manual_seed(4))
    qk = u[None, :].repeat(Q, 1) + 0.05 * torch.randn(Q, 64, generator=torch.Generator().manual_seed(5))
    mv = torch.randn(1, N, 512, generator=torch.Generator().manual_seed(6))
    oi, ow, oro = O.memory_read(mk, mv, qk)
    gi, gw, gro = _memread(mk, mv, qk)
    assert (_dense(gi, gw, N) - _dense(oi, ow, N)).abs().max() < 5e-5
    assert (gro - oro).abs().max() / oro.abs().max() < 5e-5


def test_memory_read_handles_exact_ties():
    """Duplicated memory rows give exactly tied scores at the cut; any tie-break is valid, the weights
    of the kept set and the readout must still agree."""
    N, Q = 640, 32
    g = torch.Generator().manual_seed(9)
    base = torch.randn(N // 4, 64, generator=g)
    mk = base.repeat(4, 1)                       # every row 4 times -> ties everywhere
    mvb = torch.randn(1, N // 4, 512, generator=g)
    mv = mvb.repeat(1, 4, 1)                     # tied rows carry identical values
    qk = torch.randn(Q, 64, generator=g)
    _, _, oro = O.memory_read(mk, mv, qk)
    gi, gw, gro = _memread(mk, mv, qk)
    assert all(len(set(r.tolist())) == 50 for r in gi)
    assert (gro - oro).abs().max() / oro.abs().max() < 2e-5


def test_near_tie_queries_are_the_only_ones_that_differ():
    """The claim behind the sequence tolerances, made falsifiable: two fp32 implementations of the top-50 read may select
    different rows ONLY for queries whose 50th and 51st scores are closer than fp32 rounding of the scores, and even there
    the selected set is a correct top-50 of the true scores.  Bank: 300 single rows + 300 triplets of rows that differ by
    ~1e-7 relative but carry different values, so the cut falls inside a triplet for a good part of the queries."""
    g = torch.Generator().manual_seed(21)
    single = torch.randn(300, 64, generator=g)
    base = torch.randn(300, 64, generator=g)
    trip = torch.cat([base * (1 + 1e-7 * torch.randn(300, 1, generator=g)) for _ in range(3)], 0)
    mk = torch.cat([single, trip], 0)[torch.randperm(1200, generator=g)]
    qk = torch.randn(256, 64, generator=g)
    mv = torch.randn(2, 1200, 512, generator=g)
    oi, ow, oro, gap = O.memory_read(mk, mv, qk, return_gap=True)
    gi, gw, gro = _memread(mk, mv, qk)
    S = O.affinity_logits(mk.double(), qk.double()).t()                    # [Q, N] true scores (fp64)
    near = gap < 1e-4
    assert 0.15 < near.float().mean() < 0.85, "the construction must yield both kinds of queries"
    N = mk.shape[0]
    # (1) clear-cut queries: identical selection and weights, read-out within fp32 rounding
    dd = (_dense(gi, gw, N) - _dense(oi, ow, N)).abs().max(1).values
    assert dd[~near].max() < 2e-5, float(dd[~near].max())
    err = (gro - oro).abs().amax((0, 2)) / oro.abs().max()
    assert err[~near].max() < 2e-5, float(err[~near].max())
    # (2) near-tie queries: some do differ from the oracle's choice (that is the effect) ...
    assert (dd[near] > 1e-3).any(), "no near-tie query differs: the test no longer exercises the effect"
    # ... but every selected set is a valid top-50 of the true scores up to the rounding level, with the right weights and
    # the read-out that belongs to ITS rows
    sel = torch.zeros(qk.shape[0], N, dtype=torch.bool)
    sel.scatter_(1, gi, True)
    lo = torch.where(sel, S, torch.full_like(S, float("inf"))).min(1).values
    hi = torch.where(~sel, S, torch.full_like(S, -float("inf"))).max(1).values
    assert (lo >= hi - 1e-4).all(), float((hi - lo).max())
    # round 5: candidates within 1e-4 of the fp32 cut are re-scored in fp64 inside the merge kernel (memread.hip: RESCORE_W), so the
    # selection is the top-50 of the exact scores - not merely a valid one up to rounding (1e-9: two fp64 formulas of the same score) - on THIS
    # seeded read, whose near-tie candidates all survive the per-chunk cut to 50 entries (several chunks, top-50 spread over them); a read whose
    # top-50 sits in one chunk keeps a valid fp32 top-50 instead (memread.hip, 'Scope of exact')
    assert (lo >= hi - 1e-9).all(), float((hi - lo).max())
    ws = torch.softmax(torch.gather(S, 1, gi), 1).float()
    assert (ws - gw).abs().max() < 2e-5
    own = torch.einsum("qj,kqjc->kqc", gw, mv[:, gi])
    assert (gro - own).abs().max() / own.abs().max() < 2e-5


#               N     Q   k  top_k  (h16, w16, km)
SPLIT_READS = [(1620, 333, 2, 50, None), (1620, 333, 2, 20, None), (240, 80, 2, 50, (8, 10, 5.6))]


@pytest.mark.parametrize("N,Q,k,top_k,km", SPLIT_READS, ids=["top50", "top20", "km-frame"])
def test_read_of_several_objects_without_topk_outputs_is_the_read_with_them(N, Q, k, top_k, km):
    """The read the engine runs and no other hook test reaches: k > 1 and neither topk_idx nor topk_w.  merge_readout_kernel then leaves the
    selection in the scratch of pass 1's group maxima and gather_readout_kernel gathers with one wave per (query, object); with the
    outputs given the merge kernel gathers itself.  Both add the same rows in the same order: the suite's 2e-5 (bit equality is not
    promised).  Banks: a fixed case of test_memory_read_matches_oracle at both cuts, and the "frame" bank of test_gpu_km (same draw)."""
    g = torch.Generator().manual_seed(N + Q)
    mk, qk, mv = dev(torch.randn(N, 64, generator=g)), dev(torch.randn(Q, 64, generator=g)), dev(torch.randn(k, N, 512, generator=g))
    h16, w16, sigma = km or (0, 0, 0.0)

    def read(outputs):
        idx = torch.empty(Q, top_k, dtype=torch.int32, device="cuda") if outputs else None
        w = torch.empty(Q, top_k, device="cuda") if outputs else None
        ro = torch.full((k, Q, 512), float("nan"), device="cuda")          # every read-out element must be written
        call("stcn_test_memory_read_km", stream(), mk, mv, qk, N, Q, k, top_k, h16, w16, float(sigma), None, idx, w, ro)
        return ro.cpu()

    whole, split = read(True), read(False)
    assert torch.isfinite(whole).all() and torch.isfinite(split).all()
    err = (split - whole).abs().max().item() / whole.abs().max().item()
    print(f"N={N} Q={Q} k={k} top_k={top_k} km={km}: split against merged read-out, max relative difference {err:.2e}")
    assert err < 2e-5, err


@pytest.mark.parametrize("kk", [2, 4, 6, 9, 10, 11, 17, 21, 33])
def test_attention_read_matches_oracle(kk):
    """kk = mask rows (objects + background): 2 kk channels.  Up to 9 rows run in one pass of the instantiated widths (4 / 8 / 12 / 20
    channels); beyond (more than 8 objects, round 6) the pass runs per slice of 20 channels: 10 -> one full slice, 11 -> 20 + 2, 17 -> 20 + 14,
    21 -> 20 + 20 + 2, 33 (STCN_MAX_OBJECTS + 1) -> 20 + 20 + 20 + 6."""
    h, w = 8, 10
    g = torch.Generator().manual_seed(11)
    mk, qk = torch.randn(h * w, 64, generator=g), torch.randn(h * w, 64, generator=g)
    pos = torch.rand(kk, 1, 16 * h, 16 * w, generator=g)
    neg = torch.rand(kk, 1, 16 * h, 16 * w, generator=g)
    ref = O.attention_read(mk, qk, pos, neg)
    out = torch.empty(kk, 2, 16 * h, 16 * w, device="cuda")
    call("stcn_test_attention", stream(), dev(mk), dev(qk), dev(pos), dev(neg), kk, 16 * h, 16 * w, out)
    assert (out.cpu() - ref).abs().max() < 1e-5


def test_gpu_j_and_f_equal_the_cpu_metrics_exactly():
    """J / F counts on the GPU are integer-exact: scores must equal the NumPy/SciPy implementation bit for bit
    (same special cases), incl. empty masks, frame-edge objects and a 480x854 frame (disk radius 8)."""
    import numpy as np
    from eva_vos_amd import metrics
    rng = np.random.default_rng(5)
    for (T, H, W) in [(5, 60, 90), (3, 480, 854)]:
        yy, xx = np.mgrid[0:H, 0:W]
        gt = np.zeros((T, H, W), bool)
        pr = np.zeros((T, H, W), bool)
        for t in range(T):
            cy, cx = H * (0.3 + 0.1 * t), W * (0.4 + 0.05 * t)
            gt[t] = ((yy - cy) / (0.2 * H)) ** 2 + ((xx - cx) / (0.25 * W)) ** 2 < 1
            pr[t] = ((yy - cy - 3) / (0.22 * H)) ** 2 + ((xx - cx + 4) / (0.2 * W)) ** 2 < 1
            pr[t] ^= rng.random((H, W)) < 0.002                      # speckle noise -> extra boundaries
        pr[0] = False                                                # n_fg == 0, n_gt > 0
        gt[1, :, :] = False                                          # n_gt == 0, n_fg > 0
        gt[2, -10:, -15:] = True                                     # object touching the last row / column
        got = metrics.sequence_scores_gpu(torch.from_numpy(gt).cuda(), torch.from_numpy(pr).cuda())
        jonly = metrics.sequence_scores_gpu(torch.from_numpy(gt).cuda(), torch.from_numpy(pr).cuda(), j_only=True)
        assert np.array_equal(jonly[:, 0], got[:, 0]) and np.isnan(jonly[:, 1:]).all()       # the J-only entry point: same counts
        for t in range(T):
            j, f = metrics.jaccard(gt[t], pr[t]), metrics.f_measure(gt[t], pr[t])
            assert got[t, 0] == j and got[t, 1] == f, (T, H, W, t, got[t], j, f)
    both_empty = metrics.sequence_scores_gpu(torch.zeros(1, 40, 40, dtype=torch.uint8).cuda(),
                                             torch.zeros(1, 40, 40, dtype=torch.uint8).cuda())
    assert both_empty[0].tolist() == [0.0, 1.0, 0.5]


def test_engines_on_two_streams_do_not_perturb_each_other(nets):
    """Determinism under concurrency (what bench.py relies on with several videos in flight): two engines driven from two
    host threads on two HIP streams must reproduce, bit for bit, what each gives when it runs alone."""
    import threading
    from eva_vos_amd import synth
    from mivos.inference_core import InferenceCore
    T, H, W = 8, 240, 432
    clips = [synth.synthetic_clip(T, H, W, seed=s_) for s_ in (31, 32)]
    msks = [synth.synthetic_mask(T, H, W, 1, seed=s_) for s_ in (33, 34)]
    solo = []
    for c, m in zip(clips, msks):
        core = InferenceCore(nets[0], nets[1], c, 1, mem_freq=2)
        solo.append((core.interact(m[:, 0], 0).copy(), core.interact(m[:, 5], 5).copy(), core.prob.clone()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cores = []
    for c, st in zip(clips, streams):
        with torch.cuda.stream(st):
            cores.append(InferenceCore(nets[0], nets[1], c, 1, mem_freq=2))
    torch.cuda.synchronize()
    got = [None, None]
    for rep in range(3):
        def run(i):
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[i]):
                cores[i].reset()
                a = cores[i].interact(msks[i][:, 0], 0).copy()
                b = cores[i].interact(msks[i][:, 5], 5).copy()
                got[i] = (a, b, cores[i].prob.clone())
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        [t.start() for t in th]
        [t.join() for t in th]
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(got[i][0], solo[i][0]) and np.array_equal(got[i][1], solo[i][1]), (rep, i)
            assert torch.equal(got[i][2], solo[i][2]), (rep, i)


def test_mfma_probe_reports_a_plausible_matrix_rate():
    """stcn_bench_mfma_rate (bench.py's live yardstick beside the datasheet peak): register-operand fp32 MFMAs on all CUs.  The rate
    must lie between half the datasheet peak and the peak itself (157.3 TFLOP/s at 2.4 GHz; the chip holds ~2.3 GHz on this load)."""
    import ctypes as C
    tf, ms = C.c_float(), C.c_float()
    call("stcn_bench_mfma_rate", stream(), 10, C.byref(tf), C.byref(ms))
    assert 157.3 / 2 < tf.value <= 157.3 * 1.01, tf.value
    assert 3.0 < ms.value < 60.0, ms.value
