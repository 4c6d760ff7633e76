"""CPU: ``top_k`` (1..50) on the public surface - the weight container, the C ABI's argument checks (made before any device call) - and
the oracle at ``top_k=20`` against fixtures captured from the REAL reference's ``PropagationNetwork(top_k=20)`` (tools/gen_golden_topk.py)."""
import ctypes as C

import pytest

import test_oracle_golden as TG
from conftest import load_golden
from eva_vos_amd import _lib
from eva_vos_amd.params import PropagationNetwork
from oracle import stcn_oracle as O

TOPK_TAGS = ["seqT20", "seqT20s", "seqT20k3"]
NEW_SYMBOLS = ["stcn_model_create_ex", "stcn_model_get_top_k", "stcn_test_memory_read_k", "stcn_bench_memory_read_k"]


def topk_noise(monkeypatch, module=TG):
    """check_sequence_against_golden takes its yardsticks from load_golden("selfnoise"): for the top_k fixtures they are the rows of
    selfnoise_topk.npz (the reference's PropagationNetwork(top_k=K) against itself at 1 / 2 / 4 / 8 threads).  Same checks, same bounds."""
    rows = load_golden("selfnoise_topk")
    monkeypatch.setattr(module, "load_golden", lambda name: rows if name == "selfnoise" else load_golden(name))
    return rows


def test_container_keeps_top_k_and_its_state_dict_keys():
    net = PropagationNetwork(top_k=20)
    assert net.top_k == 20 and PropagationNetwork().top_k == 50 and PropagationNetwork(top_k=1).top_k == 1
    assert list(net.state_dict().keys()) == list(PropagationNetwork().state_dict().keys())


@pytest.mark.parametrize("bad", [None, 0, 51, 20.5, True])
def test_container_refuses_unsupported_top_k(bad):
    with pytest.raises(ValueError, match=r"1\.\.50") as e:
        PropagationNetwork(top_k=bad)
    if bad is None:
        assert "dense" in str(e.value) and "not built" in str(e.value)


def test_core_takes_top_k_from_the_container_or_a_reference_style_module():
    from eva_vos_amd.inference_core import _top_k_of

    class Reader:
        top_k = 20

    class RefStyle:                      # a live reference module: no .top_k of its own, the memory reader holds it (prop_net.py:149)
        memory = Reader()

    class Bare:
        pass

    assert _top_k_of(PropagationNetwork(top_k=30)) == 30 and _top_k_of(RefStyle()) == 20 and _top_k_of(Bare()) == 50
    RefStyle.memory.top_k = None         # the reference's dense read
    with pytest.raises(ValueError, match="not built"):
        _top_k_of(RefStyle())


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_declared_and_exported(name):
    assert name in _lib.PROTOTYPES
    assert getattr(_lib.lib(), name) is not None


def test_model_create_ex_refuses_top_k_51_before_any_device_call():
    lib = _lib.lib()
    keep = (C.c_float * 4)()
    d = (_lib.WeightDesc * 1)()
    d[0].name, d[0].data, d[0].ndim = b"x", C.addressof(keep), 1
    d[0].shape[0] = 4
    h = C.c_void_p()
    opts = _lib.ModelOpts(top_k=51)
    assert lib.stcn_model_create_ex(0, d, 1, None, 0, C.byref(opts), C.byref(h)) == -1      # STCN_E_INVALID
    msg = lib.stcn_last_error().decode()
    assert "top_k=51" in msg and "50" in msg and not h.value
    v = C.c_int32()
    assert lib.stcn_model_get_top_k(None, C.byref(v)) == -1


@pytest.mark.parametrize("tag", TOPK_TAGS)
def test_oracle_at_top_k_matches_reference(tag, weights, monkeypatch):
    """The oracle with its cut set to the fixture's top_k against the reference's own masks and probabilities, in the manner of
    test_oracle_golden.test_sequence_matches_reference: this pins the yardstick of the GPU tests at top_k != 50 to the reference."""
    g = load_golden(tag)
    top_k = int(g[f"{tag}.top_k"])
    assert top_k == 20
    monkeypatch.setattr(O, "TOP_K", top_k)
    topk_noise(monkeypatch)
    cores = []

    def factory(img, k, mf):
        cores.append(O.OracleCore(weights[0], weights[1], img, k, mem_freq=mf))
        return cores[0]

    outs = TG.run_sequence(factory, tag, g)
    TG.check_sequence_against_golden(outs, tag, g, prob_atol=2e-3, ties=TG.tie_summary(cores[0]))
