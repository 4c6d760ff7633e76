"""CPU: ``km`` (the kernelized memory read, reference ``EvalMemoryReader(top_k, km)``) on the public surface - the weight container, the C
ABI's argument checks (made before any device call) - and the km restatement of tests/km_oracle.py against fixtures captured from the REAL
reference with ``net.memory.km`` set (tools/gen_golden_km.py)."""
import ctypes as C

import pytest

import km_oracle
import test_oracle_golden as TG
from conftest import load_golden
from eva_vos_amd import _lib
from eva_vos_amd.params import PropagationNetwork
from oracle import stcn_oracle as O

KM_TAGS = ["seqKM", "seqKMk3", "seqKMn"]
NEW_SYMBOLS = ["stcn_model_get_km", "stcn_test_memory_read_km", "stcn_bench_memory_read_km"]


def km_noise(monkeypatch, module=TG):
    """check_sequence_against_golden takes its yardsticks from load_golden("selfnoise"): for the km fixtures they are the rows of
    selfnoise_km.npz (the reference with memory.km set against itself at 1 / 2 / 4 / 8 threads).  Same checks, same bounds."""
    rows = load_golden("selfnoise_km")
    monkeypatch.setattr(module, "load_golden", lambda name: rows if name == "selfnoise" else load_golden(name))
    return rows


def km_oracle_for(monkeypatch, g, tag):
    """Switch the oracle to the fixture's read while the test runs: its cut and the km restatement closed over the frame's key grid."""
    T, H, W, k, _ = [int(v) for v in g[f"{tag}.shape"]]
    km, top_k = float(g[f"{tag}.km"]), int(g[f"{tag}.top_k"])
    monkeypatch.setattr(O, "TOP_K", top_k)
    monkeypatch.setattr(O, "memory_read", km_oracle.memory_read((H + 15) // 16, (W + 15) // 16, km))
    return km, top_k


def test_container_keeps_km_and_its_state_dict_keys():
    net = PropagationNetwork(km=5.6)
    assert net.km == 5.6 and net.top_k == 50 and PropagationNetwork().km is None
    assert PropagationNetwork(top_k=20, km=3).km == 3.0 and PropagationNetwork(top_k=20, km=3).top_k == 20
    assert list(net.state_dict().keys()) == list(PropagationNetwork().state_dict().keys())


@pytest.mark.parametrize("bad", [True, False, 0, 0.0, -1.5, float("nan"), float("inf"), -float("inf"), "5.6"])
def test_container_refuses_unsupported_km(bad):
    with pytest.raises(ValueError, match="km"):
        PropagationNetwork(km=bad)


def test_core_takes_km_from_the_container_or_a_reference_style_module():
    from eva_vos_amd.inference_core import _km_of

    class Reader:
        top_k, km = 50, 5.6

    class RefStyle:                      # a live reference module: the memory reader holds km (prop_net.py:149), set by the caller
        memory = Reader()

    class Bare:
        pass

    assert _km_of(PropagationNetwork(km=2.5)) == 2.5 and _km_of(PropagationNetwork()) is None
    assert _km_of(RefStyle()) == 5.6 and _km_of(Bare()) is None
    RefStyle.memory.km = None            # the reference's default
    assert _km_of(RefStyle()) is None
    RefStyle.memory.km = float("nan")
    with pytest.raises(ValueError, match="km"):
        _km_of(RefStyle())


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbols_are_declared_and_exported(name):
    assert name in _lib.PROTOTYPES
    assert getattr(_lib.lib(), name) is not None


def test_model_opts_carry_km_behind_top_k():
    assert [f[0] for f in _lib.ModelOpts._fields_] == ["top_k", "km"]
    assert _lib.ModelOpts(top_k=20).km == 0.0                  # not given


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_model_create_ex_refuses_a_non_finite_km_before_any_device_call(bad):
    lib = _lib.lib()
    keep = (C.c_float * 4)()
    d = (_lib.WeightDesc * 1)()
    d[0].name, d[0].data, d[0].ndim = b"x", C.addressof(keep), 1
    d[0].shape[0] = 4
    h = C.c_void_p()
    opts = _lib.ModelOpts(top_k=50, km=bad)
    assert lib.stcn_model_create_ex(0, d, 1, None, 0, C.byref(opts), C.byref(h)) == -1      # STCN_E_INVALID
    assert "km=" in lib.stcn_last_error().decode() and not h.value
    v = C.c_float()
    assert lib.stcn_model_get_km(None, C.byref(v)) == -1


@pytest.mark.parametrize("tag", KM_TAGS)
def test_km_oracle_matches_reference(tag, weights, monkeypatch):
    """The oracle reading through tests/km_oracle.py against the reference's own masks and probabilities with ``memory.km`` set, in the
    manner of test_oracle_golden.test_sequence_matches_reference: this pins the yardstick of the GPU tests of the kernelized read to the
    reference."""
    g = load_golden(tag)
    km, top_k = km_oracle_for(monkeypatch, g, tag)
    assert (km, top_k) == {"seqKM": (5.6, 50), "seqKMk3": (5.6, 20), "seqKMn": (1.5, 50)}[tag]
    km_noise(monkeypatch)
    cores = []

    def factory(img, k, mf):
        cores.append(O.OracleCore(weights[0], weights[1], img, k, mem_freq=mf))
        return cores[0]

    outs = TG.run_sequence(factory, tag, g)
    TG.check_sequence_against_golden(outs, tag, g, prob_atol=2e-3, ties=TG.tie_summary(cores[0]))
