"""The host side of the MLP evaluator's eval-mode forward on the device (sdrm_mlp_eval: header, ctypes table, the envelope that needs no
device), the driver's and the pipeline's wiring, and the conditions the GPU tests (tests/test_mlp_eval.py) rest on: the oracle helper
against the float64 torch module, and the ranking test's gap rule leaving no user out.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import mlp_eval_fwd_ref as fr
import mlp_eval_ref as mr
from sdrm_amd import _lib, mlp_eval, pipeline
from sdrm_amd.engine import Engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -2, -1


def toy(n_rows=37, n_items=77, n_valid=12, seed=2):
    rng = np.random.default_rng(seed)
    return (csr_matrix((rng.random((n_rows, n_items)) < 0.2).astype(np.float32)), csr_matrix((rng.random((n_valid, n_items)) < 0.3).astype(np.float32)))


# ================================================================================================ the ABI
def test_symbols_header_and_ctypes_table():
    lib = _lib.load()
    assert hasattr(lib, "sdrm_mlp_eval") and hasattr(lib, "sdrm_debug_mlp_eval_args")
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    debug = open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    for text, name, n_args in ((header, "sdrm_mlp_eval", 14), (debug, "sdrm_debug_mlp_eval_args", 12)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "typedef struct sdrm_mlp_eval_w { const float* p[9]; int n_users, n_items; } sdrm_mlp_eval_w;" in header
    assert [f[0] for f in _lib.MlpEvalW._fields_] == ["p", "n_users", "n_items"] and C.sizeof(_lib.MlpEvalW) == 9 * 8 + 8
    for line in ("mlp_benchmark.py:92", ":109", ":114"):
        assert line in header[header.index("The MLP evaluator's EVAL-MODE forward"):]
    sig = inspect.signature(Engine.mlp_eval).parameters
    assert list(sig)[1:] == ["weights", "csr_dev", "rows", "row0", "n", "batch", "logits", "out", "sse", "check"]
    assert (sig["rows"].default, sig["row0"].default, sig["n"].default, sig["batch"].default, sig["logits"].default, sig["out"].default,
            sig["sse"].default, sig["check"].default) == (None, 0, None, 1024, False, None, False, True)
    drv = inspect.signature(mlp_eval.compute_mlp_results_device).parameters
    assert list(drv) == ["training_data", "validation_data", "engine", "combine_training", "seed", "epochs", "history", "device_train"]
    assert drv["device_train"].default is True and drv["epochs"].default == 200 and drv["engine"].default is inspect.Parameter.empty
    assert "device_eval" not in inspect.signature(mlp_eval.compute_mlp_results).parameters           # the torch-evaluating driver keeps its surface
    assert list(inspect.signature(pipeline.evaluate_synthetic).parameters) == ["train", "valid", "raw", "sparsity", "engine", "hp", "seed"]


def test_host_side_envelope():
    lib = _lib.load()
    ok = dict(n_users=22, n_items=129, nnz=500, n_rows=22, rows_listed=0, row0=0, n=22, batch=8, with_out=1, with_sse=0)

    def call(addr=None, **kw):
        a = dict(ok, **kw)
        arr = None if addr is None else (C.c_uint64 * len(addr))(*addr)
        return lib.sdrm_debug_mlp_eval_args(a["n_users"], a["n_items"], a["nnz"], a["n_rows"], a["rows_listed"], a["row0"], a["n"], a["batch"],
                                            a["with_out"], a["with_sse"], arr, 0 if addr is None else len(addr))

    for kw in (dict(), dict(batch=1), dict(batch=4096), dict(n=1), dict(n_items=1), dict(n_items=36864), dict(n_users=2), dict(nnz=0),
               dict(row0=21, n=1), dict(row0=5, n=17), dict(with_out=0, with_sse=1), dict(with_sse=1), dict(rows_listed=1, n=70),
               dict(rows_listed=1, n=10 ** 6, row0=999), dict(n_items=36864, rows_listed=1, n=(2 ** 40 - 1) // 36864),
               dict(n_items=1, rows_listed=1, n=2 ** 40 - 1)):
        assert call(**kw) == 0, kw
    for kw in (dict(batch=0), dict(batch=4097), dict(n=0), dict(n=-3), dict(n_items=0), dict(n_items=36865), dict(n_users=1), dict(nnz=-1),
               dict(n_rows=0), dict(row0=-1), dict(row0=22, n=1), dict(row0=5, n=18), dict(n=23), dict(with_out=0, with_sse=0),
               dict(n_items=36864, rows_listed=1, n=(2 ** 40 - 1) // 36864 + 1), dict(n_items=1, rows_listed=1, n=2 ** 40)):
        assert call(**kw) == SHAPE, kw
    good = [4096 + 16 * 1000 * i for i in range(9)]
    assert call(addr=good) == 0
    assert call(addr=good[:8]) == ARG and call(addr=good + [4096 * 99]) == ARG                        # nine addresses
    for i in range(9):
        bad = list(good)
        bad[i] = 0
        assert call(addr=bad) == ARG, i                                                            # a null tensor
        for off in (4, 8, 12):
            bad[i] = good[i] + off
            assert call(addr=bad) == SHAPE, (i, off)                                               # off the 16-byte grid


# ================================================================================================ the driver and the pipeline
def test_device_eval_without_an_engine_is_refused():
    training, validation = toy()
    with pytest.raises(ValueError, match="compute_mlp_results_device needs an engine"):
        mlp_eval.compute_mlp_results_device(training, validation, None, epochs=1)


def recorded(monkeypatch):
    """The four evaluators and the two binarisers of `pipeline` replaced by recorders: the list of (name, args, kwargs)."""
    calls = []

    def stub(name, result):
        def f(*args, **kw):
            calls.append((name, args, kw))
            return result
        monkeypatch.setattr(pipeline, name, f)
    for name in ("compute_mf_results", "compute_mf_results_device", "compute_mf_results_resident", "compute_mlp_results_device"):
        stub(name, ("result of", name))
    stub("equal_sparsity", "dense01")
    stub("equal_sparsity_csr", "sparse01")
    return calls


class FakeEngine:
    def equal_sparsity_csr(self, raw, sparsity):
        return ("device csr of", raw, sparsity)


def test_evaluate_synthetic_reaches_the_evaluator_hp_names(monkeypatch):
    calls = recorded(monkeypatch)
    eng = FakeEngine()

    def run(hp):
        del calls[:]
        got = pipeline.evaluate_synthetic("TRAIN", "VALID", "RAW", 0.9, eng, hp, 5)
        evals = [c for c in calls if c[0].startswith("compute")]
        assert len(evals) == 1 and got == ("result of", evals[0][0])
        return evals[0], [c for c in calls if not c[0].startswith("compute")]

    # no `evaluator` key: the calls run_experiment always made
    (name, args, kw), bins = run({})
    assert (name, args, kw) == ("compute_mf_results", ("TRAIN", "VALID", "dense01"), dict(only_synthetic=True))
    assert bins == [("equal_sparsity", ("RAW", 0.9, eng), {})]
    (name, args, kw), bins = run(dict(sparse_synthetic=True, nmf=True))                              # (nmf goes with the device routes only)
    assert (name, args, kw) == ("compute_mf_results", ("TRAIN", "VALID", "sparse01"), dict(only_synthetic=True))
    assert bins == [("equal_sparsity_csr", ("RAW", 0.9, eng), {})]
    (name, args, kw), bins = run(dict(device_svd=True))
    assert (name, args, kw) == ("compute_mf_results_device", ("TRAIN", "VALID", "dense01", eng), dict(only_synthetic=True, seed=5))
    (name, args, kw), bins = run(dict(device_svd=True, nmf=True, sparse_synthetic=True))
    assert (name, args, kw) == ("compute_mf_results_device", ("TRAIN", "VALID", "sparse01", eng), dict(only_synthetic=True, seed=5, nnmf=True))
    (name, args, kw), bins = run(dict(resident_svd=True, device_svd=True))
    assert (name, args, kw) == ("compute_mf_results_resident", ("TRAIN", "VALID", ("device csr of", "RAW", 0.9), eng), dict(only_synthetic=True, seed=5))
    assert bins == []
    # the MLP route: main.py:197-214 without augmentation
    (name, args, kw), bins = run(dict(evaluator="mlp", device_svd=True))
    assert (name, args) == ("compute_mlp_results_device", ("dense01", "VALID", eng))
    assert kw == dict(device_train=True, seed=5, epochs=200)
    (name, args, kw), bins = run(dict(evaluator="mlp", mlp_epochs=7))
    assert kw["epochs"] == 7
    with pytest.raises(ValueError, match="evaluator"):
        pipeline.evaluate_synthetic("TRAIN", "VALID", "RAW", 0.9, eng, dict(evaluator="knn"), 5)
    assert "evaluate_synthetic(train, valid, raw, sparsity, net.engine(), hp, seed)" in inspect.getsource(pipeline.run_experiment)


# ================================================================================================ what the GPU tests rest on
@pytest.mark.parametrize("name", list(mr.CASES))
def test_oracle_helper_against_the_torch_module_in_float64(name):
    p0 = mr.weights(name)[0]
    n_items, n_rows, _ = mr.CASES[name]
    model = mlp_eval.MLP(n_rows, n_items)
    model.load_keras_weights([p0[t] for t in mr.NAMES])
    model = model.double().eval()
    x = torch.as_tensor(mr.matrix(name), dtype=torch.float64)
    with torch.no_grad():
        y, p = model(x).numpy(), model.predict(x).numpy()
    o = fr.oracle(name)
    assert o["y"].shape == (n_rows, n_items) and mr.normwise(y, o["y"]) <= 1e-12 and mr.normwise(p, o["p"]) <= 1e-12
    assert abs(float(((p - x.numpy()) ** 2).sum()) - o["sse"]) <= 1e-12 * o["sse"]
    # the identity the device's SSE uses: sum p^2 - sum over the entries of (2 p - 1)
    ident = float((o["p"] ** 2).sum() - (2.0 * o["p"][mr.matrix(name) == 1] - 1.0).sum())
    assert abs(ident - o["sse"]) <= 1e-12 * o["sse"]


@pytest.mark.parametrize("name", list(mr.CASES))
def test_bars_come_from_the_float32_module(name):
    bar, ref = fr.bars(name)
    print(f"{name}: module y {ref['y']:.2e} p {ref['p']:.2e} worst p {ref['p_max']:.2e} sse {ref['sse']:.2e}")
    assert 1e-7 < ref["y"] < 2e-6 and 1e-8 < ref["p"] < 2e-7 and 2e-8 < ref["p_max"] < 3e-7 and ref["sse"] < 1e-7
    assert all(bar[k] == mr.BAR_FACTOR * ref[k] and bar[k] <= 1e-4 for k in ("y", "p", "p_max"))
    assert bar["sse"] == mr.BAR_FACTOR * fr.sse_level() and ref["sse"] <= fr.sse_level() < 1e-8      # one level for the scalar: the cases' largest


@pytest.mark.parametrize("name", ["B", "C"])
def test_gap_rule_leaves_no_user_out(name):
    x, held = mr.matrix(name), fr.held_pattern(name)
    assert not (x & held).any() and held.sum(axis=1).min() >= 1 and fr.KS == (1, 3, 5, 10)
    assert 1e-6 < fr.gap(name) < 1e-5
    left = fr.users_left_out(name)
    assert left.shape == (x.shape[0],) and not left.any(), np.flatnonzero(left)
    assert fr.users_left_out(name, kmax=50).any()                                                  # why the test stops at k = 10
