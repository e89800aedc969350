"""The MLP evaluator on the host (sdrm_amd/mlp_eval.py: the module, `KerasAdam`, `compute_mlp_results`) and the host side of its device
train step (sdrm_mlp_train_steps: header, ctypes table, the argument checks that need no device).  No GPU.

The reference (mlp_benchmark.py) is Keras code that cannot run here; tests/mlp_eval_ref.py restates one step in float64 from the
formulas, and these tests hold the torch module to it under autograd in float64 (so that the GPU tests can hold the device to the
oracle), the optimizer to the closed form, and the driver to the fit's bookkeeping as the module docstring restates it."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import mlp_eval_ref as mr
from sdrm_amd import _lib, mlp_eval
from sdrm_amd.engine import Engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -2, -1
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()                                                                       # (computed once, shared, never changed)
    return _CACHE[key]


def single(name, k):
    """(x, keep) of step k of the case's call."""
    lo, hi = mr.STEPS[name][k]
    return mr.matrix(name)[mr.call_rows(name)[lo:hi]], mr.explicit_keep(name)[lo:hi]


# ================================================================================================ the oracle and the module
@pytest.mark.parametrize("name,k", mr.SINGLE)
def test_oracle_against_the_torch_module_in_float64(name, k):
    p, _, _ = mr.weights(name)
    x, keep = single(name, k)
    want, got = mr.step64(p, x, keep), mr.torch_step(p, x, keep, torch.float64)
    assert abs(got["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    for t in mr.NAMES:
        d = mr.normwise(got["grads"][t], want["grads"][t])
        assert d <= 1e-12, (name, k, t, d)
        assert np.abs(want["grads"][t]).max() > 0
    assert not want["grads"]["E"][2:].any() and want["grads"]["E"][:2].all()                        # only rows 0 and 1 are ever indexed


def test_nine_arrays_in_get_weights_order_load_and_reproduce_forward():
    name = "A"
    p, _, _ = mr.weights(name)
    n_items, n_rows, _ = mr.CASES[name]
    model = mlp_eval.MLP(n_rows, n_items)
    assert [tuple(t.shape) for t in model.engine_weights()] == list(mr.shapes(n_rows, n_items)) == list(Engine.mlp_shapes(n_rows, n_items))
    assert [n for n, _ in model.named_parameters()] == list(mr.NAMES) and len(Engine.MLP_TENSORS) == 9
    assert all(a is b for a, b in zip(model.engine_weights(), model.parameters()))                   # the parameters themselves
    model.load_keras_weights([p[t] for t in mr.NAMES])
    model = model.double().eval()
    x = mr.matrix(name)[:7]
    want = mr.step64(p, x, np.ones((7, mr.KEEP_COLS)), p_drop=0.0)["y"]                             # eval mode: k = 1, s = 1
    got = model(torch.as_tensor(x, dtype=torch.float64)).detach().numpy()
    assert mr.normwise(got, want) <= 1e-12
    assert np.allclose(model.predict(torch.as_tensor(x, dtype=torch.float64)).numpy(), 1.0 / (1.0 + np.exp(-want)), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="nine"):
        model.load_keras_weights([p[t] for t in mr.NAMES][:8])
    with pytest.raises(ValueError, match="0 / 1"):
        model(torch.full((1, n_items), 2.0, dtype=torch.float64))
    with pytest.raises(ValueError, match="keep must be"):
        model.train()(torch.zeros(2, n_items, dtype=torch.float64), torch.ones(2, 1000))


def test_initialisers_are_the_distributions():
    torch.manual_seed(0)
    m = mlp_eval.MLP(400, 100)
    std = math.sqrt(2.0 / 400)
    e = m.E.detach().numpy()
    assert abs(e.std() - std) < 0.1 * std and np.abs(e).max() <= 2.0 * std / 0.87962566103423978 + 1e-7
    for w, lim in ((m.W1, math.sqrt(6.0 / (800 + 512))), (m.W2, math.sqrt(6.0 / 768)), (m.W3, math.sqrt(6.0 / 512)), (m.W4, math.sqrt(3.0 / 256))):
        w = w.detach().numpy()
        assert np.abs(w).max() <= lim and np.abs(w).max() > 0.95 * lim and abs(w.std() - lim / math.sqrt(3.0)) < 0.05 * lim
    assert not any(getattr(m, f"b{l}").detach().numpy().any() for l in (1, 2, 3, 4))


# ================================================================================================ Keras's Adam
def test_keras_adam_against_the_closed_form_and_against_torchs():
    rng = np.random.default_rng(5)
    p0, gs = rng.normal(size=50), [rng.normal(size=50) * 10.0 ** rng.integers(-8, 1, size=50) for _ in range(3)]
    p = torch.tensor(p0, dtype=torch.float64)
    opt = mlp_eval.KerasAdam([p])
    want, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    for t, g in enumerate(gs, start=1):
        p.grad = torch.tensor(g)
        opt.step()
        m = m + (g - m) * (1 - 0.9)
        v = v + (g * g - v) * (1 - 0.999)
        want = want - 1e-3 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (np.sqrt(v) + 1e-7)
        assert np.allclose(p.numpy(), want, rtol=1e-13, atol=0) and opt.t == t
        mine = mr.keras_adam(p0 if t == 1 else prev[0], g, np.zeros(50) if t == 1 else prev[1], np.zeros(50) if t == 1 else prev[2], t)
        prev = mine
        assert np.allclose(mine[0], want, rtol=1e-7, atol=0)                                         # (its betas are the float32 ones of the C ABI)
    assert np.allclose(opt.exp_avg[0].numpy(), m, rtol=1e-13) and np.allclose(opt.exp_avg_sq[0].numpy(), v, rtol=1e-13)
    # where eps sits: one step on g = 1e-6 moves Keras's parameter by lr g / (|g| + eps / sqrt(1 - beta2)), torch's by lr g / (|g| + eps)
    a, b = torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64, requires_grad=True)
    a.grad, b.grad = torch.full((1,), 1e-6, dtype=torch.float64), torch.full((1,), 1e-6, dtype=torch.float64)
    mlp_eval.KerasAdam([a]).step()
    torch.optim.Adam([b], lr=1e-3, eps=1e-7).step()
    assert math.isclose(-a.item(), 1e-3 * 1e-6 / (1e-6 + 1e-7 / math.sqrt(1 - 0.999)), rel_tol=1e-9)
    assert math.isclose(-b.item(), 1e-3 * 1e-6 / (1e-6 + 1e-7), rel_tol=1e-9)
    assert -b.item() > 3 * -a.item()


# ================================================================================================ the driver
def toy(n_rows=37, n_items=77, n_valid=12, seed=2):
    """Case A's row counts (29 train rows: batches of 16 and 13) at 77 items: ranking at k = 50 needs more than 50 columns, which the
    45 of case A are not (the reference's own `argpartition` fails there)."""
    rng = np.random.default_rng(seed)
    return (csr_matrix((rng.random((n_rows, n_items)) < 0.2).astype(np.float32)), csr_matrix((rng.random((n_valid, n_items)) < 0.3).astype(np.float32)))


def scripted(monkeypatch, values):
    """`validation_rmse` replaced by a script; returns the list that records (rows it was given, a copy of the weights at that call)."""
    seen = []

    def stub(model, rows_csr, device):
        seen.append((rows_csr.toarray().copy(), [t.detach().clone() for t in model.engine_weights()]))
        return values[len(seen) - 1]
    monkeypatch.setattr(mlp_eval, "validation_rmse", stub)
    return seen


def test_validation_split_takes_the_last_rows_and_combine_training_appends(monkeypatch):
    training, validation = toy()
    seen = scripted(monkeypatch, [0.5])
    h = {}
    mlp_eval.compute_mlp_results(training, validation, epochs=1, history=h)
    assert np.array_equal(seen[0][0], training.toarray()[29:]) and seen[0][0].shape[0] == 37 - math.floor(0.8 * 37)
    assert len(h["train_loss"]) == 2 and h["model"].num_users == 37
    from sdrm_amd import metrics
    part, _ = metrics.split_train_test_proportion_from_csr_matrix(csr_matrix(validation), batch_size=10, random_seed=123)
    seen = scripted(monkeypatch, [0.5])
    mlp_eval.compute_mlp_results(training, validation, combine_training=True, epochs=1, history=h)
    n = 37 + part.shape[0]
    both = np.concatenate([training.toarray(), part.toarray()])
    assert np.array_equal(seen[0][0], both[math.floor(0.8 * n):])
    assert h["model"].num_users == 37 and len(h["train_loss"]) == -(-math.floor(0.8 * n) // 16)       # n_users: the rows BEFORE the append


def test_early_stop_bookkeeping_on_a_scripted_sequence(monkeypatch):
    training, validation = toy()
    # epoch 1 improves by more than min_delta; epoch 2 by EXACTLY min_delta against the stored best (no improvement: the compare is strict);
    # then nothing improves: the wait counter reaches 10 at epoch 11
    values = [0.5, 0.4, 0.4 - 0.001] + [0.4] * 20
    assert values[2] == values[1] - mlp_eval.MIN_DELTA
    seen = scripted(monkeypatch, values)
    h = {}
    mlp_eval.compute_mlp_results(training, validation, epochs=50, history=h)
    assert h["epochs_run"] == 12 and h["best_epoch"] == 1 and h["val_rmse"] == values[:12]
    for got, want in zip(h["model"].engine_weights(), seen[1][1]):
        assert torch.equal(got.detach(), want)                                                     # the best epoch's weights, stopped early
    assert not torch.equal(seen[11][1][1], seen[1][1][1])
    # all epochs ran: the best epoch's weights again
    seen = scripted(monkeypatch, [0.5, 0.3, 0.4])
    mlp_eval.compute_mlp_results(training, validation, epochs=3, history=h)
    assert h["epochs_run"] == 3 and h["best_epoch"] == 1
    for got, want in zip(h["model"].engine_weights(), seen[1][1]):
        assert torch.equal(got.detach(), want)
    stop = mlp_eval.EarlyStop()
    assert [stop.update(v) for v in (1.0, 0.9995, 0.998)] == [True, False, True] and stop.wait == 0 and stop.best_epoch == 2


def test_short_last_batch_divides_by_its_own_rows():
    p, _, _ = mr.weights("A")
    x, keep = single("A", 2)
    assert x.shape[0] == 13
    n_items, n_rows, _ = mr.CASES["A"]
    model = mlp_eval.MLP(n_rows, n_items)
    model.load_keras_weights([p[t] for t in mr.NAMES])
    model = model.double().train()
    xt = torch.as_tensor(x, dtype=torch.float64)
    got = mlp_eval.bce_from_logits(model(xt, torch.as_tensor(keep)), xt).item()
    want = mr.step64(p, x, keep)["loss"]
    assert abs(got - want) <= 1e-12 * want and abs(got - mr.step64(p, x, keep, divisor=16 * n_items)["loss"]) > 0.1 * want


def test_driver_on_a_tiny_problem_on_the_cpu():
    training, validation = toy()
    h = {}
    rec, ndcg = mlp_eval.compute_mlp_results(training, validation, seed=3, epochs=2, history=h)
    assert rec.shape == (6,) and ndcg.shape == (6,) and np.isfinite(rec).all() and np.isfinite(ndcg).all()
    assert ((0 <= rec) & (rec <= 1)).all() and ((0 <= ndcg) & (ndcg <= 1)).all()
    assert h["epochs_run"] == 2 and len(h["val_rmse"]) == 2 and len(h["train_loss"]) == 4 and h["best_epoch"] in (0, 1)
    assert h["per_user"][0].shape == (6, 12) and all(0.3 < l < 1.5 for l in h["train_loss"])
    rec2, ndcg2 = mlp_eval.compute_mlp_results(training, validation, seed=3, epochs=2)
    assert np.array_equal(rec, rec2) and np.array_equal(ndcg, ndcg2)                                # a function of the seed


def test_device_train_without_an_engine_is_refused():
    training, validation = toy()
    with pytest.raises(ValueError, match="device_train=True needs an engine"):
        mlp_eval.compute_mlp_results(training, validation, epochs=1, device_train=True)


# ================================================================================================ the cases
def chains(name):
    return cached(("chain", name), lambda: (mr.chain64(name), mr.torch_chain(name)))


@pytest.mark.parametrize("name", list(mr.CASES))
def test_case_conditions(name):
    """No float64 pre-activation of any step the GPU tests run - the one-step runs from the start state and every step of the chain -
    lies within the near-kink gap of zero: the GPU tests leave no element out."""
    p, _, _ = mr.weights(name)
    for nm, k in mr.SINGLE:
        if nm != name:
            continue
        x, keep = single(name, k)
        r64, r32 = mr.step64(p, x, keep), mr.torch_step(p, x, keep, torch.float32)
        dev = [mr.normwise(a, b) for a, b in zip(r32["z"], r64["z"])]
        assert all(0 < d < 2e-6 for d in dev), dev
        assert mr.kink_exceptions(r64["z"], dev) == [0, 0, 0], (name, k)
    c64, c32 = chains(name)
    for k, (a, b) in enumerate(zip(c64, c32)):
        dev = [mr.normwise(u, w) for u, w in zip(b["z"], a["z"])]
        assert all(0 < d < 2e-6 for d in dev), dev
        assert mr.kink_exceptions(a["z"], dev) == [0, 0, 0], (name, "chain", k)
    assert [hi - lo for lo, hi in mr.STEPS[name]] == {"A": [16, 16, 13], "B": [16, 16, 1], "C": [16, 16]}[name]
    assert (mr.CASES[name][0], mr.n_fit(name)) == {"A": (45, 29), "B": (129, 17), "C": (64, 32)}[name]
    assert mr.call_rows(name).max() < mr.n_fit(name)
    if name == "C":
        assert mr.c_conditions(mr.matrix(name)) == (True, True, True, True)


def test_philox_restatement_shape_and_rate():
    k = mr.philox_keep(5, 2, 100, 64, 0.5)
    assert k.shape == (64, 1024) and k.dtype == np.uint8 and 0.48 < k.mean() < 0.52
    assert np.array_equal(k[10:20], mr.philox_keep(5, 2, 110, 10, 0.5))                             # a function of the place, not of the call's start
    assert mr.philox_keep(5, 2, 0, 8, 0.0).all() and not np.array_equal(k, mr.philox_keep(5, 3, 100, 64, 0.5))
    assert "PURPOSE_MLP_DROP = 11" in open(os.path.join(REPO, "sdrm_amd", "csrc", "philox.h")).read()


# ================================================================================================ the ABI and the argument checks
def test_symbols_header_and_ctypes_table():
    lib = _lib.load()
    assert hasattr(lib, "sdrm_mlp_train_steps") and hasattr(lib, "sdrm_debug_mlp_train_args")
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    debug = open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    for text, name, n_args in ((header, "sdrm_mlp_train_steps", 21), (debug, "sdrm_debug_mlp_train_args", 9)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "typedef struct sdrm_mlp_train { float* p[9]; float* m[9]; float* v[9]; int n_users, n_items; } sdrm_mlp_train;" in header
    assert [f[0] for f in _lib.MlpTrain._fields_] == ["p", "m", "v", "n_users", "n_items"] and C.sizeof(_lib.MlpTrain) == 3 * 9 * 8 + 8
    sig = inspect.signature(Engine.mlp_train_steps).parameters
    assert list(sig)[1:] == ["weights", "exp_avg", "exp_avg_sq", "csr_dev", "rows", "batch", "step0", "lr", "betas", "eps", "p_drop", "seed", "call_id",
                             "keep", "grads_out", "check"]
    assert (sig["batch"].default, sig["step0"].default, sig["lr"].default, sig["betas"].default, sig["eps"].default, sig["p_drop"].default) == (
        16, 0, 1e-3, (0.9, 0.999), 1e-7, 0.5)
    assert sig["keep"].default is None and sig["grads_out"].default is None and sig["check"].default is True
    drv = inspect.signature(mlp_eval.compute_mlp_results).parameters
    assert list(drv) == ["training_data", "validation_data", "combine_training", "engine", "seed", "epochs", "device", "history", "device_train"]
    assert drv["epochs"].default == 200 and drv["device_train"].default is False and drv["combine_training"].default is False


def test_host_side_argument_check():
    lib = _lib.load()
    ok = dict(n_users=37, n_items=45, n=29, batch=16, step0=0, p_drop=0.5, with_grads=0)

    def call(addr=None, **kw):
        a = dict(ok, **kw)
        arr = None if addr is None else (C.c_uint64 * len(addr))(*addr)
        return lib.sdrm_debug_mlp_train_args(a["n_users"], a["n_items"], a["n"], a["batch"], a["step0"], a["p_drop"], a["with_grads"], arr,
                                             0 if addr is None else len(addr))

    assert call() == 0 and call(batch=1) == 0 and call(n=1) == 0 and call(n=2 ** 31 - 1) == 0 and call(n_items=1) == 0 and call(n_items=36864) == 0
    assert call(n_users=2) == 0 and call(p_drop=0.0) == 0 and call(p_drop=0.999) == 0 and call(step0=10 ** 9) == 0
    for kw in (dict(batch=0), dict(batch=17), dict(n=0), dict(n=2 ** 31), dict(n_users=1), dict(n_items=0), dict(n_items=36865), dict(p_drop=1.0),
               dict(p_drop=-0.1), dict(p_drop=float("nan")), dict(step0=-1)):
        assert call(**kw) == SHAPE, kw
    assert call(with_grads=1, n=16) == 0 and call(with_grads=1, n=17) == ARG and call(with_grads=1, n=2, batch=1) == ARG
    # the tensors' addresses: nine tensors three (or four) times over, laid out one behind the other on the 16-byte grid
    sizes = [4 * int(np.prod(s)) for s in mr.shapes(37, 45)]

    def layout(lists, base=4096):
        out, at = [], base
        for _ in range(lists):
            for s in sizes:
                out.append(at)
                at += -(-s // 16) * 16
        return out
    good3, good4 = layout(3), layout(4)
    assert call(addr=good3) == 0 and call(addr=good4, with_grads=1, n=16) == 0
    assert call(addr=good4) == ARG and call(addr=good3, with_grads=1, n=16) == ARG                   # the count goes with with_grads
    for i in (0, 1, 8, 9, 26):
        bad = list(good3)
        bad[i] = 0
        assert call(addr=bad) == ARG, i                                                            # a null pointer
        bad[i] = good3[i] + 4
        assert call(addr=bad) == ARG, i                                                            # off the 16-byte grid
    bad = list(good3)
    bad[10] = good3[1] + 16 * 100                                                                  # m[W1] inside p[W1]
    assert call(addr=bad) == ARG
    bad = list(good3)
    bad[2] = good3[1] + sizes[1] - 16                                                              # b1 on the last bytes of W1
    assert call(addr=bad) == ARG
    bad = list(good4)
    bad[27 + 3] = good4[3]                                                                         # a gradient tensor on its parameter
    assert call(addr=bad, with_grads=1, n=16) == ARG
