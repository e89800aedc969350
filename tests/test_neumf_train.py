"""The NeuMF evaluator's train steps on the device (csrc/neumf_train.h; sdrm_neumf_train_steps; `Engine.neumf_train_steps`;
`neumf.compute_neuralcf_results(device_train=True)`).  Reference: neural_cf_benchmark_pt.py:125-144 in train mode and :186-200.

CPU: tests/neumf_train_ref.py (float64, from the formulas) against the reference's own float32 gradients and losses of the fixtures
tests/golden/neumf_train_<case>.npz; `vae_adam_ref.adam_step` on the fixture's gradients against the fixture's next state; the conditions
on the cases; the host-side argument check; the symbols, the header and the ctypes table; the driver's refusal without an engine.
GPU (-m gpu): every tensor carved out of guarded arenas, the guards checked after every call.  Gradients and loss of one step per case and
step against the restatement, at BAR_FACTOR x the reference's own float32 deviation on the same tensor and step (the same terms in another
order: the evaluator's factor); Adam at tests/test_vae_adam.py's bars; chaining; the PHILOX mode against restated masks; bad ids; the
refusals; the driver."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import neumf_train_ref as tr
import vae_adam_ref as adam
from vae_adam_ref import rel_max
from sdrm_amd import _lib, neumf
from sdrm_amd.engine import Engine, SdrmError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TOL = 1e-4                 # the project's fp32 bar
EPS = 1e-8
GUARD, SENTINEL = 8, 12345.0
SHAPE, ARG = -2, -1
TABLES = tr.NAMES[:4]


def shapes(F, n_users, n_items):
    return ((n_users, F), (n_items, F), (n_users, 4 * F), (n_items, 4 * F), (4 * F, 8 * F), (4 * F,), (2 * F, 4 * F), (2 * F,), (F, 2 * F), (F,),
            (1, 2 * F), (1,))


def split(flat, shp):
    out, at = [], 0
    for s in shp:
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    assert at == flat.size
    return out


class Case:
    """A case of tr.CASES with its fixture: inputs rebuilt from the stored seed, per step k the lists p[k], m[k], v[k] (state BEFORE the
    step), g[k], loss[k] of the reference, keep[k] and tri[k] of the step's batch, ref[k] the float64 restatement at p[k]."""

    def __init__(self, name):
        self.name = name
        self.F, self.n_users, self.n_items, self.n, self.batches, _ = tr.CASES[name]
        fx = np.load(os.path.join(GOLDEN, f"neumf_train_{name}.npz"))
        self.seed = int(fx[f"{name}_seed"])
        self.w0, self.triples = tr.case_inputs(name, self.seed)
        self.shapes = shapes(self.F, self.n_users, self.n_items)
        self.keep_all = np.unpackbits(fx[f"{name}_keep"], axis=1)[:, :14 * self.F]
        self.dev = fx[f"{name}_dev"]
        self.distinct = len(set(self.batches)) == len(self.batches)
        zeros = [np.zeros(s, dtype=np.float32) for s in self.shapes]
        self.p, self.m, self.v, self.g, self.loss, self.tri, self.keep, self.ref = [], [], [], [], [], [], [], []
        for k, (lo, hi) in enumerate(self.batches):
            self.p.append(split(fx[f"{name}_s{k}_p"], self.shapes))
            self.m.append(split(fx[f"{name}_s{k}_m"], self.shapes) if k else zeros)
            self.v.append(split(fx[f"{name}_s{k}_v"], self.shapes) if k else zeros)
            self.g.append(split(fx[f"{name}_s{k}_g"], self.shapes))
            self.loss.append(float(fx[f"{name}_s{k}_loss"]))
            self.tri.append(self.triples[lo:hi])
            self.keep.append(self.keep_all[lo:hi] if self.distinct else self.keep_all[k:k + 1])
            self.ref.append(tr.step64(dict(zip(tr.NAMES, self.p[k])), self.tri[k], self.keep[k]))
        self.final_p = split(fx[f"{name}_final_p"], self.shapes)
        for a, b in zip(self.p[0], self.w0.values()):
            assert np.array_equal(a, b)                                                            # the stored seed rebuilds the inputs

    def p_after(self, k):
        return self.p[k + 1] if k + 1 < len(self.p) else self.final_p


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)                                                                  # (computed once, shared, never changed)
    return _CASES[name]


STEPS = [(name, k) for name in tr.CASES for k in range(tr.STEPS)]


# ================================================================================================ CPU
@pytest.mark.parametrize("name,k", STEPS)
def test_restatement_against_the_references_gradients_and_loss(name, k):
    c = case(name)
    for t, got in zip(tr.NAMES, c.g[k]):
        d = tr.normwise(got, c.ref[k]["grads"][t])
        assert 0 < d <= TOL, (name, k, t, d)
    d = abs(c.loss[k] - c.ref[k]["loss"]) / abs(c.ref[k]["loss"])
    print(name, k, "reference loss", c.loss[k], "float64", c.ref[k]["loss"], "relative", d)
    assert d <= TOL


def adam_bars(p, m, v, p0, want, what):
    """tests/test_vae_adam.py's bars for one tensor: m, v rel_max <= 1e-4 (exactly zero where the expectation is all zero),
    |p - p_ref| <= 2^-24 |p_ref| + 1e-4 max|p_ref - p_0|.  Returns the worst figures."""
    p_ref, m_ref, v_ref = want
    worst = {}
    for key, a, r in (("m", m, m_ref), ("v", v, v_ref)):
        if a is None:
            continue
        if np.abs(r).max() > 0:
            worst[key] = rel_max(a, r)
            assert worst[key] <= TOL, (what, key, worst[key])
        else:
            assert not np.asarray(a).any(), (what, key)
    bound = 2.0 ** -24 * np.abs(p_ref) + TOL * np.abs(p_ref - np.asarray(p0, dtype=np.float64)).max()
    err = np.abs(np.asarray(p, dtype=np.float64) - p_ref)
    worst["p"] = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (what, float(err.max()), float(bound.min()))
    return worst


@pytest.mark.parametrize("name,k", STEPS)
def test_adam_restatement_on_the_fixtures_gradients(name, k):
    c = case(name)
    nxt = k + 1 < tr.STEPS
    for i, t in enumerate(tr.NAMES):
        want = adam.adam_step(c.p[k][i], c.g[k][i], c.m[k][i], c.v[k][i], k + 1, tr.LR, (0.9, 0.999), EPS)
        adam_bars(c.p_after(k)[i], c.m[k + 1][i] if nxt else None, c.v[k + 1][i] if nxt else None, c.p[k][i], want, (name, k, t))
        assert np.abs(want[0] - c.p[k][i]).max() > 0


@pytest.mark.parametrize("name", list(tr.CASES))
def test_case_conditions(name):
    c = case(name)
    for k in range(tr.STEPS):
        assert tr.kink_exceptions(c.ref[k]["z"], c.dev[k]) == [0, 0, 0], (name, k)
        assert (c.dev[k] > 0).all() and (c.dev[k] < 1e-6).all()
    assert [hi - lo for lo, hi in c.batches] == {"f8": [256, 256, 37], "f16": [70, 70, 1], "one": [1, 1, 1]}[name]
    assert (c.F, c.n_users, c.n_items, c.n) == {"f8": (8, 300, 47, 549), "f16": (16, 23, 19, 141), "one": (8, 5, 7, 1)}[name]
    if name == "f8":
        assert tr.f8_conditions(c.triples, c.batches, c.n_users) == (True, True, True, True)


def test_philox_restatement_shape_and_rate():
    k = tr.philox_keep(5, 2, 100, 64, 8, 0.5)
    assert k.shape == (64, 112) and k.dtype == np.uint8 and 0.45 < k.mean() < 0.55
    assert np.array_equal(k[10:20], tr.philox_keep(5, 2, 110, 10, 8, 0.5))                          # a function of the place, not of the call's start
    assert tr.philox_keep(5, 2, 0, 8, 16, 0.0).all() and not np.array_equal(k, tr.philox_keep(5, 3, 100, 64, 8, 0.5))
    assert "PURPOSE_NEUMF_DROP = 10" in open(os.path.join(REPO, "sdrm_amd", "csrc", "philox.h")).read()


def test_host_side_argument_check():
    lib = _lib.load()
    ok = dict(n_users=300, n_items=47, factor=8, n=549, batch=256, step0=0, p_drop=0.5)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdrm_debug_neumf_train_args(a["n_users"], a["n_items"], a["factor"], a["n"], a["batch"], a["step0"], a["p_drop"])

    assert call() == 0 and call(factor=16) == 0 and call(batch=1) == 0 and call(batch=1024) == 0 and call(n=1) == 0 and call(n=2 ** 31 - 1) == 0
    assert call(p_drop=0.0) == 0 and call(p_drop=0.999) == 0 and call(step0=10 ** 9) == 0 and call(n_users=1, n_items=1) == 0
    for kw in (dict(factor=32), dict(factor=4), dict(batch=0), dict(batch=1025), dict(n=0), dict(n=2 ** 31), dict(n_users=0), dict(n_items=0)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(p_drop=1.0), dict(p_drop=-0.1), dict(p_drop=float("nan")), dict(step0=-1)):
        assert call(**kw) == ARG, kw


def test_symbols_header_and_ctypes_table():
    lib = _lib.load()
    assert hasattr(lib, "sdrm_neumf_train_steps") and hasattr(lib, "sdrm_debug_neumf_train_args")
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    debug = open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    for text, name, n_args in ((header, "sdrm_neumf_train_steps", 18), (debug, "sdrm_debug_neumf_train_args", 7)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "typedef struct sdrm_neumf_train" in header
    assert [f[0] for f in _lib.NeumfTrain._fields_] == ["p", "m", "v", "n_users", "n_items", "factor"] and C.sizeof(_lib.NeumfTrain) == 3 * 12 * 8 + 16
    sig = inspect.signature(Engine.neumf_train_steps).parameters
    assert list(sig)[1:] == ["weights", "exp_avg", "exp_avg_sq", "triples", "batch", "step0", "lr", "betas", "eps", "p_drop", "seed", "call_id", "keep",
                             "grads", "check"]
    assert sig["lr"].default == 1e-3 and sig["p_drop"].default == 0.5 and sig["keep"].default is None and sig["check"].default is True
    assert inspect.signature(neumf.compute_neuralcf_results).parameters["device_train"].default is False


def toy(seed=1, n_users=40, n_items=90):
    """(training, validation) triples of tests/test_neumf_eval.py's 40-user toy: 24 training and 6 validation pairs per user, random labels."""
    rng = np.random.default_rng(seed)
    training, validation = [], []
    for u in range(n_users):
        for j, i in enumerate(rng.permutation(n_items)[:30]):
            (training if j < 24 else validation).append((u, int(i), int(rng.random() < 0.5)))
    return np.asarray(training), np.asarray(validation)


def test_device_train_without_an_engine_is_refused():
    training, validation = toy()
    with pytest.raises(ValueError, match="device_train=True needs an engine"):
        neumf.compute_neuralcf_results(training, validation, 40, 90, seed=3, epochs=1, device_train=True)


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


class Arena:
    """Arrays of one dtype carved out of one device buffer, GUARD sentinel elements or more between neighbours and at both ends, every
    array on a 64-element boundary."""

    def __init__(self, arrays, sentinel=SENTINEL):
        arrays = [np.ascontiguousarray(a) for a in arrays]
        self.offs, at = [], GUARD
        for a in arrays:
            at = -(-at // 64) * 64
            self.offs.append(at)
            at += a.size + GUARD
        self.host = np.full(at, sentinel, dtype=arrays[0].dtype)
        self.inside = np.zeros(at, dtype=bool)
        for o, a in zip(self.offs, arrays):
            self.host[o:o + a.size] = a.ravel()
            self.inside[o:o + a.size] = True
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.views = [self.dev[o:o + a.size].view(a.shape) for o, a in zip(self.offs, arrays)]
        self.shapes = [a.shape for a in arrays]

    def arrays(self):
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[~self.inside], self.host[~self.inside]), "a guard was written"
        return [got[o:o + int(np.prod(s))].reshape(s) for o, s in zip(self.offs, self.shapes)]

    def unchanged(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.host)


class Run:
    """One `neumf_train_steps` call on arenas: p, m, v, g (twelve tensors each), the triples and the masks."""

    def __init__(self, engine, p, m, v, tri, keep, batch, step0, p_drop=tr.P_DROP, want_grads=True, **kw):
        self.A = {k: Arena(x) for k, x in (("p", p), ("m", m), ("v", v))}
        self.A["g"] = Arena([np.full(a.shape, 777.0, dtype=np.float32) for a in p])
        self.tri = Arena([np.asarray(tri, dtype=np.int32)], sentinel=-7)
        self.keep = Arena([np.asarray(keep, dtype=np.uint8)], sentinel=1) if keep is not None else None
        n0 = engine.launch_count()
        losses = engine.neumf_train_steps(self.A["p"].views, self.A["m"].views, self.A["v"].views, self.tri.views[0], batch, step0, lr=tr.LR,
                                          eps=EPS, p_drop=p_drop, keep=self.keep.views[0] if self.keep else None,
                                          grads=self.A["g"].views if want_grads else None, **kw)
        self.launches = engine.launch_count() - n0
        self.losses = losses.cpu().numpy()
        self.p, self.m, self.v, self.g = (self.A[k].arrays() for k in "pmvg")
        self.tri.unchanged()
        if self.keep:
            self.keep.unchanged()


_RUNS = {}


def one_step(engine, name, k):
    """Step k of a case from the FIXTURE's state before it, EXPLICIT masks, gradients out (run once, shared by the tests)."""
    if (name, k) not in _RUNS:
        c = case(name)
        _RUNS[name, k] = Run(engine, c.p[k], c.m[k], c.v[k], c.tri[k], c.keep[k], tr.BATCH[name], k)
    return _RUNS[name, k]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", STEPS)
def test_gradients_and_loss_of_one_step(engine, name, k):
    """Every gradient and the loss of one step at BAR_FACTOR x the reference's own float32 deviation from the float64 restatement.
    Measured on one MI355X (DESIGN §4w has the table): all 108 gradient tensors meet their bars, the worst at 2.24 x the reference's
    deviation (one step 1, MLP_layers.4.bias: 9.47e-8 against 4.23e-8); the nine losses stand at 1.8e-9 .. 4.1e-7 against bars of
    1.56e-8 .. 1.5e-5, the closest f16 step 2, a batch of one pair, at 6.76e-8 against 1.04e-7, then f8 step 1 at 2.31e-9 against
    1.56e-8 (the reference's float32 loss happens to lie 3.9e-9 from the float64 one there).  The forward's dot products are
    compensated (csrc/neumf_train.h: nt_dot2_step): with plain fmaf chains these two losses missed their bars."""
    c, r = case(name), one_step(engine, name, k)
    assert r.launches == 4 and r.losses.shape == (1,)
    failures = []
    for i, t in enumerate(tr.NAMES):
        want = c.ref[k]["grads"][t]
        ref_dev, dev_dev = tr.normwise(c.g[k][i], want), tr.normwise(r.g[i], want)
        print(f"{name} step {k} {t}: device {dev_dev:.3e} reference {ref_dev:.3e} bar {tr.BAR_FACTOR * ref_dev:.3e}")
        if not dev_dev <= tr.BAR_FACTOR * ref_dev:
            failures.append((t, dev_dev, ref_dev))
        if t in TABLES:                                                                            # rows no pair names: exactly zero
            named = np.unique(c.tri[k][:, 0 if "user" in t else 1])
            rest = np.setdiff1d(np.arange(r.g[i].shape[0]), named)
            assert not r.g[i][rest].any(), t
            assert r.g[i][named].any(), t
    want = c.ref[k]["loss"]
    ref_dev, dev_dev = abs(c.loss[k] - want) / abs(want), abs(float(r.losses[0]) - want) / abs(want)
    print(f"{name} step {k} loss: device {dev_dev:.3e} reference {ref_dev:.3e} bar {tr.BAR_FACTOR * ref_dev:.3e}")
    if not dev_dev <= tr.BAR_FACTOR * ref_dev:
        failures.append(("loss", dev_dev, ref_dev))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", STEPS)
def test_adam_of_one_step(engine, name, k):
    c, r = case(name), one_step(engine, name, k)
    moved_outside = 0
    for i, t in enumerate(tr.NAMES):
        want = adam.adam_step(c.p[k][i], r.g[i], c.m[k][i], c.v[k][i], k + 1, tr.LR, (0.9, 0.999), EPS)
        worst = adam_bars(r.p[i], r.m[i], r.v[i], c.p[k][i], want, (name, k, t))
        print(name, k, t, {key: f"{val:.2e}" for key, val in worst.items()})
        if t in TABLES and k > 0:                                                                  # rows outside the batch whose moments are non-zero still move
            named = np.unique(c.tri[k][:, 0 if "user" in t else 1])
            rest = np.setdiff1d(np.arange(r.p[i].shape[0]), named)
            assert not r.g[i][rest].any()
            p0 = c.p[k][i].astype(np.float64)
            # ... wherever the restatement moves them by more than twice the bar on p (a moment left by a saturated pair can be too small to)
            bound = 2.0 ** -24 * np.abs(want[0]) + TOL * np.abs(want[0] - p0).max()
            live = [row for row in rest if (np.abs(want[0][row] - p0[row]) > 2 * bound[row]).any()]
            moved_outside += len(live)
            assert all((r.p[i][row] != c.p[k][i][row]).any() for row in live), t
    if name == "f8" and k > 0:
        assert moved_outside > 0


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f8", "f16"])
def test_one_call_equals_one_call_per_batch(engine, name):
    c = case(name)
    batch, steps = tr.BATCH[name], len(c.batches)
    whole = Run(engine, c.p[0], c.m[0], c.v[0], c.triples, c.keep_all, batch, 0, want_grads=False)
    assert whole.launches == 4 * steps and whole.losses.shape == (steps,) and np.isfinite(whole.losses).all()
    again = Run(engine, c.p[0], c.m[0], c.v[0], c.triples, c.keep_all, batch, 0, want_grads=False)
    for key in "pmv":
        assert same_bits(getattr(whole, key), getattr(again, key)), key
    assert np.array_equal(whole.losses, again.losses)
    p, m, v, losses = c.p[0], c.m[0], c.v[0], []
    for k, (lo, hi) in enumerate(c.batches):
        r = Run(engine, p, m, v, c.triples[lo:hi], c.keep_all[lo:hi], batch, k, want_grads=False)
        p, m, v = r.p, r.m, r.v
        losses.append(r.losses[0])
    assert same_bits(whole.p, p) and same_bits(whole.m, m) and same_bits(whole.v, v)
    assert np.array_equal(whole.losses, np.asarray(losses))
    assert not same_bits(whole.p, c.p[0])


@pytest.mark.gpu
@pytest.mark.parametrize("p_drop", [0.5, 0.3, 0.0])
@pytest.mark.parametrize("name", ["f8", "f16"])
def test_philox_mode_equals_explicit_restated_masks(engine, name, p_drop):
    c = case(name)
    batch, seed, call_id = tr.BATCH[name], 0x1234567887654321, 3
    ph = Run(engine, c.p[0], c.m[0], c.v[0], c.triples, None, batch, 0, p_drop=p_drop, seed=seed, call_id=call_id)
    keep = tr.philox_keep(seed, call_id, 0, c.n, c.F, p_drop)
    if p_drop == 0.0:
        assert keep.all()
    else:
        assert abs(keep.mean() - (1 - p_drop)) < 0.02
    ex = Run(engine, c.p[0], c.m[0], c.v[0], c.triples, keep, batch, 0, p_drop=p_drop)
    for key in "pmvg":
        assert same_bits(getattr(ph, key), getattr(ex, key)), key
    assert np.array_equal(ph.losses, ex.losses)
    other = Run(engine, c.p[0], c.m[0], c.v[0], c.triples, None, batch, 0, p_drop=p_drop, seed=seed, call_id=call_id + 1, want_grads=False)
    assert same_bits(other.p, ph.p) == (p_drop == 0.0)                                             # the call id keys the draw


@pytest.mark.gpu
def test_bad_ids_add_nothing_and_raise_the_status(engine):
    c = case("f8")
    tri = c.tri[0].copy()
    tri[5, 0] = c.n_users                                                                          # a user behind the table
    tri[200, 1] = -1                                                                               # an item in front of it
    alive = np.ones(tri.shape[0], dtype=bool)
    alive[[5, 200]] = False
    want = tr.step64(c.w0, tri[alive], c.keep[0][alive], divisor=tri.shape[0])
    r = Run(engine, c.p[0], c.m[0], c.v[0], tri, c.keep[0], 256, 0, check=False)
    with pytest.raises(SdrmError) as err:
        engine.feed_status()
    assert "row id" in str(err.value) and "column index" in str(err.value)
    engine.feed_status()                                                                           # reported once
    for i, t in enumerate(tr.NAMES):
        ref_dev, dev_dev = tr.normwise(c.g[0][i], c.ref[0]["grads"][t]), tr.normwise(r.g[i], want["grads"][t])
        print(f"{t}: device {dev_dev:.3e} bar {tr.BAR_FACTOR * ref_dev:.3e}")
        assert dev_dev <= tr.BAR_FACTOR * ref_dev, t
    ref_dev = abs(c.loss[0] - c.ref[0]["loss"]) / abs(c.ref[0]["loss"])
    assert abs(float(r.losses[0]) - want["loss"]) / abs(want["loss"]) <= tr.BAR_FACTOR * ref_dev
    assert tr.normwise(r.g[4], c.ref[0]["grads"][tr.NAMES[4]]) > 50 * tr.BAR_FACTOR * tr.normwise(c.g[0][4], c.ref[0]["grads"][tr.NAMES[4]])   # (the two pairs did count before)
    good = one_step(engine, "f8", 0) if ("f8", 0) in _RUNS else Run(engine, c.p[0], c.m[0], c.v[0], c.tri[0], c.keep[0], 256, 0)
    engine.feed_status()
    assert np.isfinite(good.losses).all()


@pytest.mark.gpu
def test_refusals_write_nothing(engine):
    c = case("one")
    A = {k: Arena(x) for k, x in (("p", c.p[0]), ("m", c.m[0]), ("v", c.v[0]), ("g", c.p[0]))}
    tri = torch.from_numpy(np.repeat(c.triples, 1100, axis=0)).cuda()
    keep = torch.ones(1100, 14 * c.F, dtype=torch.uint8, device="cuda")
    w32 = [torch.from_numpy(a).cuda() for a in tr.weights(32, 5, 7, 1).values()]
    z32 = [torch.zeros_like(t) for t in w32]

    def call(p=None, m=None, v=None, triples=tri[:1], batch=1, step0=0, **kw):
        return engine.neumf_train_steps(A["p"].views if p is None else p, A["m"].views if m is None else m, A["v"].views if v is None else v,
                                        triples, batch, step0, **kw)

    short = list(A["m"].views)
    short[4] = short[4][:-1]
    bad = dict(factor_32=(dict(p=w32, m=z32, v=z32), "SDRM_ERR_SHAPE"), batch_1025=(dict(triples=tri, batch=1025, keep=keep), "SDRM_ERR_SHAPE"),
               batch_0=(dict(batch=0), "SDRM_ERR_SHAPE"), step0_negative=(dict(step0=-1), "SDRM_ERR_ARG"), p_drop_one=(dict(p_drop=1.0), "SDRM_ERR_ARG"),
               weights_float64=(dict(p=[t.double() for t in A["p"].views]), "float32"),
               moments_on_the_host=(dict(m=[t.cpu() for t in A["m"].views]), "device"), triples_int64=(dict(triples=tri[:1].long()), "int32"),
               moments_of_another_shape=(dict(m=short), "SDRM_ERR_SHAPE"), eleven_moments=(dict(v=A["v"].views[:11]), "SDRM_ERR_SHAPE"),
               keep_of_another_shape=(dict(keep=keep[:1, :5]), "keep"), keep_float=(dict(keep=keep[:1].float()), "keep"),
               grads_of_another_shape=(dict(grads=short), "SDRM_ERR_SHAPE"), moments_are_the_weights=(dict(m=A["p"].views), "SDRM_ERR_ARG"))
    for name, (kw, text) in bad.items():
        with pytest.raises(SdrmError, match=text):
            call(**kw)
        for a in A.values():
            a.unchanged()
    # EXPLICIT without masks: the Python surface cannot say it, the C ABI refuses it
    rec = _lib.NeumfTrain()
    for i in range(12):
        rec.p[i], rec.m[i], rec.v[i] = (A[k].views[i].data_ptr() for k in "pmv")
    rec.n_users, rec.n_items, rec.factor = c.n_users, c.n_items, c.F
    args = (engine._h, C.byref(rec), C.c_void_p(tri.data_ptr()), 1, 1, 0, 1e-3, 0.9, 0.999, 1e-8, 0.5)
    with pytest.raises(SdrmError, match="SDRM_ERR_ARG.*needs keep"):
        engine._check(engine.lib.sdrm_neumf_train_steps(*args, 0, None, 0, 0, None, None, None), "sdrm_neumf_train_steps")
    with pytest.raises(SdrmError, match="SDRM_ERR_ARG"):
        engine._check(engine.lib.sdrm_neumf_train_steps(*args, 2, None, 0, 0, None, None, None), "sdrm_neumf_train_steps")
    rec.factor = 32
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine._check(engine.lib.sdrm_neumf_train_steps(*args, 1, None, 0, 0, None, None, None), "sdrm_neumf_train_steps")
    for a in A.values():
        a.unchanged()
    call()                                                                                         # ... and the accepted call does write
    assert not np.array_equal(A["p"].dev.cpu().numpy(), A["p"].host)


@pytest.mark.gpu
def test_driver_with_device_train(engine):
    training, validation = toy()
    seed, epochs = 2, 2
    h = {}
    got = neumf.compute_neuralcf_results(training, validation, 40, 90, engine=engine, seed=seed, epochs=epochs, eval_recall=False, history=h,
                                         device_train=True)
    # the driver's own numpy draws replayed, the engine called per epoch directly
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = neumf.NCF(40, 90, factor=8, layers=3, dropout=0.5).to(engine.device)
    w_init = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    live = model.engine_weights()
    m, v = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
    n_hold = int(math.ceil(0.2 * training.shape[0]))
    after, parts, losses, step0 = [], [], [], 0
    for epoch in range(epochs):
        perm = rng.permutation(training.shape[0])
        part = training[perm[n_hold:]]
        negatives = part[part[:, 2] == 0]
        n_pos = int((part[:, 2] == 1).sum())
        part = np.concatenate([part, negatives[rng.integers(0, negatives.shape[0], size=n_pos)]])
        part = part[rng.permutation(part.shape[0])]
        parts.append(part)
        out = engine.neumf_train_steps(live, m, v, torch.from_numpy(part.astype(np.int32)).to(engine.device), 256, step0, seed=seed, call_id=epoch)
        step0 += out.numel()
        losses.append(out.cpu().numpy())
        after.append([t.clone() for t in live])
    assert h["epochs_run"] == epochs and 0 <= h["best_epoch"] < epochs and not h["reference_has_no_checkpoint"]
    for name, a, b in zip(tr.NAMES, h["model"].state_dict().values(), after[h["best_epoch"]]):
        assert torch.equal(a, b), name
    per_epoch = [-(-p.shape[0] // 256) for p in parts]
    assert len(h["train_loss"]) == sum(per_epoch) and np.array_equal(np.asarray(h["train_loss"]), np.concatenate(losses))
    first = tr.step64(w_init, parts[0][:256], tr.philox_keep(seed, 0, 0, 256, 8, 0.5))["loss"]
    c = case("f8")
    loss_bar = tr.BAR_FACTOR * max(abs(c.loss[k] - c.ref[k]["loss"]) / abs(c.ref[k]["loss"]) for k in range(tr.STEPS))
    d = abs(h["train_loss"][0] - first) / first
    print("first train loss", h["train_loss"][0], "float64", first, "relative", d, "bar", loss_bar)
    means = [float(np.mean(x)) for x in losses]
    print("mean train loss per epoch", means)
    assert d <= loss_bar
    assert means[-1] < means[0]
    ht = {}
    torch_trained = neumf.compute_neuralcf_results(training, validation, 40, 90, engine=engine, seed=seed, epochs=epochs, eval_recall=False, history=ht)
    for a, b in zip(got, torch_trained):
        assert a.shape == b.shape == (6,) and np.array_equal(np.isnan(a), np.isnan(b))
    assert "train_loss" not in ht
