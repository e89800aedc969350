"""The MLP evaluator's train steps on the device (csrc/mlp_train.h; sdrm_mlp_train_steps; `Engine.mlp_train_steps`;
`mlp_eval.compute_mlp_results(device_train=True)`).  Every test needs the GPU; tests/test_mlp_host.py holds what does not.

The reference is Keras code that cannot run here, so there is no fixture: the oracle is tests/mlp_eval_ref.py (float64, held to the
torch module in float64 by the host tests), and the reference-side figure behind every bar is the deviation of the FLOAT32 torch module
on the CPU from that oracle for the same tensor and step, measured here.  BAR_FACTOR (4, the NeuMF train tests') times that covers
another summation order; nothing may exceed the project's 1e-4.  Every tensor the engine writes is carved out of guarded arenas and
the guards are checked after every call."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import mlp_eval_ref as mr
from vae_adam_ref import rel_max
from sdrm_amd import _lib, mlp_eval
from sdrm_amd.engine import Engine, SdrmError

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # the project's fp32 bar
GUARD, SENTINEL = 8, 12345.0
SHAPE, ARG = -2, -1
STEP_LAUNCHES, CALL_LAUNCHES = 15, 2   # csrc/mlp_train.h: per step, and once per call (B_f of the weights as they stand)


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


class Arena:
    """Arrays of one dtype carved out of one device buffer, GUARD sentinel elements or more between neighbours and at both ends, every
    array on a 64-element boundary (so on the 16-byte grid)."""

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


def as_list(d):
    return [d[t] for t in mr.NAMES]


class Run:
    """One `mlp_train_steps` call on arenas: p, m, v (and g), the row ids and the masks.  `state`: (p, m, v) lists of float32 arrays."""

    def __init__(self, engine, csr_dev, state, rows, keep, step0, want_grads=False, batch=16, check=True, **kw):
        self.A = {k: Arena(x) for k, x in zip("pmv", state)}
        if want_grads:
            self.A["g"] = Arena([np.full(a.shape, 777.0, dtype=np.float32) for a in state[0]])
        self.rows = Arena([np.asarray(rows, dtype=np.int64)], sentinel=-7)
        self.keep = Arena([np.asarray(keep, dtype=np.uint8)], sentinel=1) if keep is not None else None
        n0 = engine.launch_count()
        losses = engine.mlp_train_steps(self.A["p"].views, self.A["m"].views, self.A["v"].views, csr_dev, self.rows.views[0], batch, step0, lr=mr.LR,
                                        betas=mr.BETAS, eps=mr.EPS, p_drop=mr.P_DROP, keep=self.keep.views[0] if self.keep else None,
                                        grads_out=self.A["g"].views if want_grads else None, check=check, **kw)
        self.launches = engine.launch_count() - n0
        self.losses = losses.cpu().numpy()
        self.p, self.m, self.v = (self.A[k].arrays() for k in "pmv")
        self.g = self.A["g"].arrays() if want_grads else None
        self.rows.unchanged()
        if self.keep:
            self.keep.unchanged()

    def state(self):
        return self.p, self.m, self.v


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()                                                                       # (computed once, shared, never changed)
    return _CACHE[key]


def csr_of(engine, name):
    return cached(("csr", name), lambda: engine.csr_to_device(csr_matrix(mr.matrix(name).astype(np.float32))))


def start(name):
    return cached(("start", name), lambda: tuple(as_list(d) for d in mr.weights(name)))


def batch_of(name, k):
    lo, hi = mr.STEPS[name][k]
    return mr.call_rows(name)[lo:hi], mr.explicit_keep(name)[lo:hi]


def references(name, k):
    """(float64 oracle, float32 torch module on the CPU) of step k of the case from its start state."""
    def make():
        rows, keep = batch_of(name, k)
        x = mr.matrix(name)[rows]
        return mr.step64(mr.weights(name)[0], x, keep), mr.torch_step(mr.weights(name)[0], x, keep, torch.float32)
    return cached(("ref", name, k), make)


def one_step(engine, name, k):
    """Step k of a case from the start state, EXPLICIT masks, gradients out (run once, shared by the tests)."""
    def make():
        rows, keep = batch_of(name, k)
        return Run(engine, csr_of(engine, name), start(name), rows, keep, mr.STEP0, want_grads=True)
    return cached(("run", name, k), make)


def check_gradients(what, got_g, got_loss, want, ref):
    """Every gradient and the loss at BAR_FACTOR x the float32 torch module's own deviation from the oracle, never above 1e-4.  Returns
    the worst ratio device / reference."""
    failures, worst = [], 0.0
    for i, t in enumerate(mr.NAMES):
        ref_dev, dev_dev = mr.normwise(ref["grads"][t], want["grads"][t]), mr.normwise(got_g[i], want["grads"][t])
        print(f"{what} {t}: device {dev_dev:.3e} reference {ref_dev:.3e} bar {mr.BAR_FACTOR * ref_dev:.3e}")
        worst = max(worst, dev_dev / ref_dev)
        if not (dev_dev <= mr.BAR_FACTOR * ref_dev and dev_dev <= TOL):
            failures.append((t, dev_dev, ref_dev))
    ref_dev, dev_dev = abs(ref["loss"] - want["loss"]) / abs(want["loss"]), abs(got_loss - want["loss"]) / abs(want["loss"])
    print(f"{what} loss: device {dev_dev:.3e} reference {ref_dev:.3e} bar {mr.BAR_FACTOR * ref_dev:.3e}")
    if not (dev_dev <= mr.BAR_FACTOR * ref_dev and dev_dev <= TOL):
        failures.append(("loss", dev_dev, ref_dev))
    assert not failures, (what, failures)
    return worst


@pytest.mark.parametrize("name,k", mr.SINGLE)
def test_gradients_and_loss_of_one_step(engine, name, k):
    """All nine gradients and the loss of one step against the float64 oracle.  The figures measured on one MI355X are in DESIGN 4y."""
    r = one_step(engine, name, k)
    want, ref = references(name, k)
    assert r.launches == CALL_LAUNCHES + STEP_LAUNCHES and r.losses.shape == (1,)
    check_gradients(f"{name} step {k}", r.g, float(r.losses[0]), want, ref)
    assert not r.g[0][2:].any() and r.g[0][:2].all()                                               # dE: rows 0 and 1 and nothing else


def adam_bars(p, m, v, p0, want, what):
    """tests/test_vae_adam.py's bars for one tensor: m, v rel_max <= 1e-4 (exactly zero where the expectation is all zero),
    |p - p_ref| <= 2^-24 |p_ref| + 1e-4 max|p_ref - p_0|."""
    p_ref, m_ref, v_ref = want
    for key, a, r in (("m", m, m_ref), ("v", v, v_ref)):
        if np.abs(r).max() > 0:
            assert rel_max(a, r) <= TOL, (what, key, rel_max(a, r))
        else:
            assert not np.asarray(a).any(), (what, key)
    bound = 2.0 ** -24 * np.abs(p_ref) + TOL * np.abs(p_ref - np.asarray(p0, dtype=np.float64)).max()
    err = np.abs(np.asarray(p, dtype=np.float64) - p_ref)
    assert (err <= bound).all(), (what, float(err.max()), float(bound.min()))


@pytest.mark.parametrize("name,k", mr.SINGLE)
def test_update_after_one_step(engine, name, k):
    """p, m, v after the step against Keras's Adam in float64 applied to the gradients the device returned."""
    r = one_step(engine, name, k)
    p0, m0, v0 = start(name)
    for i, t in enumerate(mr.NAMES):
        want = mr.keras_adam(p0[i], r.g[i], m0[i], v0[i], mr.STEP0 + 1)
        adam_bars(r.p[i], r.m[i], r.v[i], p0[i], want, (name, k, t))
        assert np.abs(want[0] - p0[i]).max() > 0
    for got, was in zip((r.p[0], r.m[0], r.v[0]), (p0[0], m0[0], v0[0])):
        assert np.array_equal(got[2:], was[2:])                                                    # rows 2 .. of E do not move
    assert not r.m[0][2:].any() and not r.v[0][2:].any()


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["A", "B"])
def test_chaining(engine, name):
    """One call of three steps (the last one the 13-row / the 1-row batch) = three calls of one step, bit for bit, step0 carried on; a
    second identical call gives the same bits; the parameters follow the float64 chain within BAR_FACTOR x what the CPU checker's chain
    (float32 torch module + KerasAdam) deviates by at that step, measured on each tensor's movement p_k - p_0."""
    csr, rows, keep, steps = csr_of(engine, name), mr.call_rows(name), mr.explicit_keep(name), mr.STEPS[name]
    whole = Run(engine, csr, start(name), rows, keep, mr.STEP0)
    assert whole.launches == CALL_LAUNCHES + 3 * STEP_LAUNCHES and whole.losses.shape == (3,)
    again = Run(engine, csr, start(name), rows, keep, mr.STEP0)
    for a, b in zip(whole.state(), again.state()):
        assert same_bits(a, b)
    assert np.array_equal(whole.losses, again.losses)
    state, parts = start(name), []
    for k, (lo, hi) in enumerate(steps):
        parts.append(Run(engine, csr, state, rows[lo:hi], keep[lo:hi], mr.STEP0 + k))
        state = parts[-1].state()
    for a, b in zip(whole.state(), state):
        assert same_bits(a, b)
    assert np.array_equal(whole.losses, np.concatenate([q.losses for q in parts]))
    c64, c32 = mr.chain64(name), mr.torch_chain(name)
    p0, failures = start(name)[0], []
    for k in range(3):
        for i, t in enumerate(mr.NAMES):
            move = c64[k]["p"][t] - p0[i]
            ref_dev, dev_dev = mr.normwise(c32[k]["p"][t] - p0[i], move), mr.normwise(parts[k].p[i].astype(np.float64) - p0[i], move)
            print(f"{name} chain step {k} {t}: device {dev_dev:.3e} checker {ref_dev:.3e} bar {mr.BAR_FACTOR * ref_dev:.3e}")
            if not dev_dev <= mr.BAR_FACTOR * ref_dev:
                failures.append((k, t, dev_dev, ref_dev))
        want = c64[k]["loss"]
        ref_dev, dev_dev = abs(c32[k]["loss"] - want) / want, abs(float(whole.losses[k]) - want) / want
        print(f"{name} chain step {k} loss: device {dev_dev:.3e} checker {ref_dev:.3e} bar {mr.BAR_FACTOR * ref_dev:.3e}")
        if not (dev_dev <= mr.BAR_FACTOR * ref_dev and dev_dev <= TOL):
            failures.append((k, "loss", dev_dev, ref_dev))
    assert not failures, failures


def test_philox_mode_equals_explicit_with_restated_masks(engine):
    name, seed, call_id = "A", 77, 3
    csr, rows = csr_of(engine, name), mr.call_rows(name)
    a = Run(engine, csr, start(name), rows, None, mr.STEP0, seed=seed, call_id=call_id)
    b = Run(engine, csr, start(name), rows, mr.philox_keep(seed, call_id, 0, rows.shape[0], mr.P_DROP), mr.STEP0)
    for x, y in zip(a.state(), b.state()):
        assert same_bits(x, y)
    assert np.array_equal(a.losses, b.losses)
    c = Run(engine, csr, start(name), rows, None, mr.STEP0, seed=seed, call_id=call_id + 1)
    assert not np.array_equal(a.losses, c.losses)                                                  # another call id: other masks


def test_bad_row_id_and_bad_column_index(engine):
    """A row id outside the matrix and a column index outside [0, n_items) are reported, add nothing (the divisor still counts them),
    and no store lands outside the tensors (the arenas' guards)."""
    name = "A"
    n_items, n_rows, _ = mr.CASES[name]
    rows, keep = batch_of(name, 0)
    x = mr.matrix(name)
    p0 = mr.weights(name)[0]
    for bad_id in (n_rows, -1):
        bad_rows = rows.copy()
        bad_rows[4] = bad_id
        r = Run(engine, csr_of(engine, name), start(name), bad_rows, keep, mr.STEP0, want_grads=True, check=False)
        with pytest.raises(SdrmError, match="row id outside"):
            engine.feed_status()
        live = np.delete(np.arange(16), 4)
        want = mr.step64(p0, x[rows[live]], keep[live], divisor=16 * n_items)
        ref = mr.torch_step(p0, x[rows[live]], keep[live], torch.float32, divisor=16 * n_items)
        check_gradients(f"bad row {bad_id}", r.g, float(r.losses[0]), want, ref)
    # a column index outside the matrix in row rows[2]: that entry is skipped
    m = csr_matrix(x.astype(np.float32))
    m.sort_indices()
    victim = int(rows[2])
    assert m.indptr[victim + 1] - m.indptr[victim] >= 2
    at = int(m.indptr[victim])
    lost = int(m.indices[at])
    for bad_col in (n_items + 3, -2):
        indices = m.indices.astype(np.int32).copy()
        indices[at] = bad_col
        csr_dev = (torch.from_numpy(m.indptr.astype(np.int64)).cuda(), torch.from_numpy(indices).cuda(), None, m.shape)
        r = Run(engine, csr_dev, start(name), rows, keep, mr.STEP0, want_grads=True, check=False)
        with pytest.raises(SdrmError, match="column index outside"):
            engine.feed_status()
        xb = x[rows].copy()
        xb[2, lost] = 0
        want, ref = mr.step64(p0, xb, keep), mr.torch_step(p0, xb, keep, torch.float32)
        check_gradients(f"bad column {bad_col}", r.g, float(r.losses[0]), want, ref)
    engine.feed_status()                                                                           # the word was cleared


def test_refused_calls_launch_nothing(engine):
    name = "A"
    n_items, n_rows, _ = mr.CASES[name]
    indptr, indices, _, _ = csr_of(engine, name)
    A = {k: Arena(x) for k, x in zip("pmv", start(name))}
    A["g"] = Arena([np.zeros(a.shape, dtype=np.float32) for a in start(name)[0]])
    rows = torch.from_numpy(mr.call_rows(name)).cuda()
    keep = torch.from_numpy(mr.explicit_keep(name)).cuda()
    losses = torch.zeros(3, dtype=torch.float64, device="cuda")
    n0 = engine.launch_count()

    def call(p=None, m=None, v=None, g=None, n=16, batch=16, mode=0, keep_t=keep, rows_t=rows):
        """The C call itself; p, m, v: lists of nine addresses (default: the arenas' tensors), g: nine tensors or None."""
        rec = _lib.MlpTrain()
        for field, given, key in ((rec.p, p, "p"), (rec.m, m, "m"), (rec.v, v, "v")):
            addrs = given if given is not None else [t.data_ptr() for t in A[key].views]
            for i in range(9):
                field[i] = addrs[i]
        rec.n_users, rec.n_items = n_rows, n_items
        gptr = None if g is None else (C.c_void_p * 9)(*[t.data_ptr() for t in g])

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())
        return engine.lib.sdrm_mlp_train_steps(engine._h, C.byref(rec), ptr(indptr), ptr(indices), n_rows, ptr(rows_t), n, batch, mr.STEP0, mr.LR, 0.9,
                                               0.999, mr.EPS, mr.P_DROP, mode, ptr(keep_t), 0, 0, ptr(losses), gptr, None)

    assert call(batch=17, n=17) == SHAPE and call(batch=0) == SHAPE and call(n=0) == SHAPE
    assert call(g=A["g"].views, n=32) == ARG                                                       # grads_out with two steps
    views = A["p"].views
    overlap = [t.data_ptr() for t in A["m"].views]
    overlap[3] = views[1].data_ptr() + 4096                                                        # m[W2] inside p[W1]
    assert call(m=overlap) == ARG
    null = [t.data_ptr() for t in views]
    null[5] = None
    assert call(p=null) == ARG                                                                     # a null tensor
    assert call(rows_t=None) == ARG and call(keep_t=None) == ARG and call(mode=2) == ARG           # null rows; EXPLICIT without keep; unknown mode
    off = [t.data_ptr() for t in A["v"].views]
    off[2] += 4                                                                                    # v[b1] off the 16-byte grid
    assert call(v=off) == ARG
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.mlp_train_steps(views, A["m"].views, A["v"].views, csr_of(engine, name), rows[:17], 17, 0, keep=keep[:17])
    assert engine.launch_count() == n0
    for k in "pmvg":
        A[k].unchanged()
    assert not losses.any()
    assert call(g=A["g"].views) == 0                                                               # the same arguments, one step: accepted
    torch.cuda.synchronize()
    assert engine.launch_count() == n0 + CALL_LAUNCHES + STEP_LAUNCHES
    engine.feed_status()


def test_driver_trains_on_the_device(engine):
    """`compute_mlp_results(device_train=True)` on case A's row counts (37 rows: 29 train rows, batches of 16 and 13) at 77 items -
    ranking at k = 50 needs more than 50 columns, which the 45 of case A are not (the reference's own `argpartition` fails there).
    The first step's loss against the oracle on the driver's own start weights, row order and Philox masks."""
    seed, n_rows, n_items = 3, 37, 77
    rng = np.random.default_rng(2)
    x = (rng.random((n_rows, n_items)) < 0.2).astype(np.float32)
    training, validation = csr_matrix(x), csr_matrix((rng.random((12, n_items)) < 0.3).astype(np.float32))
    h = {}
    rec, ndcg = mlp_eval.compute_mlp_results(training, validation, engine=engine, seed=seed, epochs=2, history=h, device_train=True)
    assert rec.shape == (6,) and ndcg.shape == (6,) and np.isfinite(rec).all() and np.isfinite(ndcg).all()
    assert ((0 <= rec) & (rec <= 1)).all() and ((0 <= ndcg) & (ndcg <= 1)).all()
    assert h["epochs_run"] == 2 and len(h["val_rmse"]) == 2 and len(h["train_loss"]) == 4 and h["best_epoch"] in (0, 1)
    assert all(np.isfinite(h["val_rmse"])) and h["per_user"][0].shape[0] == 6 and h["per_user"][0].shape == h["per_user"][1].shape
    assert next(h["model"].parameters()).device == engine.device
    torch.manual_seed(seed)
    w0 = {t: q.detach().numpy().copy() for t, q in zip(mr.NAMES, mlp_eval.MLP(n_rows, n_items).engine_weights())}
    order = np.random.default_rng(seed).permutation(29)[:16]
    keep = mr.philox_keep(seed, 0, 0, 16, 0.5)
    want, ref = mr.step64(w0, x[order], keep), mr.torch_step(w0, x[order], keep, torch.float32)
    ref_dev, dev_dev = abs(ref["loss"] - want["loss"]) / want["loss"], abs(h["train_loss"][0] - want["loss"]) / want["loss"]
    print(f"driver first loss: device {dev_dev:.3e} reference {ref_dev:.3e} bar {mr.BAR_FACTOR * ref_dev:.3e}")
    assert dev_dev <= mr.BAR_FACTOR * ref_dev and dev_dev <= TOL
