"""Float64 restatement of ONE train step of the MLP evaluator (sdrm_amd/mlp_eval.py restates the Keras model of mlp_benchmark.py; its
docstring names the Keras facts): forward with the three dropouts, the logits form of binary cross-entropy over all b I elements, every
gradient, Keras's Adam; the case table the host and the device tests build their inputs from; and a restatement of the engine's Philox
keep masks (csrc/mlp_train.h).  numpy only; the Philox words are oracle/philox_ref.py's.

No fixture from the reference exists (it is TensorFlow code): the oracle is computed at test time, and the reference-side figure every
bar is a multiple of is the deviation of the float32 torch module on the CPU from this oracle (`torch_step` below, the one place that
imports torch)."""
from __future__ import annotations

import numpy as np

from oracle.philox_ref import philox4x32_10

NAMES = ("E", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")
F, WIDTHS, KEEP_COLS = 8, (512, 256, 256), 1024
PURPOSE_MLP_DROP = 11
P_DROP, LR, BETAS, EPS = 0.5, 1e-3, (0.9, 0.999), 1e-7
STEP0 = 5                            # Adam's step count before the first step of a case
GAP_FACTOR, BAR_FACTOR = 8.0, 4.0    # tests/neumf_train_ref.py's: gap = GAP_FACTOR x BAR_FACTOR x dev x max|z|

# name: (n_items, rows of the matrix, seed).  The TRAIN part is the first floor(0.8 rows) rows (the fit's validation split).
#   A  8 x 45 is no multiple of 64; 29 train rows: batches of 16 and 13
#   B  17 train rows: batches of 16 and 1
#   C  32 train rows: a batch of 16 with an all-zero row, an item in no row and two equal rows, then one with an item in all 16 rows (an
#      all-zero row and an item in every row cannot share a batch)
CASES = {"A": (45, 37, 4103), "B": (129, 22, 4224), "C": (64, 40, 4329)}
# the rows of a case's CALL of three steps (two for C: rows 0 .. 31 in order), as places in `call_rows`
STEPS = {"A": ((0, 16), (16, 32), (32, 45)), "B": ((0, 16), (16, 32), (32, 33)), "C": ((0, 16), (16, 32))}
# the steps the one-step tests run from the case's start state
SINGLE = (("A", 0), ("A", 2), ("B", 0), ("B", 2), ("C", 0), ("C", 1))


def n_fit(name):
    return int(np.floor(0.8 * CASES[name][1]))


def shapes(n_users, n_items):
    h1, h2, h3 = WIDTHS
    return ((n_users, F), (F * n_items, h1), (h1,), (h1, h2), (h2,), (h2, h3), (h3,), (h3, n_items), (n_items,))


def matrix(name):
    """The case's 0 / 1 matrix [rows, n_items], uint8."""
    n_items, n_rows, seed = CASES[name]
    rng = np.random.default_rng(seed)
    x = (rng.random((n_rows, n_items)) < 0.2).astype(np.uint8)
    if name == "C":
        x[12] = 0                    # batch 0 (rows 0 .. 15): an all-zero row,
        x[:16, 7] = 0                # an item in no row,
        x[9] = x[5]                  # two equal rows
        x[16:32, 20] = 1             # batch 1 (rows 16 .. 31): an item in all 16 rows
    return x


def c_conditions(x):
    """Case C's four conditions on its two batches of 16, as booleans."""
    b0, b1 = x[:16], x[16:32]
    return (bool((b0.sum(axis=1) == 0).any()), bool((b0.sum(axis=0) == 0).any()), bool((b1.sum(axis=0) == 16).any()),
            bool(np.array_equal(b0[9], b0[5]) and b0[5].any()))


def weights(name):
    """The case's start state: (p, m, v) dicts of float32 by NAMES.  Kernels and E from the initialisers' distributions, small random
    biases (so that their gradients' paths carry something), small random moments - zero on E's rows 2 .., which never move."""
    n_items, n_rows, seed = CASES[name]
    rng = np.random.default_rng(seed + 1)
    p, m, v = {}, {}, {}
    for t, shp in zip(NAMES, shapes(n_rows, n_items)):
        if t == "E":
            w = rng.normal(0.0, np.sqrt(2.0 / n_rows), shp)
        elif t.startswith("W"):
            limit = np.sqrt(3.0 / shp[0]) if t == "W4" else np.sqrt(6.0 / (shp[0] + shp[1]))
            w = rng.uniform(-limit, limit, shp)
        else:
            w = rng.normal(0.0, 0.01, shp)
        p[t] = w.astype(np.float32)
        m[t] = (1e-4 * rng.normal(size=shp)).astype(np.float32)
        v[t] = (1e-8 * rng.random(shp)).astype(np.float32)
    m["E"][2:] = 0
    v["E"][2:] = 0
    return p, m, v


def call_rows(name):
    """int64 row ids of the case's call: permutations of the train part one after the other, cut to the call's length (C: rows 0 .. 31)."""
    n_items, n_rows, seed = CASES[name]
    total = STEPS[name][-1][1]
    if name == "C":
        return np.arange(32, dtype=np.int64)
    rng = np.random.default_rng(seed + 2)
    return np.concatenate([rng.permutation(n_fit(name)) for _ in range(-(-total // n_fit(name)))])[:total].astype(np.int64)


def explicit_keep(name):
    """uint8 [call length, 1024]: the case's EXPLICIT masks, one row per place of `call_rows`."""
    n_items, n_rows, seed = CASES[name]
    rng = np.random.default_rng(seed + 3)
    return (rng.random((STEPS[name][-1][1], KEEP_COLS)) >= P_DROP).astype(np.uint8)


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32))


def scale(p):
    return np.float32(1.0 / (1.0 - np.float64(np.float32(p))))


def philox_keep(seed, call_id, j0, n, p):
    """uint8 [n, 1024]: the engine's PHILOX-mode keep decisions for the rows at places j0 .. j0 + n - 1 of a call's row array: column c is
    word c & 3 of Philox4x32-10 with counter (j, c >> 2, PURPOSE_MLP_DROP, call_id) and key seed, kept iff >= floor(p 2^32)."""
    j = np.arange(j0, j0 + n, dtype=np.uint64)[:, None]
    q = np.arange(KEEP_COLS // 4, dtype=np.uint64)[None, :]
    words = philox4x32_10(j, q, PURPOSE_MLP_DROP, call_id, seed)
    w = np.stack([np.broadcast_to(x, (n, q.shape[1])) for x in words], axis=2).reshape(n, KEEP_COLS)
    return (w >= np.uint64(threshold(p))).astype(np.uint8)


def step64(w, x, keep, p_drop=P_DROP, divisor=None):
    """One step in float64 from float32 inputs.  w: the nine tensors by name; x: 0 / 1 [b, I]; keep: [b, 1024] (non-zero = kept).
    Returns dict(loss, grads {name: array}, z (z1, z2, z3 [b, .]), y [b, I]).  `divisor`: what the mean divides by (default b I) - a
    batch whose dead rows were taken out keeps the b it had."""
    w = {k: np.asarray(a, dtype=np.float64) for k, a in w.items()}
    xi = np.asarray(x).astype(np.int64)
    x = xi.astype(np.float64)
    b, n_items = x.shape
    div = float(b * n_items if divisor is None else divisor)
    s = float(scale(p_drop))
    keep = np.asarray(keep) != 0
    k = (keep[:, :512], keep[:, 512:768], keep[:, 768:1024])
    a0 = w["E"][xi].reshape(b, F * n_items)
    a, z, h = [a0], [], a0
    for l in range(3):
        z.append(h @ w[f"W{l + 1}"] + w[f"b{l + 1}"])
        h = np.maximum(z[l], 0.0) * k[l] * s
        a.append(h)
    y = h @ w["W4"] + w["b4"]
    loss = float((np.maximum(y, 0.0) - y * x + np.log1p(np.exp(-np.abs(y)))).sum() / div)
    with np.errstate(over="ignore"):
        d = (1.0 / (1.0 + np.exp(-y)) - x) / div
    grads = {"W4": a[3].T @ d, "b4": d.sum(axis=0)}
    dh = d @ w["W4"].T
    for l in (2, 1, 0):
        dz = dh * k[l] * s * (z[l] > 0)
        grads[f"W{l + 1}"] = a[l].T @ dz
        grads[f"b{l + 1}"] = dz.sum(axis=0)
        dh = dz @ w[f"W{l + 1}"].T
    dE = np.zeros_like(w["E"])
    np.add.at(dE, xi.reshape(-1), dh.reshape(b * n_items, F))
    grads["E"] = dE
    return dict(loss=loss, grads=grads, z=tuple(z), y=y)


def keras_adam(p, g, m, v, step, lr=LR, betas=BETAS, eps=EPS):
    """One update of Keras's Adam in float64: (p, m, v) after step `step` >= 1.  1 - beta is taken from the float32 beta the C ABI carries."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    alpha = float(np.float32(lr)) * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    m = m + (g - m) * (1.0 - b1)
    v = v + (g * g - v) * (1.0 - b2)
    return p - alpha * m / (np.sqrt(v) + float(np.float32(eps))), m, v


def chain64(name):
    """The case's call in float64: a list, per step, of dict(p, m, v AFTER the step, loss, z, grads); the state before step 0 is `weights`."""
    p, m, v = ({k: a.astype(np.float64) for k, a in d.items()} for d in weights(name))
    x, rows, keep = matrix(name), call_rows(name), explicit_keep(name)
    out = []
    for k, (lo, hi) in enumerate(STEPS[name]):
        r = step64(p, x[rows[lo:hi]], keep[lo:hi])
        nxt = {t: keras_adam(p[t], r["grads"][t], m[t], v[t], STEP0 + k + 1) for t in NAMES}
        p, m, v = ({t: nxt[t][i] for t in NAMES} for i in range(3))
        out.append(dict(p=p, m=m, v=v, loss=r["loss"], z=r["z"], grads=r["grads"]))
    return out


def normwise(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def kink_exceptions(z64, dev):
    """Pre-activations of one step that lie within gap = GAP_FACTOR x BAR_FACTOR x dev x max|z| of zero, per layer (see
    tests/neumf_train_ref.py).  z64: (z1, z2, z3); dev: the three normwise deviations of the float32 pre-activations from them."""
    return [int((np.abs(z) < GAP_FACTOR * BAR_FACTOR * float(d) * np.abs(z).max()).sum()) for z, d in zip(z64, dev)]


def torch_step(w, x, keep, dtype, p_drop=P_DROP, divisor=None):
    """The same step by the torch module (sdrm_amd.mlp_eval.MLP) on the CPU under autograd: dict(loss, grads, z) as numpy float64 of what
    torch computed in `dtype`.  z: the module's own arithmetic repeated without autograd."""
    import torch

    from sdrm_amd import mlp_eval
    n_users, n_items = w["E"].shape[0], w["b4"].shape[0]
    model = mlp_eval.MLP(n_users, n_items, dropout=p_drop)
    model.load_keras_weights([w[t] for t in NAMES])
    model = model.to(dtype)
    model.train()
    xt = torch.as_tensor(np.asarray(x), dtype=dtype)
    kt = torch.as_tensor(np.asarray(keep))
    y = model(xt, kt)
    loss = (torch.clamp(y, min=0) - y * xt + torch.log1p(torch.exp(-y.abs()))).sum() / (y.numel() if divisor is None else divisor)
    loss.backward()
    grads = {t: p.grad.double().numpy() for t, p in zip(NAMES, model.engine_weights())}
    with torch.no_grad():
        z, h, at = [], model.E[xt.long()].reshape(xt.shape[0], -1), 0
        for l, width in enumerate(WIDTHS):
            z.append(h @ getattr(model, f"W{l + 1}") + getattr(model, f"b{l + 1}"))
            h = torch.relu(z[l]) * (kt[:, at:at + width] != 0).to(dtype) * float(scale(p_drop))
            at += width
    return dict(loss=float(loss.double().item()), grads=grads, z=tuple(a.double().numpy() for a in z))


def torch_chain(name, dtype=None):
    """The case's call by the CPU checker: the torch module's step (`torch_step`) and `mlp_eval.KerasAdam`, in `dtype` (default float32).
    A list, per step, of dict(p AFTER the step as float64 numpy, loss, z)."""
    import torch

    from sdrm_amd import mlp_eval
    dtype = torch.float32 if dtype is None else dtype
    p0, m0, v0 = weights(name)
    params = [torch.tensor(p0[t], dtype=dtype) for t in NAMES]
    opt = mlp_eval.KerasAdam(params, lr=LR, betas=BETAS, eps=EPS)
    opt.exp_avg = [torch.tensor(m0[t], dtype=dtype) for t in NAMES]
    opt.exp_avg_sq = [torch.tensor(v0[t], dtype=dtype) for t in NAMES]
    opt.t = STEP0
    x, rows, keep = matrix(name), call_rows(name), explicit_keep(name)
    out = []
    for lo, hi in STEPS[name]:
        r = torch_step({t: q.numpy() for t, q in zip(NAMES, params)}, x[rows[lo:hi]], keep[lo:hi], dtype)
        for t, q in zip(NAMES, params):
            q.grad = torch.as_tensor(r["grads"][t]).to(dtype)
        opt.step()
        out.append(dict(p={t: q.double().numpy().copy() for t, q in zip(NAMES, params)}, loss=r["loss"], z=r["z"]))
    return out
