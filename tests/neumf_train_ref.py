"""Float64 restatement of ONE train step of the NeuMF evaluator (reference neural_cf_benchmark_pt.py:125-144 in train mode, :195-200:
forward with the three dropouts, BCEWithLogitsLoss, the gradients of all twelve tensors), the case table that
tests/golden/make_neumf_train_golden.py and tests/test_neumf_train.py rebuild their inputs from, and a restatement of the engine's Philox
keep masks (csrc/neumf_train.h).  Checker only: numpy, no torch.  Adam is tests/vae_adam_ref.adam_step.

A case is drawn from ONE seed (`numpy.random.default_rng`): the twelve tensors by `neumf_ref.weights(..., seed)`, the triples by
`triples(..., seed)`.  The seed itself is found by the generator (the first one from the case's base seed whose float64 pre-activations
keep clear of zero, see `kink_exceptions`) and stored in the fixture; so are the dropout masks, which are torch's."""
from __future__ import annotations

import numpy as np

from neumf_ref import NAMES, normwise, weights  # noqa: F401  (re-exported: the tests take them from here)
from oracle.philox_ref import philox4x32_10

PURPOSE_NEUMF_DROP = 10
P_DROP = 0.5
LR = 1e-3
STEPS = 3            # consecutive steps stored per case
GAP_FACTOR, BAR_FACTOR = 8.0, 4.0   # gap = GAP_FACTOR x BAR_FACTOR x dev x max|z| (tests/test_neumf_eval.py's near-tie gap, on pre-activations)

# name: (factor, n_users, n_items, triples n, the (start, stop) of every step's batch in the triple array, base seed)
CASES = {
    "f8": (8, 300, 47, 549, ((0, 256), (256, 512), (512, 549)), 700),
    "f16": (16, 23, 19, 141, ((0, 70), (70, 140), (140, 141)), 800),
    "one": (8, 5, 7, 1, ((0, 1), (0, 1), (0, 1)), 900),
}
BATCH = {"f8": 256, "f16": 70, "one": 1}


def triples(n_users, n_items, n, seed):
    """int32 [n, 3]: random users, items and 0 / 1 labels (a pair may repeat: the step does not care)."""
    rng = np.random.default_rng(seed + 1000)
    return np.stack([rng.integers(0, n_users, n), rng.integers(0, n_items, n), rng.integers(0, 2, n)], axis=1).astype(np.int32)


def case_inputs(name, seed):
    """(weights dict of float32, triples int32 [n, 3]) of a case at `seed`."""
    F, n_users, n_items, n, _, _ = CASES[name]
    return weights(F, n_users, n_items, seed), triples(n_users, n_items, n, seed)


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32))


def scale(p):
    return np.float32(1.0 / (1.0 - np.float64(np.float32(p))))


def philox_keep(seed, call_id, j0, n, factor, p):
    """uint8 [n, 14 factor]: the engine's PHILOX-mode keep decisions for the pairs at positions j0 .. j0 + n - 1 of a call's triple array:
    column c is word c & 3 of Philox4x32-10 with counter (j, c >> 2, PURPOSE_NEUMF_DROP, call_id) and key seed, kept iff >= floor(p 2^32)."""
    j = np.arange(j0, j0 + n, dtype=np.uint64)[:, None]
    q = np.arange(14 * factor // 4, dtype=np.uint64)[None, :]
    words = philox4x32_10(j, q, PURPOSE_NEUMF_DROP, call_id, seed)
    w = np.stack([np.broadcast_to(x, (n, q.shape[1])) for x in words], axis=2).reshape(n, 14 * factor)
    return (w >= np.uint64(threshold(p))).astype(np.uint8)


def step64(w, tri, keep, p_drop=P_DROP, divisor=None):
    """One step in float64 from float32 inputs.  w: the twelve tensors by name; tri: int [b, 3]; keep: [b, 14F] (non-zero = kept).
    Returns dict(loss, grads {name: array}, z (z1, z2, z3 pre-activations [b, .]), y [b]).  `divisor`: what the mean divides by
    (default b) - a batch whose dead pairs were taken out keeps the b it had."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    tri = np.asarray(tri, dtype=np.int64)
    u, i, lab = tri[:, 0], tri[:, 1], tri[:, 2].astype(np.float64)
    b = tri.shape[0]
    div = float(b if divisor is None else divisor)
    F = w[NAMES[0]].shape[1]
    s = float(scale(p_drop))
    keep = np.asarray(keep) != 0
    k = (keep[:, :8 * F], keep[:, 8 * F:12 * F], keep[:, 12 * F:14 * F])
    W, B = [w[NAMES[4]], w[NAMES[6]], w[NAMES[8]]], [w[NAMES[5]], w[NAMES[7]], w[NAMES[9]]]
    x0 = np.concatenate([w[NAMES[2]][u], w[NAMES[3]][i]], axis=1)
    a, z, h = [], [], x0
    for l in range(3):
        a.append(h * k[l] * s)
        z.append(a[l] @ W[l].T + B[l])
        h = np.maximum(z[l], 0.0)
    pu, qi = w[NAMES[0]][u], w[NAMES[1]][i]
    g = pu * qi
    wp, bp = w[NAMES[10]][0], w[NAMES[11]][0]
    y = np.concatenate([g, h], axis=1) @ wp + bp
    loss = float((np.maximum(y, 0.0) - y * lab + np.log1p(np.exp(-np.abs(y)))).sum() / div)
    with np.errstate(over="ignore"):
        dy = (1.0 / (1.0 + np.exp(-y)) - lab) / div
    grads = {NAMES[11]: np.array([dy.sum()]), NAMES[10]: (dy[:, None] * np.concatenate([g, h], axis=1)).sum(axis=0)[None, :]}
    dg = dy[:, None] * wp[None, :F]
    dh = dy[:, None] * wp[None, F:]
    for l in (2, 1, 0):
        dz = dh * (z[l] > 0)
        grads[NAMES[4 + 2 * l]] = dz.T @ a[l]
        grads[NAMES[5 + 2 * l]] = dz.sum(axis=0)
        dh = (dz @ W[l]) * k[l] * s
    for name, rows, d in ((NAMES[0], u, dg * qi), (NAMES[1], i, dg * pu), (NAMES[2], u, dh[:, :4 * F]), (NAMES[3], i, dh[:, 4 * F:])):
        t = np.zeros_like(w[name])
        np.add.at(t, rows, d)
        grads[name] = t
    return dict(loss=loss, grads=grads, z=tuple(z), y=y)


def kink_exceptions(z64, dev):
    """Pre-activations of one step that lie within gap = GAP_FACTOR x BAR_FACTOR x dev x max|z| of zero, per layer: a float32 evaluation
    may put such a z on the other side of ReLU's kink, and the gradients then differ by a whole term.  z64: (z1, z2, z3); dev: the three
    normwise deviations of the reference's float32 pre-activations from them."""
    return [int((np.abs(z) < GAP_FACTOR * BAR_FACTOR * float(d) * np.abs(z).max()).sum()) for z, d in zip(z64, dev)]


def f8_conditions(tri, batches, n_users):
    """The four things the f8 case is there for, as booleans: (a user AND an item repeated within a batch, an id more than twice in one
    batch, a partial last batch, a user row that step 0 names and step 1 does not)."""
    (a0, b0), (a1, b1) = batches[0], batches[1]
    first = tri[a0:b0]
    cu, ci = np.bincount(first[:, 0], minlength=n_users), np.bincount(first[:, 1])
    return (bool(cu.max() >= 2 and ci.max() >= 2), bool(max(cu.max(), ci.max()) > 2), batches[-1][1] - batches[-1][0] < b0 - a0,
            bool(np.setdiff1d(first[:, 0], tri[a1:b1, 0]).size > 0))
