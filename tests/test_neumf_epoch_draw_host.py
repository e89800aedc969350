"""The host side of the NeuMF evaluator's epoch draw (sdrm_neumf_epoch_draw, csrc/neumf_draw.h; `Engine.neumf_epoch_draw`;
`neumf.compute_neuralcf_results(device_draw=True)`), no GPU: the numpy restatement tests/neumf_draw_ref.py held to the definition's own
properties (bijection, walk bound, marginal uniformity, the draw's bookkeeping), `neumf.RankingProblem.select` against
`neumf.ranking_problem`, the envelope behind `sdrm_debug_neumf_draw_args`, the symbols / header / ctypes table, the driver's refusals."""
import inspect
import os
import re

import numpy as np
import pytest

import neumf_draw_ref as ref
from test_neumf_train import toy
from sdrm_amd import _lib, neumf
from sdrm_amd.engine import Engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -2, -1
SIZES = (1, 2, 3, 4, 5, 7, 16, 17, 255, 256, 257, 1000, 4097, 65536, 65537, 70001)


@pytest.mark.parametrize("n", SIZES)
def test_perm_is_a_bijection_inside_the_walk_bound(n):
    for seed, epoch, draw in ((0, 0, 0), (3, 1, 2), (2 ** 40 + 5, 7, 0)):
        walks = []
        p = ref.perm(n, seed, epoch, draw, walks_out=walks)       # (asserts the bound itself)
        assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch, draw)
        assert walks[0] < ref.MAX_WALKS
    assert 4 ** ref.half_bits(n) >= n and (n <= 2 or 4 ** (ref.half_bits(n) - 1) < n)


def test_perm_depends_on_draw_epoch_and_seed():
    base = ref.perm(1000, 1, 1, 0)
    for kw in (dict(draw=2), dict(epoch=2), dict(seed=2)):
        other = ref.perm(1000, **{**dict(seed=1, epoch=1, draw=0), **kw})
        assert not np.array_equal(base, other), kw
    assert np.array_equal(base, ref.perm(1000, 1, 1, 0))


def test_perm_places_are_marginally_uniform():
    """The place of element 0 under perm(1000, seed = s, epoch = 1, draw = 2), s = 0 .. 1999, in ten bins of 100: chi-square at most 27.88,
    the 99.9 % point for 9 degrees of freedom.  (Uniformity over all n! orders is NOT claimed: a Feistel network reaches only part of them.)"""
    places = np.asarray([int(np.flatnonzero(ref.perm(1000, s, 1, 2) == 0)[0]) for s in range(2000)])
    observed = np.bincount(places // 100, minlength=10)
    chi2 = float(((observed - 200.0) ** 2 / 200.0).sum())
    print("chi-square", chi2, "bins", observed.tolist())
    assert chi2 <= 27.88


def mixed(n=1000, seed=0, ones=0.4, n_users=50, n_items=300):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, n_users, n), rng.integers(0, n_items, n), (rng.random(n) < ones).astype(np.int64)], axis=1).astype(np.int32)


def rows_sorted(a):
    return a[np.lexsort(a.T[::-1])]


def test_epoch_draw_properties():
    T = mixed()
    T[:, 1] = np.arange(1000)                                    # (every row distinct: rows can be told apart)
    n_hold = 200
    hold, out, (n_pos, n_neg, m), present = ref.epoch_draw(T, n_hold, seed=4, epoch=3, n_users=50)
    p0 = ref.perm(1000, 4, 3, 0)
    part = T[p0[n_hold:]]
    assert np.array_equal(hold, T[p0[:n_hold]])
    assert np.array_equal(rows_sorted(np.concatenate([hold, part])), rows_sorted(T))            # hold ++ part is T as a multiset
    assert n_pos == int((part[:, 2] == 1).sum()) and n_neg == int((part[:, 2] == 0).sum()) and n_pos and n_neg
    assert m == 800 + n_pos and out.shape == (m, 3)
    # out is (part ++ extra) shuffled: every part row once more than its copies among the extra rows, every extra row a label-0 row of part
    ids, counts = np.unique(out[:, 1], return_counts=True)
    assert np.array_equal(ids, np.sort(part[:, 1]))
    extra_items = np.repeat(ids, counts - 1)
    assert extra_items.shape[0] == n_pos and np.all(T[extra_items, 2] == 0)
    assert np.array_equal(np.flatnonzero(present), np.unique(hold[:, 0]))
    # no label 0, or no label 1: nothing is drawn again
    for label in (0, 1):
        U = T.copy()
        U[:, 2] = label
        _, out1, (n_pos1, n_neg1, m1), _ = ref.epoch_draw(U, n_hold, seed=4, epoch=3)
        assert m1 == 800 and (n_pos1, n_neg1) == ((800, 0) if label else (0, 800))
        assert np.array_equal(rows_sorted(out1), rows_sorted(U[p0[n_hold:]]))
    # a label-2 row passes through and counts in neither
    V = T.copy()
    where = int(p0[n_hold + 17])
    V[where, 2] = 2
    _, out2, (n_pos2, n_neg2, m2), _ = ref.epoch_draw(V, n_hold, seed=4, epoch=3)
    assert n_pos2 + n_neg2 == 799 and m2 == 800 + n_pos2 and int((out2[:, 2] == 2).sum()) == 1


def awkward():
    """Duplicate pairs, label-0 pairs, a held-out item that never occurs in training, a user only in the held-out array."""
    training = np.asarray([(u, i, (u + i) % 2) for u in (0, 2, 3, 7) for i in range(0, 60, 1 + u % 3)] + [(2, 4, 1), (2, 4, 0), (7, 0, 1)])
    heldout = np.asarray([(0, 1, 1), (0, 1, 1), (2, 999, 1), (2, 6, 0), (3, 3, 1), (5, 2, 1), (7, 59, 1), (7, 58, 1)])
    return training, heldout


def same_csr(a, b):
    return (a.shape == b.shape and a.indptr.dtype == b.indptr.dtype and a.indices.dtype == b.indices.dtype and a.data.dtype == b.data.dtype
            and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data))


@pytest.mark.parametrize("case", [toy, awkward])
def test_ranking_problem_select_is_ranking_problem(case):
    training, heldout = case()
    problem = neumf.RankingProblem(training, heldout)
    every = np.unique(np.concatenate([training[:, 0], heldout[:, 0]]))
    rng = np.random.default_rng(0)
    lists = [every, rng.choice(every, size=2 * every.shape[0] // 3, replace=True), np.asarray([every.max() + 5, -3, 1000000]),
             np.concatenate([every[:2], [every.max() + 1]]), np.asarray([], dtype=np.int64), []]
    for users in lists:
        want, got = neumf.ranking_problem(training, heldout, users), problem.select(users)
        assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0])
        assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1])
        assert same_csr(got[2], want[2]) and same_csr(got[3], want[3]), users
        assert got[2].has_sorted_indices and got[3].has_sorted_indices


def test_rank_all_items_with_a_problem_is_unchanged():
    import torch
    training, validation = toy()
    torch.manual_seed(0)
    model = neumf.NCF(40, 90)
    users = validation[::3, 0]
    want = neumf.rank_all_items(model, training, validation, users)
    got = neumf.rank_all_items(model, training, validation, users, problem=neumf.RankingProblem(training, validation))
    assert np.array_equal(want[0], got[0], equal_nan=True) and np.array_equal(want[1], got[1], equal_nan=True)


def test_debug_neumf_draw_args_envelope():
    lib = _lib.load()

    def call(n=1000, n_hold=200, capacity=1600, with_present=1, n_users=5):
        return lib.sdrm_debug_neumf_draw_args(n, n_hold, capacity, with_present, n_users)

    assert call() == 0 and call(n=2, n_hold=1, capacity=2) == 0 and call(n_hold=1, capacity=1998) == 0 and call(n_hold=999, capacity=2) == 0
    assert call(n=2 ** 30, n_hold=2 ** 29, capacity=2 ** 30) == 0 and call(n_users=1) == 0 and call(with_present=0, n_users=0) == 0
    assert call(capacity=10 ** 12) == 0
    for kw in (dict(n=1, n_hold=1), dict(n=1, n_hold=0, capacity=2), dict(n=0), dict(n=2 ** 30 + 1, n_hold=2 ** 29, capacity=2 ** 31), dict(n_hold=0, capacity=2000),
               dict(n_hold=1000), dict(n_hold=-1), dict(n_hold=1001), dict(capacity=1599), dict(capacity=0), dict(n_users=0), dict(n_users=-4)):
        assert call(**kw) == SHAPE, kw


def test_symbols_header_and_ctypes_table():
    lib = _lib.load()
    assert hasattr(lib, "sdrm_neumf_epoch_draw") and hasattr(lib, "sdrm_debug_neumf_draw_args")
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    debug = open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    for text, name, n_args in ((header, "sdrm_neumf_epoch_draw", 12), (debug, "sdrm_debug_neumf_draw_args", 5)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert "stream" not in decl.group(1)                     # device-synchronous: no stream, under any name
    assert "PURPOSE_NEUMF_EPOCH = 12" in open(os.path.join(REPO, "sdrm_amd", "csrc", "philox.h")).read() and ref.PURPOSE_NEUMF_EPOCH == 12
    sig = inspect.signature(Engine.neumf_epoch_draw).parameters
    assert list(sig)[1:] == ["triples", "n_hold", "seed", "epoch", "n_users", "out"]
    assert sig["n_hold"].default is None and sig["seed"].default == 0 and sig["epoch"].default == 0 and sig["n_users"].default is None and sig["out"].default is None


def test_existing_signatures_keep_their_defaults():
    drv = inspect.signature(neumf.compute_neuralcf_results).parameters
    assert list(drv) == ["training", "validation", "n_users", "n_items", "engine", "seed", "epochs", "eval_recall", "device", "history", "device_train",
                         "device_draw"]
    assert drv["device_draw"].default is False and drv["device_train"].default is False and drv["engine"].default is None and drv["seed"].default == 0
    assert drv["epochs"].default == 20 and drv["eval_recall"].default is True and drv["device"].default is None and drv["history"].default is None
    rank = inspect.signature(neumf.rank_all_items).parameters
    assert list(rank) == ["model", "training", "heldout", "users", "engine", "problem"] and rank["engine"].default is None and rank["problem"].default is None
    loss = inspect.signature(neumf.validation_loss).parameters
    assert list(loss) == ["model", "triples", "engine"] and loss["engine"].default is None


def test_device_draw_without_device_train_or_engine_is_refused():
    training, validation = toy()
    for kw in (dict(device_draw=True), dict(device_draw=True, device_train=True), dict(device_draw=True, engine=object())):
        with pytest.raises(ValueError, match="device_draw=True needs device_train=True and an engine"):
            neumf.compute_neuralcf_results(training, validation, 40, 90, seed=3, epochs=1, **kw)
