"""The host side of the NeuMF evaluator's device ranking problem (csrc/neumf_rank.h): the numpy restatement tests/neumf_rank_ref.py against
the project's own host code (`RankingProblem.from_parts`, `RankingProblem(assemble_triples(parts)[0], heldout)`, `.select`), the header text
and the ctypes table of the three entry points and the debug function, every refusal of sdrm_neumf_rank_problem's envelope through the
library's host side, the driver's and the pipeline's new arguments, and the signatures other tests pin.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import neumf_rank_ref as rr
from sdrm_amd import _lib, neumf, pipeline
from sdrm_amd.engine import Engine, SdrmError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, SHAPE = -1, -2                        # SDRM_ERR_ARG, SDRM_ERR_SHAPE (include/sdrm_hip.h)


# ================================================================================================ the restatement
def random_parts(seed, n_items=23, absent=(7, 19)):
    """Four scipy parts: two over the same users with a pair in common, one that overlaps them partly, one further up; no part holds an
    item of `absent`."""
    rng = np.random.default_rng(seed)
    shapes = [(9, 0.3, 0), (9, 0.3, 0), (6, 0.4, 5), (4, 0.5, 14)]
    mats = []
    for rows, p, _ in shapes:
        m = (rng.random((rows, n_items)) < p).astype(np.float32)
        m[:, list(absent)] = 0
        mats.append(m)
    mats[0][2, 3] = mats[1][2, 3] = 1.0
    return [(csr_matrix(m), user0, k % 2) for k, (m, (_, _, user0)) in enumerate(zip(mats, shapes))]


def ref_parts(parts):
    return [(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.shape[0], u, l) for m, u, l in parts]


def heldout_of(seed, n_users, n_items, n=40):
    rng = np.random.default_rng(seed)
    t = np.stack([rng.integers(0, n_users, n), rng.integers(0, n_items, n), rng.integers(0, 2, n)], axis=1).astype(np.int64)
    return np.concatenate([t, t[:5], [[3, 7, 1], [n_users - 1, 19, 1]]])        # duplicates, and two absent items


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_is_the_host_ranking_problem(seed):
    parts = random_parts(seed)
    n_items, n_rows = 23, 20                                      # users 18 and 19: beyond every part, below n_rows
    triples, _ = neumf.assemble_triples(parts)
    present = np.zeros(n_items, dtype=np.uint8)
    present[triples[:, 1]] = 1
    heldout = heldout_of(seed, n_rows, n_items)
    cols, seen, relevant, counts, status = rr.rank_problem_ref(ref_parts(parts), n_items, present, heldout, n_rows)
    assert status == 0 and counts[3] == 0 and counts[0] == cols.shape[0] < n_items and 7 not in cols
    from_parts = neumf.RankingProblem.from_parts(parts, np.flatnonzero(present), heldout)
    from_triples = neumf.RankingProblem(triples, heldout)
    for want in (from_parts, from_triples):
        np.testing.assert_array_equal(cols, want.cols)
        for got, ref in ((rr.host_form(seen), want._seen), (rr.host_form(relevant), want._relevant)):
            for x, y in zip(got, ref):
                assert x.dtype == y.dtype
                np.testing.assert_array_equal(x, y)
    for users in ([0, 2, 5, 17], [19], [3, 18, 40, 77], list(range(n_rows))):
        _, w_cols, w_rel, w_seen = from_parts.select(users)
        users = np.unique(users)
        for got, want in ((rr.select(relevant, users, cols.shape[0]), w_rel), (rr.select(seen, users, cols.shape[0]), w_seen)):
            assert got.shape == want.shape
            np.testing.assert_array_equal(got.indptr, want.indptr)
            np.testing.assert_array_equal(got.indices, want.indices)


def test_restatement_defects():
    parts = ref_parts(random_parts(4))
    present = np.ones(23, dtype=np.uint8)
    held = np.array([[0, 1, 1], [-1, 1, 1], [20, 1, 0], [0, 23, 1], [0, -1, 0], [25, 30, 1]], dtype=np.int64)
    _, _, relevant, counts, status = rr.rank_problem_ref(parts, 23, present, held, 20)
    assert counts[3] == 5 and counts[2] == 1 and status == rr.BAD_ROW | rr.BAD_COL
    np.testing.assert_array_equal(relevant[1], [1])
    _, seen, _, counts, status = rr.rank_problem_ref(parts, 23, present, held[:1], 16)     # the last part's users 16, 17 have no row
    assert status == rr.BAD_ROW and seen[0].shape[0] == 17
    assert rr.rank_users_ref([0, 3, 0, 1]).tolist() == [1, 3] and rr.rank_users_ref([0, 3, 0, 1]).dtype == np.int32


def test_footing_restatement_is_the_host_formula():
    idcg = neumf._idcg_table()[1]
    ndcg = np.array([[0.5, np.nan, 1.0]] * 6)
    out = rr.neumf_footing(ndcg, np.array([2, 0, 70]), idcg, 300, neumf.K_LIST)
    assert out[0, 1] == 0.0 and out[5, 2] == 1.0 * idcg[50] / idcg[50] and out[3, 0] == 0.5 * idcg[2] / idcg[10]


# ================================================================================================ header, bindings, envelope
def _header(name="sdrm_hip.h"):
    with open(os.path.join(REPO, "include", name)) as f:
        return f.read()


def test_header_and_bindings():
    text = _header()
    for name, n_args in (("sdrm_neumf_rank_problem", 18), ("sdrm_neumf_rank_users", 6), ("sdrm_rank_metrics_rows", 20)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is C.c_int
    debug = re.search(r"int sdrm_debug_neumf_rank_args\(([^;]*)\);", _header("sdrm_hip_debug.h"))
    assert len(debug.group(1).split(",")) == 8 == len(_lib.SIGNATURES["sdrm_debug_neumf_rank_args"][1])
    args = re.sub(r"\s+", " ", re.search(r"int sdrm_neumf_rank_problem\(([^;]*)\);", text).group(1))
    assert args == ("sdrm_engine* e, const sdrm_triple_part* parts, int n_parts, int n_items, const uint8_t* item_present, const int32_t* heldout, "
                    "int64_t n_heldout, int64_t n_rows, int32_t* cols_out, int64_t capacity_cols, int64_t* seen_indptr, int32_t* seen_indices, "
                    "int64_t capacity_seen, int64_t* relevant_indptr, int32_t* relevant_indices, int64_t capacity_relevant, int64_t* counts_dev, "
                    "void* hip_stream")
    assert _lib.SIGNATURES["sdrm_neumf_rank_problem"][1][1]._type_ is _lib.TriplePart
    # the definition and the rules stand in the header comments
    for phrase in ("DENSE BY USER ID", "dropped silently", "neural_cf_benchmark_pt.py:294-326", "the same bytes on every run", "tests/neumf_rank_ref.py"):
        assert phrase in text, phrase
    for phrase in ("not the shortcut dcg / idcg[min(I, k)]", "rows[q] outside"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", text), phrase
    lib = _lib.load()
    assert lib.sdrm_neumf_rank_problem(None, None, 1, 4, None, None, 0, 1, None, 4, None, None, 0, None, None, 0, None, None) == ARG
    assert lib.sdrm_neumf_rank_users(None, None, 1, None, None, None) == ARG
    assert lib.sdrm_rank_metrics_rows(None, None, 1, 1, None, 1, None, None, 0, None, None, 0, None, 1, None, None, None, None, 0, None) == ARG


def _part(n_rows=4, capacity=4, user0=0, label=1, indptr=1, indices=1):
    return dict(n_rows=n_rows, capacity=capacity, user0=user0, label=label, indptr=indptr, indices=indices)


def _args(parts, n_items=16, n_heldout=3, n_rows=8, cols=None, seen=None, relevant=None, n_parts=None):
    """sdrm_debug_neumf_rank_args of part descriptions (pointers are only compared with null: 1 stands for an address)."""
    desc = (_lib.TriplePart * max(len(parts), 1))()
    for d, p in zip(desc, parts):
        d.indptr, d.indices, d.n_rows, d.capacity, d.user0, d.label = p["indptr"] or None, p["indices"] or None, p["n_rows"], p["capacity"], p["user0"], p["label"]
    cap = sum(p["capacity"] for p in parts)
    return _lib.load().sdrm_debug_neumf_rank_args(desc, len(parts) if n_parts is None else n_parts, n_items, n_heldout, n_rows,
                                                  n_items if cols is None else cols, cap if seen is None else seen,
                                                  n_heldout if relevant is None else relevant)


def test_envelope_refusals_need_no_device():
    """Every SDRM_ERR_SHAPE / SDRM_ERR_ARG case the header lists, both sides of each bound."""
    assert _args([_part()]) == 0 and _args([_part()] * 8) == 0
    assert _args([_part()] * 8, n_parts=9) == SHAPE and _args([_part()], n_parts=0) == SHAPE
    assert _lib.load().sdrm_debug_neumf_rank_args(None, 1, 16, 0, 4, 16, 4, 0) == ARG
    assert _args([_part()], n_items=1) == 0 and _args([_part()], n_items=0) == SHAPE
    assert _args([_part()], n_items=2 ** 22, n_rows=1) == 0 and _args([_part()], n_items=2 ** 22 + 1, n_rows=1) == SHAPE
    assert _args([_part()], n_rows=1) == 0 and _args([_part()], n_rows=0) == SHAPE
    assert _args([_part()], n_items=64, n_rows=2 ** 22) == 0 and _args([_part()], n_items=64, n_rows=2 ** 22 + 1) == SHAPE
    # one bit table: n_rows x ceil(n_items / 64) x 8 bytes, at most 2^31
    assert _args([_part()], n_items=64 * 64, n_rows=2 ** 22) == 0 and _args([_part()], n_items=64 * 64 + 1, n_rows=2 ** 22) == SHAPE
    assert _args([_part()], n_items=2 ** 22, n_rows=2 ** 12) == 0 and _args([_part()], n_items=2 ** 22, n_rows=2 ** 12 + 1) == SHAPE
    assert _args([_part()], n_heldout=0) == 0 and _args([_part()], n_heldout=-1) == SHAPE
    assert _args([_part()], n_heldout=2 ** 30) == 0 and _args([_part()], n_heldout=2 ** 30 + 1) == SHAPE
    assert _args([_part(n_rows=2 ** 22)]) == 0 and _args([_part(n_rows=2 ** 22), _part(n_rows=1)]) == SHAPE
    assert _args([_part(n_rows=0)]) == SHAPE and _args([_part(n_rows=0), _part(n_rows=1)]) == 0 and _args([_part(n_rows=-1), _part()]) == SHAPE
    assert _args([_part(label=0)]) == 0 and _args([_part(label=2)]) == SHAPE and _args([_part(label=-1)]) == SHAPE
    assert _args([_part(user0=-1)]) == SHAPE
    assert _args([_part(n_rows=5, user0=2 ** 31 - 1 - 5)]) == 0 and _args([_part(n_rows=5, user0=2 ** 31 - 5)]) == SHAPE
    assert _args([_part(capacity=-1)], seen=4) == SHAPE
    assert _args([_part(capacity=2 ** 30)]) == 0 and _args([_part(capacity=2 ** 30 + 1)]) == SHAPE
    assert _args([_part()], cols=16) == 0 and _args([_part()], cols=15) == SHAPE
    assert _args([_part(capacity=3), _part(capacity=4)], seen=7) == 0 and _args([_part(capacity=3), _part(capacity=4)], seen=6) == SHAPE
    assert _args([_part()], relevant=3) == 0 and _args([_part()], relevant=2) == SHAPE
    assert _args([_part(indptr=0)]) == ARG and _args([_part(indices=0)]) == ARG
    assert _args([_part(indices=0, capacity=0)]) == 0


def test_engine_methods_refuse_on_the_host():
    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    eng = Engine.__new__(Engine)
    eng.device, eng.lib, eng._h = torch.device("cpu"), NoLaunch(), None
    indptr, indices = torch.tensor([0, 1, 3], dtype=torch.int64), torch.tensor([1, 0, 2], dtype=torch.int32)
    good = ((indptr, indices, (2, 4)), 0, 1)
    present, held = torch.ones(4, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.int32)
    for parts in ([], [good] * 9, [((indptr, indices, (2, 4)), 0, 2)], [((indptr, indices, (2, 4)), -1, 1)], [(indptr, indices, (2, 4))],
                  [((indptr, indices, (2, 5)), 0, 1)]):
        with pytest.raises(SdrmError):
            eng.neumf_rank_problem(parts, 4, present, held, 2)
    for kw in (dict(item_present=present[:3]), dict(item_present=present.to(torch.int32)), dict(heldout=held.to(torch.int64)), dict(heldout=held[:, :2]),
               dict(n_rows=0), dict(n_rows=2 ** 22 + 1)):
        call = dict(dict(item_present=present, heldout=held, n_rows=2), **kw)
        with pytest.raises(SdrmError):
            eng.neumf_rank_problem([good], 4, **call)
    for mask in (torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8), np.zeros(3, dtype=np.uint8)):
        with pytest.raises(SdrmError):
            eng.neumf_rank_users(mask)
    scores, rows = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32)
    csr = (indptr, indices, None, (2, 4))
    for args in ((scores, rows.to(torch.int64), csr), (scores, rows[:1], csr), (scores.double(), rows, csr), (scores, rows, (indptr, indices, None, (2, 5))),
                 (scores, rows, csr, (torch.tensor([0, 1, 3, 3], dtype=torch.int64), indices, None, (3, 4))), (torch.zeros(4), rows, csr)):
        with pytest.raises(SdrmError):
            eng.rank_metrics_rows(*args)


# ================================================================================================ the driver and the route
def test_pinned_signatures_still_hold():
    assert list(inspect.signature(neumf.rank_all_items).parameters) == ["model", "training", "heldout", "users", "engine", "problem"]
    old, new = inspect.signature(neumf.compute_neuralcf_results).parameters, inspect.signature(neumf.compute_neuralcf_results_resident).parameters
    assert list(old) == ["training", "validation", "n_users", "n_items", "engine", "seed", "epochs", "eval_recall", "device", "history", "device_train",
                         "device_draw"]
    assert list(new) == list(old) + ["training_dev", "problem"]
    syn = inspect.signature(neumf.compute_neuralcf_results_synthetic).parameters
    assert list(syn) == ["train_shape", "valid", "raw", "sparsity", "engine", "seed", "epochs", "eval_recall", "history", "device_ranking"]
    assert syn["device_ranking"].default is False
    assert list(inspect.signature(neumf.DeviceRankingProblem.build).parameters) == ["engine", "device_parts", "n_items", "item_present", "validation", "n_rows"]
    assert list(inspect.signature(Engine.neumf_rank_problem).parameters) == ["self", "parts", "n_items", "item_present", "heldout", "n_rows", "check"]
    assert list(inspect.signature(Engine.rank_metrics_rows).parameters) == ["self", "scores", "rows", "heldout", "train", "ks", "full_idcg"]
    assert list(inspect.signature(Engine.neumf_rank_users).parameters) == ["self", "mask"]


def test_evaluate_synthetic_forwards_the_key_only_when_present(monkeypatch):
    calls = []

    def driver(*args, **kw):
        calls.append((args, kw))
        return "neumf result"
    monkeypatch.setattr(pipeline, "compute_neuralcf_results_synthetic", driver)

    class Train:
        shape = (20, 16)

    eng = object()
    pipeline.evaluate_synthetic(Train(), "VALID", "RAW", 0.9, eng, dict(evaluator="neumf"), 5)
    assert calls.pop() == (((20, 16), "VALID", "RAW", 0.9, eng), dict(seed=5, epochs=20, eval_recall=True))
    pipeline.evaluate_synthetic(Train(), "VALID", "RAW", 0.9, eng, dict(evaluator="neumf", neumf_device_ranking=True, neumf_epochs=2), 5)
    assert calls.pop() == (((20, 16), "VALID", "RAW", 0.9, eng), dict(seed=5, epochs=2, eval_recall=True, device_ranking=True))
    pipeline.evaluate_synthetic(Train(), "VALID", "RAW", 0.9, eng, dict(evaluator="neumf", neumf_device_ranking=0), 5)
    assert calls.pop() == (((20, 16), "VALID", "RAW", 0.9, eng), dict(seed=5, epochs=20, eval_recall=True, device_ranking=False))


def test_rank_all_items_with_a_host_problem_is_unchanged():
    """`problem=<RankingProblem>` and `problem=None` still give the same arrays on the host path (no engine), and a device problem needs
    its engine."""
    rng = np.random.default_rng(11)
    dense = rng.random((30, 70)) < 0.3
    dense[:, :60] |= np.eye(30, 60, dtype=bool)
    u, i = np.nonzero(dense)
    training = np.stack([u, i, rng.integers(0, 2, u.shape[0])], axis=1).astype(np.int64)
    heldout = np.stack([rng.integers(0, 30, 50), rng.integers(0, 70, 50), rng.integers(0, 2, 50)], axis=1).astype(np.int64)
    torch.manual_seed(0)
    model = neumf.NCF(30, 70).eval()
    users = [3, 7, 7, 21, 29]
    plain = neumf.rank_all_items(model, training, heldout, users)
    selected = neumf.rank_all_items(model, training, heldout, users, problem=neumf.RankingProblem(training, heldout))
    for a, b in zip(plain, selected):
        assert a.shape == (6, 4) and np.array_equal(a, b, equal_nan=True)
    device_problem = neumf.DeviceRankingProblem.__new__(neumf.DeviceRankingProblem)
    device_problem.engine = object()
    with pytest.raises(ValueError, match="DeviceRankingProblem"):
        neumf.rank_all_items(model, training, heldout, users, problem=device_problem)
