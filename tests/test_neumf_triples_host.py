"""The NeuMF arm's triple assembly (main.py:218-283), host side: the header entry and its binding, the triple set of
`neumf.synthetic_parts_host` + `assemble_triples` against a pandas restatement of the reference's frames, `RankingProblem.from_parts`,
the driver's and the pipeline's new arguments, and the envelope of sdrm_neumf_triples through the library.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.sparse import csr_matrix

import neumf_triples_ref as tr
from sdrm_amd import _lib, metrics, neumf, pipeline
from sdrm_amd.engine import Engine, SdrmError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -2, -1


# ================================================================================================ header and binding
def test_header_carries_the_entry_and_the_table_binds_it():
    with open(os.path.join(REPO, "include", "sdrm_hip.h")) as f:
        text = f.read()
    proto = re.search(r"int sdrm_neumf_triples\(([^;]*)\);", text)
    assert proto is not None
    args = re.sub(r"\s+", " ", proto.group(1))
    assert args == ("sdrm_engine* e, const sdrm_triple_part* parts, int n_parts, int n_items, int32_t* triples_out, int64_t capacity_out, "
                    "uint8_t* item_present, int64_t* counts_dev, void* hip_stream")
    struct = re.sub(r"\s+", " ", re.search(r"typedef struct sdrm_triple_part \{(.*?)\} sdrm_triple_part;", text, flags=re.S).group(1)).strip()
    assert struct == "const int64_t* indptr; const int32_t* indices; int64_t n_rows; int64_t capacity; int32_t user0; int32_t label;"
    comment = re.sub(r"\s*\n \*\s*", " ", text[:proto.start()].rsplit("/*", 1)[1])
    for phrase in ("the parts in the order given", "the rows ascending", "their stored order", "(parts[p].user0 + r, indices[j], parts[p].label)",
                   "leaves no hole", "rows m .. capacity_out - 1 are left as they were", "spans more than n_items entries", "EMPTY",
                   "max user + 1 and max item + 1", "the call zeroes it and sets byte i", "Integer atomics only", "SDRM_ERR_ARG", "SDRM_ERR_SHAPE",
                   "above 2^30"):
        assert phrase in comment, phrase
    res, argtypes = _lib.SIGNATURES["sdrm_neumf_triples"]
    assert res is C.c_int and len(argtypes) == 9 and argtypes[1] is not C.c_void_p and argtypes[1]._type_ is _lib.TriplePart
    assert [n for n, _ in _lib.TriplePart._fields_] == ["indptr", "indices", "n_rows", "capacity", "user0", "label"]
    assert C.sizeof(_lib.TriplePart) == 40 and _lib.TriplePart.user0.offset == 32 and _lib.TriplePart.label.offset == 36
    lib = _lib.load()
    assert lib.sdrm_neumf_triples(None, None, 1, 4, None, 4, None, None, None) == ARG


def _part(n_rows=2, capacity=2, user0=0, label=1, indptr=1, indices=1):
    return dict(indptr=indptr, indices=indices, n_rows=n_rows, capacity=capacity, user0=user0, label=label)


def _args(parts, n_items=16, capacity_out=None, n_parts=None):
    """sdrm_debug_neumf_triples_args of part descriptions (pointers are only compared with null: 1 stands for an address)."""
    desc = (_lib.TriplePart * max(len(parts), 1))()
    for d, p in zip(desc, parts):
        d.indptr, d.indices, d.n_rows, d.capacity, d.user0, d.label = p["indptr"] or None, p["indices"] or None, p["n_rows"], p["capacity"], p["user0"], p["label"]
    cap = sum(p["capacity"] for p in parts) if capacity_out is None else capacity_out
    return _lib.load().sdrm_debug_neumf_triples_args(desc, len(parts) if n_parts is None else n_parts, n_items, cap)


def test_envelope_refusals_need_no_device():
    """Every SDRM_ERR_SHAPE / SDRM_ERR_ARG case the header lists, both sides of each bound, from the library's host side."""
    assert _args([_part()]) == 0 and _args([_part()] * 8) == 0
    assert _args([_part()] * 8, n_parts=9) == SHAPE and _args([_part()], n_parts=0) == SHAPE
    assert _lib.load().sdrm_debug_neumf_triples_args(None, 1, 16, 4) == ARG
    assert _args([_part()], n_items=1) == 0 and _args([_part()], n_items=0) == SHAPE
    assert _args([_part()], n_items=2 ** 22) == 0 and _args([_part()], n_items=2 ** 22 + 1) == SHAPE
    assert _args([_part(n_rows=2 ** 22)]) == 0 and _args([_part(n_rows=2 ** 22), _part(n_rows=1)]) == SHAPE
    assert _args([_part(n_rows=0)]) == SHAPE and _args([_part(n_rows=0), _part(n_rows=1)]) == 0 and _args([_part(n_rows=-1), _part()]) == SHAPE
    assert _args([_part(label=0)]) == 0 and _args([_part(label=2)]) == SHAPE and _args([_part(label=-1)]) == SHAPE
    assert _args([_part(user0=-1)]) == SHAPE
    assert _args([_part(n_rows=5, user0=2 ** 31 - 1 - 5)]) == 0 and _args([_part(n_rows=5, user0=2 ** 31 - 5)]) == SHAPE
    assert _args([_part(capacity=3), _part(capacity=4)], capacity_out=7) == 0 and _args([_part(capacity=3), _part(capacity=4)], capacity_out=6) == SHAPE
    assert _args([_part(capacity=-1)], capacity_out=4) == SHAPE
    assert _args([_part()], capacity_out=2 ** 30) == 0 and _args([_part()], capacity_out=2 ** 30 + 1) == SHAPE
    assert _args([_part(indptr=0)]) == ARG and _args([_part(indices=0)]) == ARG
    assert _args([_part(indices=0, capacity=0)]) == 0


def test_engine_method_refuses_on_the_host():
    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    eng = Engine.__new__(Engine)
    eng.device, eng.lib, eng._h = torch.device("cpu"), NoLaunch(), None
    indptr, indices = torch.tensor([0, 1, 3], dtype=torch.int64), torch.tensor([1, 0, 2], dtype=torch.int32)
    good = ((indptr, indices, (2, 4)), 0, 1)
    for parts in ([], [good] * 9, [((indptr, indices, (2, 4)), 0, 2)], [((indptr, indices, (2, 4)), -1, 1)], [((indptr, indices, (2, 4)), 2 ** 31 - 2, 1)],
                  [((indptr.to(torch.int32), indices, (2, 4)), 0, 1)], [(indptr, indices, (2, 4))], [((indptr, indices, (2, 5)), 0, 1)]):
        with pytest.raises(SdrmError):
            eng.neumf_triples(parts, 4)
    with pytest.raises(SdrmError, match="out must be"):
        eng.neumf_triples([good], 4, out=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(SdrmError, match="out must be"):
        eng.neumf_triples([good], 4, out=torch.zeros(3, 3, dtype=torch.int64))


# ================================================================================================ the triple set
TRAIN_SHAPE, SPARSITY = (20, 16), 0.8


def fixture():
    rng = np.random.default_rng(20261021)
    raw = rng.standard_normal(TRAIN_SHAPE)
    dense = (rng.random((12, 16)) < 0.35).astype(np.float64)
    dense[4] = 0.0
    dense[4, 9] = 1.0                      # the 1-item user the split drops
    dense[0, :4] = 1.0
    return raw, csr_matrix(dense)


def tails(raw, sparsity):
    return csr_matrix((raw >= np.quantile(raw.flatten(), sparsity)).astype(int)), csr_matrix((raw <= np.quantile(raw.flatten(), 1 - sparsity)).astype(int))


def pandas_frames(train_shape, valid, raw, sparsity):
    """main.py:218-283 with `args.augment_training_data` false, in frames: (data, valid_data, n_users, n_items)."""
    def frame(m):
        coo = m.tocoo()
        return pd.DataFrame([coo.row, coo.col, coo.data]).T.sort_values(by=0)
    row_valid = frame(valid)
    row_valid[0] += train_shape[0]
    valid_train, valid_test = metrics.split_train_test_proportion_from_csr_matrix(valid.copy(), batch_size=10, random_seed=123, ignore_zeros=True)
    train_no_zeros, test_no_zeros = frame(valid_train), frame(valid_test)
    train_no_zeros[0] += train_shape[0]
    test_no_zeros[0] += train_shape[0]
    only_zeros = row_valid[row_valid[2] == 0].sample(frac=1, random_state=123)
    half = int(only_zeros.shape[0] / 2)
    row_valid_train = pd.concat([only_zeros[:half], train_no_zeros])
    valid_data = pd.concat([only_zeros[half:], test_no_zeros])
    upper, lower = tails(raw, sparsity)
    ones, zeros = frame(upper), frame(lower)
    zeros[2] = 0
    equal = pd.concat([zeros, ones])
    data = pd.concat([equal, row_valid_train])
    equal[0] = equal[0] + (train_shape[0] + valid.shape[0])          # after the concat: it does not reach `data`
    return data, valid_data, int(data[0].max()) + 1, int(data[1].max()) + 1


def sorted_rows(a):
    a = np.asarray(a).astype(np.int64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def test_triple_set_is_the_reference_frames():
    raw, valid = fixture()
    ones, zeros = tails(raw, SPARSITY)
    assert ones.nnz > 0 and zeros.nnz > 0 and ones.multiply(zeros).nnz == 0
    data, valid_data, n_users, n_items = pandas_frames(TRAIN_SHAPE, valid, raw, SPARSITY)
    parts, validation = neumf.synthetic_parts_host(TRAIN_SHAPE, valid, ones, zeros)
    assert [(u, l) for _, u, l in parts] == [(0, 0), (0, 1), (20, 1)]
    assert parts[2][0].shape[0] == 11                                # twelve users, one dropped: the split renumbers
    triples, dims = neumf.assemble_triples(parts)
    assert triples.dtype == np.int64 and triples.shape == (data.shape[0], 3)
    np.testing.assert_array_equal(sorted_rows(triples), sorted_rows(data.to_numpy()))
    assert dims == (n_users, n_items)
    assert validation.dtype == np.int64
    np.testing.assert_array_equal(sorted_rows(validation), sorted_rows(valid_data.to_numpy()))
    # row-major as it stands, and the order of the parts is the header's: the numpy restatement of the device call gives the same array
    assert np.all(np.diff(validation[:, 0]) >= 0)
    ref_parts = [(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.shape[0], u, l) for m, u, l in parts]
    out, counts, present, status = tr.triples_ref(ref_parts, 16, triples.shape[0])
    np.testing.assert_array_equal(out, triples.astype(np.int32))
    assert counts == (triples.shape[0], int((triples[:, 2] == 1).sum())) + dims and status == 0
    np.testing.assert_array_equal(np.flatnonzero(present), np.unique(triples[:, 1]))


@pytest.mark.parametrize("value", [0.0, 2.0])
def test_valid_with_another_stored_value_is_refused(value):
    raw, valid = fixture()
    ones, zeros = tails(raw, SPARSITY)
    valid = valid.copy()
    valid.data[3] = value
    with pytest.raises(ValueError, match="main.py:242"):
        neumf.synthetic_parts_host(TRAIN_SHAPE, valid, ones, zeros)


# ================================================================================================ the ranking problem
def _same_problem(a, b):
    np.testing.assert_array_equal(a.cols, b.cols)
    assert a.cols.dtype == b.cols.dtype
    for x, y in zip(a._relevant + a._seen, b._relevant + b._seen):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)


def test_from_parts_is_the_ranking_problem_of_the_triples():
    rng = np.random.default_rng(5)
    a, b, c = ((rng.random(shape) < p).astype(np.float32) for shape, p in (((9, 12), 0.3), ((9, 12), 0.3), ((4, 12), 0.4)))
    for m in (a, b, c):
        m[:, 7] = 0                         # an item no part holds
    a[2, 3] = b[2, 3] = 1.0                 # a pair two parts hold
    parts = [(csr_matrix(a), 0, 0), (csr_matrix(b), 0, 1), (csr_matrix(c), 9, 1)]
    triples, _ = neumf.assemble_triples(parts)
    assert ((triples[:, 0] == 2) & (triples[:, 1] == 3)).sum() == 2 and 7 not in triples[:, 1]
    heldout = np.array([[9, 7, 1], [9, 1, 1], [10, 2, 0], [11, 5, 1], [30, 4, 1]], dtype=np.int64)   # (item 7 is no column; user 30 occurs nowhere else)
    want = neumf.RankingProblem(triples, heldout)
    got = neumf.RankingProblem.from_parts(parts, np.unique(triples[:, 1]), heldout)
    _same_problem(got, want)
    for users in ([9, 10, 11, 12], [0, 2, 30], [77]):
        for x, y in zip(got.select(users), want.select(users)):
            if isinstance(x, np.ndarray):
                np.testing.assert_array_equal(x, y)
            else:
                assert x.shape == y.shape
                np.testing.assert_array_equal(x.indptr, y.indptr)
                np.testing.assert_array_equal(x.indices, y.indices)
    users, cols, relevant, seen = got.select([77, 500])             # ids that occur nowhere: empty rows
    assert users.tolist() == [77, 500] and relevant.shape == seen.shape == (2, cols.shape[0]) and relevant.nnz == 0 and seen.nnz == 0


# ================================================================================================ the driver and the route
def test_resident_arguments_need_the_device_draw():
    training = np.array([[0, 1, 1], [1, 0, 0], [2, 1, 1]], dtype=np.int64)
    validation = np.array([[2, 0, 1]], dtype=np.int64)
    problem = neumf.RankingProblem(training, validation)
    dev = torch.zeros(3, 3, dtype=torch.int32)
    for kw in (dict(training_dev=dev), dict(problem=problem), dict(training_dev=dev, problem=problem),
               dict(training_dev=dev, problem=problem, device_train=True)):
        with pytest.raises(ValueError, match="device_draw"):
            neumf.compute_neuralcf_results_resident(training, validation, 3, 2, **kw)
    with pytest.raises(ValueError, match="training is None"):
        neumf.compute_neuralcf_results_resident(None, validation, 3, 2)
    with pytest.raises(ValueError, match="come together"):
        neumf.compute_neuralcf_results_resident(training, validation, 3, 2, device_draw=True, training_dev=dev)
    # the two keywords live on the sibling: `compute_neuralcf_results` keeps the parameter list its own tests pin, and is the sibling without them
    import inspect
    old, new = inspect.signature(neumf.compute_neuralcf_results).parameters, inspect.signature(neumf.compute_neuralcf_results_resident).parameters
    assert list(new) == list(old) + ["training_dev", "problem"] and new["training_dev"].default is None and new["problem"].default is None
    assert all(new[k].default == old[k].default for k in old)


def test_evaluate_synthetic_reaches_the_neumf_driver(monkeypatch):
    calls = []

    def driver(*args, **kw):
        calls.append((args, kw))
        return "neumf result"
    monkeypatch.setattr(pipeline, "compute_neuralcf_results_synthetic", driver)

    class Train:
        shape = (20, 16)

    eng = object()
    assert pipeline.evaluate_synthetic(Train(), "VALID", "RAW", 0.9, eng, dict(evaluator="neumf"), 5) == "neumf result"
    assert calls.pop() == (((20, 16), "VALID", "RAW", 0.9, eng), dict(seed=5, epochs=20, eval_recall=True))
    pipeline.evaluate_synthetic(Train(), "VALID", "RAW", 0.9, eng, dict(evaluator="neumf", neumf_epochs=3, neumf_eval_recall=False, device_svd=True), 7)
    assert calls.pop() == (((20, 16), "VALID", "RAW", 0.9, eng), dict(seed=7, epochs=3, eval_recall=False))
    with pytest.raises(ValueError, match="evaluator") as err:
        pipeline.evaluate_synthetic(Train(), "VALID", "RAW", 0.9, eng, dict(evaluator="knn"), 5)
    assert "'mlp'" in str(err.value) and "'neumf'" in str(err.value) and not calls
    with pytest.raises(ValueError, match="needs an engine"):
        neumf.compute_neuralcf_results_synthetic((20, 16), None, np.zeros((2, 2)), 0.5, None)
