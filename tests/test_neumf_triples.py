"""The NeuMF evaluator's triples assembled on the device (csrc/neumf_triples.h; sdrm_neumf_triples; `Engine.neumf_triples`;
`neumf.compute_neuralcf_results_synthetic`; `pipeline.evaluate_synthetic` with hp["evaluator"] == "neumf") against the numpy restatement
tests/neumf_triples_ref.py: integer work, so every comparison is exact.  Every buffer the call writes stands between guard bands and
starts as a sentinel.  Row lengths sit on the edges of the fill's chunks (a wave's 64, the work-group's 256 lanes, 1024 triples), the
row counts on both sides of a work-group's 16 rows.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import neumf_triples_ref as tr
import stream_harness as sh
from sdrm_amd import _lib, neumf, pipeline
from sdrm_amd.engine import Engine, SdrmError

SENTINEL, GUARD = -77, 64
OTHER_TEXTS = ("a row id outside", "negative or not ordered", "sdrm_holdout_split", "sdrm_csr_transpose:", "sdrm_csr_vstack: a column")


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def make_part(rng, lengths, n_items, user0, label, front=0):
    """(indptr, indices, n_rows, user0, label) with the given row lengths: distinct columns per row in a random (unsorted) stored order;
    `front`: unused elements in front of the first row, so that indptr does not start at 0."""
    lengths = np.asarray(lengths, dtype=np.int64)
    indptr = front + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cols = [rng.permutation(n_items)[:n] for n in lengths]
    indices = np.concatenate([np.full(front, n_items + 5, dtype=np.int64)] + cols).astype(np.int32) if len(cols) else np.zeros(0, dtype=np.int32)
    return indptr, indices, int(lengths.shape[0]), int(user0), int(label)


def cases():
    rng = np.random.default_rng(20261021)
    out = {}
    out["one"] = ([make_part(rng, [1], 5, 0, 1)], 5)
    three = [make_part(rng, [7], 97, 0, 0), make_part(rng, rng.integers(0, 41, 70), 97, 0, 1), make_part(rng, rng.integers(0, 41, 300), 97, 1000, 1)]
    out["three"] = (three, 97)
    out["edges"] = ([make_part(rng, [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 0], 4099, 3, 1)], 4099)
    out["long-and-short"] = ([make_part(rng, [3000] + [1] * 40 + [3000, 1], 4099, 0, 0)], 4099)
    out["empty-part"] = ([make_part(rng, [3, 0, 5], 20, 0, 0), make_part(rng, [0, 0, 0], 20, 0, 1), make_part(rng, [2, 2], 20, 9, 1)], 20)
    whole = make_part(rng, rng.integers(0, 30, 40), 97, 0, 1, front=11)
    out["row-range"] = ([(whole[0][5:26], whole[1], 20, 5, 1)], 97)
    out["user0"] = ([make_part(rng, rng.integers(0, 9, 17), 33, 0, 0), make_part(rng, rng.integers(0, 9, 17), 33, 1000, 1),
                     make_part(rng, rng.integers(1, 9, 17), 33, 2 ** 31 - 1 - 17, 1)], 33)
    out["eight"] = ([make_part(rng, rng.integers(0, 20, 5 + 3 * k), 64, 100 * k, k % 2) for k in range(8)], 64)
    out["one-item"] = ([make_part(rng, rng.integers(0, 2, 50), 1, 0, 1), make_part(rng, rng.integers(0, 2, 50), 1, 50, 0)], 1)
    return out


CASES = cases()


def run_raw(engine, parts, n_items, capacity_out=None, with_present=True):
    """The C call itself with every written buffer between guard bands of GUARD elements: (out rows [capacity_out, 3] with the guards cut
    off, counts int64 [4], item_present | None), after the guards have been found untouched."""
    dev = engine.device
    cap = sum(p[1].shape[0] for p in parts) if capacity_out is None else capacity_out
    big = torch.full((GUARD + max(cap, 1) + GUARD, 3), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((GUARD + 4 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    present = torch.full((GUARD + n_items + GUARD,), 0x5A, dtype=torch.uint8, device=dev) if with_present else None
    desc = (_lib.TriplePart * len(parts))()
    keep = []
    for d, (indptr, indices, n_rows, user0, label) in zip(desc, parts):
        ip, ix = torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev)
        keep += [ip, ix]
        d.indptr, d.indices = ip.data_ptr(), ix.data_ptr() if ix.numel() else None
        d.n_rows, d.capacity, d.user0, d.label = n_rows, ix.numel(), user0, label
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = engine.lib.sdrm_neumf_triples(engine._h, desc, len(parts), n_items, C.c_void_p(big[GUARD:].data_ptr()), max(cap, 1),
                                       None if present is None else C.c_void_p(present[GUARD:].data_ptr()), C.c_void_p(counts[GUARD:].data_ptr()), stream)
    assert rc == 0, engine.lib.sdrm_last_error(engine._h)
    big, counts = big.cpu().numpy(), counts.cpu().numpy()
    assert (big[:GUARD] == SENTINEL).all() and (big[-GUARD:] == SENTINEL).all(), "a store outside triples_out"
    assert (counts[:GUARD] == SENTINEL).all() and (counts[-GUARD:] == SENTINEL).all(), "a store outside counts_dev"
    if present is not None:
        present = present.cpu().numpy()
        assert (present[:GUARD] == 0x5A).all() and (present[-GUARD:] == 0x5A).all(), "a store outside item_present"
        present = present[GUARD:-GUARD]
    return big[GUARD:-GUARD], counts[GUARD:-GUARD], present


def status_of(engine):
    """The status bits `feed_status()` names (it clears them), from its message."""
    try:
        engine.feed_status()
    except SdrmError as exc:
        text = str(exc)
        assert not [t for t in OTHER_TEXTS if t in text], text
        return (tr.STACK_PTR if tr.PTR_TEXT in text else 0) | (tr.BAD_COL if tr.COL_TEXT in text else 0)
    return 0


def check(engine, parts, n_items, capacity_out=None, with_present=True, expect_status=0):
    cap = max(sum(p[1].shape[0] for p in parts) if capacity_out is None else capacity_out, 1)
    before = np.full((cap, 3), SENTINEL, dtype=np.int32)
    want, w_counts, w_present, w_status = tr.triples_ref(parts, n_items, cap, before=before, with_present=with_present)
    got, counts, present = run_raw(engine, parts, n_items, cap, with_present)
    status = status_of(engine)
    print("counts", counts.tolist(), "restated", w_counts, "status", status, "restated", w_status)
    assert tuple(counts.tolist()) == w_counts
    np.testing.assert_array_equal(got, want)            # (rows m .. capacity_out - 1 are the sentinel in both)
    if with_present:
        np.testing.assert_array_equal(present, w_present)
    assert status == w_status == expect_status
    return got, counts, present


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_restatement(engine, name):
    parts, n_items = CASES[name]
    _, counts, _ = check(engine, parts, n_items)
    assert counts[0] == sum(int(p[0][p[2]] - p[0][0]) for p in parts)        # (clean inputs: every entry is a triple)


@pytest.mark.gpu
def test_without_item_present(engine):
    parts, n_items = CASES["three"]
    check(engine, parts, n_items, with_present=False)


@pytest.mark.gpu
def test_slack_behind_m_is_left_alone(engine):
    parts, n_items = CASES["eight"]
    check(engine, parts, n_items, capacity_out=sum(p[1].shape[0] for p in parts) + 301)


def _defect(kind):
    """CASES['three'] with one defect in its 70-row part (rows of at most 40 entries, 97 items); (parts, n_items, the bits it must raise)."""
    parts, n_items = CASES["three"]
    indptr, indices, n_rows, user0, label = parts[1]
    indptr, indices = indptr.copy(), indices.copy()
    r = int(np.flatnonzero(np.diff(indptr) >= 3)[4])
    bits = tr.STACK_PTR
    if kind == "out-of-order":
        indptr[r + 1] = indptr[r] - 2            # row r ends in front of its start; row r + 1 is longer and still inside the array
    elif kind == "negative":
        indptr[0] = -3
    elif kind == "behind-capacity":
        indptr[n_rows] = indices.shape[0] + 5
    elif kind == "too-long":
        indptr[r + 1:n_rows] = indptr[r + 1]     # rows r + 1 .. n_rows - 2 empty, the last one takes all their entries: more than 97
        assert indptr[n_rows] - indptr[n_rows - 1] > n_items
    elif kind == "col-high":
        indices[indptr[r] + 1], bits = n_items, tr.BAD_COL
    elif kind == "col-negative":
        indices[indptr[r + 1] - 1], bits = -1, tr.BAD_COL
    return [parts[0], (indptr, indices, n_rows, user0, label), parts[2]], n_items, bits


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["out-of-order", "negative", "behind-capacity", "too-long", "col-high", "col-negative"])
def test_bad_rows_are_empty_and_reported(engine, kind):
    parts, n_items, bits = _defect(kind)
    clean = sum(int(p[0][p[2]] - p[0][0]) for p in CASES["three"][0])
    cap = sum(p[1].shape[0] for p in parts) + 100                           # (the out-of-order pair makes the next row longer)
    _, counts, _ = check(engine, parts, n_items, capacity_out=cap, expect_status=bits)
    assert counts[0] != clean


@pytest.mark.gpu
def test_rows_that_share_entries_stop_at_capacity_out(engine):
    """The checked lengths can add up to more than the array holds only behind an out-of-order pair: rows [0, 90), [90, 30) and [30, 90) of
    90 entries.  With room all 150 triples appear; with the least capacity_out the call accepts the output is filled to the brim, the rest
    is dropped, m says so - and nothing lands behind it."""
    rng = np.random.default_rng(3)
    _, indices, _, _, _ = make_part(rng, [30, 30, 30], 97, 0, 1)
    part = (np.array([0, 90, 30, 90], dtype=np.int64), indices, 3, 4, 1)
    _, counts, _ = check(engine, [part], 97, capacity_out=200, expect_status=tr.STACK_PTR)
    assert counts[0] == 150
    _, counts, _ = check(engine, [part], 97, capacity_out=90, expect_status=tr.STACK_PTR)
    assert counts[0] == 90


@pytest.mark.gpu
def test_same_bytes_behind_a_larger_call(engine):
    parts, n_items = CASES["edges"]
    first = run_raw(engine, parts, n_items)
    run_raw(engine, *CASES["long-and-short"])
    run_raw(engine, *CASES["three"])
    again = run_raw(engine, parts, n_items)
    assert status_of(engine) == 0
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_engine_method(engine):
    """The wrapper: the view is sized by the one readback, `out` is filled in place, rows behind m keep what they held, check=True raises."""
    rng = np.random.default_rng(8)
    a = csr_matrix((rng.random((37, 77)) < 0.2).astype(np.float32))
    b = csr_matrix((rng.random((12, 77)) < 0.3).astype(np.float32))
    a_dev, b_dev = engine.csr_to_device(a), engine.csr_to_device(b)
    parts = [((a_dev[0], a_dev[1], a.shape), 0, 0), (b_dev, 37, 1)]
    want, dims = neumf.assemble_triples([(a, 0, 0), (b, 37, 1)])
    triples, counts, present = engine.neumf_triples(parts, 77)
    assert triples.dtype == torch.int32 and tuple(triples.shape) == want.shape and triples.is_contiguous()
    np.testing.assert_array_equal(triples.cpu().numpy(), want.astype(np.int32))
    assert counts == (want.shape[0], b.nnz) + dims
    np.testing.assert_array_equal(np.flatnonzero(present.cpu().numpy()), np.unique(want[:, 1]))
    out = torch.full((want.shape[0] + 9, 3), SENTINEL, dtype=torch.int32, device=engine.device)
    view, counts2, none = engine.neumf_triples(parts, 77, out=out, present=False)
    assert none is None and counts2 == counts and view.data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy()[:want.shape[0]], want.astype(np.int32))
    assert (out.cpu().numpy()[want.shape[0]:] == SENTINEL).all()
    bad = a_dev[1].clone()
    bad[3] = 77
    with pytest.raises(SdrmError, match="column index outside"):
        engine.neumf_triples([((a_dev[0], bad, a.shape), 0, 0)], 77)
    triples, counts, _ = engine.neumf_triples([((a_dev[0], bad, a.shape), 0, 0)], 77, check=False)
    assert status_of(engine) == tr.BAD_COL and counts[0] < a.nnz


def stream_case(b=33):
    """The stream-order case of sdrm_neumf_triples, built like the entries of tests/stream_harness.py's table from its own helpers: the
    harness's feed matrix with label 0, and a row range of it (an indptr that does not start at 0) as other users with label 1."""
    m = sh._feed(b)

    def parts(x):
        return [(sh._csr(x, m.shape), 0, 0), ((x["csr_indptr"][5:], x["csr_indices"], None, (b - 5, sh.ITEMS)), 1000, 1)]

    def make(device):
        return sh._csr_inputs(m, device)

    def call(e, x, alloc):
        return e.neumf_triples(parts(x), sh.ITEMS, check=False)

    def anchor(inp, res):   # the numpy restatement, byte for byte; the counts are host values the harness compares with the twin's
        ip, ix = inp["csr_indptr"].numpy(), inp["csr_indices"].numpy()
        want, counts, present, status = tr.triples_ref([(ip, ix, b, 0, 0), (ip[5:], ix, b - 5, 1000, 1)], sh.ITEMS, 2 * ix.shape[0])
        assert status == 0 and np.array_equal(res[0].numpy(), want[:counts[0]]) and np.array_equal(res[1].numpy(), present)

    return sh._util("neumf-triples", ("sdrm_neumf_triples",), make, call, anchor=anchor)


@pytest.mark.gpu
@pytest.mark.parametrize("pool, variant", [("warm", "late"), ("warm", "busy"), ("cold", "late"), ("cold", "busy")])
def test_on_a_busy_side_stream(engine_cls, pool, variant):
    """sdrm_neumf_triples with inputs that arrive late on a non-blocking side stream, the default stream busy as well in "busy", warm and as
    the engine's first call of the family: it returns with its inputs pending (asserted in the warm pool, as the harness does for every
    entry point), and the side stream alone sees the default-stream twin's bytes, which are the restatement's (tests/stream_harness.py's
    run_case, as tests/test_stream_order.py runs its table)."""
    case = stream_case()
    assert case.nosync == ("sdrm_neumf_triples",) and case.feed
    sh.run_case(case, engine_cls, pool, variant)


# ================================================================================================ end to end
def tiny_problem():
    rng = np.random.default_rng(20261)
    raw = rng.standard_normal((40, 64)).astype(np.float32)
    valid = (rng.random((12, 64)) < 0.3).astype(np.float64)
    valid[:, :2] = 1.0                                    # every validation user keeps two entries or more
    return raw, csr_matrix(valid), 0.8


@pytest.mark.gpu
def test_route_equals_the_host_assembled_run(engine):
    """`evaluate_synthetic(evaluator="neumf")` against `compute_neuralcf_results(device_train=True, device_draw=True)` on the triples that
    `assemble_triples(synthetic_parts_host(...))` builds on the host: the same bytes reach the same draws and the same train steps (no float
    atomics), so the metrics and the histories are EQUAL."""
    raw, valid, sparsity = tiny_problem()
    train = csr_matrix((40, 64), dtype=np.float64)
    raw_dev = torch.from_numpy(raw).to(engine.device)
    ones = pipeline.equal_sparsity_csr(raw_dev, sparsity, engine)
    zeros = pipeline.equal_sparsity_csr(raw_dev, 1 - sparsity, engine, side="<=")
    parts, validation = neumf.synthetic_parts_host(train.shape, valid, ones, zeros)
    triples, (n_users, n_items) = neumf.assemble_triples(parts)
    assert np.unique(triples[:, 1]).shape[0] == 64 and ones.multiply(zeros).nnz == 0 and ones.nnz > 0 and zeros.nnz > 0
    h_host, h_dev = {}, {}
    want = neumf.compute_neuralcf_results(triples, validation, n_users, n_items, engine=engine, seed=3, epochs=2, history=h_host, device_train=True,
                                          device_draw=True)
    got = pipeline.evaluate_synthetic(train, valid, raw_dev, sparsity, engine, dict(evaluator="neumf", neumf_epochs=2), 3)
    again = neumf.compute_neuralcf_results_synthetic(train.shape, valid, raw_dev, sparsity, engine, seed=3, epochs=2, history=h_dev)
    print("host", want, "route", got)
    for a, b, c in zip(want, got, again):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    assert h_dev["valid_loss"] == h_host["valid_loss"] and len(h_host["valid_loss"]) == 2
    assert h_dev["draw_counts"] == h_host["draw_counts"] and h_dev["train_loss"] == h_host["train_loss"] and len(h_host["train_loss"]) > 2
    assert h_dev["recall10"] == h_host["recall10"] or all(np.isnan(x) == np.isnan(y) and (x == y or np.isnan(x)) for x, y in zip(h_dev["recall10"], h_host["recall10"]))
