"""The NeuMF evaluator's ranking problem built and selected on the device (csrc/neumf_rank.h; sdrm_neumf_rank_problem, sdrm_neumf_rank_users,
sdrm_rank_metrics_rows; `Engine.neumf_rank_problem` / `neumf_rank_users` / `rank_metrics_rows`; `neumf.DeviceRankingProblem`;
`compute_neuralcf_results_synthetic(device_ranking=True)`; hp["neumf_device_ranking"]) against the numpy restatement tests/neumf_rank_ref.py and
the host path: integer work and the host's own float64 operations, so every comparison is exact.  Every array the build writes stands between
guard bands and starts as a sentinel.  Item counts sit on the word edges of the bit table (63 / 64 / 65, 128, 4099), row lengths on a wave's 64 and
the work-group's 256 lanes, user counts on the scan's chunk of 2048.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import neumf_rank_ref as rr
import neumf_ref as nr
import stream_harness as sh
import test_neumf_triples as tt
from sdrm_amd import _lib, neumf, pipeline
from sdrm_amd.engine import Engine, SdrmError

SENTINEL, GUARD = -77, 64
OTHER_TEXTS = ("negative or not ordered", "sdrm_holdout_split", "sdrm_csr_transpose:", "sdrm_csr_vstack: a column")


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


# ================================================================================================ build
def sorted_rows(part):
    """The part with every row's columns ascending, as the engine's own CSR stores them."""
    indptr, indices, n_rows, user0, label = part
    indices = indices.copy()
    for r in range(n_rows):
        indices[indptr[r]:indptr[r + 1]].sort()
    return indptr, indices, n_rows, user0, label


def present_of(parts, n_items):
    """item_present as sdrm_neumf_triples leaves it for clean parts: the items of every stored entry inside a row."""
    present = np.zeros(n_items, dtype=np.uint8)
    for indptr, indices, n_rows, _, _ in parts:
        present[indices[indptr[0]:indptr[n_rows]]] = 1
    return present


def held_of(rng, n_rows, n_items, n, present):
    """n random triples with labels 0 and 1, five of them twice, and a label-1 triple on every absent item (at most three)."""
    t = np.stack([rng.integers(0, n_rows, n), rng.integers(0, n_items, n), rng.integers(0, 2, n)], axis=1)
    absent = np.flatnonzero(present == 0)[:3]
    extra = np.stack([rng.integers(0, n_rows, absent.shape[0]), absent, np.ones_like(absent)], axis=1)
    return np.concatenate([t, t[:5], extra]).astype(np.int32)


def cases():
    """name -> (parts, n_items, n_rows, heldout int32 [n, 3])."""
    rng = np.random.default_rng(20261021)
    mk = tt.make_part
    out = {}

    def add(name, parts, n_items, n_rows, n_held=60):
        out[name] = (parts, n_items, n_rows, held_of(rng, n_rows, n_items, n_held, present_of(parts, n_items)))

    add("one", [mk(rng, [1], 1, 0, 1)], 1, 1, n_held=3)
    for n_items in (63, 64, 65, 128):
        # two parts over the same 70 users (stored order random and ascending), one that overlaps them partly; users 100 .. 103 beyond every part
        lengths = rng.integers(0, min(n_items, 40) + 1, 70)
        lengths[:3] = (n_items, n_items - 1, 1)
        add(f"items-{n_items}", [mk(rng, lengths, n_items, 0, 0), sorted_rows(mk(rng, rng.integers(0, 9, 70), n_items, 0, 1)),
                                 mk(rng, rng.integers(0, 9, 70), n_items, 30, 1)], n_items, 104)
    lengths = np.concatenate([[0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 0], rng.integers(0, 30, 289)])
    add("edges-4099", [sorted_rows(mk(rng, lengths, 4099, 3, 1)), mk(rng, [64, 65, 256, 257], 4099, 5, 0)], 4099, 303, n_held=300)
    add("shared-pair", [(np.array([0, 2, 3], dtype=np.int64), np.array([4, 9, 9], dtype=np.int32), 2, 0, 0),
                        (np.array([0, 2, 4], dtype=np.int64), np.array([9, 6, 9, 1], dtype=np.int32), 2, 0, 1)], 12, 2, n_held=10)
    add("empty-part", [mk(rng, [3, 0, 5], 20, 0, 0), mk(rng, [0, 0, 0], 20, 0, 1), mk(rng, [2, 2], 20, 9, 1)], 20, 11, n_held=20)
    add("eight", [mk(rng, rng.integers(0, 20, 5 + 3 * k), 64, 10 * k, k % 2) for k in range(8)], 64, 100)
    whole = mk(rng, rng.integers(0, 30, 40), 97, 0, 1, front=11)
    add("row-range", [(whole[0][5:26], whole[1], 20, 5, 1)], 97, 30)
    for n_rows in (2047, 2048, 2049):
        add(f"users-{n_rows}", [mk(rng, rng.integers(0, 12, 300), 70, 1700, 1), mk(rng, rng.integers(0, 12, 300), 70, n_rows - 300, 0)], 70, n_rows, n_held=200)
    return out


CASES = cases()


def run_raw(engine, parts, n_items, present, heldout, n_rows, slack=0):
    """The C call itself with every written array between guard bands of GUARD elements: (cols [n_items], seen indptr, seen indices
    [capacity], relevant indptr, relevant indices [capacity], counts int64 [4]) with the guards cut off, after they were found untouched."""
    dev = engine.device
    cap_seen = max(sum(p[1].shape[0] for p in parts), 1) + slack
    n_held = heldout.shape[0]
    cap_rel = max(n_held, 1) + slack

    def band(n, dtype):
        return torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    bufs = [band(n_items, torch.int32), band(n_rows + 1, torch.int64), band(cap_seen, torch.int32), band(n_rows + 1, torch.int64),
            band(cap_rel, torch.int32), band(4, torch.int64)]
    ptr = [C.c_void_p(b[GUARD:].data_ptr()) for b in bufs]
    desc = (_lib.TriplePart * len(parts))()
    keep = []
    for d, (indptr, indices, rows_p, user0, label) in zip(desc, parts):
        ip, ix = torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev)
        keep += [ip, ix]
        d.indptr, d.indices = ip.data_ptr(), ix.data_ptr() if ix.numel() else None
        d.n_rows, d.capacity, d.user0, d.label = rows_p, ix.numel(), user0, label
    present_dev = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8)).to(dev)
    held_dev = torch.from_numpy(np.ascontiguousarray(heldout, dtype=np.int32)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = engine.lib.sdrm_neumf_rank_problem(engine._h, desc, len(parts), n_items, C.c_void_p(present_dev.data_ptr()),
                                            C.c_void_p(held_dev.data_ptr()) if n_held else None, n_held, n_rows, ptr[0], n_items, ptr[1], ptr[2], cap_seen,
                                            ptr[3], ptr[4], cap_rel, ptr[5], stream)
    assert rc == 0, engine.lib.sdrm_last_error(engine._h)
    out = []
    for b, name in zip(bufs, ("cols_out", "seen_indptr", "seen_indices", "relevant_indptr", "relevant_indices", "counts_dev")):
        b = b.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), f"a store outside {name}"
        out.append(b[GUARD:-GUARD])
    return out


def status_of(engine):
    """The status bits `feed_status()` names (it clears them), from its message."""
    try:
        engine.feed_status()
    except SdrmError as exc:
        text = str(exc)
        assert not [t for t in OTHER_TEXTS if t in text], text
        return (rr.BAD_ROW if rr.ROW_TEXT in text else 0) | (rr.BAD_COL if rr.COL_TEXT in text else 0) | (rr.STACK_PTR if rr.PTR_TEXT in text else 0)
    return 0


def expected(parts, n_items, present, heldout, n_rows, got):
    """The restatement laid into arrays of the buffers' sizes: the sentinel stands wherever the call leaves an element as it was."""
    cols, seen, relevant, counts, status = rr.rank_problem_ref(parts, n_items, present, heldout, n_rows)
    want = [np.full(g.shape, SENTINEL, dtype=g.dtype) for g in got]
    want[0][:counts[0]] = cols
    want[1][:], want[2][:counts[1]] = seen[0], seen[1]
    want[3][:], want[4][:counts[2]] = relevant[0], relevant[1]
    want[5][:] = counts
    return want, counts, status


def check(engine, parts, n_items, present, heldout, n_rows, expect_status=0, slack=0):
    got = run_raw(engine, parts, n_items, present, heldout, n_rows, slack)
    status = status_of(engine)
    want, counts, w_status = expected(parts, n_items, present, heldout, n_rows, got)
    print("counts", got[5].tolist(), "restated", counts, "status", status, "restated", w_status)
    for g, w, name in zip(got, want, ("cols", "seen indptr", "seen indices", "relevant indptr", "relevant indices", "counts")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert status == w_status == expect_status
    return got, counts


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_restatement(engine, name):
    parts, n_items, n_rows, heldout = CASES[name]
    present = present_of(parts, n_items)
    _, counts = check(engine, parts, n_items, present, heldout, n_rows)
    assert counts[3] == 0 and counts[0] == int(present.sum())
    if name == "edges-4099":
        assert counts[0] < n_items                                       # items no part holds: col_of is -1 for them
    if name == "shared-pair":
        assert counts[1] == 5                                            # user 0: {4, 6, 9}, user 1: {1, 9} - seven stored entries


@pytest.mark.gpu
def test_absent_items_are_no_columns(engine):
    """Items no part holds - and items `item_present` leaves out although a part holds them - are no columns: C < n_items, col_of is -1, a
    seen entry and a held-out triple on them are dropped silently."""
    parts, n_items, n_rows, heldout = CASES["items-128"]
    present = present_of(parts, n_items)
    present[[5, 64, 127]] = 0
    heldout = np.concatenate([heldout, [[1, 5, 1], [2, 64, 1], [3, 127, 1]]]).astype(np.int32)
    _, counts = check(engine, parts, n_items, present, heldout, n_rows)
    assert counts[0] == int(present.sum()) < n_items and counts[3] == 0


@pytest.mark.gpu
def test_heldout_range_defects_are_dropped_counted_and_reported(engine):
    parts, n_items, n_rows, heldout = CASES["items-65"]
    present = present_of(parts, n_items)
    bad = np.array([[-1, 3, 1], [n_rows, 3, 1], [4, -1, 1], [4, n_items, 0], [n_rows + 7, n_items + 7, 1]], dtype=np.int32)
    _, counts = check(engine, parts, n_items, present, np.concatenate([heldout[:20], bad, heldout[20:]]), n_rows, expect_status=rr.BAD_ROW | rr.BAD_COL)
    assert counts[3] == 5
    _, counts = check(engine, parts, n_items, present, np.concatenate([heldout, bad[:2]]), n_rows, expect_status=rr.BAD_ROW)
    assert counts[3] == 2
    _, counts = check(engine, parts, n_items, present, np.concatenate([bad[2:4], heldout]), n_rows, expect_status=rr.BAD_COL)
    assert counts[3] == 2


@pytest.mark.gpu
def test_without_heldout_triples(engine):
    parts, n_items, n_rows, _ = CASES["eight"]
    _, counts = check(engine, parts, n_items, present_of(parts, n_items), np.zeros((0, 3), dtype=np.int32), n_rows)
    assert counts[2] == 0


@pytest.mark.gpu
def test_slack_behind_the_counts_is_left_alone(engine):
    parts, n_items, n_rows, heldout = CASES["empty-part"]
    check(engine, parts, n_items, present_of(parts, n_items), heldout, n_rows, slack=301)


@pytest.mark.gpu
def test_a_part_row_beyond_n_rows_is_dropped_and_reported(engine):
    parts, n_items, _, heldout = CASES["empty-part"]                     # users 0 .. 2 and 9, 10
    present = present_of(parts, n_items)
    held = heldout[heldout[:, 0] < 10]
    _, counts = check(engine, parts, n_items, present, held, 10, expect_status=rr.BAD_ROW)
    assert counts[1] < sum(p[1].shape[0] for p in parts)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["out-of-order", "negative", "behind-capacity", "too-long", "col-high", "col-negative"])
def test_bad_rows_contribute_nothing_and_are_reported(engine, kind):
    """tests/test_neumf_triples.py's six row defects in the 70-row part of its 'three' case (97 items; users 0 .. 69 and 1000 .. 1299)."""
    parts, n_items, bits = tt._defect(kind)
    clean_parts = tt.CASES["three"][0]
    present = present_of(clean_parts, n_items)
    rng = np.random.default_rng(5)
    heldout = held_of(rng, 1300, n_items, 50, present)
    assert (tt.tr.STACK_PTR, tt.tr.BAD_COL) == (rr.STACK_PTR, rr.BAD_COL)
    _, counts = check(engine, parts, n_items, present, heldout, 1300, expect_status=bits, slack=100)
    clean = rr.rank_problem_ref(clean_parts, n_items, present, heldout, 1300)[3]
    assert counts[1] != clean[1] and counts[2] == clean[2]


@pytest.mark.gpu
def test_same_bytes_behind_a_larger_call(engine):
    parts, n_items, n_rows, heldout = CASES["items-65"]
    present = present_of(parts, n_items)
    first = run_raw(engine, parts, n_items, present, heldout, n_rows)
    for name in ("edges-4099", "users-2049"):
        p, i, r, h = CASES[name]
        run_raw(engine, p, i, present_of(p, i), h, r)
    again = run_raw(engine, parts, n_items, present, heldout, n_rows)
    assert status_of(engine) == 0
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def scipy_parts(seed=8):
    rng = np.random.default_rng(seed)
    a = (rng.random((37, 77)) < 0.2).astype(np.float32)
    b = (rng.random((37, 77)) < 0.2).astype(np.float32)
    c = (rng.random((12, 77)) < 0.3).astype(np.float32)
    for m in (a, b, c):
        m[:, [7, 70]] = 0                                                 # items no part holds
    a[2, 3] = b[2, 3] = 1.0                                               # a pair two parts hold
    return [(csr_matrix(a), 0, 0), (csr_matrix(b), 0, 1), (csr_matrix(c), 37, 1)]


@pytest.mark.gpu
def test_to_host_equals_from_parts(engine):
    """`Engine.neumf_rank_problem` behind `Engine.neumf_triples`, wrapped by `DeviceRankingProblem.build`: the views are cut to the counts
    and `to_host()` is `RankingProblem.from_parts`' object, array for array."""
    parts = scipy_parts()
    dev_parts = [(engine.csr_to_device(m), u, l) for m, u, l in parts]
    triples, counts, present = engine.neumf_triples(dev_parts, 77)
    rng = np.random.default_rng(9)
    heldout = np.stack([rng.integers(37, 49, 60), rng.integers(0, 77, 60), rng.integers(0, 2, 60)], axis=1).astype(np.int64)
    heldout = np.concatenate([heldout, heldout[:4], [[40, 7, 1]]])
    problem = neumf.DeviceRankingProblem.build(engine, dev_parts, 77, present, heldout, counts[2])
    want = neumf.RankingProblem.from_parts(parts, np.flatnonzero(present.cpu().numpy()), heldout)
    assert problem.n_rows == counts[2] == 49 and problem.counts[0] == want.cols.shape[0] == 75 and problem.counts[3] == 0
    assert problem.cols.dtype == torch.int32 and problem.seen[1].numel() == problem.counts[1] and problem.relevant[1].numel() == problem.counts[2]
    assert problem.seen[3] == problem.relevant[3] == (49, 75) and problem.seen[2] is None
    got = problem.to_host()
    np.testing.assert_array_equal(got.cols, want.cols)
    assert got.cols.dtype == want.cols.dtype
    for x, y in zip(got._relevant + got._seen, want._relevant + want._seen):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    bad = torch.tensor([[49, 1, 1]], dtype=torch.int32, device=engine.device)
    with pytest.raises(SdrmError, match="row id outside"):
        engine.neumf_rank_problem(dev_parts, 77, present, bad, 49)
    record = engine.neumf_rank_problem(dev_parts, 77, present, bad, 49, check=False)
    assert status_of(engine) == rr.BAD_ROW and record.counts[2:] == (0, 1)


# ================================================================================================ select and rank
@pytest.mark.gpu
@pytest.mark.parametrize("n, kind", [(1, "zero"), (1, "one"), (255, "random"), (256, "random"), (257, "random"), (257, "zero"), (257, "one"),
                                     (2047, "random"), (2048, "one"), (2049, "random")])
def test_users_of_a_mask(engine, n, kind):
    rng = np.random.default_rng(n)
    mask = {"zero": np.zeros(n, dtype=np.uint8), "one": np.ones(n, dtype=np.uint8), "random": (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)}[kind]
    dev = engine.device
    users = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    count = torch.full((GUARD + 1 + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    mask_dev = torch.from_numpy(mask).to(dev)
    rc = engine.lib.sdrm_neumf_rank_users(engine._h, C.c_void_p(mask_dev.data_ptr()), n, C.c_void_p(users[GUARD:].data_ptr()), C.c_void_p(count[GUARD:].data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, engine.lib.sdrm_last_error(engine._h)
    want = rr.rank_users_ref(mask)
    full = np.full(GUARD + n + GUARD, SENTINEL, dtype=np.int32)
    full[GUARD:GUARD + want.shape[0]] = want
    np.testing.assert_array_equal(users.cpu().numpy(), full)
    np.testing.assert_array_equal(count.cpu().numpy(), [SENTINEL] * GUARD + [want.shape[0]] + [SENTINEL] * GUARD)
    view = engine.neumf_rank_users(mask_dev)
    assert view.dtype == torch.int32 and view.shape == want.shape
    np.testing.assert_array_equal(view.cpu().numpy(), want)


_RANK = {}


def rank_case():
    """A random 37 x 300 score matrix (with ties) over two resident matrices of 50 rows, and a permuted, repeating row list; made once."""
    if not _RANK:
        rng = np.random.default_rng(77)
        scores = np.round(rng.standard_normal((37, 300)), 1).astype(np.float32)
        held = (rng.random((50, 300)) < 0.02).astype(np.float32)
        held[11] = 0                                                        # a user without a relevant item
        held, train = csr_matrix(held), csr_matrix((rng.random((50, 300)) < 0.3).astype(np.float32))
        rows = np.concatenate([rng.permutation(50)[:30], [11, 11, 3, 49, 0, 3, 11]]).astype(np.int32)
        _RANK.update(scores=scores, held=held, train=train, rows=rows)
    return _RANK["scores"], _RANK["held"], _RANK["train"], _RANK["rows"]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [True, False])
def test_rank_metrics_rows_equals_rank_metrics_on_the_gathered_rows(engine, masked):
    scores, held, train, rows = rank_case()
    assert rows.shape[0] == 37 and np.unique(rows).shape[0] < 37 and np.diff(held.indptr)[11] == 0
    dev = engine.device
    scores_dev, rows_dev = torch.from_numpy(scores).to(dev), torch.from_numpy(rows).to(dev)
    held_dev, train_dev = engine.csr_to_device(held), engine.csr_to_device(train) if masked else None
    want = engine.rank_metrics(scores_dev, held[rows], train[rows] if masked else None, ks=neumf.K_LIST)
    want = [w.cpu().numpy() for w in want]
    got = [g.cpu().numpy() for g in engine.rank_metrics_rows(scores_dev, rows_dev, held_dev, train_dev, ks=neumf.K_LIST)]
    assert status_of(engine) == 0 and got[0].shape == (6, 37) and np.isnan(got[0][:, rows == 11]).all() and np.isnan(got[1][:, rows == 11]).all()
    assert same(got[0], want[0]) and same(got[1], want[1])
    # the NeuMF footing: the host's three operations on rank_metrics' NDCG; recall untouched
    foot = [g.cpu().numpy() for g in engine.rank_metrics_rows(scores_dev, rows_dev, held_dev, train_dev, ks=neumf.K_LIST, full_idcg=True)]
    assert status_of(engine) == 0
    w_foot = rr.neumf_footing(want[1], np.diff(held[rows].indptr), neumf._idcg_table()[1], 300, neumf.K_LIST)
    assert same(foot[0], want[0]) and same(foot[1], w_foot) and (foot[1][:, rows == 11] == 0).all() and not np.isnan(foot[1]).any()


@pytest.mark.gpu
def test_a_row_id_out_of_range_is_an_empty_row(engine):
    scores, held, train, rows = rank_case()
    dev = engine.device
    scores_dev = torch.from_numpy(scores).to(dev)
    held_dev, train_dev = engine.csr_to_device(held), engine.csr_to_device(train)
    empty = csr_matrix((1, 300), dtype=np.float32)
    from scipy.sparse import vstack
    for bad_id in (50, -1):
        bad = rows.copy()
        bad[4] = bad_id
        got = [g.cpu().numpy() for g in engine.rank_metrics_rows(scores_dev, torch.from_numpy(bad).to(dev), held_dev, train_dev, ks=neumf.K_LIST)]
        assert status_of(engine) == rr.BAD_ROW
        pick = lambda m: vstack([m[rows[:4]], empty, m[rows[5:]]]).tocsr()
        want = [w.cpu().numpy() for w in engine.rank_metrics(scores_dev, pick(held), pick(train), ks=neumf.K_LIST)]
        assert same(got[0], want[0]) and same(got[1], want[1]) and np.isnan(got[0][:, 4]).all()


def triples_as_parts(engine, training, n_users, n_items):
    """(device parts, host parts, item_present on the device) of training triples: the label-0 pairs and the label-1 pairs as two CSR parts."""
    host = []
    for label in (0, 1):
        t = training[training[:, 2] == label]
        host.append((csr_matrix((np.ones(t.shape[0], dtype=np.float32), (t[:, 0], t[:, 1])), shape=(n_users, n_items)), 0, label))
    present = np.zeros(n_items, dtype=np.uint8)
    present[training[:, 1]] = 1
    return [(engine.csr_to_device(m), u, l) for m, u, l in host], host, torch.from_numpy(present).to(engine.device)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nr.RANK_CASES))
def test_rank_all_items_with_a_device_problem_equals_the_host_problem(engine, name):
    """The quirk case and the 120 x 300 split of tests/neumf_ref.py: the same `neumf_scores` call on the same ids, the same ranking body and
    the footing's same operations - equality, not a tolerance; for the users as ids and as the device mask."""
    from test_neumf_eval import module_of
    w, training, heldout = nr.rank_inputs(name)
    _, n_users, n_items = nr.RANK_CASES[name][:3]
    model = module_of(w, engine.device)
    dev_parts, _, present = triples_as_parts(engine, training, n_users, n_items)
    device_problem = neumf.DeviceRankingProblem.build(engine, dev_parts, n_items, present, heldout, n_users)
    host_problem = neumf.RankingProblem(training, heldout)
    want = neumf.rank_all_items(model, training, heldout, heldout[:, 0], engine, problem=host_problem)
    got = neumf.rank_all_items(model, None, None, heldout[:, 0], engine, problem=device_problem)
    assert got[0].dtype == got[1].dtype == np.float64 and got[0].shape == want[0].shape == (6, np.unique(heldout[:, 0]).shape[0])
    assert same(got[0], want[0]) and same(got[1], want[1])
    mask = torch.zeros(n_users, dtype=torch.uint8, device=engine.device)
    mask[torch.from_numpy(np.unique(heldout[:, 0])).to(engine.device)] = 1
    masked = neumf.rank_all_items(model, None, None, mask, engine, problem=device_problem)
    assert same(masked[0], want[0]) and same(masked[1], want[1])
    if name == nr.QUIRK:
        assert np.isnan(want[0]).any() and (want[1] == 0).any()
    nobody = neumf.rank_all_items(model, None, None, torch.zeros(n_users, dtype=torch.uint8, device=engine.device), engine, problem=device_problem)
    assert nobody[0].shape == nobody[1].shape == (6, 0)


# ================================================================================================ stream order
def stream_case_problem(b=33):
    """sdrm_neumf_rank_problem on the harness's feed matrix with label 0 and a row range of it (an indptr that does not start at 0) as
    users 40 .. with label 1; every item present but two; held-out triples over all 80 users."""
    m = sh._feed(b)
    n_rows = 80
    rng = np.random.default_rng(6)
    present = np.ones(sh.ITEMS, dtype=np.uint8)
    present[[3, 64]] = 0
    held = np.stack([rng.integers(0, n_rows, 90), rng.integers(0, sh.ITEMS, 90), rng.integers(0, 2, 90)], axis=1).astype(np.int32)

    def parts(x):
        return [(sh._csr(x, m.shape), 0, 0), ((x["csr_indptr"][5:], x["csr_indices"], None, (b - 5, sh.ITEMS)), 40, 1)]

    def make(device):
        return dict(sh._csr_inputs(m, device), present=sh._dev(present, device), held=sh._dev(held, device))

    def call(e, x, alloc):
        r = e.neumf_rank_problem(parts(x), sh.ITEMS, x["present"], x["held"], n_rows, check=False)
        return r.cols, r.seen[0], r.seen[1], r.relevant[0], r.relevant[1], r.counts

    def anchor(inp, res):   # the numpy restatement, byte for byte; the counts are host values the harness compares with the twin's
        ip, ix = inp["csr_indptr"].numpy(), inp["csr_indices"].numpy()
        cols, seen, relevant, counts, status = rr.rank_problem_ref([(ip, ix, b, 0, 0), (ip[5:], ix, b - 5, 40, 1)], sh.ITEMS, present, held, n_rows)
        assert status == 0 and counts[0] == sh.ITEMS - 2
        for got, want in zip(res, (cols, seen[0], seen[1], relevant[0], relevant[1])):
            assert np.array_equal(got.numpy(), want)

    return sh._util("neumf-rank-problem", ("sdrm_neumf_rank_problem",), make, call, anchor=anchor)


def stream_case_users(n=300):
    mask = (np.random.default_rng(4).random(n) < 0.3).astype(np.uint8)

    def make(device):
        return dict(mask=sh._dev(mask, device))

    def call(e, x, alloc):
        return e.neumf_rank_users(x["mask"])

    def anchor(inp, res):
        assert np.array_equal(res[0].numpy(), rr.rank_users_ref(mask))

    return sh._util("neumf-rank-users", ("sdrm_neumf_rank_users",), make, call, anchor=anchor, feed=False)


def stream_case_rows():
    scores, held, train, rows = rank_case()

    def make(device):
        return dict(sh._csr_inputs(held, device, "held"), **sh._csr_inputs(train, device, "train"), scores=sh._dev(scores, device), rows=sh._dev(rows, device))

    def call(e, x, alloc):
        return e.rank_metrics_rows(x["scores"], x["rows"], sh._csr(x, held.shape, "held"), sh._csr(x, train.shape, "train"), ks=neumf.K_LIST, full_idcg=True)

    def anchor(inp, res):   # oracle/rank_metrics_ref.py on the gathered rows, the footing by the host's formula: exactly
        from oracle import rank_metrics_ref
        recall, ndcg = rank_metrics_ref.rank_metrics(scores, held[rows], train[rows], ks=neumf.K_LIST)
        ndcg = rr.neumf_footing(ndcg, np.diff(held[rows].indptr), neumf._idcg_table()[1], 300, neumf.K_LIST)
        assert same(res[0].numpy(), recall) and same(res[1].numpy(), ndcg)

    return sh._util("rank-metrics-rows", ("sdrm_rank_metrics_rows",), make, call, anchor=anchor)


@pytest.mark.gpu
@pytest.mark.parametrize("pool, variant", [("warm", "late"), ("warm", "busy"), ("cold", "late"), ("cold", "busy")])
@pytest.mark.parametrize("entry", ["problem", "users", "rows"])
def test_on_a_busy_side_stream(engine_cls, entry, pool, variant):
    """The three entry points with inputs that arrive late on a non-blocking side stream, the default stream busy as well in "busy", warm
    and as the engine's first call of the family: each returns with its inputs pending (asserted in the warm pool), and the side stream alone
    sees the default-stream twin's bytes, which are the restatement's (tests/stream_harness.py's run_case)."""
    case = {"problem": stream_case_problem, "users": stream_case_users, "rows": stream_case_rows}[entry]()
    assert len(case.nosync) == 1 and case.nosync[0] in case.covers
    sh.run_case(case, engine_cls, pool, variant)


# ================================================================================================ the route
def _same_history(a, b):
    assert a["valid_loss"] == b["valid_loss"] and a["train_loss"] == b["train_loss"] and a["draw_counts"] == b["draw_counts"]
    assert len(a["recall10"]) == len(b["recall10"]) == 2
    assert all((x == y) or (np.isnan(x) and np.isnan(y)) for x, y in zip(a["recall10"], b["recall10"]))
    for x, y in zip(a["per_user"], b["per_user"]):
        assert x.shape == y.shape and same(x, y)


@pytest.mark.gpu
def test_route_with_the_device_ranking_equals_the_route_without(engine, monkeypatch):
    """tests/test_neumf_triples.py's tiny problem (40 x 64, 12 validation users, 2 epochs, seed 3): the same bytes reach the same draws and
    train steps, and both rankings make the same operations, so the metrics and the histories are EQUAL - also through
    `pipeline.evaluate_synthetic` with the hp key.  With the device ranking the tails are not read back and `from_parts` is not called."""
    raw, valid, sparsity = tt.tiny_problem()
    train = csr_matrix((40, 64), dtype=np.float64)
    raw_dev = torch.from_numpy(raw).to(engine.device)
    h_host, h_dev = {}, {}
    want = neumf.compute_neuralcf_results_synthetic(train.shape, valid, raw_dev, sparsity, engine, seed=3, epochs=2, history=h_host)
    calls = []
    original = neumf.RankingProblem.from_parts.__func__
    monkeypatch.setattr(neumf.RankingProblem, "from_parts", classmethod(lambda cls, *a, **k: calls.append(1) or original(cls, *a, **k)))
    got = neumf.compute_neuralcf_results_synthetic(train.shape, valid, raw_dev, sparsity, engine, seed=3, epochs=2, history=h_dev, device_ranking=True)
    assert not calls
    print("host ranking", want, "device ranking", got)
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    _same_history(h_dev, h_host)
    routed = pipeline.evaluate_synthetic(train, valid, raw_dev, sparsity, engine, dict(evaluator="neumf", neumf_epochs=2, neumf_device_ranking=True), 3)
    assert not calls
    for a, b in zip(want, routed):
        np.testing.assert_array_equal(a, b)
