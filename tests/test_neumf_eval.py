"""The NeuMF evaluator: eval-mode forward and ranking on the device (csrc/neumf.h; sdrm_neumf_scores / sdrm_neumf_pair_loss;
sdrm_amd/neumf.py).

References: tests/neumf_ref.py - the float64 oracle of the forward and of the reference's testing block, and the case tables -, and
tests/golden/neumf_eval.npz - the reference's own float32 logits and ranking figures for those cases (make_neumf_golden.py).

Bars.  The reference's float32 forward deviates from the float64 oracle by 1.0e-7 .. 3.4e-7 normwise on the cases here (computed in the
tests from the fixture, never from the device).  The device sums the same number of terms in another order, so its bar is a fixed
multiple of that, BAR_FACTOR = 4, case by case.  The loss bar is the same multiple of the relative deviation of the reference's float32
BCEWithLogitsLoss from the float64 one on the loss case (5e-8).  Ranking: a user's figures must equal the host path's unless two of
its unmasked reference scores, both among its top 51 or its relevant items, lie closer than 8 x bar x max|score| - only there may
float32 order two items the other way; at most 2 % of the users may be exempt, and every user has at least 51 unmasked columns."""
import os

import numpy as np
import pytest
import torch

import neumf_ref as nr
from sdrm_amd import _lib, neumf
from sdrm_amd.engine import Engine, SdrmError

BAR_FACTOR, GAP_FACTOR, EXEMPT_SHARE = 4.0, 8.0, 0.02
SHAPE, ARG = -2, -1
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neumf_eval.npz")


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


_CACHE = {}


def case(name):
    """(weights, users, items, items_is_none, float64 scores) of a forward case, computed once."""
    if name not in _CACHE:
        w, users, items, none = nr.case_inputs(name)
        ref = nr.scores64(w, users, items)
        ref.setflags(write=False)
        _CACHE[name] = (w, users, items, none, ref)
    return _CACHE[name]


def rank_case(name):
    """(weights, training, heldout, users, cols, relevant, seen, float64 scores) of a ranking case, computed once."""
    key = ("rank", name)
    if key not in _CACHE:
        w, training, heldout = nr.rank_inputs(name)
        users, cols, relevant, seen = nr.rank_problem(training, heldout)
        ref = nr.scores64(w, users, cols)
        ref.setflags(write=False)
        _CACHE[key] = (w, training, heldout, users, cols, relevant, seen, ref)
    return _CACHE[key]


def module_of(w, device="cpu"):
    n_users, F = w[nr.NAMES[0]].shape
    model = neumf.NCF(n_users, w[nr.NAMES[1]].shape[0], factor=F)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return model.to(device).eval()


def toy(seed=1, n_users=40, n_items=90):
    """(training, validation) triples of the 40-user toy: 24 training and 6 validation pairs per user, random labels."""
    rng = np.random.default_rng(seed)
    training, validation = [], []
    for u in range(n_users):
        for j, i in enumerate(rng.permutation(n_items)[:30]):
            (training if j < 24 else validation).append((u, int(i), int(rng.random() < 0.5)))
    return np.asarray(training), np.asarray(validation)


# ================================================================================================ CPU
@pytest.mark.parametrize("name", list(nr.CASES))
def test_oracle_against_the_references_logits(fixture, name):
    """The float64 restatement against the reference's own float32 logits: they differ by float32 rounding only (1.0e-7 .. 3.4e-7 normwise,
    2.3e-7 on the issue's 50 x 37 trial), far below the 2e-6 a wrong term or a swapped table would exceed by orders."""
    w, users, items, _, ref = case(name)
    got = fixture[f"{name}_logits"]
    assert got.shape == ref.shape and got.dtype == np.float32
    dev = nr.normwise(got, ref)
    print(name, "reference fp32 deviation", dev)
    assert 0 < dev < 2e-6


def test_loss_oracle_against_the_references_loss(fixture):
    w, users, items, labels = nr.loss_inputs()
    x64 = nr.forward64(w, users, items)
    for y in (0.0, 1.0):
        assert (x64[labels == y] > 18).any() and (x64[labels == y] < -18).any()
    assert nr.normwise(fixture["loss_logits"], x64) < 2e-6
    assert abs(float(fixture["loss_value"]) - nr.bce64(x64, labels)) / nr.bce64(x64, labels) < 1e-6
    assert abs(nr.bce64(fixture["loss_logits"], labels) - nr.bce64(x64, labels)) / nr.bce64(x64, labels) < 1e-6


def test_module_loads_upstream_keys_and_reproduces_the_fixture_bit_for_bit(fixture):
    """`NCF` takes a state_dict under the reference's keys and shapes, and its eval forward on the CPU is the reference's, bit for bit."""
    for name in nr.CASES:
        w, users, items, _, _ = case(name)
        model = module_of(w)
        assert tuple(model.state_dict()) == nr.NAMES == Engine.NEUMF_TENSORS
        assert [tuple(t.shape) for t in model.state_dict().values()] == [v.shape for v in w.values()]
        got = neumf.host_scores(model, users, items)
        assert got.dtype == np.float32 and np.array_equal(got, fixture[f"{name}_logits"]), name
    w, users, items, labels = nr.loss_inputs()
    model = module_of(w)
    with torch.no_grad():
        x = model(torch.from_numpy(users), torch.from_numpy(items))
    assert np.array_equal(x.numpy(), fixture["loss_logits"])
    assert neumf.validation_loss(model, np.stack([users, items, labels.astype(np.int32)], axis=1)) == float(fixture["loss_value"])
    fresh = neumf.NCF(30, 20)   # the reference's initialisation: small tables, zero biases, a bounded tower
    init = {k: v.numpy() for k, v in fresh.state_dict().items()}
    assert abs(init["embed_user_MLP.weight"].std() - 0.01) < 2e-3 and all(np.abs(v).max() == 0 for k, v in init.items() if k.endswith("bias"))
    assert np.abs(init["MLP_layers.1.weight"]).max() <= (6.0 / (64 + 32)) ** 0.5 and np.abs(init["predict_layer.weight"]).max() <= (3.0 / 16) ** 0.5


def test_rank_conditions_hold_on_the_reference_scores(fixture):
    """What the ranking tests rely on, from the float64 scores alone: at least 51 unmasked columns per user, at most 2 % near-tie users."""
    for name in nr.RANK_CASES:
        _, _, _, users, _, relevant, seen, ref = rank_case(name)
        gap = GAP_FACTOR * BAR_FACTOR * float(fixture[f"{name}_dev"]) * np.abs(ref).max()
        fewest, exempt = nr.rank_conditions(ref, relevant, seen, gap)
        print(name, "fewest unmasked", fewest, "exempt", exempt)
        assert fewest >= 51 and len(exempt) <= EXEMPT_SHARE * len(users)


def test_host_ranking_reproduces_the_references_testing_block(fixture):
    """`rank_all_items(engine=None)` on the quirk case against the figures the reference's `utilities` functions gave on the reference's
    logits, to 1e-12: the case has a user without a positive held-out item (recall nan, NDCG 0), a held-out item that never occurs in
    training (dropped), label-0 training pairs (masked all the same), fewer relevant items than k, and the ideal DCG of min(columns, k)."""
    w, training, heldout, users, cols, relevant, seen, _ = rank_case(nr.QUIRK)
    assert (relevant.sum(axis=1) == 0).any() and not np.isin(heldout[heldout[:, 2] > 0, 1], cols).all()
    assert ((training[:, 2] == 0) & np.isin(training[:, 0], users)).any() and (relevant.sum(axis=1) < 10).all()
    recall, ndcg = neumf.rank_all_items(module_of(w), training, heldout, heldout[:, 0])
    assert recall.shape == ndcg.shape == (6, len(users))
    np.testing.assert_allclose(recall, fixture["quirk_recall"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(ndcg, fixture["quirk_ndcg"], rtol=0, atol=1e-12)
    nobody = relevant.sum(axis=1) == 0
    assert np.isnan(recall[:, nobody]).all() and (ndcg[:, nobody] == 0).all() and not np.isnan(recall[:, ~nobody]).any()
    ref_recall, ref_ndcg = nr.rank_metrics64(fixture["quirk_logits"], relevant, seen)
    np.testing.assert_allclose(ref_recall, fixture["quirk_recall"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(ref_ndcg, fixture["quirk_ndcg"], rtol=0, atol=1e-12)
    u2, c2, rel2, seen2 = neumf.ranking_problem(training, heldout, heldout[:, 0])
    assert np.array_equal(u2, users) and np.array_equal(c2, cols) and np.array_equal(rel2.toarray() > 0, relevant) and np.array_equal(seen2.toarray() > 0, seen)


def test_refusals_need_no_device():
    """F = 12, a two-layer tower, a table with the wrong row count, int64 id lists and a labels length mismatch are refused by the Engine
    methods on the host before anything is called; the C side's own envelope check refuses F = 12 as well.  ABI signature lengths."""
    lib = _lib.load()
    assert lib.sdrm_debug_neumf_args(5, 6, 8, 3, 4) == 0 and lib.sdrm_debug_neumf_args(5, 6, 16, 1, 1) == 0 and lib.sdrm_debug_neumf_args(5, 6, 32, 2 ** 20 - 16, 2 ** 19) == 0
    for bad in ((5, 6, 12, 3, 4), (5, 6, 64, 3, 4), (0, 6, 8, 3, 4), (5, 0, 8, 3, 4), (5, 6, 8, 0, 4), (5, 6, 8, 3, 0), (5, 6, 8, 2 ** 20 - 15, 1),
                (5, 6, 8, 1, 2 ** 22 + 1), (5, 6, 8, 2 ** 20, 2 ** 20)):
        assert lib.sdrm_debug_neumf_args(*bad) == SHAPE, bad
    assert lib.sdrm_neumf_scores(None, None, None, 1, None, 1, None, None) == ARG
    assert lib.sdrm_neumf_pair_loss(None, None, None, None, None, 1, None, None, None) == ARG
    assert len(_lib.SIGNATURES["sdrm_neumf_scores"][1]) == 8 and len(_lib.SIGNATURES["sdrm_neumf_pair_loss"][1]) == 9
    assert len(_lib.SIGNATURES["sdrm_debug_neumf_args"][1]) == 5 and len(_lib.Neumf._fields_) == 15

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    eng = Engine.__new__(Engine)       # the methods' own checks, on the host: any call into the library fails the test
    eng.device, eng.lib, eng._h = torch.device("cpu"), NoLaunch(), None
    good = list(neumf.NCF(9, 11, factor=8).state_dict().values())
    users, items = torch.arange(4, dtype=torch.int32), torch.arange(4, dtype=torch.int32)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE.*factor 12"):
        eng.neumf_scores(list(neumf.NCF(9, 11, factor=12).state_dict().values()), users)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE.*THREE"):
        eng.neumf_scores(list(neumf.NCF(9, 11, factor=8, layers=2).state_dict().values()), users)
    wrong_rows = list(good)
    wrong_rows[2] = torch.zeros(10, 32)
    for call in (lambda w: eng.neumf_scores(w, users), lambda w: eng.neumf_pair_logits(w, users, items)):
        with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE.*embed_user_MLP"):
            call(wrong_rows)
    half = list(good)
    half[4] = half[4].double()
    with pytest.raises(SdrmError, match="float32"):
        eng.neumf_scores(half, users)
    with pytest.raises(SdrmError, match="int32"):
        eng.neumf_scores(good, users.long())
    with pytest.raises(SdrmError, match="int32"):
        eng.neumf_scores(good, users, items.long())
    with pytest.raises(SdrmError, match="int32"):
        eng.neumf_pair_logits(good, users, items.long())
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        eng.neumf_pair_logits(good, users, items[:3])
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE.*labels"):
        eng.neumf_pair_logits(good, users, items, labels=torch.zeros(5))
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE.*out"):
        eng.neumf_scores(good, users, items, out=torch.zeros(4, 5))


def test_driver_on_the_host_is_reproducible():
    """`compute_neuralcf_results(engine=None, epochs=2)` on the 40-user toy runs, gives the same figures and losses under one seed and
    others under another; numpy's global generator is not consumed, torch's global generator is seeded with `seed` on entry."""
    training, validation = toy()
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    h1, h2, h3 = {}, {}, {}
    r1 = neumf.compute_neuralcf_results(training, validation, 40, 90, seed=3, epochs=2, history=h1)
    assert torch.initial_seed() == 3 and np.array_equal(np.random.get_state()[1], before)
    r2 = neumf.compute_neuralcf_results(training, validation, 40, 90, seed=3, epochs=2, history=h2)
    r3 = neumf.compute_neuralcf_results(training, validation, 40, 90, seed=4, epochs=2, history=h3)
    assert r1[0].shape == r1[1].shape == (6,) and np.isfinite(r1[0]).all() and np.isfinite(r1[1]).all()
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and h1["valid_loss"] == h2["valid_loss"] and len(h1["valid_loss"]) == 2
    assert h1["valid_loss"] != h3["valid_loss"]
    assert h1["epochs_run"] == 2 and h1["best_epoch"] == 0 and len(h1["recall10"]) == 2
    h4 = {}
    neumf.compute_neuralcf_results(training, validation, 40, 90, seed=3, epochs=2, eval_recall=False, history=h4)
    assert h4["recall10"] == [] and h4["best_epoch"] == int(np.argmin(h4["valid_loss"])) and h4["valid_loss"] == h1["valid_loss"]


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def dev_weights(engine, w):
    return [torch.from_numpy(w[k]).to(engine.device) for k in nr.NAMES]


def ids(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(engine.device)


def device_scores(engine, name):
    key = ("dev", name)
    if key not in _CACHE:
        w, users, items, none, _ = case(name)
        _CACHE[key] = engine.neumf_scores(dev_weights(engine, w), ids(engine, users), None if none else ids(engine, items)).cpu().numpy()
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nr.CASES))
def test_scores_against_the_oracle(engine, fixture, name):
    """Normwise against the float64 oracle, within 4 x the reference's own float32 deviation on the same case.  Measured on an MI355X:
    see DESIGN 4u."""
    _, users, items, _, ref = case(name)
    got = device_scores(engine, name)
    assert got.shape == ref.shape and got.dtype == np.float32
    bar = BAR_FACTOR * nr.normwise(fixture[f"{name}_logits"], ref)
    dev = nr.normwise(got, ref)
    print(f"{name}: device deviation {dev:.3e}, reference fp32 deviation {bar / BAR_FACTOR:.3e}, bar {bar:.3e}")
    assert dev <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f8_lists", "f16_all_items", "f32", "past_tiles"])
def test_bitwise_identities(engine, name):
    """One call = two calls on halves of the users list = two calls on halves of the items list; a repeated user gives identical rows;
    listed pairs give the matching entries of the matrix (one chunk, and 65536 + 300 pairs across the pair kernel's staging chunk);
    two runs give the same bits, loss sum included."""
    w, users, items, none, _ = case(name)
    full = device_scores(engine, name)
    wd = dev_weights(engine, w)
    hu, hi = max(1, len(users) // 2), max(1, len(items) // 2)
    by_users = torch.cat([engine.neumf_scores(wd, ids(engine, users[:hu]), ids(engine, items)), engine.neumf_scores(wd, ids(engine, users[hu:]), ids(engine, items))])
    by_items = torch.cat([engine.neumf_scores(wd, ids(engine, users), ids(engine, items[:hi])), engine.neumf_scores(wd, ids(engine, users), ids(engine, items[hi:]))], dim=1)
    assert np.array_equal(by_users.cpu().numpy(), full) and np.array_equal(by_items.cpu().numpy(), full)
    if name == "f8_lists":
        assert users[-1] == users[0] and np.array_equal(full[-1], full[0]) and not np.array_equal(full[1], full[0])
    rng = np.random.default_rng(7)
    for n in (200,) + ((65536 + 300,) if name == "past_tiles" else ()):
        r, c = rng.integers(0, len(users), n), rng.integers(0, len(items), n)
        labels = torch.from_numpy(rng.integers(0, 2, n).astype(np.float32)).to(engine.device)
        logits, loss = engine.neumf_pair_logits(wd, ids(engine, users[r]), ids(engine, items[c]), labels)
        assert np.array_equal(logits.cpu().numpy(), full[r, c])
        logits2, loss2 = engine.neumf_pair_logits(wd, ids(engine, users[r]), ids(engine, items[c]), labels)
        assert torch.equal(logits, logits2) and loss.dtype == torch.float64 and loss.item() == loss2.item()
        only_logits, none_loss = engine.neumf_pair_logits(wd, ids(engine, users[r]), ids(engine, items[c]))
        assert none_loss is None and torch.equal(only_logits, logits)
        want = nr.bce64(full[r, c], labels.cpu().numpy())   # the float64 loss of the DEVICE's logits: the sum itself, to float32 terms
        assert abs(loss.item() / n - want) <= 4e-7 * want
    again = engine.neumf_scores(wd, ids(engine, users), None if none else ids(engine, items))
    assert np.array_equal(again.cpu().numpy(), full)


@pytest.mark.gpu
def test_loss_against_the_oracle(engine, fixture):
    """loss_sum / n against float64 BCEWithLogits of the oracle's logits, |x| up to about 25 on both sides of each label; the bar is 4 x
    the relative deviation of the reference's float32 loss on the same pairs."""
    w, users, items, labels = nr.loss_inputs()
    x64 = nr.forward64(w, users, items)
    want = nr.bce64(x64, labels)
    bar = BAR_FACTOR * abs(float(fixture["loss_value"]) - want) / want
    logits, loss_sum = engine.neumf_pair_logits(dev_weights(engine, w), ids(engine, users), ids(engine, items), torch.from_numpy(labels).to(engine.device))
    got = loss_sum.item() / len(users)
    print(f"loss: device {got!r}, float64 {want!r}, relative deviation {abs(got - want) / want:.3e}, reference fp32 {bar / BAR_FACTOR:.3e}, bar {bar:.3e}")
    assert nr.normwise(logits.cpu().numpy(), x64) <= BAR_FACTOR * nr.normwise(fixture["loss_logits"], x64)
    assert abs(got - want) / want <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["user -1", "user n_users", "item n_items"])
def test_range_checks(engine, fault):
    """An id outside its table, in both kernels: the call returns, the offending row / column / logit is zero, every other output keeps
    its bits, `feed_status()` raises once with the feed's message and is clear afterwards, and the next call works."""
    w, users, items, _, _ = case("f8_lists")
    full = device_scores(engine, "f8_lists")
    wd = dev_weights(engine, w)
    n_users, n_items = w[nr.NAMES[0]].shape[0], w[nr.NAMES[1]].shape[0]
    bad_u, bad_i = users.copy(), items.copy()
    if fault.startswith("user"):
        bad_u[3] = -1 if fault == "user -1" else n_users
        message = r"a row id outside \[0, n_rows\)"
    else:
        bad_i[5] = n_items
        message = r"a column index outside \[0, n_items\)"
    expect = full.copy()
    if fault.startswith("user"):
        expect[3, :] = 0
    else:
        expect[:, 5] = 0
    engine.feed_status()
    got = engine.neumf_scores(wd, ids(engine, bad_u), ids(engine, bad_i), check=False)
    assert np.array_equal(got.cpu().numpy(), expect)
    with pytest.raises(SdrmError, match=message):
        engine.feed_status()
    engine.feed_status()
    with pytest.raises(SdrmError, match=message):
        engine.neumf_scores(wd, ids(engine, bad_u), ids(engine, bad_i))          # check=True raises at once
    engine.feed_status()
    # the pair kernel: pair j is (users[j % U], items[j % I]); the faulty id sits in several pairs
    n = 300
    r, c = np.arange(n) % len(users), np.arange(n) % len(items)
    labels = torch.from_numpy((np.arange(n) % 2).astype(np.float32)).to(engine.device)
    clean_logits, clean_loss = engine.neumf_pair_logits(wd, ids(engine, users[r]), ids(engine, items[c]), labels)
    logits, loss = engine.neumf_pair_logits(wd, ids(engine, bad_u[r]), ids(engine, bad_i[c]), labels, check=False)
    hit = (r == 3) if fault.startswith("user") else (c == 5)
    assert hit.sum() > 3 and np.array_equal(logits.cpu().numpy(), np.where(hit, np.float32(0), expect[r, c]))
    assert np.array_equal(clean_logits.cpu().numpy(), full[r, c])
    x, y = clean_logits.cpu().numpy().astype(np.float64)[~hit], labels.cpu().numpy()[~hit]
    without = float(np.sum(np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))))
    assert abs(loss.item() - without) <= 4e-7 * without and loss.item() < clean_loss.item()   # the faulty pairs add nothing
    with pytest.raises(SdrmError, match=message):
        engine.feed_status()
    engine.feed_status()
    assert np.array_equal(engine.neumf_scores(wd, ids(engine, users), ids(engine, items)).cpu().numpy(), full)


def _compare_per_user(got, want, exempt, n_users):
    assert len(exempt) <= EXEMPT_SHARE * n_users
    keep = np.setdiff1d(np.arange(n_users), exempt)
    for g, w_ in zip(got, want):
        np.testing.assert_allclose(g[:, keep], w_[:, keep], rtol=0, atol=1e-12, equal_nan=True)
    with np.errstate(invalid="ignore"):
        for g, w_ in zip(got, want):
            means_g = np.array([np.round(np.nanmean(g[q][keep]), 4) for q in range(6)])
            means_w = np.array([np.round(np.nanmean(w_[q][keep]), 4) for q in range(6)])
            assert np.abs(means_g - means_w).max() <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nr.RANK_CASES))
def test_ranking_through_the_engine(engine, fixture, name):
    """`rank_all_items(..., engine)` against the host path, per user and k, on the fixture's quirk case and on the 120 x 300 split."""
    w, training, heldout, users, cols, relevant, seen, ref = rank_case(name)
    gap = GAP_FACTOR * BAR_FACTOR * float(fixture[f"{name}_dev"]) * np.abs(ref).max()
    fewest, exempt = nr.rank_conditions(ref, relevant, seen, gap)
    assert fewest >= 51
    host = neumf.rank_all_items(module_of(w), training, heldout, heldout[:, 0])
    dev = neumf.rank_all_items(module_of(w, engine.device), training, heldout, heldout[:, 0], engine)
    assert dev[0].shape == dev[1].shape == (6, len(users)) and dev[0].dtype == np.float64
    _compare_per_user(dev, host, exempt, len(users))
    if name == nr.QUIRK:
        np.testing.assert_allclose(dev[0], fixture["quirk_recall"], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(dev[1], fixture["quirk_ndcg"], rtol=0, atol=1e-12)
    # the twelve rounded means over ALL users, exempt ones included
    with np.errstate(invalid="ignore"):
        for d, h in zip(dev, host):
            diff = np.abs(np.round(np.nanmean(d, axis=1), 4) - np.round(np.nanmean(h, axis=1), 4)).max()
            print(name, "largest difference of a rounded mean", diff, "exempt users", exempt)
            assert diff <= 1e-4


@pytest.mark.gpu
def test_driver_through_the_engine(engine, fixture):
    """`compute_neuralcf_results(engine=..., epochs=2)` on the 40-user toy against `engine=None` under the same seed, the same torch
    training in both (on the CPU, where it is deterministic): finite figures, per-epoch validation losses within the loss bar, the same
    epochs kept, and final per-user figures equal under the ranking rule."""
    training, validation = toy()
    w, users, items, labels = nr.loss_inputs()
    want = nr.bce64(nr.forward64(w, users, items), labels)
    loss_bar = BAR_FACTOR * abs(float(fixture["loss_value"]) - want) / want
    hh, hd = {}, {}
    # seed 2: one of the seeds (2, 4, 7 of 1 .. 8) after whose two epochs no user's float64 scores hold a near-tie; 2 % of 40 users is none
    host = neumf.compute_neuralcf_results(training, validation, 40, 90, seed=2, epochs=2, device="cpu", history=hh)
    dev = neumf.compute_neuralcf_results(training, validation, 40, 90, engine=engine, seed=2, epochs=2, device="cpu", history=hd)
    assert np.isfinite(dev[0]).all() and np.isfinite(dev[1]).all()
    for a, b in zip(hd["valid_loss"], hh["valid_loss"]):
        print("validation loss: engine", a, "host", b, "relative", abs(a - b) / b, "bar", loss_bar)
        assert abs(a - b) / b <= loss_bar
    assert hd["best_epoch"] == hh["best_epoch"] and hd["epochs_run"] == hh["epochs_run"] == 2
    final = {k: v.detach().cpu().numpy() for k, v in hh["model"].state_dict().items()}
    users_r, cols, relevant, seen = nr.rank_problem(training, validation)
    ref = nr.scores64(final, users_r, cols)
    gap = GAP_FACTOR * BAR_FACTOR * float(fixture[f"{nr.QUIRK}_dev"]) * np.abs(ref).max()
    _, exempt = nr.rank_conditions(ref, relevant, seen, gap)
    assert not exempt, exempt          # the seed was picked for that
    _compare_per_user(hd["per_user"], hh["per_user"], exempt, len(users_r))
    assert np.abs(dev[0] - host[0]).max() <= 1e-4 and np.abs(dev[1] - host[1]).max() <= 1e-4
    # without the per-epoch ranking the epoch with the lowest validation loss is kept: the same training, so the same losses
    hl = {}
    neumf.compute_neuralcf_results(training, validation, 40, 90, engine=engine, seed=2, epochs=2, eval_recall=False, device="cpu", history=hl)
    assert hl["recall10"] == [] and hl["best_epoch"] == int(np.argmin(hh["valid_loss"]))
    assert all(abs(a - b) / b <= loss_bar for a, b in zip(hl["valid_loss"], hh["valid_loss"]))
