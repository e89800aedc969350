"""The NMF evaluator on the device (csrc/nmf.h; sdrm_nmf_fit / sdrm_nmf_init / sdrm_nmf_scores; pipeline.compute_mf_results_device(nnmf=True)).

The parity claim has three parts (tests/nmf_ref.py, tests/golden/make_nmf_golden.py):
  * the SOLVER is held to sklearn's own W, H and n_iter_ from the same start, at SOLVER_BAR;
  * the START is held to the restatement of `_initialize_nmf` fed the device's own truncated SVD, at INIT_BAR;
  * the END-TO-END metrics are held to the spread of sklearn's NMF over the random draws of its start.

About that spread.  The reference's `compute_mf_results` reseeds numpy's global generator itself - its hold-out split calls
np.random.seed(123) - so under np.random.seed(0 .. 7) its eight results are ONE result (the fixture's ref_recall / ref_ndcg, eight equal
rows).  What varies the start of sklearn's NMF is the generator its randomized SVD draws from: the fixture's seed_recall / seed_ndcg are
the same chain with `NMF(random_state=RandomState(s))`, s = 0 .. 7, unrounded, and their mean and standard deviation (ddof 1) are what
test (b) below is held to.  Measured where the fixture was made: Recall@{1,3,5,10,20,50} mean .5329 .4588 .3984 .3610 .3699 .4892, std
.0096 .0031 .0043 .0017 .0034 .0033; NDCG std .0096 .0021 .0031 .0016 .0018 .0013."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import nmf_ref as nr
import svd_eval_ref as sr
from sdrm_amd import pipeline
from sdrm_amd.engine import Engine, SdrmError

SHAPE, ARG = -2, -1
# 100 x the largest normwise deviation of nmf_ref.fit(reverse=True) from sklearn over the eight solver cases, measured on the CPU by
# make_nmf_golden.py: 1.81e-13 (70x45_ones; the unreversed restatement gives sklearn's bits there); capped at 1e-10
SOLVER_BAR = min(100 * 1.81e-13, 1e-10)
# 10 x the deviation of nmf_ref's NNDSVDa in float64 from the same with U rounded through float32, on the 70 x 45 all-ones case with the exact
# SVD's float32 components, measured on the CPU: 1.94e-8 in W (3.4e-9 in H)
INIT_BAR = 10 * 1.94e-8


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def _device_fit(engine, name, **kw):
    x, w0, h0, max_iter, tol = nr.solver_inputs(name)
    csr_dev, csc_dev = engine.csr_to_device(x), engine.csc_to_device(x)
    assert (csr_dev[2] is not None) == bool((x.data != 1).any())       # the all-ones form travels without values
    assert name.endswith("_values") <= (csr_dev[2] is not None)
    return engine.nmf_fit(csr_dev, csc_dev, n_components=w0.shape[1], max_iter=max_iter, tol=tol, init=(w0, h0), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(nr.SOLVER_CASES))
def test_solver_against_sklearn_from_a_custom_start(engine, name):
    """W, H and n_iter against the fixture's (sklearn, init='custom').  70 x 45: rows no multiple of any tile, more than one work-group
    of the product; 300 x 33, k = 16: the full stride, two work-groups of the sweep; 33 x 129, k = 3.  Values given and all ones;
    70x45_ones has an empty row and an empty column; 70x45_zero4 starts with component 4 zero in W0 and H0, so H H^T[4][4] == 0 and
    the coordinate must stay 0."""
    x, w0, h0, max_iter, tol = nr.solver_inputs(name)
    fx = nr.fixture()
    w, h, n_iter, violations = _device_fit(engine, name)
    assert w.dtype == h.dtype == torch.float64 and tuple(w.shape) == w0.shape and tuple(h.shape) == h0.shape
    w, h = w.cpu().numpy(), h.cpu().numpy()
    ew, eh = nr.normwise(w, fx[f"{name}_W"]), nr.normwise(h, fx[f"{name}_H"])
    print(f"{name}: n_iter {n_iter}, W {ew:.2e}, H {eh:.2e} normwise against sklearn (bar {SOLVER_BAR:.2e})")
    assert n_iter == int(fx[f"{name}_n_iter"]) and violations.shape == (n_iter,)
    assert ew <= SOLVER_BAR and eh <= SOLVER_BAR
    assert (w >= 0).all() and (h >= 0).all()
    if name == "70x45_zero4":
        assert not w[:, 4].any() and not h[4].any()
    if name == "70x45_ones":
        assert x.getnnz(axis=1)[1] == 0 and x.getnnz(axis=0)[2] == 0


@pytest.mark.gpu
def test_early_stop_on_the_device(engine):
    """A 64 x 40 matrix of exact non-negative rank 3, k = 3, a start near the factors, tol = 1e-2, max_iter = 50: sklearn stops at
    2 <= n_iter_ < 50 with v_i / v_1 at least 1.5 x under tol there and at least 1.5 x above it one iteration earlier (asserted by the
    generator and by tests/test_nmf_host.py).  The device stops at the same iteration, its factors meet the solver's bar - the launches
    queued behind the stop wrote nothing -, and its violations are the restatement's to 1e-9 relative."""
    name = nr.EARLY
    x, w0, h0, max_iter, tol = nr.solver_inputs(name)
    fx = nr.fixture()
    want_iter = int(fx[f"{name}_n_iter"])
    assert 2 <= want_iter < max_iter
    launches = engine.launch_count()
    w, h, n_iter, violations = _device_fit(engine, name)
    assert engine.launch_count() - launches == 5 * max_iter          # the whole fit was queued; the stop is the device's
    _, _, ref_iter, ref_viol = nr.fit(x, w0, h0, max_iter, tol)
    assert n_iter == want_iter == ref_iter
    ew, eh = nr.normwise(w.cpu().numpy(), fx[f"{name}_W"]), nr.normwise(h.cpu().numpy(), fx[f"{name}_H"])
    rel = np.abs(violations / ref_viol - 1).max()
    print(f"{name}: n_iter {n_iter}, W {ew:.2e}, H {eh:.2e} normwise, violations {rel:.2e} relative")
    assert ew <= SOLVER_BAR and eh <= SOLVER_BAR
    assert violations.shape == ref_viol.shape and rel <= 1e-9


@pytest.mark.gpu
def test_two_fits_give_the_same_bytes(engine):
    a = _device_fit(engine, "70x45_values")
    b = _device_fit(engine, "70x45_values")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3].tobytes() == b[3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["70x45_ones", "70x45_values"])
def test_init_against_the_restated_nndsvda(engine, name):
    """nmf_init against nmf_ref's NNDSVDa fed the device's own components and singular values (U = X V^T / sigma in float64 from the
    float32 V, as the device forms it).  Every entry is positive, and the entries the oracle fills with the mean equal X.mean() exactly."""
    x, _, _, _, _ = nr.solver_inputs(name)
    csr_dev, csc_dev = engine.csr_to_device(x), engine.csc_to_device(x)
    w0, h0 = engine.nmf_init(csr_dev, csc_dev, n_components=15, seed=3)
    # the factors nmf_init made its start from: the same fit again (the same bits on every call); 15 >= 0.1 x 45, so 'auto' is 4 iterations
    components, sigma = engine.svd_fit(csr_dev, csc_dev, n_components=15, n_iter=4, seed=3)
    assert tuple(w0.shape) == (70, 15) and tuple(h0.shape) == (15, 45) and w0.dtype == h0.dtype == torch.float64
    w0, h0 = w0.cpu().numpy(), h0.cpu().numpy()
    want_w, want_h = nr.nndsvda_from_components(x, components.cpu().numpy(), sigma)
    ew, eh = nr.normwise(w0, want_w), nr.normwise(h0, want_h)
    print(f"{name}: W0 {ew:.2e}, H0 {eh:.2e} normwise against the restated NNDSVDa (bar {INIT_BAR:.2e})")
    assert ew <= INIT_BAR and eh <= INIT_BAR
    assert (w0 > 0).all() and (h0 > 0).all()
    mean = nr.x_mean(x)
    assert (want_w == mean).any() and (want_h == mean).any()
    assert (w0[want_w == mean] == mean).all() and (h0[want_h == mean] == mean).all()


@pytest.mark.gpu
def test_scores_are_rounded_once(engine):
    """nmf_scores within 1 float32 ulp of np.float32(W[rows] @ H) computed in float64, for a row list (out of order, one row twice) and
    for a row0 range; n_items = 257 (two column blocks, the second with one column), batches that are no multiple of the row tile."""
    rng = np.random.RandomState(5)
    w, h = rng.random_sample((300, 15)) * 3, rng.random_sample((15, 257)) * 3
    full = w @ h
    rows = np.array([299, 0, 17, 17, 1, 150, 33], dtype=np.int64)
    for got, want in ((engine.nmf_scores(w, h, rows=torch.from_numpy(rows)), full[rows]), (engine.nmf_scores(w, h, row0=13, b=37), full[13:50]),
                      (engine.nmf_scores(torch.from_numpy(w), torch.from_numpy(h)), full)):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        got, want32 = got.cpu().numpy(), want.astype(np.float32)
        ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
        print(f"nmf_scores {want.shape}: at most {ulps.max():.1f} ulp from the float64 product rounded once, {(ulps > 0).mean():.2%} of the elements off it")
        assert ulps.max() <= 1.0
    got = engine.nmf_scores(w, h, rows=torch.tensor([3, 300, -1, 5]), check=False)
    with pytest.raises(SdrmError, match="row id"):
        engine.feed_status()
    got = got.cpu().numpy()
    assert (got[1] == 0).all() and (got[2] == 0).all() and np.abs(got[0] - full[3]).max() <= 1e-5 and np.abs(got[3] - full[5]).max() <= 1e-5


@pytest.mark.gpu
def test_refusals_and_range_checks(engine):
    """k = 17 and max_iter = 0 are SDRM_ERR_SHAPE from the library before any launch; a column index outside the matrix and an indptr pair
    out of order raise the feed status word without a fault; nmf_init refuses a 20 x 40 matrix (svd_fit's panel); and the next fit on
    the same engine is sklearn's."""
    name = "70x45_ones"
    x, w0, h0, max_iter, tol = nr.solver_inputs(name)
    csr_dev, csc_dev = engine.csr_to_device(x), engine.csc_to_device(x)
    w = torch.zeros(70, 16, dtype=torch.float64, device=engine.device)
    ht = torch.zeros(45, 16, dtype=torch.float64, device=engine.device)
    tail = torch.zeros(64, dtype=torch.float64, device=engine.device)

    def raw(k, iters, tol_=1e-4):
        (ip, ix, _, _), (cp, cx, _, _) = csr_dev, csc_dev
        return engine.lib.sdrm_nmf_fit(engine._h, ip.data_ptr(), ix.data_ptr(), None, cp.data_ptr(), cx.data_ptr(), None, 70, 45, int(ix.numel()), k, iters,
                                       tol_, w.data_ptr(), ht.data_ptr(), tail.data_ptr() + 8 * 60, tail.data_ptr(), None)
    launches = engine.launch_count()
    assert raw(17, 50) == SHAPE and raw(0, 50) == SHAPE and raw(15, 0) == SHAPE and raw(15, 10001) == SHAPE and raw(15, 50, -1.0) == SHAPE
    assert engine.launch_count() == launches and not w.any() and not tail.any()
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.nmf_fit(csr_dev, csc_dev, n_components=17, init=(np.ones((70, 17)), np.ones((17, 45))))
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.nmf_fit(csr_dev, csc_dev, n_components=15, max_iter=0, init=(w0, h0))
    bad = engine.csr_to_device(x)
    bad[1][5] = 45                                                      # one behind the last column
    with pytest.raises(SdrmError, match="column index"):
        engine.nmf_fit(bad, csc_dev, n_components=15, max_iter=2, init=(w0, h0))
    bad = engine.csr_to_device(x)
    bad[0][7] = bad[0][6] - 1                                           # an indptr pair out of order (rows 6 and 7)
    with pytest.raises(SdrmError, match="indptr"):
        engine.nmf_fit(bad, csc_dev, n_components=15, max_iter=2, init=(w0, h0))
    engine.feed_status()                                                # cleared
    small = csr_matrix((np.random.RandomState(0).random_sample((20, 40)) < 0.4).astype(np.float64))
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.nmf_init(engine.csr_to_device(small), engine.csc_to_device(small), n_components=3)
    fx = nr.fixture()
    got = _device_fit(engine, name)
    assert got[2] == int(fx[f"{name}_n_iter"]) and nr.normwise(got[0].cpu().numpy(), fx[f"{name}_W"]) <= SOLVER_BAR


# ------------------------------------------------------------------------------------------------ end to end, ML-100k fixture
@pytest.fixture(scope="module")
def ml100k_seed0(engine):
    train, valid, synthetic = sr.ml100k_inputs()
    return pipeline.mf_per_user_device(train, valid.copy(), synthetic, engine, only_synthetic=True, seed=0, nnmf=True)


@pytest.mark.gpu
def test_ml100k_per_user_figures_against_the_oracle_chain(engine, ml100k_seed0):
    """(a) mf_per_user_device(nnmf=True) against the oracle chain - nmf_ref.fit from the device's own start, float64 scores, the host
    metrics: at most 2 of the 95 users may differ in any entry (a float32 tie at a cut-off is the only allowed cause; the CPU check
    found 0, even with the whole fit in float32)."""
    combined, lo, held = sr.ml100k_stacked()
    users = held.shape[0]
    w0, h0 = engine.nmf_init(engine.csr_to_device(combined), engine.csc_to_device(combined), n_components=15, seed=0)
    w, h, n_iter, _ = nr.fit(combined, w0.cpu().numpy(), h0.cpu().numpy(), max_iter=50, tol=1e-4)
    want = sr.per_user_metrics((w @ h)[lo:lo + users], combined[lo:lo + users], held)
    differs = np.zeros(users, dtype=bool)
    for wnt, got in zip(want, ml100k_seed0):
        assert got.shape == wnt.shape == (len(pipeline.K_LIST), users)
        differs |= ~np.isclose(wnt, got, rtol=0, atol=1e-12, equal_nan=True).all(axis=0)
    print(f"ML-100k, NMF: oracle n_iter {n_iter}; {int(differs.sum())} of {users} users differ from the oracle chain in some entry")
    assert users == 95 and differs.sum() <= 2


@pytest.mark.gpu
def test_ml100k_means_lie_within_the_references_seed_spread(engine, ml100k_seed0):
    """(b) engine seeds 0 .. 4: for each of the 12 metrics the mean over the seeds lies within 3 fixture standard deviations of the
    fixture's mean over the 8 seeds of sklearn's start (module docstring: which spread that is)."""
    train, valid, synthetic = sr.ml100k_inputs()
    fx = nr.fixture()
    runs = [ml100k_seed0] + [pipeline.mf_per_user_device(train, valid.copy(), synthetic, engine, only_synthetic=True, seed=s, nnmf=True) for s in range(1, 5)]
    for which, key in ((0, "seed_recall"), (1, "seed_ndcg")):
        means = np.stack([np.nanmean(r[which], axis=1) for r in runs]).mean(axis=0)
        ref_mean, ref_std = fx[key].mean(axis=0), fx[key].std(axis=0, ddof=1)
        print(f"{key}: device mean over 5 seeds {np.round(means, 4)}, reference mean {np.round(ref_mean, 4)}, std {np.round(ref_std, 4)}, "
              f"distance in std {np.round(np.abs(means - ref_mean) / ref_std, 2)}")
        assert (ref_std > 0).all()
        assert (np.abs(means - ref_mean) <= 3 * ref_std).all()
    rounded = pipeline.compute_mf_results_device(train, valid.copy(), synthetic, engine, only_synthetic=True, seed=0, nnmf=True)
    for which in (0, 1):
        assert rounded[which].tolist() == [np.round(np.nanmean(r), 4) for r in ml100k_seed0[which]]


@pytest.mark.gpu
def test_ml100k_resident_route_equals_the_uploaded_one(engine, ml100k_seed0):
    """(c) the stack and the CSC form made on the device give the uploaded route's figures bit for bit."""
    train, valid, synthetic = sr.ml100k_inputs()
    got = pipeline.mf_per_user_resident(train, valid.copy(), engine.csr_to_device(synthetic), engine, only_synthetic=True, seed=0, nnmf=True)
    for a, b in zip(got, ml100k_seed0):
        assert a.tobytes() == b.tobytes()
