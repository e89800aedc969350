"""The rank-20 truncated-SVD evaluator on the device (csrc/svd_eval.h; sdrm_svd_fit / sdrm_svd_scores; pipeline.compute_mf_results_device).

References: tests/svd_eval_ref.py - the float64 oracle (exact SVD, exact rank-k reconstruction, host metrics) and a numpy restatement of
the device scheme.  The bar on a reconstruction is the project's 1e-4 normwise; measured values stand in the docstrings.

Bounds that are this file's own:
  * n_iter = 0 against the restatement fed the same q0: the two run the same arithmetic in the same number formats and differ in the
    order of their float32 sums (2^-24 relative per sum).  A perturbation of q0 of that size moves the restatement's reconstruction by
    0.9e-7 .. 2.9e-7 normwise on the four matrices here, so 1e-4 - the project's bar - holds with three orders of room.
  * orth(Y) against the restatement's orth of the same panel: CholeskyQR's factor is unique; rounding moves it by about cond(Y) 2^-24
    (cond <= 120 on these matrices: 7e-6), so 1e-4 again.
"""
import ctypes

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import svd_eval_ref as ref
from sdrm_amd import _lib, pipeline
from sdrm_amd.engine import Engine, SdrmError

BAR = 1e-4
U24 = 2.0 ** -24
SHAPE, ARG = -2, -1


def _ml100k_metrics(scores_of_valid_rows):
    combined, lo, held = ref.ml100k_stacked()
    return ref.per_user_metrics(scores_of_valid_rows, combined[lo:lo + held.shape[0]], held)


# ================================================================================================ CPU
@pytest.mark.parametrize("name", ["33x37", "70x61", "300x259", "ml100k"])
def test_restatement_matches_the_oracle(name):
    """float32 panels, float64 Gram / Cholesky / closing problem: 100 iterations reproduce the exact rank-k reconstruction to 0.8e-7 ..
    3.9e-7 normwise (two start panels each) and the singular values to 1.1e-7 relative; on the ML-100k fixture's stacked matrix
    (938 x 1008: sigma 20 / 21 = 16.34 / 16.19) all twelve rounded means are the oracle's."""
    a, k, (recon, sigma, _) = ref.case(name)
    for seed in (0, 1):
        v, s = ref.fit(a, k, 100, ref.start_panel(a.shape[1], seed))
        got = ref.scores(a, v)
        err, serr = ref.normwise(got, recon), float(np.abs(s / sigma - 1).max())
        print(f"{name} seed {seed}: reconstruction {err:.2e} normwise, singular values {serr:.2e} relative")
        assert err <= BAR and serr <= BAR
        if name == "ml100k":
            _, lo, held = ref.ml100k_stacked()
            rows = slice(lo, lo + held.shape[0])
            want, have = ref.rounded_means(*_ml100k_metrics(recon[rows])), ref.rounded_means(*_ml100k_metrics(got[rows]))
            assert want[0].tolist() == have[0].tolist() and want[1].tolist() == have[1].tolist(), (want, have)


def test_oracle_is_what_truncated_svd_converges_to():
    """The reference's evaluator, `TruncatedSVD(20, n_iter=100)` + inverse_transform(fit_transform(.)), against the oracle on the
    ML-100k stacked matrix: 5.7e-9 normwise as the issue measured (two seeds), identical per-user Recall / NDCG at all six k."""
    decomposition = pytest.importorskip("sklearn.decomposition")
    a, k, (recon, _, _) = ref.case("ml100k")
    dense = a.toarray()
    _, lo, held = ref.ml100k_stacked()
    rows = slice(lo, lo + held.shape[0])
    want = _ml100k_metrics(recon[rows])
    svd = decomposition.TruncatedSVD(n_components=k, n_iter=100, random_state=0)
    got = svd.inverse_transform(svd.fit_transform(dense))
    err = ref.normwise(got, recon)
    print(f"TruncatedSVD against the exact rank-{k} reconstruction: {err:.2e} normwise")
    assert err <= 1e-6
    have = _ml100k_metrics(got[rows])
    for w, h in zip(want, have):
        np.testing.assert_array_equal(w, h)


def test_refusals_need_no_device():
    """k + 10 > 32, k < 1 and min(m, n) < 32 are SDRM_ERR_SHAPE from the C side's own envelope check and from Engine.svd_fit before it
    calls anything; a null handle is SDRM_ERR_ARG."""
    lib = _lib.load()
    assert lib.sdrm_debug_svd_args(40, 40, 100, 20, 100) == 0 and lib.sdrm_debug_svd_args(32, 32, 0, 22, 0) == 0
    assert lib.sdrm_debug_svd_args(40, 40, 100, 23, 100) == SHAPE and lib.sdrm_debug_svd_args(40, 40, 100, 0, 100) == SHAPE
    assert lib.sdrm_debug_svd_args(31, 40, 100, 20, 100) == SHAPE and lib.sdrm_debug_svd_args(40, 31, 100, 20, 100) == SHAPE
    assert lib.sdrm_debug_svd_args(40, 40, -1, 20, 100) == SHAPE and lib.sdrm_debug_svd_args(40, 40, 100, 20, -1) == SHAPE
    assert lib.sdrm_debug_svd_args(2 ** 22 + 1, 40, 100, 20, 100) == SHAPE
    assert lib.sdrm_svd_fit(None, None, None, None, None, None, None, 40, 40, 100, 20, 100, 0, 0, None, None, None, None) == ARG
    assert lib.sdrm_svd_scores(None, None, None, None, 40, 100, None, 0, 4, 40, None, 20, None, None) == ARG
    assert len(_lib.SIGNATURES["sdrm_svd_fit"][1]) == 18 and len(_lib.SIGNATURES["sdrm_svd_scores"][1]) == 14

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    eng = Engine.__new__(Engine)       # the method's own checks, on the host: any call into the library fails the test
    eng.device, eng.lib, eng._h = torch.device("cpu"), NoLaunch(), None

    def forms(m):
        c = m.tocsc()
        shape = m.shape
        return ((torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int32)), None, shape),
                (torch.from_numpy(c.indptr.astype(np.int64)), torch.from_numpy(c.indices.astype(np.int32)), None, shape))
    ok = ref.planted(40, 40, 3, seed=1)
    for kw in (dict(n_components=23), dict(n_components=0), dict(n_iter=-1)):
        with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
            eng.svd_fit(*forms(ok), **kw)
    for small in (ref.planted(31, 40, 3, seed=2), ref.planted(40, 31, 3, seed=3)):
        with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
            eng.svd_fit(*forms(small))
    with pytest.raises(SdrmError, match="not one matrix"):
        eng.svd_fit(forms(ok)[0], forms(ref.planted(40, 41, 3, seed=1))[1])
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        eng.svd_scores(forms(ok)[0], torch.zeros(23, 40), row0=0, b=4)


class _HostEngine:
    """Stands in for the five Engine calls of pipeline.mf_per_user_device on the host, with the restatement behind them."""

    def __init__(self):
        self.calls = []

    def csr_to_device(self, m):
        m = m.tocsr()
        return (torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int32)), None, m.shape)

    def csc_to_device(self, m):
        c = m.tocsc()
        return (torch.from_numpy(c.indptr.astype(np.int64)), torch.from_numpy(c.indices.astype(np.int32)), None, m.shape)

    @staticmethod
    def _scipy(t):
        indptr, indices, _, shape = t
        indptr = indptr.numpy()
        return csr_matrix((np.ones(int(indptr[-1] - indptr[0])), indices.numpy()[indptr[0]:indptr[-1]], indptr - indptr[0]), shape=shape)

    def svd_fit(self, csr_dev, csc_dev, n_components=20, n_iter=100, seed=0, draw=0, q0=None):
        a = self._scipy(csr_dev)
        assert (self._scipy((csc_dev[0], csc_dev[1], None, csc_dev[3][::-1])).T != a).nnz == 0
        self.calls.append(("svd_fit", a.shape, n_components, n_iter, seed))
        return ref.fit(a, n_components, n_iter, ref.start_panel(a.shape[1], seed))

    def svd_scores(self, csr_dev, components, rows=None, row0=0, b=None, check=True):
        self.calls.append(("svd_scores", row0, b))
        return torch.from_numpy(ref.scores(self._scipy(csr_dev)[row0:row0 + b], components))

    def rank_metrics(self, scores, heldout, train=None, ks=(1,), row0=0):
        self.calls.append(("rank_metrics", tuple(scores.shape), tuple(ks)))
        assert tuple(ks) == pipeline.K_LIST and row0 == 0
        rec, ndcg = ref.per_user_metrics(scores.numpy(), self._scipy(train), self._scipy(heldout))
        return torch.from_numpy(rec), torch.from_numpy(ndcg)


def test_pipeline_stacks_splits_and_ranks_like_compute_mf_results():
    """compute_mf_results_device with the restatement behind the engine's calls gives the oracle's twelve rounded means on the ML-100k
    inputs: the same split, the same stacking, the validation users' rows and their mask - from sparse and from dense synthetic data."""
    train, valid, synthetic = ref.ml100k_inputs()
    _, _, (recon, _, _) = ref.case("ml100k")
    _, lo, held = ref.ml100k_stacked()
    want = ref.rounded_means(*_ml100k_metrics(recon[lo:lo + held.shape[0]]))
    for data in (synthetic, synthetic.toarray().astype(int)):
        eng = _HostEngine()
        got = pipeline.compute_mf_results_device(train, valid.copy(), data, eng, only_synthetic=True, seed=3)
        assert [c[0] for c in eng.calls] == ["svd_fit", "svd_scores", "rank_metrics"]
        assert eng.calls[0] == ("svd_fit", (lo + held.shape[0], train.shape[1]), 20, 100, 3) and eng.calls[1] == ("svd_scores", lo, held.shape[0])
        for w, g in zip(want, got):
            assert g.shape == (len(pipeline.K_LIST),) and w.tolist() == g.tolist(), (want, got)


def test_run_experiment_routes_the_three_evaluations(monkeypatch, tmp_path):
    """Without `device_svd` (or with it False) run_experiment makes today's three compute_mf_results calls; with it, all three tags go
    to compute_mf_results_device with the net's engine and the run's seed.  Nothing of it reaches train_SDRM."""
    from sdrm_amd import train_SDRM as ts
    import sdrm_amd.engine as engine_mod

    class Net:
        def engine(self):
            return "engine"

    class Vae:
        def sample(self, n):
            return "V"

    train_kw, calls = [], []
    monkeypatch.setattr(ts, "train_SDRM", lambda *a, **kw: (train_kw.append(set(kw)), (Net(), Vae()))[1])
    monkeypatch.setattr(ts, "sample_ddpm", lambda n, net, vae, latent, nd, timesteps=None, n_timesteps=None: torch.zeros(1) + (1 if timesteps else 2))
    monkeypatch.setattr(pipeline, "DeviceFeed", lambda *a, **k: "feed")
    monkeypatch.setattr(engine_mod, "utility_engine", lambda *a, **k: None)
    monkeypatch.setattr(pipeline, "equal_sparsity", lambda raw, sparsity, engine: ("bin", raw if isinstance(raw, str) else int(raw)))
    monkeypatch.setattr(pipeline, "compute_mf_results", lambda *a, **kw: calls.append(("host", a, kw)) or "host")
    monkeypatch.setattr(pipeline, "compute_mf_results_device", lambda *a, **kw: calls.append(("device", a, kw)) or "device")
    m = ref.planted(40, 40, 3, seed=1)
    hp = dict(batch=16, vae_hidden=16, latent=8, vae_batch=16, vae_lr=1e-3, H=1, lr=1e-3, epochs=1, T=5, nd=1.0)
    for extra in (dict(), dict(device_svd=False)):
        calls.clear()
        out = pipeline.run_experiment((m, m, m), dict(hp, **extra), 11, str(tmp_path))
        assert out == {"M": "host", "F": "host", "V": "host"}
        assert [(c[0], c[1][2], c[2]) for c in calls] == [("host", ("bin", 1), dict(only_synthetic=True)), ("host", ("bin", 2), dict(only_synthetic=True)),
                                                          ("host", ("bin", "V"), dict(only_synthetic=True))]
        assert all(c[1][0] is m and c[1][1] is m and len(c[1]) == 3 for c in calls)
    calls.clear()
    out = pipeline.run_experiment((m, m, m), dict(hp, device_svd=True), 11, str(tmp_path))
    assert out == {"M": "device", "F": "device", "V": "device"}
    assert [(c[0], c[1][2:], c[2]) for c in calls] == [("device", (("bin", tag), "engine"), dict(only_synthetic=True, seed=11)) for tag in (1, 2, "V")]
    assert train_kw[0] == train_kw[-1] and "device_svd" not in train_kw[-1] and "device_svd" not in pipeline.VAE_FLAGS


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def _stage_matrix(name):
    if name == "values2":
        return ref.planted(70, 61, 5, seed=9, value=2.0)
    return ref.planted_case(name)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("name", ["33x37", "70x61", "300x259", "values2"])
def test_stage_product_and_orthonormalisation(engine, name, transposed):
    """One product and one CholeskyQR2 on a caller's panel.  The product against scipy's in float64, elementwise within
    (r - 1) 2^-24 sum|terms| + 2^-24 |result| (r the row's entry count: any fixed summation order meets it); Y^T Y - I after the
    orthonormalisation at most 1e-5 in the largest element (measured on the MI355X: 1.3e-8 .. 5.5e-8 over the eight cases); the
    orthonormal panel against the restatement's of the same product; two runs the same bits.  70 x 61 has an empty row and an empty
    column, 300 x 259 a row and a column of ones (more entries than a gather chunk), "values2" stores 2.0."""
    a = _stage_matrix(name)
    op = a.T.tocsr() if transposed else a
    sp_dev = engine.csc_to_device(a) if transposed else engine.csr_to_device(a)
    assert (sp_dev[2] is not None) == (name == "values2")
    q = np.random.RandomState(11).standard_normal((op.shape[1], 32)).astype(np.float32)
    y, y_orth = engine.debug_svd_stage(sp_dev, q, transposed=transposed)
    y2, y_orth2 = engine.debug_svd_stage(sp_dev, q, transposed=transposed)
    assert torch.equal(y, y2) and torch.equal(y_orth, y_orth2)
    y, y_orth = y.cpu().numpy(), y_orth.cpu().numpy()
    q64 = q.astype(np.float64)
    want = op @ q64
    terms = abs(op) @ np.abs(q64)
    r = np.diff(op.indptr)[:, None]
    bound = np.maximum(r - 1, 0) * U24 * terms + U24 * np.abs(want)
    excess = np.abs(y.astype(np.float64) - want) - bound
    assert (excess <= 0).all(), (float(excess.max()), np.argwhere(excess > 0)[:4])
    assert (y[r[:, 0] == 0] == 0).all()
    gram = y_orth.astype(np.float64).T @ y_orth.astype(np.float64)
    off = float(np.abs(gram - np.eye(32)).max())
    err = ref.normwise(y_orth, ref.orth(y).astype(np.float64))
    print(f"{name} {'csc' if transposed else 'csr'}: |Y^T Y - I|_max = {off:.2e}, orth(Y) against the restatement {err:.2e}")
    assert off <= 1e-5
    assert err <= BAR


def _reconstruction(engine, csr_dev, components):
    return engine.svd_scores(csr_dev, components, row0=0, b=csr_dev[3][0]).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["33x37", "70x61", "300x259"])
def test_fit_against_the_restatement_and_the_oracle(engine, name):
    """sdrm_svd_fit + sdrm_svd_scores of all rows.  n_iter = 0 with an explicit q0 against the restatement fed the same q0; n_iter = 100
    from that q0 and from the Philox start panel against the exact rank-k reconstruction, 1e-4 normwise, singular values 1e-4 relative
    (measured on the MI355X: 0.8e-7 .. 2.0e-7 and at most 4.4e-8; the n_iter = 0 fits equal the restatement's to the last bit of the
    reconstruction - with all-ones data the two products add the same numbers in the same order)."""
    a, k, (recon, sigma, _) = ref.case(name)
    csr_dev, csc_dev = engine.csr_to_device(a), engine.csc_to_device(a)
    q0 = ref.start_panel(a.shape[1], 4)
    v, s = engine.svd_fit(csr_dev, csc_dev, n_components=k, n_iter=0, q0=q0)
    assert tuple(v.shape) == (k, a.shape[1]) and v.dtype == torch.float32 and s.shape == (k,) and (np.diff(s) <= 0).all()
    v_ref, s_ref = ref.fit(a, k, 0, q0)
    err0 = ref.normwise(_reconstruction(engine, csr_dev, v), ref.scores(a, v_ref).astype(np.float64))
    print(f"{name}: n_iter = 0 against the restatement {err0:.2e} normwise, singular values {np.abs(s / s_ref - 1).max():.2e}")
    assert err0 <= BAR and np.abs(s / s_ref - 1).max() <= BAR
    for label, kw in (("q0", dict(q0=q0)), ("philox", dict(seed=5, draw=1))):
        v, s = engine.svd_fit(csr_dev, csc_dev, n_components=k, n_iter=100, **kw)
        err, serr = ref.normwise(_reconstruction(engine, csr_dev, v), recon), float(np.abs(s / sigma - 1).max())
        print(f"{name} {label}: n_iter = 100 against the oracle {err:.2e} normwise, singular values {serr:.2e} relative")
        assert err <= BAR and serr <= BAR
        rows = np.linalg.norm(v.cpu().numpy().astype(np.float64), axis=1)
        assert np.abs(rows - 1).max() <= 1e-6
    v2, s2 = engine.svd_fit(csr_dev, csc_dev, n_components=k, n_iter=100, seed=5, draw=1)
    assert torch.equal(v, v2) and s.tobytes() == s2.tobytes()          # the same bits from call to call


@pytest.fixture(scope="module")
def fitted(engine):
    a, k, _ = ref.case("300x259")
    csr_dev = engine.csr_to_device(a)
    v, _ = engine.svd_fit(csr_dev, engine.csc_to_device(a), n_components=k, n_iter=2, seed=1)
    return a, csr_dev, v, _reconstruction(engine, csr_dev, v)


@pytest.mark.gpu
def test_scores_of_row_batches(engine, fitted):
    """An explicit row list (out of order, one row twice), row0 / b, and batches that are no multiple of the kernel's row tile of 16:
    a row's scores are the same bits wherever it sits, and they are the float32 restatement's to rounding."""
    a, csr_dev, v, full = fitted
    assert ref.normwise(full, ref.scores(a, v.cpu().numpy()).astype(np.float64)) <= 1e-5
    rows = np.array([299, 0, 17, 17, 1, 150, 33], dtype=np.int64)
    got = engine.svd_scores(csr_dev, v, rows=torch.from_numpy(rows)).cpu().numpy()
    assert got.shape == (7, 259) and got.tobytes() == full[rows].tobytes()
    for row0, b in ((0, 1), (5, 16), (13, 37), (283, 17)):
        got = engine.svd_scores(csr_dev, v, row0=row0, b=b).cpu().numpy()
        assert got.tobytes() == full[row0:row0 + b].tobytes(), (row0, b)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.svd_scores(csr_dev, v, row0=290, b=11)                   # ends behind the matrix: refused on the host


@pytest.mark.gpu
def test_scores_range_checks(engine, fitted):
    """A row id outside the matrix and a column index outside it raise the feed status word; the row, and the row whose only entry is
    the bad one, come back all zeros, and their neighbours are untouched."""
    a, csr_dev, v, full = fitted
    rows = torch.tensor([3, 300, -1, 5], dtype=torch.int64)
    got = engine.svd_scores(csr_dev, v, rows=rows, check=False)
    with pytest.raises(SdrmError, match="row id"):
        engine.feed_status()
    got = got.cpu().numpy()
    assert (got[1] == 0).all() and (got[2] == 0).all()
    assert got[0].tobytes() == full[3].tobytes() and got[3].tobytes() == full[5].tobytes()
    engine.feed_status()                                                # cleared
    small = csr_matrix((np.ones(5), np.array([2, 200, 7, 9, 258]), np.array([0, 2, 3, 5])), shape=(3, 259))
    bad = engine.csr_to_device(small)
    bad[1][2] = 259                                                     # row 1's only entry, one behind the last column
    got = engine.svd_scores(bad, v, row0=0, b=3, check=False)
    with pytest.raises(SdrmError, match="column index"):
        engine.feed_status()
    got = got.cpu().numpy()
    want = ref.scores(small, v.cpu().numpy())
    assert (got[1] == 0).all() and np.abs(got[[0, 2]] - want[[0, 2]]).max() <= 1e-5 * np.abs(want).max()
    bad[0][3] = 7                                                       # an indptr pair that reaches behind the index array
    got = engine.svd_scores(bad, v, row0=0, b=3, check=False)
    with pytest.raises(SdrmError, match="indptr"):
        engine.feed_status()
    assert (got.cpu().numpy()[2] == 0).all()


@pytest.mark.gpu
def test_ml100k_device_evaluator_against_the_host_one(engine, monkeypatch):
    """pipeline.compute_mf_results_device against pipeline.compute_mf_results on the ML-100k inputs.  Per user and k, Recall and NDCG
    against those of the oracle's scores: a (user, k) pair may be left out only where the oracle's score gap at that cut-off is below
    1e-5 of the row's largest score, at most 2 % of the pairs may be, and every other pair is equal.  The rounded means may differ from
    the oracle's and from compute_mf_results' by one left-out pair's weight.  (The restatement on the CPU left out 0 of 570 and
    differed in none; on the MI355X 2 of the 570 pairs are such close calls and none differs.)"""
    train, valid, synthetic = ref.ml100k_inputs()
    combined, lo, held = ref.ml100k_stacked()
    users = held.shape[0]
    _, _, (recon, _, _) = ref.case("ml100k")
    oracle_scores = recon[lo:lo + users]
    want = _ml100k_metrics(oracle_scores)
    got = pipeline.mf_per_user_device(train, valid.copy(), synthetic, engine, only_synthetic=True, seed=0)
    masked = np.array(oracle_scores)
    masked[combined[lo:lo + users].nonzero()] = -np.inf
    ranked = -np.sort(-masked, axis=1)
    top = np.abs(oracle_scores).max(axis=1)
    close_call = np.stack([(ranked[:, k - 1] - ranked[:, k]) < 1e-5 * top for k in pipeline.K_LIST])      # [6, users]
    differs = np.zeros_like(close_call)
    for w, g in zip(want, got):
        assert g.shape == w.shape == (len(pipeline.K_LIST), users)
        differs |= ~np.isclose(w, g, rtol=0, atol=1e-12, equal_nan=True)
    print(f"ML-100k: {int(close_call.sum())} of {close_call.size} (user, k) pairs are close calls, {int(differs.sum())} differ")
    assert not (differs & ~close_call).any(), np.argwhere(differs & ~close_call)[:5]
    assert differs.sum() <= 0.02 * differs.size
    slack = (differs.any(axis=1) / users) + 1e-12
    means = pipeline.compute_mf_results_device(train, valid.copy(), synthetic, engine, only_synthetic=True, seed=0)
    oracle_means = ref.rounded_means(*want)
    decomposition = pytest.importorskip("sklearn.decomposition")
    real = decomposition.TruncatedSVD
    monkeypatch.setattr(decomposition, "TruncatedSVD", lambda **kw: real(random_state=0, **kw))
    host_means = pipeline.compute_mf_results(train, valid.copy(), synthetic, only_synthetic=True)
    for m, o, h in zip(means, oracle_means, host_means):
        assert m.shape == (len(pipeline.K_LIST),)
        assert (np.abs(m - o) <= slack + (1e-4 * (slack > 1e-9))).all(), (m, o)
        assert (np.abs(m - h) <= slack + (1e-4 * (slack > 1e-9))).all(), (m, h)


@pytest.mark.gpu
def test_refusals_and_breakdown(engine):
    """k = 23 and a matrix of 31 rows are SDRM_ERR_SHAPE from the library itself; a 40 x 40 matrix of rank 5 breaks the panel's
    factorisation down and the fit raises; the next fit on the same engine matches the oracle."""
    a, k, (recon, sigma, _) = ref.case("33x37")
    csr_dev, csc_dev = engine.csr_to_device(a), engine.csc_to_device(a)
    out, sig = torch.zeros(23, 37, device=engine.device), np.zeros(23)

    def raw(m, n, kk, forms):
        (ip, ix, _, _), (cp, cx, _, _) = forms
        return engine.lib.sdrm_svd_fit(engine._h, ip.data_ptr(), ix.data_ptr(), None, cp.data_ptr(), cx.data_ptr(), None, m, n, int(ix.numel()), kk, 1, 0, 0,
                                       None, out.data_ptr(), sig.ctypes.data_as(ctypes.c_void_p), None)
    launches = engine.launch_count()
    assert raw(33, 37, 23, (csr_dev, csc_dev)) == SHAPE and raw(33, 37, 0, (csr_dev, csc_dev)) == SHAPE
    small = ref.planted(31, 40, 3, seed=2)
    assert raw(31, 40, 3, (engine.csr_to_device(small), engine.csc_to_device(small))) == SHAPE
    assert engine.launch_count() == launches and not out.any()           # refused before any launch
    rng = np.random.RandomState(0)
    low = csr_matrix((rng.random_sample((40, 5)) < 0.5).astype(np.float64) @ (rng.random_sample((5, 40)) < 0.5).astype(np.float64))
    assert np.linalg.matrix_rank(low.toarray()) == 5
    for _ in range(2):
        with pytest.raises(SdrmError, match="breakdown"):
            engine.svd_fit(engine.csr_to_device(low), engine.csc_to_device(low), n_components=3, n_iter=3, seed=1)
    with pytest.raises(SdrmError, match="breakdown"):
        engine.debug_svd_stage(engine.csr_to_device(low), np.random.RandomState(1).standard_normal((40, 32)).astype(np.float32))
    v, s = engine.svd_fit(csr_dev, csc_dev, n_components=k, n_iter=100, seed=2)
    assert np.isfinite(v.cpu().numpy()).all()
    assert ref.normwise(_reconstruction(engine, csr_dev, v), recon) <= BAR and np.abs(s / sigma - 1).max() <= BAR
