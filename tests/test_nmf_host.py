"""The NMF evaluator's host side (csrc/nmf.h; sdrm_nmf_fit / sdrm_nmf_init / sdrm_nmf_scores): what needs no GPU - the numpy
restatement of tests/nmf_ref.py against sklearn's own results and sklearn's own start, the C ABI's declarations, and the routing of
`nnmf=True` through sdrm_amd/pipeline.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import nmf_ref as nr
from sdrm_amd import _lib, pipeline

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdrm_nmf_fit", "sdrm_nmf_init", "sdrm_nmf_scores")
SHAPE, ARG = -2, -1


@pytest.mark.parametrize("name", list(nr.SOLVER_CASES) + [nr.EARLY])
def test_restatement_matches_sklearn_on_every_solver_case(name):
    """nmf_ref.fit from the case's start against the W, H and n_iter_ that `NMF(init='custom')` left in the fixture.  Where the fixture
    was generated the restatement gave sklearn's bits (0.0 normwise on all eight cases); 1e-12 leaves room for another BLAS's order of
    the dense products (reversing every sum moves the result by at most 1.8e-13, make_nmf_golden.py)."""
    x, w0, h0, max_iter, tol = nr.solver_inputs(name)
    fx = nr.fixture()
    # the inputs rebuilt from the seed are the ones sklearn was given
    assert np.array_equal(x.toarray(), fx[f"{name}_X"]) and np.array_equal(w0, fx[f"{name}_W0"]) and np.array_equal(h0, fx[f"{name}_H0"])
    w, h, n_iter, violations = nr.fit(x, w0, h0, max_iter, tol)
    assert n_iter == int(fx[f"{name}_n_iter"]) and violations.shape == (n_iter,)
    assert nr.normwise(w, fx[f"{name}_W"]) <= 1e-12 and nr.normwise(h, fx[f"{name}_H"]) <= 1e-12
    if name == "70x45_zero4":     # H H^T[4][4] == 0: the coordinate is never moved
        assert not w[:, 4].any() and not h[4].any() and not fx[f"{name}_W"][:, 4].any()
    if name == nr.EARLY:
        assert 2 <= n_iter < max_iter
        ratio = violations / violations[0]
        assert ratio[n_iter - 1] * 1.5 <= tol and ratio[n_iter - 2] >= 1.5 * tol


def test_restated_nndsvda_matches_sklearns_start():
    """nmf_ref.nndsvda fed the exact truncated SVD against `_initialize_nmf(init='nndsvda')` on a 60 x 48 non-negative matrix of exact
    rank 20 with k = 15: sklearn's randomized SVD with its 10 oversampling columns spans the whole range there and is exact, and the
    signs it flips do not matter to NNDSVD."""
    nmf = pytest.importorskip("sklearn.decomposition._nmf")
    rng = np.random.RandomState(3)
    x = rng.random_sample((60, 20)) @ rng.random_sample((20, 48))
    assert np.linalg.matrix_rank(x) == 20
    k = 15
    u, s, vt = np.linalg.svd(x, full_matrices=False)
    w, h = nr.nndsvda(csr_matrix(x), u[:, :k], s[:k], vt[:k])
    w_sk, h_sk = nmf._initialize_nmf(x, k, init="nndsvda", random_state=0)
    assert (w > 0).all() and (h > 0).all()
    assert nr.normwise(w, w_sk) <= 1e-9 and nr.normwise(h, h_sk) <= 1e-9
    filled = w_sk == x.mean()
    assert filled.any() and ((w == x.mean()) == filled).all()     # the same entries were below eps and took the mean
    # from the right factor alone, as the device does it: U = X V^T / sigma
    w2, h2 = nr.nndsvda_from_components(csr_matrix(x), vt[:k].astype(np.float32), s[:k])
    assert nr.normwise(w2, w_sk) <= 1e-5 and nr.normwise(h2, h_sk) <= 1e-5


def test_reversed_sums_are_the_same_mathematics():
    """The flag the GPU bars are derived from: reversing every product's summation order moves the result at rounding level only."""
    x, w0, h0, max_iter, tol = nr.solver_inputs("33x129_values")
    a, b = nr.fit(x, w0, h0, 10, tol), nr.fit(x, w0, h0, 10, tol, reverse=True)
    dev = max(nr.normwise(b[0], a[0]), nr.normwise(b[1], a[1]))
    assert 0 < dev <= 1e-12, dev


def test_cabi_declares_and_binds_the_three_entry_points():
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/sdrm_hip.h"
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), params)
        assert hasattr(lib, name)
    # no engine: refused before anything is touched
    assert lib.sdrm_nmf_fit(None, None, None, None, None, None, None, 4, 4, 4, 3, 5, 1e-4, None, None, None, None, None) == ARG
    assert lib.sdrm_nmf_init(None, None, None, None, 4, 4, 4, 3, None, None, None, None, None) == ARG
    assert lib.sdrm_nmf_scores(None, None, None, 4, 3, None, 0, 4, 4, None, None) == ARG


def test_pipeline_routes_nnmf():
    """`nnmf=False` is the default of all five functions; with nnmf=True the device routes call `nmf_fit` / `nmf_scores` (never
    `svd_fit` directly), and `run_experiment` hands `hp["nmf"]` to the device routes."""
    import inspect
    for fn in (pipeline.compute_mf_results, pipeline.mf_per_user_device, pipeline.compute_mf_results_device, pipeline.mf_per_user_resident,
               pipeline.compute_mf_results_resident):
        assert inspect.signature(fn).parameters["nnmf"].default is False, fn.__name__

    calls = []

    class FakeEngine:
        def csr_to_device(self, m):
            return ("csr", m.shape)

        def csc_to_device(self, m):
            return ("csc", m.shape)

        def svd_fit(self, *a, **kw):
            raise AssertionError("nnmf=True must not run the SVD evaluator")

        def nmf_fit(self, csr_dev, csc_dev, **kw):
            calls.append(("nmf_fit", kw))
            raise StopIteration

    import svd_eval_ref as sr
    train, valid, synthetic = sr.ml100k_inputs()
    with pytest.raises(StopIteration):
        pipeline.mf_per_user_device(train, valid.copy(), synthetic, FakeEngine(), only_synthetic=True, seed=3, nnmf=True)
    assert calls == [("nmf_fit", dict(n_components=15, max_iter=50, seed=3))]


def test_run_experiment_hands_nmf_to_the_device_routes(monkeypatch, tmp_path):
    """`hp["nmf"]` reaches compute_mf_results_device and compute_mf_results_resident as nnmf=True; the host route and an `hp` without
    the key make the calls they always made."""
    import torch
    from sdrm_amd import train_SDRM as ts
    import sdrm_amd.engine as engine_mod

    class Eng:
        def equal_sparsity_csr(self, raw, sparsity):
            return "csr"

    eng = Eng()

    class Net:
        def engine(self):
            return eng

    class Vae:
        def sample(self, n):
            return "V"

    calls = []
    monkeypatch.setattr(ts, "train_SDRM", lambda *a, **kw: (Net(), Vae()))
    monkeypatch.setattr(ts, "sample_ddpm", lambda *a, **kw: torch.zeros(1))
    monkeypatch.setattr(pipeline, "DeviceFeed", lambda *a, **k: "feed")
    monkeypatch.setattr(engine_mod, "utility_engine", lambda *a, **k: None)
    monkeypatch.setattr(pipeline, "equal_sparsity", lambda raw, sparsity, engine: "bin")
    for route in ("compute_mf_results", "compute_mf_results_device", "compute_mf_results_resident"):
        monkeypatch.setattr(pipeline, route, lambda *a, _r=route, **kw: calls.append((_r, kw)))
    m = csr_matrix(np.eye(40))
    hp = dict(batch=16, vae_hidden=16, latent=8, vae_batch=16, vae_lr=1e-3, H=1, lr=1e-3, epochs=1, T=5, nd=1.0)
    for extra, route, kw in ((dict(nmf=True), "compute_mf_results", dict(only_synthetic=True)),
                             (dict(device_svd=True), "compute_mf_results_device", dict(only_synthetic=True, seed=11)),
                             (dict(device_svd=True, nmf=True), "compute_mf_results_device", dict(only_synthetic=True, seed=11, nnmf=True)),
                             (dict(resident_svd=True, nmf=True), "compute_mf_results_resident", dict(only_synthetic=True, seed=11, nnmf=True))):
        calls.clear()
        pipeline.run_experiment((m, m, m), dict(hp, **extra), 11, str(tmp_path))
        assert calls == [(route, kw)] * 3, (extra, calls)


def test_host_form_has_the_references_nmf_branch(monkeypatch):
    """compute_mf_results(nnmf=True) fits `NMF(n_components=15, max_iter=50)` in the place of the truncated SVD, as svd_benchmark.py:49-50."""
    decomposition = pytest.importorskip("sklearn.decomposition")
    made = []
    real = decomposition.NMF

    def spy(**kw):
        made.append(kw)
        return real(random_state=0, **kw)
    monkeypatch.setattr(decomposition, "NMF", spy)
    monkeypatch.setattr(decomposition, "TruncatedSVD", lambda **kw: (_ for _ in ()).throw(AssertionError("nnmf=True fits no SVD")))
    rng = np.random.RandomState(0)
    train = csr_matrix((rng.random_sample((40, 60)) < 0.3).astype(np.float64))
    valid = csr_matrix((rng.random_sample((12, 60)) < 0.3).astype(np.float64))
    rec, ndcg = pipeline.compute_mf_results(train, valid, train.toarray(), only_synthetic=True, nnmf=True)
    assert made == [dict(n_components=15, max_iter=50)]
    assert rec.shape == ndcg.shape == (6,) and np.isfinite(rec).all() and (rec >= 0).all() and (rec <= 1).all()
