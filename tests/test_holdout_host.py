"""The host side of the device hold-out split (sdrm_holdout_split, csrc/holdout.h), no GPU: the envelope and the held-out count
behind `sdrm_debug_holdout_args`, the reference restatement tests/holdout_ref.py against the host split it stands in for
(sdrm_amd/metrics.py:50-85, utilities.py:174-236) and against uniformity, and the pre-stage's flag with the model on the host."""
import contextlib
import ctypes as C
import io
import math
import os
import sys

import numpy as np
import torch
from scipy.sparse import csr_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_ref as ref  # noqa: E402
from sdrm_amd import _lib, metrics  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPE, ARG = -2, -1   # SDRM_ERR_SHAPE, SDRM_ERR_ARG


def test_status_codes_are_the_headers():
    assert _lib.STATUS[SHAPE] == "SDRM_ERR_SHAPE" and _lib.STATUS[ARG] == "SDRM_ERR_ARG"


def test_debug_holdout_args_is_math_ceil_and_the_envelope():
    lib = _lib.load()
    m = C.c_int64()
    for prop in (0.2, 0.1, 0.3, 1 / 3, 0.5):
        for n in range(0, 5001):
            assert lib.sdrm_debug_holdout_args(4600, 200, 100000, prop, n, C.byref(m)) == 0
            want = 0 if n < 2 else min(n, math.ceil(prop * n))
            assert m.value == want == ref.held_count(prop, n), (prop, n, m.value, want)
    assert lib.sdrm_debug_holdout_args(1, 1, 0, 0.5, 7, None) == 0
    assert lib.sdrm_debug_holdout_args(1 << 20, (1 << 31) - 1, (1 << 40) - 1, 0.999, 7, C.byref(m)) == 0 and m.value == 7
    ok = dict(n_items=4600, n_rows=200, nnz=100000, test_prop=0.2)
    for bad in (dict(n_items=0), dict(n_items=(1 << 20) + 1), dict(n_rows=0), dict(n_rows=1 << 31), dict(nnz=-1), dict(nnz=1 << 40),
                dict(test_prop=0.0), dict(test_prop=1.0), dict(test_prop=-0.2), dict(test_prop=1.5), dict(test_prop=float("nan"))):
        a = dict(ok, **bad)
        assert lib.sdrm_debug_holdout_args(a["n_items"], a["n_rows"], a["nnz"], a["test_prop"], 10, C.byref(m)) == SHAPE, bad


def _ml100k():
    z = np.load(os.path.join(GOLDEN, "ml100k.npz"))
    return csr_matrix((z["train_test_data"].astype(np.float32), z["train_test_indices"].astype(np.int32),
                       z["train_test_indptr"].astype(np.int64)), shape=tuple(int(v) for v in z["train_test_shape"]))


def test_reference_split_counts_what_the_host_split_counts():
    m = _ml100k()
    # two short users among the real ones: the host split drops them, the reference keeps them as empty rows
    lil = m.tolil()
    lil[5] = 0
    lil[9] = 0
    lil[9, 3] = 4.0
    m = csr_matrix(lil.tocsr())
    m.eliminate_zeros()
    np.random.seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        h_train, h_held = metrics.split_train_test_proportion_from_csr_matrix(m.copy(), test_prop=0.2)
    tp, ti, hp, hi = ref.split(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.shape[1], 0.2, seed=77, draw=3)
    n = np.diff(m.indptr)
    kept = np.flatnonzero(n >= 2)
    assert h_train.shape[0] == kept.size == m.shape[0] - 2
    np.testing.assert_array_equal(np.flatnonzero(np.diff(hp) > 0), kept)          # the same users count ...
    np.testing.assert_array_equal(np.flatnonzero(np.diff(tp) + np.diff(hp) > 0), kept)
    np.testing.assert_array_equal(np.diff(hp)[kept], np.diff(h_held.indptr))      # ... with the same held and train counts
    np.testing.assert_array_equal(np.diff(tp)[kept], np.diff(h_train.indptr))
    # and per user the two parts are the row, disjoint, in CSR order
    for u in kept[:50]:
        a, b = ti[tp[u]:tp[u + 1]], hi[hp[u]:hp[u + 1]]
        np.testing.assert_array_equal(np.sort(np.concatenate([a, b])), m.indices[m.indptr[u]:m.indptr[u + 1]])
        assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all()


def test_reference_split_is_uniform():
    """Every entry of a row is held out with probability m / n.  4000 draws at a fixed seed: a row of 10 with m = 2, the frequency
    of each entry within 5 sigma of 0.2, sigma = sqrt(0.2 * 0.8 / 4000); a row of 64 (m = 13) within the same 5 sigma of 13 / 64
    (whose own binomial sigma is a little larger: the bound is not widened for it)."""
    draws = np.arange(4000, dtype=np.uint64)[:, None]
    sigma = math.sqrt(0.16 / 4000)
    for n, prop, u in ((10, 0.2, 17), (64, 0.2, 4)):
        m = ref.held_count(prop, n)
        mask = ref.held_mask(0x1234567, draws, u, n, prop)
        assert mask.shape == (4000, n) and (mask.sum(axis=1) == m).all()
        freq = mask.mean(axis=0)
        assert np.abs(freq - m / n).max() <= 5 * sigma, (n, freq, m / n)


def test_device_holdout_is_ignored_with_the_model_on_the_host(tmp_path):
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    rs = np.random.RandomState(3)
    m = csr_matrix((rs.random_sample((60, 41)) < 0.2).astype(np.float32))

    def run(where, **kw):
        torch.manual_seed(5)
        np.random.seed(6)
        vae = VAE(41, 12, 4)
        with contextlib.redirect_stdout(io.StringIO()):
            train_variational_autoencoder(vae, m, m, 2, 25, 1e-3, "Recall@5", str(where), **kw)
        return [p.detach().clone() for p in vae.parameters()], np.random.get_state()
    p0, s0 = run(tmp_path / "a")
    p1, s1 = run(tmp_path / "b", device_feed=True, device_holdout=True)
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)
    assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]
