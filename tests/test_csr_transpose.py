"""Device CSR -> CSC transpose and row stacking (csrc/csr_transpose.h; sdrm_csr_transpose / sdrm_csr_vstack; Engine.csr_transpose /
Engine.csr_vstack) and the resident form of the SVD evaluator on top of them (pipeline.compute_mf_results_resident).

The reference is scipy - `tocsr().tocsc()` + `sort_indices()`, `scipy.sparse.vstack` - and every comparison is `array_equal` on
integers or on float32 bit patterns: there is no tolerance in this file.  tests/csr_transpose_ref.py holds the shared inputs and a numpy
restatement of the bit-table scheme."""
import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix, vstack

import csr_transpose_ref as ref
import svd_eval_ref
from sdrm_amd import _lib, pipeline
from sdrm_amd.engine import Engine, SdrmError

SHAPE, ARG = -2, -1


def _bits(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """Integers, or float32 bit patterns."""
    if want is None:
        assert got is None
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if want.dtype == np.float32:
        got, want = _bits(got), _bits(want)
    np.testing.assert_array_equal(got, want)


# ================================================================================================ CPU
def test_refusals_need_no_device():
    """The signatures' argument counts; a null handle is SDRM_ERR_ARG from both calls; the transpose's envelope - both sides of 2^22 rows and
    columns, both sides of a bit table of 2^26 words, a negative capacity - from the library's host side; Engine.csr_transpose and
    Engine.csr_vstack refuse wrong dtypes and more than 8 parts before they call anything."""
    lib = _lib.load()
    assert len(_lib.SIGNATURES["sdrm_csr_transpose"][1]) == 11 and len(_lib.SIGNATURES["sdrm_csr_vstack"][1]) == 9
    assert len(_lib.SIGNATURES["sdrm_debug_csr_transpose_args"][1]) == 3
    assert lib.sdrm_csr_transpose(None, None, None, None, 4, 4, 4, None, None, None, None) == ARG
    assert lib.sdrm_csr_vstack(None, None, 1, 4, None, None, None, 4, None) == ARG
    args = lib.sdrm_debug_csr_transpose_args
    assert args(1, 1, 0) == 0 and args(6638, 3125, 1040000) == 0
    assert args(2 ** 22, 16, 0) == 0 and args(2 ** 22 + 1, 16, 0) == SHAPE
    assert args(16, 2 ** 22, 0) == 0 and args(16, 2 ** 22 + 1, 0) == SHAPE
    assert args(0, 16, 0) == SHAPE and args(16, 0, 0) == SHAPE
    assert args(64 * 2 ** 10, 2 ** 16, 0) == 0 and args(64 * 2 ** 10 + 1, 2 ** 16, 0) == SHAPE     # ceil(m / 64) n = 2^26, and one block more
    assert args(64 * 2 ** 10, 2 ** 16 + 1, 0) == SHAPE
    assert args(16, 16, -1) == SHAPE and args(16, 16, 2 ** 40 - 1) == 0 and args(16, 16, 2 ** 40) == SHAPE

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    eng = Engine.__new__(Engine)       # the methods' own checks, on the host: any call into the library fails the test
    eng.device, eng.lib, eng._h = torch.device("cpu"), NoLaunch(), None
    a = svd_eval_ref.planted(40, 37, 3, seed=1)
    indptr, indices = torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int32))
    good = (indptr, indices, None, a.shape)
    for bad in ((indptr.to(torch.int32), indices, None, a.shape), (indptr, indices.to(torch.int64), None, a.shape),
                (indptr, indices, torch.ones(a.nnz, dtype=torch.float64), a.shape), (indptr[:-1], indices, None, a.shape),
                (indptr, indices, torch.ones(a.nnz - 1), a.shape)):
        with pytest.raises(SdrmError):
            eng.csr_transpose(bad)
        with pytest.raises(SdrmError):
            eng.csr_vstack([good, bad])
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        eng.csr_transpose((torch.zeros(64 * 2 ** 10 + 2, dtype=torch.int64), indices, None, (64 * 2 ** 10 + 1, 2 ** 16)))
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        eng.csr_vstack([good] * 9)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        eng.csr_vstack([])
    with pytest.raises(SdrmError, match="one width"):
        eng.csr_vstack([good, (indptr, indices, None, (40, 38))])


def test_run_experiment_routes_resident_svd(monkeypatch, tmp_path):
    """With `resident_svd` all three tags go to compute_mf_results_resident with the tuple the net's engine made - no host copy - and
    the run's seed; without the key run_experiment makes the calls it made before.  Nothing of it reaches train_SDRM."""
    from sdrm_amd import train_SDRM as ts
    import sdrm_amd.engine as engine_mod

    class Eng:
        def equal_sparsity_csr(self, raw, sparsity):
            return ("tuple", raw if isinstance(raw, str) else int(raw), sparsity)

    eng = Eng()

    class Net:
        def engine(self):
            return eng

    class Vae:
        def sample(self, n):
            return "V"

    train_kw, calls = [], []
    monkeypatch.setattr(ts, "train_SDRM", lambda *a, **kw: (train_kw.append(set(kw)), (Net(), Vae()))[1])
    monkeypatch.setattr(ts, "sample_ddpm", lambda n, net, vae, latent, nd, timesteps=None, n_timesteps=None: torch.zeros(1) + (1 if timesteps else 2))
    monkeypatch.setattr(pipeline, "DeviceFeed", lambda *a, **k: "feed")
    monkeypatch.setattr(engine_mod, "utility_engine", lambda *a, **k: None)
    monkeypatch.setattr(pipeline, "equal_sparsity", lambda raw, sparsity, engine: ("bin", raw if isinstance(raw, str) else int(raw)))
    monkeypatch.setattr(pipeline, "equal_sparsity_csr", lambda *a, **kw: calls.append(("host csr", a, kw)) or "host csr")
    monkeypatch.setattr(pipeline, "compute_mf_results", lambda *a, **kw: calls.append(("host", a, kw)) or "host")
    monkeypatch.setattr(pipeline, "compute_mf_results_device", lambda *a, **kw: calls.append(("device", a, kw)) or "device")
    monkeypatch.setattr(pipeline, "compute_mf_results_resident", lambda *a, **kw: calls.append(("resident", a, kw)) or "resident")
    m = svd_eval_ref.planted(40, 40, 3, seed=1)
    sparsity = 1 - m.nnz / 1600
    hp = dict(batch=16, vae_hidden=16, latent=8, vae_batch=16, vae_lr=1e-3, H=1, lr=1e-3, epochs=1, T=5, nd=1.0)
    for extra in (dict(), dict(resident_svd=False)):
        calls.clear()
        out = pipeline.run_experiment((m, m, m), dict(hp, **extra), 11, str(tmp_path))
        assert out == {"M": "host", "F": "host", "V": "host"}
        assert [(c[0], c[1][2], c[2]) for c in calls] == [("host", ("bin", tag), dict(only_synthetic=True)) for tag in (1, 2, "V")]
    calls.clear()
    out = pipeline.run_experiment((m, m, m), dict(hp, resident_svd=True), 11, str(tmp_path))
    assert out == {"M": "resident", "F": "resident", "V": "resident"}
    assert [(c[0], c[1][2:], c[2]) for c in calls] == [("resident", (("tuple", tag, sparsity), eng), dict(only_synthetic=True, seed=11)) for tag in (1, 2, "V")]
    assert all(c[1][0] is m and c[1][1] is m and len(c[1]) == 4 for c in calls)
    assert train_kw[0] == train_kw[-1] and "resident_svd" not in train_kw[-1] and "resident_svd" not in pipeline.VAE_FLAGS


@pytest.mark.parametrize("with_data", [False, True], ids=["ones", "values"])
@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_matches_scipy(name, with_data):
    """The bit-table scheme in numpy equals scipy's tocsc() + sort_indices() on every case the device is held to, from sorted rows and
    from rows in a random order, and raises nothing."""
    a = ref.case(name)
    indptr, indices, data = ref.arrays(a, with_data)
    want = ref.scipy_transpose(indptr, indices, data, a.shape)
    for src in ((indptr, indices, data), ref.shuffled(indptr, indices, data)):
        colptr, rowidx, cdata, raised = ref.transpose_restated(*src, *a.shape)
        assert not raised
        _same(colptr, want[0])
        _same(rowidx, want[1])
        _same(cdata, want[2])


def test_restatement_checks():
    """The restatement's range checks on the inputs of the device's bad-input cases: the entry or the row is left out, a doubled column
    is reported, and no place outside the arrays is computed."""
    a = ref.case("65x70")
    indptr, indices, data = ref.arrays(a, True)
    for which, want_raised in (("col", {ref.BAD_COL}), ("ptr", {ref.BAD_PTR}), ("dup", {ref.DUP})):
        (ip, ix, dv), dropped = _bad_input(which, indptr, indices, data)
        colptr, rowidx, cdata, raised = ref.transpose_restated(ip, ix, dv, *a.shape)
        assert raised == want_raised
        if dropped is not None:
            want = ref.scipy_transpose(*dropped, a.shape)
            n = int(want[0][-1])
            _same(colptr, want[0])
            _same(rowidx[:n], want[1])
            _same(cdata[:n], want[2])
            assert (rowidx[n:] == -1).all()


def _bad_input(which, indptr, indices, data):
    """((indptr, indices, data) with one defect, the same arrays as a valid matrix without what the defect costs - or None for the doubled
    column, whose output is unspecified)."""
    indptr, indices = indptr.copy(), indices.copy()
    if which == "col":      # one column equal to n_cols and one of -1, in two rows: the transpose of the matrix without those entries
        p1, p2 = int(indptr[3]), int(indptr[64])
        indices[p1], indices[p2] = 70, -1
        keep = np.ones(len(indices), dtype=bool)
        keep[[p1, p2]] = False
        ip = indptr.copy()
        ip[4:] -= 1
        ip[65:] -= 1
        return (indptr, indices, data), (ip, indices[keep], data[keep])
    if which == "ptr":      # the last row's pair descends: that row is absent
        ip = indptr.copy()
        ip[65] = ip[64]
        indptr[65] = indptr[64] - 1
        return (indptr, indices, data), (ip, indices, data)
    p = int(indptr[3])      # row 3 holds its first column twice
    assert indptr[4] - p >= 2
    indices[p + 1] = indices[p]
    return (indptr, indices, data), None


# ================================================================================================ GPU
@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def _dev(engine, indptr, indices, data, shape):
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)
    return (t(indptr), t(indices), t(data), tuple(int(v) for v in shape))


def _host(x):
    return None if x is None else x.cpu().numpy()


def _check_transpose(got, want):
    colptr, rowidx, cdata, _ = got
    n = int(want[0][-1])
    _same(_host(colptr), want[0])
    _same(_host(rowidx)[:n], want[1])
    _same(None if cdata is None else _host(cdata)[:n], want[2])


FORMS = {"atomics": 1, "lds": 2}   # the two forms of the mark pass (Engine.debug_set(csrt_mark=...)); the other tests run the one the width picks


@pytest.fixture
def mark_form(engine, request):
    engine.debug_set(csrt_mark=FORMS[request.param])
    yield request.param
    engine.debug_set(csrt_mark=0)


@pytest.mark.gpu
@pytest.mark.parametrize("mark_form", list(FORMS), indirect=True)
@pytest.mark.parametrize("with_data", [False, True], ids=["ones", "values"])
@pytest.mark.parametrize("name", ref.CASES)
def test_transpose_against_scipy(engine, name, with_data, mark_form):
    """colptr, rowidx[:nnz] and cdata[:nnz] are scipy's tocsc() + sort_indices(), bitwise: from the canonical input, from the same matrix with
    the columns of every row shuffled (values along with them), and - transposed once more, the result read as the CSR of the transpose -
    back to the sorted input.  With the mark pass on 64-bit global atomics and on LDS column tiles (700 x 4100 is wider than one tile)."""
    a = ref.case(name)
    indptr, indices, data = ref.arrays(a, with_data)
    want = ref.scipy_transpose(indptr, indices, data, a.shape)
    got = engine.csr_transpose(_dev(engine, indptr, indices, data, a.shape))
    assert got[3] == a.shape and (got[2] is None) == (not with_data) and got[1].numel() == a.nnz
    _check_transpose(got, want)
    _check_transpose(engine.csr_transpose(_dev(engine, *ref.shuffled(indptr, indices, data), a.shape)), want)
    back = engine.csr_transpose((got[0], got[1], got[2], a.shape[::-1]))
    _check_transpose(back, (indptr, indices, data))


@pytest.mark.gpu
def test_transpose_of_a_row_range(engine):
    """Rows 30 .. 99 of the 300 x 259 arrays, passed as an indptr slice with its absolute offsets, equal scipy's transpose of that slice."""
    a = ref.case("300x259")
    indptr, indices, data = ref.arrays(a, True)
    full = _dev(engine, indptr, indices, data, a.shape)
    got = engine.csr_transpose((full[0][30:101], full[1], full[2], (70, 259)))
    assert indptr[30] > 0
    _check_transpose(got, ref.scipy_transpose(indptr[30:101], indices, data, (70, 259)))


@pytest.mark.gpu
def test_transpose_scratch_hygiene_and_determinism(engine):
    """700 x 4100, then 65 x 70, then 700 x 4100 again on one engine: every result is scipy's, and the two large ones are the same bytes
    over their whole arrays."""
    big, small = ref.case("700x4100"), ref.case("65x70")
    outs = []
    for a in (big, small, big):
        indptr, indices, data = ref.arrays(a, True)
        got = engine.csr_transpose(_dev(engine, indptr, indices, data, a.shape))
        _check_transpose(got, ref.scipy_transpose(indptr, indices, data, a.shape))
        outs.append(got)
    for x, y in zip(outs[0][:3], outs[2][:3]):
        assert _host(x).tobytes() == _host(y).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mark_form", list(FORMS), indirect=True)
@pytest.mark.parametrize("which,message", [("col", ref.BAD_COL), ("ptr", ref.BAD_PTR), ("dup", ref.DUP)])
def test_transpose_bad_input(engine, which, message, mark_form):
    """A column equal to n_cols and a column of -1: the transpose of the matrix without those entries.  A descending indptr pair: that
    row is absent.  A row with one column twice: the bit of its own is raised.  The outputs sit between guard bands of a sentinel value,
    which stay untouched; the status is read with feed_status() and the message matched; the next call on the same engine is clean."""
    a = ref.case("65x70")
    indptr, indices, data = ref.arrays(a, True)
    (ip, ix, dv), dropped = _bad_input(which, indptr, indices, data)
    G, cap, n = 64, len(ix), a.shape[1]
    colptr = torch.full((n + 1 + 2 * G,), -7, dtype=torch.int64, device=engine.device)
    rowidx = torch.full((cap + 2 * G,), -7, dtype=torch.int32, device=engine.device)
    cdata = torch.full((cap + 2 * G,), -7.0, dtype=torch.float32, device=engine.device)
    out = (colptr[G:G + n + 1], rowidx[G:G + cap], cdata[G:G + cap])
    got = engine.csr_transpose(_dev(engine, ip, ix, dv, a.shape), check=False, out=out)
    with pytest.raises(SdrmError, match=message):
        engine.feed_status()
    for t, size in ((colptr, n + 1), (rowidx, cap), (cdata, cap)):
        t = _host(t)
        assert (t[:G] == -7).all() and (t[G + size:] == -7).all()
    if dropped is not None:
        _check_transpose(got, ref.scipy_transpose(*dropped, a.shape))
    else:
        cp = _host(got[0])
        assert cp[0] == 0 and (np.diff(cp) >= 0).all() and cp[-1] == cap - 1      # one bit fewer than entries
    engine.feed_status()                                                           # cleared
    clean = engine.csr_transpose(_dev(engine, indptr, indices, data, a.shape))     # check=True: raises if anything is left
    _check_transpose(clean, ref.scipy_transpose(indptr, indices, data, a.shape))


def _scipy_of(csr_dev):
    """The scipy matrix of a device CSR tuple, read back (3- or 4-tuple; absolute offsets; arrays longer than the entry count)."""
    indptr, indices = _host(csr_dev[0]).astype(np.int64), _host(csr_dev[1])
    data, shape = (_host(csr_dev[2]), csr_dev[3]) if len(csr_dev) == 4 else (None, csr_dev[2])
    lo, hi = int(indptr[0]), int(indptr[-1])
    vals = np.ones(hi - lo, dtype=np.float32) if data is None else data[lo:hi]
    return csr_matrix((vals, indices[lo:hi], indptr - lo), shape=tuple(shape))


def _check_stack(got, parts, values):
    want = vstack(parts).tocsr()
    indptr, indices, data, shape = got
    assert tuple(shape) == want.shape and indptr.dtype == torch.int64 and indices.dtype == torch.int32
    n = want.nnz
    _same(_host(indptr), want.indptr.astype(np.int64))
    _same(_host(indices)[:n], want.indices.astype(np.int32))
    if values:
        _same(_host(data)[:n], want.data.astype(np.float32))
    else:
        assert data is None


@pytest.mark.gpu
def test_vstack_three_parts(engine):
    """An empty 5 x 37, a 33 x 37, and rows 10 .. 29 of a 40 x 37 as an indptr slice with a nonzero first offset (its arrays are the whole
    matrix's): scipy.sparse.vstack of the three, bitwise."""
    empty, a, b = csr_matrix((5, 37), dtype=np.float64), svd_eval_ref.planted_case("33x37")[0], svd_eval_ref.planted(40, 37, 3, seed=4)
    b_dev = engine.csr_to_device(b)
    assert b.indptr[10] > 0
    got = engine.csr_vstack([engine.csr_to_device(empty), engine.csr_to_device(a), (b_dev[0][10:31], b_dev[1], None, (20, 37))])
    assert got[1].numel() == a.nnz + b.nnz
    _check_stack(got, [empty, a, b[10:30]], False)


@pytest.mark.gpu
def test_vstack_takes_a_holdout_split_as_it_is(engine):
    """The train half of Engine.holdout_split of the 70 x 61 case - arrays of the input's nnz, filled up to indptr[-1] - under a planted
    40 x 61; the expectation is built from the split's own read-back."""
    top = svd_eval_ref.planted(40, 61, 3, seed=6)
    train_dev, _ = engine.holdout_split(engine.csr_to_device(ref.case("70x61")), test_prop=0.2, seed=1)
    train = _scipy_of(train_dev)
    assert train.nnz < train_dev[1].numel()
    _check_stack(engine.csr_vstack([engine.csr_to_device(top), train_dev]), [top, train], False)


@pytest.mark.gpu
def test_vstack_mixed_values(engine):
    """One part with values, one without: data_out holds the values and ones."""
    a = ref.case("70x61")
    indptr, indices, data = ref.arrays(a, True)
    valued = csr_matrix((data, indices, indptr), shape=a.shape)
    ones = svd_eval_ref.planted(40, 61, 3, seed=6)
    got = engine.csr_vstack([_dev(engine, indptr, indices, data, a.shape), engine.csr_to_device(ones)])
    _check_stack(got, [valued, ones.astype(np.float32)], True)
    _check_stack(engine.csr_vstack([engine.csr_to_device(ones), _dev(engine, indptr, indices, data, a.shape)]), [ones.astype(np.float32), valued], True)


@pytest.mark.gpu
def test_vstack_takes_the_equal_sparsity_tuple(engine):
    """The 3-tuple of Engine.equal_sparsity_csr on a random 50 x 61 score matrix as a part."""
    raw = torch.from_numpy(np.random.RandomState(8).standard_normal((50, 61)).astype(np.float32)).to(engine.device)
    syn = engine.equal_sparsity_csr(raw, 0.8)
    assert len(syn) == 3
    under = svd_eval_ref.planted(40, 61, 3, seed=6)
    _check_stack(engine.csr_vstack([syn, engine.csr_to_device(under)]), [_scipy_of(syn), under], False)


@pytest.mark.gpu
def test_vstack_bad_rows_are_empty(engine):
    """A part with a column outside the width, and one with a descending indptr pair: that row is empty in the output, the status is
    raised, and every other row is intact; the next call is clean."""
    a, b = svd_eval_ref.planted_case("33x37")[0], svd_eval_ref.planted(40, 37, 3, seed=4)
    for defect, message in (("col", "sdrm_csr_vstack: a column index"), ("ptr", "sdrm_csr_vstack: an indptr pair")):
        b_dev = engine.csr_to_device(b)
        want_b = b.copy().tolil()
        if defect == "col":
            assert b.indptr[8] - b.indptr[7] >= 2
            b_dev[1][int(b.indptr[7]) + 1] = 37
            want_b[7, :] = 0
        else:
            b_dev[0][40] = int(b.indptr[39]) - 1
            want_b[39, :] = 0
        want_b = want_b.tocsr()
        got = engine.csr_vstack([engine.csr_to_device(a), b_dev], check=False)
        with pytest.raises(SdrmError, match=message):
            engine.feed_status()
        _check_stack(got, [a, want_b], False)
    _check_stack(engine.csr_vstack([engine.csr_to_device(a), engine.csr_to_device(b)]), [a, b], False)


@pytest.mark.gpu
def test_fit_from_the_device_forms_is_the_same_bits(engine):
    """svd_fit from csr_vstack's and csr_transpose's tuples returns the bits of the fit from csr_to_device and csc_to_device."""
    a, k = svd_eval_ref.planted_case("70x61")
    stack_dev = engine.csr_vstack([engine.csr_to_device(a)])
    v, s = engine.svd_fit(stack_dev, engine.csr_transpose(stack_dev), n_components=k, n_iter=5, seed=3)
    v0, s0 = engine.svd_fit(engine.csr_to_device(a), engine.csc_to_device(a), n_components=k, n_iter=5, seed=3)
    assert torch.equal(v, v0) and s.tobytes() == s0.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("only_synthetic", [True, False])
def test_resident_evaluator_equals_the_device_one(engine, only_synthetic):
    """mf_per_user_resident from the uploaded synthetic matrix equals mf_per_user_device from the host one on the ML-100k inputs, per user
    and k, NaNs in the same places."""
    train, valid, synthetic = svd_eval_ref.ml100k_inputs()
    want = pipeline.mf_per_user_device(train, valid.copy(), synthetic, engine, only_synthetic=only_synthetic, seed=3)
    got = pipeline.mf_per_user_resident(train, valid.copy(), engine.csr_to_device(synthetic), engine, only_synthetic=only_synthetic, seed=3)
    for w, g in zip(want, got):
        assert g.shape == w.shape and g.shape[0] == len(pipeline.K_LIST)
        np.testing.assert_array_equal(g, w)
    means = pipeline.compute_mf_results_resident(train, valid.copy(), engine.csr_to_device(synthetic), engine, only_synthetic=only_synthetic, seed=3)
    for m, w in zip(means, want):
        np.testing.assert_array_equal(m, np.array([np.round(np.nanmean(w[q]), 4) for q in range(len(pipeline.K_LIST))]))
