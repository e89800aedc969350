"""The per-user hold-out split on the device (sdrm_holdout_split, csrc/holdout.h; utilities.py:174-236) and the evaluation half
of the VAE pre-stage on it.  Bar: the two output CSRs equal the numpy restatement tests/holdout_ref.py bit for bit; their
consumers (`csr_rows_to_dense`, `rank_metrics` in its device form, `evaluate_holdout`) give what the same steps give on the
read-back matrices."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77
SPLITS = [(0x9E3779B97F4A7C15 & (2 ** 63 - 1), 0, 0.2), (0x9E3779B97F4A7C15 & (2 ** 63 - 1), 0, 1 / 3), (12345, 7, 0.2), (12345, 7, 1 / 3)]


@pytest.fixture(scope="module")
def engine():
    from sdrm_amd.engine import Engine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case():
    m, lengths = ref.case_feed()
    return dict(m=m, lengths=lengths, indptr=m.indptr.astype(np.int64), indices=m.indices.astype(np.int32))


@pytest.fixture(scope="module")
def case_dev(engine, case):
    return engine.csr_to_device(case["m"])


@pytest.fixture(scope="module")
def reference(case):
    """The reference split of the case feed per (seed, draw, test_prop), computed once and never changed."""
    cache = {}

    def get(seed, draw, prop):
        key = (seed, draw, prop)
        if key not in cache:
            cache[key] = tuple(a.copy() for a in ref.split(case["indptr"], case["indices"], ref.N_ITEMS, prop, seed, draw))
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]
    return get


def run_split(engine, csr_dev, prop, seed, draw, check=True):
    """(train_indptr, train_indices, held_indptr, held_indices) as numpy arrays; the index arrays at their full capacity, filled
    with SENTINEL before the call."""
    nnz = int(csr_dev[1].numel())
    out = tuple(torch.full((nnz,), SENTINEL, dtype=torch.int32, device=engine.device) for _ in range(2))
    tr, he = engine.holdout_split(csr_dev, test_prop=prop, seed=seed, draw=draw, check=check, out=out)
    assert tr[1] is out[0] and he[1] is out[1] and tr[2] is None and he[2] is None and tuple(tr[3]) == tuple(he[3]) == tuple(csr_dev[3])
    return tr[0].cpu().numpy(), tr[1].cpu().numpy(), he[0].cpu().numpy(), he[1].cpu().numpy()


def assert_split_equal(got, want):
    tp, ti, hp, hi = got
    wtp, wti, whp, whi = want
    np.testing.assert_array_equal(tp, wtp)
    np.testing.assert_array_equal(hp, whp)
    np.testing.assert_array_equal(ti[:tp[-1]], wti)
    np.testing.assert_array_equal(hi[:hp[-1]], whi)
    assert (ti[tp[-1]:] == SENTINEL).all() and (hi[hp[-1]:] == SENTINEL).all()     # nothing stored behind indptr[n_rows]


def test_case_feed_has_every_boundary_length(case):
    assert case["m"].shape == (ref.CASE_ROWS, ref.N_ITEMS) and case["m"].has_canonical_format
    assert set(ref.BOUNDARY_LENGTHS) <= set(np.diff(case["indptr"]).tolist())
    assert ref.HOLD_TILE + 1 in ref.BOUNDARY_LENGTHS and ref.N_ITEMS > 2 * ref.HOLD_TILE
    assert list(np.diff(case["indptr"])[:len(ref.BOUNDARY_LENGTHS)]) != ref.BOUNDARY_LENGTHS   # shuffled


@pytest.mark.parametrize("seed,draw,prop", SPLITS)
def test_split_equals_the_reference_bit_for_bit_and_stores_nothing_behind(engine, case_dev, reference, seed, draw, prop):
    assert_split_equal(run_split(engine, case_dev, prop, seed, draw), reference(seed, draw, prop))


@pytest.mark.parametrize("seed,draw,prop", SPLITS[1:3])
def test_invariants_without_the_reference(engine, case, case_dev, seed, draw, prop):
    tp, ti, hp, hi = run_split(engine, case_dev, prop, seed, draw)
    indptr, indices = case["indptr"], case["indices"]
    assert tp[0] == 0 and hp[0] == 0
    for u in range(ref.CASE_ROWS):
        row = indices[indptr[u]:indptr[u + 1]]
        a, b = ti[tp[u]:tp[u + 1]], hi[hp[u]:hp[u + 1]]
        if row.size < 2:
            assert a.size == 0 and b.size == 0, u
            continue
        assert b.size == ref.held_count(prop, row.size) and a.size + b.size == row.size, u
        assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all(), u
        assert np.intersect1d(a, b).size == 0, u
        np.testing.assert_array_equal(np.union1d(a, b), row)


def test_split_is_a_function_of_the_row(engine, case, case_dev):
    seed, draw, prop = SPLITS[0]
    first = run_split(engine, case_dev, prop, seed, draw)
    again = run_split(engine, case_dev, prop, seed, draw)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    # the first k rows alone: the prefix of the whole feed's split
    k = 61
    nnz_k = int(case["indptr"][k])
    sub = (case_dev[0][:k + 1].clone(), case_dev[1][:nnz_k].clone(), None, (k, ref.N_ITEMS))
    tp, ti, hp, hi = run_split(engine, sub, prop, seed, draw)
    np.testing.assert_array_equal(tp, first[0][:k + 1])
    np.testing.assert_array_equal(hp, first[2][:k + 1])
    np.testing.assert_array_equal(ti[:tp[-1]], first[1][:tp[-1]])
    np.testing.assert_array_equal(hi[:hp[-1]], first[3][:hp[-1]])
    assert (ti[tp[-1]:] == SENTINEL).all() and (hi[hp[-1]:] == SENTINEL).all()
    # another draw: another split (the counts are the same)
    other = run_split(engine, case_dev, prop, seed, draw + 1)
    np.testing.assert_array_equal(other[2], first[2])
    hp = first[2]
    changed = [u for u in range(ref.CASE_ROWS) if case["lengths"][u] >= 8 and not np.array_equal(other[3][hp[u]:hp[u + 1]], first[3][hp[u]:hp[u + 1]])]
    assert changed


def test_out_of_range_rows_are_empty_in_both_outputs_and_reported(engine, case, case_dev, reference):
    from sdrm_amd.engine import SdrmError
    seed, draw, prop = SPLITS[2]
    lengths, indptr = case["lengths"], case["indptr"]
    rows = [int(u) for u in np.flatnonzero((lengths >= 40) & (lengths <= 400))]
    r_col, r_neg, r_ptr = rows[1], rows[4], 0
    assert lengths[r_ptr] >= 2 and r_ptr not in (r_col, r_neg)
    # a column >= n_items in the middle of one row, a negative one at the end of another
    bad_idx = case_dev[1].clone()
    bad_idx[int(indptr[r_col]) + 17] = ref.N_ITEMS
    bad_idx[int(indptr[r_neg + 1]) - 1] = -1
    # an indptr pair out of order: row 0 starts behind its end (no row in front of it shares the offset)
    bad_ptr = case_dev[0].clone()
    bad_ptr[r_ptr] = bad_ptr[r_ptr + 1] + 5
    got = run_split(engine, (bad_ptr, bad_idx, None, case_dev[3]), prop, seed, draw, check=False)
    with pytest.raises(SdrmError) as err:
        engine.feed_status()
    assert "column index outside" in str(err.value) and "indptr pair" in str(err.value) and "sdrm_holdout_split" in str(err.value)
    engine.feed_status()   # the record was cleared
    # what the reference makes of the same arrays; and, those three rows aside, the clean feed's split
    want = ref.split(bad_ptr.cpu().numpy(), bad_idx.cpu().numpy(), ref.N_ITEMS, prop, seed, draw)
    assert_split_equal(got, want)
    tp, ti, hp, hi = got
    ctp, cti, chp, chi = reference(seed, draw, prop)
    for u in range(ref.CASE_ROWS):
        if u in (r_col, r_neg, r_ptr):
            assert tp[u + 1] == tp[u] and hp[u + 1] == hp[u], u
        else:
            np.testing.assert_array_equal(ti[tp[u]:tp[u + 1]], cti[ctp[u]:ctp[u + 1]])
            np.testing.assert_array_equal(hi[hp[u]:hp[u + 1]], chi[chp[u]:chp[u + 1]])
    # an indptr pair that reaches behind nnz, and a row longer than n_items
    far = case_dev[0].clone()
    far[-1] += 3
    got = run_split(engine, (far, case_dev[1], None, case_dev[3]), prop, seed, draw, check=False)
    assert got[0][-1] == got[0][-2] and got[2][-1] == got[2][-2]
    with pytest.raises(SdrmError, match="indptr pair"):
        engine.feed_status()
    narrow = (case_dev[0], case_dev[1].clamp(max=99), None, (ref.CASE_ROWS, 100))    # rows of more than 100 entries in a feed of 100 columns
    tp, ti, hp, hi = run_split(engine, narrow, prop, seed, draw, check=False)
    for u in range(ref.CASE_ROWS):
        assert (tp[u + 1] - tp[u]) + (hp[u + 1] - hp[u]) == (lengths[u] if 2 <= lengths[u] <= 100 else 0), u
    with pytest.raises(SdrmError, match="indptr pair"):
        engine.feed_status()
    with pytest.raises(SdrmError):     # checked call: raises at once
        engine.holdout_split((bad_ptr, bad_idx, None, case_dev[3]), test_prop=prop, seed=seed, draw=draw)
    assert_split_equal(run_split(engine, case_dev, prop, seed, draw), reference(seed, draw, prop))


def test_host_argument_errors(engine, case_dev):
    from sdrm_amd.engine import SdrmError, _ptr
    for prop in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
            engine.holdout_split(case_dev, test_prop=prop)
    indptr, indices, _, (n_rows, n_items) = case_dev
    nnz = int(indices.numel())
    tp, hp = torch.empty_like(indptr), torch.empty_like(indptr)
    ti, hi = torch.empty_like(indices), torch.empty_like(indices)

    def call(n_items=n_items, nnz=nnz, n_rows=n_rows, outs=(tp, ti, hp, hi)):
        return engine.lib.sdrm_holdout_split(engine._h, _ptr(indptr), _ptr(indices), n_rows, n_items, nnz, 0.2, 1, 0,
                                             _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), None)
    assert call(n_items=0) == -2 and call(nnz=-1) == -2 and call(n_rows=0) == -2 and call(n_items=(1 << 20) + 1) == -2   # SDRM_ERR_SHAPE
    for k in range(4):
        outs = [tp, ti, hp, hi]
        outs[k] = None
        assert call(outs=outs) == -1, k                                                                                   # SDRM_ERR_ARG
    torch.cuda.synchronize()
    engine.feed_status()


def test_an_empty_matrix_splits_into_two_empty_matrices(engine):
    tr, he = engine.holdout_split(engine.csr_to_device(csr_matrix((5, 9), dtype=np.float32)))
    assert tr[0].cpu().tolist() == [0] * 6 and he[0].cpu().tolist() == [0] * 6 and tr[1].numel() == 0 and he[1].numel() == 0


def test_consumers_take_the_outputs_as_they_are(engine, case_dev, reference):
    seed, draw, prop = SPLITS[3]
    wtp, wti, whp, whi = reference(seed, draw, prop)
    tr, he = engine.holdout_split(case_dev, test_prop=prop, seed=seed, draw=draw)
    dense = engine.csr_rows_to_dense(tr, row0=0, b=ref.CASE_ROWS).cpu().numpy()
    np.testing.assert_array_equal(dense, ref.to_scipy(wtp, wti, ref.N_ITEMS).toarray())
    # rank_metrics, device form at row0 > 0 against the scipy form on the read-back matrices' row slice
    tr_m = ref.to_scipy(tr[0].cpu().numpy(), tr[1].cpu().numpy(), ref.N_ITEMS)
    he_m = ref.to_scipy(he[0].cpu().numpy(), he[1].cpu().numpy(), ref.N_ITEMS)
    row0, U = 37, 90
    scores = torch.randn(U, ref.N_ITEMS, device=engine.device, generator=torch.Generator(engine.device).manual_seed(9))
    ks = (1, 10, 50)
    rec_d, ndcg_d = engine.rank_metrics(scores, he, train=tr, ks=ks, row0=row0)
    rec_s, ndcg_s = engine.rank_metrics(scores, he_m[row0:row0 + U], train=tr_m[row0:row0 + U], ks=ks)
    np.testing.assert_array_equal(rec_d.cpu().numpy(), rec_s.cpu().numpy())
    np.testing.assert_array_equal(ndcg_d.cpu().numpy(), ndcg_s.cpu().numpy())
    assert np.isfinite(rec_d.cpu().numpy()).any()
    tables = engine._rank_tables(ks)
    assert engine._rank_tables(ks) is tables                       # cached per ks: a batch uploads nothing
    from sdrm_amd.engine import SdrmError
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.rank_metrics(scores, he, train=tr, ks=ks, row0=ref.CASE_ROWS - U + 1)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.rank_metrics(scores[:, :100].contiguous(), he, train=tr, ks=ks)


VAE_ITEMS, VAE_USERS = 1009, 700


@pytest.fixture(scope="module")
def vae_feed():
    rs = np.random.RandomState(21)
    counts = rs.binomial(VAE_ITEMS, 0.03, size=VAE_USERS)
    counts[[3, 499, 500, 699]] = [0, 1, 1, 0]          # users the reference's split drops, on both sides of the batch boundary
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rs.choice(VAE_ITEMS, size=c, replace=False)) for c in counts]).astype(np.int32)
    return csr_matrix((rs.randint(1, 6, size=indices.size).astype(np.float32), indices, indptr), shape=(VAE_USERS, VAE_ITEMS))


def test_evaluate_holdout_equals_the_same_steps_on_the_read_back_split(engine, vae_feed):
    from sdrm_amd.vae_hooks import VAE, evaluate_holdout
    torch.manual_seed(4)
    vae = VAE(VAE_ITEMS, 64, 16).to(engine.device)
    test_dev = engine.csr_to_device(vae_feed)
    seed, draw = 99, 5
    for metric in ("Recall@10", "NDCG@20"):
        got = evaluate_holdout(vae, engine, test_dev, seed, draw, metric, batch=500)
        engine.feed_status()
        assert got.dtype == torch.float64 and got.shape == (VAE_USERS,) and got.device == engine.device
        assert not vae.training and vae.is_training == 0
        tr, he = engine.holdout_split(test_dev, seed=seed, draw=draw)
        tr_m = ref.to_scipy(tr[0].cpu().numpy(), tr[1].cpu().numpy(), VAE_ITEMS)
        he_m = ref.to_scipy(he[0].cpu().numpy(), he[1].cpu().numpy(), VAE_ITEMS)
        tr_dev = engine.csr_to_device(tr_m)
        k = int(metric.split("@")[1])
        want = []
        with torch.no_grad():
            for lo in range(0, VAE_USERS, 500):
                hi = min(lo + 500, VAE_USERS)
                pred, _ = vae(engine.csr_rows_to_dense(tr_dev, row0=lo, b=hi - lo))
                rec, ndcg = engine.rank_metrics(pred, he_m[lo:hi], train=tr_m[lo:hi], ks=(k,))
                want.append((rec if "Recall" in metric else ndcg)[0].cpu().numpy())
        want = np.concatenate(want)
        got = got.cpu().numpy()
        np.testing.assert_array_equal(got, want)                  # (nan == nan positions included)
        assert np.flatnonzero(np.isnan(got)).tolist() == [3, 499, 500, 699] and np.isfinite(np.nanmean(got))


def test_pre_stage_with_device_holdout_never_calls_the_host_split(engine, vae_feed, tmp_path, monkeypatch, capsys):
    from sdrm_amd import metrics
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder

    class HostSplitCalled(Exception):
        pass

    def boom(*a, **kw):
        raise HostSplitCalled()
    monkeypatch.setattr(metrics, "split_train_test_proportion_from_csr_matrix", boom)

    def run(where, **kw):
        torch.manual_seed(5)
        np.random.seed(6)
        vae = VAE(VAE_ITEMS, 64, 16).to(engine.device)
        train_variational_autoencoder(vae, vae_feed, vae_feed, 3, 250, 1e-3, "Recall@10", str(where), verbose=True, **kw)
        return vae
    vae = run(tmp_path / "on", device_feed=True, device_holdout=True)
    assert vae.model_is_trained and vae.is_training == 0
    shown = re.findall(r"Epoch: (\d+), Loss: (\S+), Recall@10: (\S+)", capsys.readouterr().out)
    assert [int(e) for e, _, _ in shown] == [0, 1, 2]
    metric = [float(v) for _, _, v in shown]
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in metric) and all(np.isfinite(float(v)) for _, v, _ in shown)
    saved = sorted(os.listdir(tmp_path / "on"))
    assert "epoch-0.pth" in saved and all(re.fullmatch(r"epoch-\d+\.pth", f) for f in saved)
    # epoch-<best>.pth: an epoch is saved when it beats every earlier one (the printed metric is rounded: the best shown is among them)
    assert max(metric) in [metric[int(f[6:-4])] for f in saved]
    with pytest.raises(HostSplitCalled):     # the flag is what removes the host split
        run(tmp_path / "off", device_feed=True, device_holdout=False)
