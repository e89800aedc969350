"""the sparse batch feed on the device (dataloaders.py:46-79 + `.to_dense()`, train_SDRM.py:323).
Bar: the dense batch is identical to scipy's `csr[rows].toarray()` (a copy of stored values: bit-exact)."""
import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from sdrm_amd import synth


@pytest.fixture(scope="module")
def engine():
    from sdrm_amd.engine import Engine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def test_interaction_generator_is_disjoint_and_has_edge_users():
    train, held = synth.synth_interactions(30, 200, seed=3)
    assert train.multiply(held).nnz == 0
    assert held[0].nnz == 0 and held[1].nnz > 50 and train[2].nnz == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows,n_items", [(938, 1008), (300, 8582), (50, 3), (7, 1)])   # 8582*4 is not a multiple of 16
@pytest.mark.parametrize("weighted", [False, True])
def test_rows_to_dense_matches_scipy(engine, n_rows, n_items, weighted):
    rs = np.random.RandomState(n_rows + n_items)
    dense = (rs.random_sample((n_rows, n_items)) < 0.06).astype(np.float32)
    if weighted:
        dense *= rs.random_sample((n_rows, n_items)).astype(np.float32) + 0.5
    dense[n_rows // 2] = 0          # an empty row
    m = csr_matrix(dense)
    dev = engine.csr_to_device(m)
    assert (dev[2] is None) == (not weighted)
    rows = rs.permutation(n_rows)[: max(1, n_rows // 3)].astype(np.int64)
    got = engine.csr_rows_to_dense(dev, rows=torch.from_numpy(rows)).cpu().numpy()
    np.testing.assert_array_equal(got, m[rows].toarray().astype(np.float32))
    lo, b = n_rows // 4, max(1, n_rows // 2)
    got = engine.csr_rows_to_dense(dev, row0=lo, b=b).cpu().numpy()
    np.testing.assert_array_equal(got, dense[lo:lo + b])


@pytest.mark.gpu
def test_device_feed_yields_what_the_host_feed_yields(engine):
    from sdrm_amd.pipeline import DeviceFeed, EpochFeed
    train, _ = synth.synth_interactions(101, 257, seed=4, p_train=0.1)
    host, dev = EpochFeed(train, 32, seed=11, device="cuda"), DeviceFeed(train, 32, engine, seed=11)
    for epoch in range(2):                       # a fresh permutation per epoch on both sides
        hb, db = list(host), list(dev)
        assert len(hb) == len(db) == 4 and db[-1][0].shape[0] == 101 - 3 * 32
        for (hx, _), (dx, _) in zip(hb, db):
            assert torch.equal(hx.to_dense(), dx.to_dense())


@pytest.mark.gpu
def test_feed_argument_errors(engine):
    from sdrm_amd.engine import SdrmError
    dev = engine.csr_to_device(csr_matrix(np.eye(5, dtype=np.float32)))
    with pytest.raises(SdrmError):
        engine.csr_rows_to_dense(dev, rows=torch.tensor([0, 5]))
    with pytest.raises(SdrmError):
        engine.csr_rows_to_dense(dev, row0=3, b=3)


@pytest.mark.gpu
def test_out_of_range_csr_is_caught_on_the_device_not_written_out_of_bounds(engine):
    """VERDICT r4 item 7 (dataloaders.py:46-79 hands a scipy CSR to the feed; a corrupt one must not become a stray device store):
    a row id outside the matrix leaves that output row zero, a column index outside [0, n_items) skips that entry, every other
    row / entry is delivered as scipy would, and the handle reports SDRM_ERR_ARG at the next status read (then is clean again)."""
    from sdrm_amd.engine import SdrmError
    rs = np.random.RandomState(5)
    dense = (rs.random_sample((12, 37)) < 0.3).astype(np.float32)
    m = csr_matrix(dense)
    indptr, indices, data, shape = engine.csr_to_device(m)
    # (1) row ids: -1 and n_rows among good ones; a guard band behind the output shows nothing was written past it
    rows = torch.tensor([3, -1, 7, 12, 0], dtype=torch.int64)
    out = engine.csr_rows_to_dense((indptr, indices, data, shape), rows=rows, check=False).cpu().numpy()
    np.testing.assert_array_equal(out[[0, 2, 4]], dense[[3, 7, 0]])
    assert not out[1].any() and not out[3].any()
    with pytest.raises(SdrmError, match="row id outside"):
        engine.feed_status()
    engine.feed_status()                        # the record was cleared
    # (2) column indices: one entry of row 2 points behind the row, one is negative
    bad = indices.clone()
    lo, hi = int(m.indptr[2]), int(m.indptr[3])
    assert hi - lo >= 2
    bad[lo] = 37
    bad[lo + 1] = -4
    out = engine.csr_rows_to_dense((indptr, bad, data, shape), row0=0, b=12, check=False).cpu().numpy()
    want = dense.copy()
    want[2, m.indices[lo]] = 0
    want[2, m.indices[lo + 1]] = 0
    np.testing.assert_array_equal(out, want)
    with pytest.raises(SdrmError, match="column index outside"):
        engine.feed_status()
    # (3) checked call: raises at once; an unordered indptr pair is a zero row, not a wild loop
    with pytest.raises(SdrmError):
        engine.csr_rows_to_dense((indptr, bad, data, shape), row0=0, b=12)
    badptr = indptr.clone()
    badptr[5] = badptr[6] + 3
    out = engine.csr_rows_to_dense((badptr, indices, data, shape), row0=5, b=1, check=False).cpu().numpy()
    assert not out.any()
    with pytest.raises(SdrmError, match="indptr"):
        engine.feed_status()
    good = engine.csr_rows_to_dense((indptr, indices, data, shape), row0=0, b=12).cpu().numpy()
    np.testing.assert_array_equal(good, dense)


@pytest.mark.gpu
def test_a_matrix_without_entries_goes_through_every_feed_entry(engine):
    """A `csr_to_device` matrix with nnz = 0 has an empty `indices` tensor, to which torch gives no address: every entry point on the
    feed takes it all the same, and delivers what a batch of empty rows is - zeros, the bias, a loss of zero."""
    from vae_encode_ref import rel_l2, rel_max
    from test_vae_encode import TOL
    n_rows, n_items, hidden = 5, 70, 24
    empty = engine.csr_to_device(csr_matrix((n_rows, n_items), dtype=np.float32))
    assert empty[1].numel() == 0
    dense = engine.csr_rows_to_dense(empty, row0=0, b=n_rows, check=False)
    assert dense.shape == (n_rows, n_items) and not dense.any()
    # train-mode input layer: the accumulator is +0 and fmaf(0, rs, b) is b; the norm is 0, so rowscale = scale / 1e-12 in float32
    w1, b1, w2, b2 = tensors = synth.synth_vae_encoder(n_items, hidden, 6, seed=51)
    b1_d = torch.from_numpy(b1).cuda()
    pre, rowscale = engine.vae_input_layer_fwd(torch.from_numpy(w1).cuda(), b1_d, empty, row0=0, b=n_rows, seed=3, step=1, p_drop=0.5, check=False)
    assert torch.equal(pre.view(torch.int32), b1_d.expand(n_rows, hidden).contiguous().view(torch.int32))
    want_rs = np.float32(1.0 / (1.0 - 0.5)) / np.float32(1e-12)
    assert want_rs == np.float32(2.0 / 1e-12)
    np.testing.assert_array_equal(rowscale.cpu().numpy(), np.full(n_rows, want_rs, np.float32))
    # loss head: no entry, no term; lse does not read the CSR
    logits = torch.from_numpy(np.random.RandomState(52).standard_normal((n_rows, n_items)).astype(np.float32)).cuda()
    full = engine.csr_to_device(synth.synth_feed_csr(n_rows, n_items, 0.2, seed=53))
    loss, lse = engine.multinomial_nll_csr(logits, empty, row0=0, b=n_rows, check=False)
    _, lse_full = engine.multinomial_nll_csr(logits, full, row0=0, b=n_rows, check=False)
    assert float(loss) == 0.0
    assert torch.equal(lse.view(torch.int32), lse_full.view(torch.int32))
    # frozen encode hook: the CSR form against the dense form of a zero batch
    engine.vae_encoder_load(*tensors)
    z_csr = engine.vae_encode_csr(empty, row0=0, b=n_rows, check=False).cpu().numpy()
    z_dense = engine.vae_encode(torch.zeros(n_rows, n_items)).cpu().numpy()
    print(f"empty matrix, csr vs dense encode: rel_max {rel_max(z_csr, z_dense):.2e} rel_l2 {rel_l2(z_csr, z_dense):.2e}")
    assert rel_max(z_csr, z_dense) <= TOL and rel_l2(z_csr, z_dense) <= TOL
    engine.feed_status()   # nothing was raised


@pytest.mark.gpu
def test_rows_or_row0_and_b(engine):
    """Each method that takes a batch of the feed, called with neither `rows` nor `b`, says so under its own name."""
    from sdrm_amd.engine import SdrmError
    dev = engine.csr_to_device(csr_matrix(np.eye(5, dtype=np.float32)))
    logits = torch.zeros(5, 5, device="cuda")
    w1, b1, w2, b2 = (torch.from_numpy(t).cuda() for t in synth.synth_vae_encoder(5, 8, 2, seed=61))
    engine.vae_encoder_load(w1, b1, w2, b2)
    calls = {
        "csr_rows_to_dense": lambda: engine.csr_rows_to_dense(dev),
        "vae_encode_csr": lambda: engine.vae_encode_csr(dev),
        "multinomial_nll_csr": lambda: engine.multinomial_nll_csr(logits, dev),
        "multinomial_nll_csr_grad": lambda: engine.multinomial_nll_csr_grad(logits, torch.zeros(5, device="cuda"), dev),
        "vae_input_layer_fwd": lambda: engine.vae_input_layer_fwd(w1, b1, dev),
    }
    for name, call in calls.items():
        with pytest.raises(SdrmError, match=rf"\b{name}: give `rows` or `row0` and `b`"):
            call()
