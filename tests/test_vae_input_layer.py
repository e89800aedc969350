"""The input layer of the VAE encoder in train mode on the engine (reference train_SDRM.py:242-244, first Linear, and its weight's
share of :148), straight from the feed's CSR rows (forward) and CSC columns (weight gradient).

CPU: tests/vae_input_layer_ref.py (float64, from the formulas) against torch float64 autograd; the keep bits' statistics; what the
cases cover; the header and the ctypes table; `SparseFeed`; the host-side argument check; `sparse_input=True` ignored on the host.
GPU (-m gpu): parity with the restatement and with the device's own dense expression; the bit-level promises; autograd; the
loaded encoder left alone; the range checks; the pre-stage with `sparse_input=True`.

Bars: pre and dW1 rel_max and rel_l2 <= 1e-4 (the project's fp32 bar); rowscale relative <= 1e-5 (one over the root of a sum of
positive terms: condition number 1); loss of the first train batch <= 1e-5 relative."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import vae_input_layer_ref as ref
from vae_input_layer_ref import rel_l2, rel_max
from sdrm_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_SCALE, TOL_LOSS = 1e-4, 1e-5, 1e-5


@pytest.fixture(scope="module")
def cases():
    """Inputs and the float64 reference of every case, computed once: case dict + pre, rowscale, xt, dw1, db1."""
    out = []
    for i in range(len(ref.CASES)):
        c = ref.case_inputs(i)
        c["pre"], c["rowscale"], c["xt"] = ref.forward(c["w1"], c["b1"], c["m"], c["rows"], c["seed"], c["step"], c["p"])
        c["dw1"], c["db1"] = ref.backward(c["xt"], c["dpre"])
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- CPU
def test_restatement_matches_torch_float64_autograd(cases):
    for i, c in enumerate(cases):
        x = torch.from_numpy(c["m"][c["rows"]].toarray().astype(np.float64))
        mask = torch.from_numpy(ref.keep_mask(c["seed"], c["step"], c["rows"], c["n_items"], c["p"]).astype(np.float64))
        w1 = torch.from_numpy(c["w1"].astype(np.float64)).requires_grad_()
        b1 = torch.from_numpy(c["b1"].astype(np.float64)).requires_grad_()
        pre = (F.normalize(x, p=2, dim=1) * mask * float(ref.scale(c["p"]))) @ w1.T + b1
        pre.backward(torch.from_numpy(c["dpre"].astype(np.float64)))
        err = (rel_max(c["pre"], pre.detach().numpy()), rel_max(c["dw1"], w1.grad.numpy()), rel_max(c["db1"], b1.grad.numpy()))
        print(f"case {i}: pre {err[0]:.2e} dW1 {err[1]:.2e} db1 {err[2]:.2e}")
        assert max(err) <= 1e-12, (i, err)


def test_keep_bits():
    seed, n_rows, n_cols = 0x1234_5678_9ABC_DEF0, 200, 1000
    rows, cols = np.arange(n_rows)[:, None], np.arange(n_cols)[None, :]
    n = n_rows * n_cols
    assert n >= 200_000
    assert ref.keep_bits(seed, 5, rows, cols, 0.0).all()
    for p in (0.5, 0.3):
        share = ref.keep_bits(seed, 5, rows, cols, p).mean()
        sigma = np.sqrt(p * (1 - p) / n)
        print(f"p {p}: kept share {share:.5f}, {abs(share - (1 - p)) / sigma:.2f} sigma")
        assert abs(share - (1 - p)) <= 4 * sigma
    a, b = ref.keep_bits(seed, 5, rows, cols, 0.5), ref.keep_bits(seed, 6, rows, cols, 0.5)
    agree = (a == b).mean()
    print(f"two steps agree on {agree:.5f}")
    assert abs(agree - 0.5) <= 4 * np.sqrt(0.25 / n)
    # a row's bits do not depend on which other rows are asked for
    alone = ref.keep_mask(seed, 5, [37], n_cols, 0.5)
    among = ref.keep_mask(seed, 5, [3, 199, 37, 0], n_cols, 0.5)
    assert np.array_equal(alone[0], among[2]) and np.array_equal(alone[0], a[37])
    assert ref.threshold(0.5) == 2 ** 31 and ref.threshold(0.0) == 0 and float(ref.scale(0.5)) == 2.0


def test_cases_cover_what_the_kernels_branch_on(cases):
    hiddens, widths, batches = {c[0] for c in ref.CASES}, {c[1] for c in ref.CASES}, {c[2] for c in ref.CASES}
    assert {37, 200, 600, 1030} <= hiddens and max(hiddens) > 2048     # a wave per row, the work-group, two and four slices per thread
    assert {70, 1009} <= widths and {1, 33, 300} <= batches
    assert {c[3] for c in ref.CASES} == {"ones", "zeros"} and any(c[4] == 0 for c in ref.CASES)
    seen = dict(empty=False, long=False, dropped=False, full_column=False)
    for c in cases:
        m, rows = c["m"], c["rows"]
        assert m.shape == (ref.FEED_ROWS, c["n_items"]) and c["b"] < ref.FEED_ROWS          # non-members exist
        assert m.has_canonical_format and np.array_equal(c["order"][ref.LO:ref.LO + c["b"]], rows)
        assert np.array_equal(np.sort(c["order"]), np.arange(ref.FEED_ROWS))
        assert (m.data == 1).all() == (c["kind"] == "ones")
        if c["kind"] == "zeros":
            assert (m.data == 0).any() and m.data.max() == 5
        counts = np.diff(m.indptr)
        assert counts[ref.ROW_EMPTY] == 0 and counts[ref.ROW_SINGLE] == 1 and counts[ref.ROW_LONG] == min(600, c["n_items"] - 1)
        assert m.tocsc()[:, c["n_items"] - 2].nnz == 0                                       # a column nobody touches
        seen["empty"] |= ref.ROW_EMPTY in rows
        if c["n_items"] > 600:
            seen["long"] |= ref.ROW_LONG in rows
        if ref.ROW_SINGLE in rows and c["p"] > 0:
            col = m.indices[m.indptr[ref.ROW_SINGLE]]
            assert not ref.keep_bits(c["seed"], c["step"], [ref.ROW_SINGLE], [col], c["p"])[0]
            assert not c["xt"][list(rows).index(ref.ROW_SINGLE)].any()
            seen["dropped"] = True
        if c["b"] == 300:
            mc = m.tocsc()
            assert np.isin(rows, mc.indices[mc.indptr[ref.ALL_COLUMN]:mc.indptr[ref.ALL_COLUMN + 1]]).all()   # 300 members: more than one chunk of 256
            seen["full_column"] = True
    assert all(seen.values()), seen


def test_header_and_ctypes_table_carry_the_entry_points():
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    from sdrm_amd import _lib
    for name, n_args in (("sdrm_vae_input_layer_fwd", 18), ("sdrm_vae_input_layer_wgrad", 17)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "PURPOSE_VAE_DROP = 7" in open(os.path.join(REPO, "sdrm_amd", "csrc", "philox.h")).read()
    from sdrm_amd import train_SDRM as ts, vae_hooks
    assert ts.sparse_input_linear is vae_hooks.sparse_input_linear and ts.SparseFeed is vae_hooks.SparseFeed


def test_host_side_argument_check():
    from sdrm_amd import _lib
    lib = _lib.load()
    thr, scale = C.c_uint32(), C.c_float()
    ok = dict(n_items=1009, hidden=600, n_rows=400, first=17, b=33, contiguous=1)

    def call(p=0.5, **kw):
        a = dict(ok, **kw)
        return lib.sdrm_debug_input_layer_args(a["n_items"], a["hidden"], a["n_rows"], a["first"], a["b"], a["contiguous"], p, C.byref(thr), C.byref(scale))

    for p in (0.0, 0.3, 0.5, 0.999):
        assert call(p) == 0
        assert thr.value == ref.threshold(p) and np.float32(scale.value) == ref.scale(p), (p, thr.value, scale.value)
    assert lib.sdrm_debug_input_layer_args(1, 1, 1, 0, 1, 1, 0.5, None, None) == 0
    assert call(hidden=4096) == 0 and call(n_items=1 << 20) == 0 and call(first=367) == 0 and call(first=390, contiguous=0) == 0
    for bad in (dict(hidden=4097), dict(hidden=0), dict(n_items=0), dict(n_items=(1 << 20) + 1), dict(n_rows=0), dict(n_rows=1 << 31), dict(b=0),
                dict(b=(1 << 22) + 1), dict(first=-1), dict(first=368)):
        assert call(**bad) == -2, bad                                                          # SDRM_ERR_SHAPE
    for p in (1.0, -0.1, 1.5, float("nan")):
        assert call(p) == -2, p


class _HostEngine:
    """`csr_to_device` / `csc_to_device` of the engine, on the host (the two methods touch nothing else of it)."""
    device = torch.device("cpu")
    from sdrm_amd.engine import Engine
    csr_to_device, csc_to_device = Engine.csr_to_device, Engine.csc_to_device


def test_sparse_feed_forms_and_order():
    import scipy.sparse
    from sdrm_amd.vae_hooks import SparseFeed
    from sdrm_amd.engine import SdrmError
    ones = synth.synth_feed_csr(53, 40, 0.2, seed=71, ratings=False)
    rated = ref.case_feed(70, "zeros", *ref.case_seed(0), 0.5)
    assert (rated.data == 0).any()
    dup = scipy.sparse.coo_matrix((np.ones(4, np.float32), ([0, 0, 2, 1], [3, 3, 1, 0])), shape=(3, 5))   # a duplicate: summed to 2
    for m in (ones, rated, dup):
        feed = SparseFeed(m, engine=_HostEngine())
        indptr, indices, data, shape = feed.csr
        colptr, rowidx, cdata, cshape = feed.csc
        assert tuple(shape) == tuple(cshape) == m.shape == feed.shape
        assert (data is None) == (cdata is None) == (m is ones)
        assert indptr.dtype == colptr.dtype == torch.int64 and indices.dtype == rowidx.dtype == torch.int32
        want = np.asarray(m.toarray(), np.float32)
        a = scipy.sparse.csr_matrix((np.ones(indices.numel(), np.float32) if data is None else data.numpy(), indices.numpy(), indptr.numpy()), shape=m.shape)
        b = scipy.sparse.csc_matrix((np.ones(rowidx.numel(), np.float32) if cdata is None else cdata.numpy(), rowidx.numpy(), colptr.numpy()), shape=m.shape)
        assert np.array_equal(a.toarray(), want) and np.array_equal(b.toarray(), want)
        assert a.nnz == b.nnz == (3 if m is dup else m.nnz)                                    # duplicates summed, stored zeros stay stored
        assert all(np.all(np.diff(rowidx.numpy()[colptr[c]:colptr[c + 1]]) > 0) for c in range(m.shape[1]))
        assert feed.order is None and feed.pos is None
        order = np.random.RandomState(5).permutation(m.shape[0])
        feed.set_order(order)
        assert feed.order.dtype == torch.int64 and feed.pos.dtype == torch.int32
        assert np.array_equal(feed.order.numpy(), order) and np.array_equal(feed.pos.numpy()[order], np.arange(m.shape[0]))
        with pytest.raises(SdrmError):
            feed.set_order(np.zeros(m.shape[0], np.int64))


def test_sparse_input_is_ignored_for_a_model_on_the_host(tmp_path):
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    m = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)

    def run(where, **kw):
        torch.manual_seed(3)
        np.random.seed(4)
        vae = VAE(60, 16, 8)
        train_variational_autoencoder(vae, m, m, 2, 16, 1e-3, "Recall@10", str(where), **kw)
        return vae, sorted(f for f in os.listdir(where) if f.startswith("epoch-")), np.random.get_state()

    a, best_a, state_a = run(tmp_path / "a")
    b, best_b, state_b = run(tmp_path / "b", device_feed=True, sparse_input=True)
    c, best_c, _ = run(tmp_path / "c", sparse_input=True)
    assert best_a == best_b == best_c and a.model_is_trained and b.model_is_trained and c.model_is_trained
    assert np.array_equal(state_a[1], state_b[1]) and state_a[2:] == state_b[2:]               # no extra draw either
    for (name, p), (_, q), (_, r) in zip(a.state_dict().items(), b.state_dict().items(), c.state_dict().items()):
        assert torch.equal(p, q) and torch.equal(p, r), name


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def engine():
    from sdrm_amd.engine import utility_engine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return utility_engine()


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _close(got, want, what, tol=TOL):
    print(f"{what}: rel_max {rel_max(got, want):.2e} rel_l2 {rel_l2(got, want):.2e}")
    assert got.shape == want.shape, what
    assert rel_max(got, want) <= tol and rel_l2(got, want) <= tol, (what, rel_max(got, want), rel_l2(got, want))


def _pos(order):
    pos = np.empty(order.size, np.int32)
    pos[order] = np.arange(order.size, dtype=np.int32)
    return pos


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_hip_input_layer_vs_fp64(engine, cases, i):
    c = cases[i]
    csr, csc = engine.csr_to_device(c["m"]), engine.csc_to_device(c["m"])
    assert (csr[2] is None) == (csc[2] is None) == (c["kind"] == "ones")
    w1, b1, dpre = _cuda(c["w1"]), _cuda(c["b1"]), _cuda(c["dpre"])
    kw = dict(seed=c["seed"], step=c["step"], p_drop=c["p"])
    pre, rowscale = engine.vae_input_layer_fwd(w1, b1, csr, rows=_cuda(c["rows"]), **kw)
    _close(pre.cpu().numpy(), c["pre"], f"case {i} pre")
    rs_err = np.abs(rowscale.cpu().numpy() / c["rowscale"] - 1).max()
    print(f"case {i} rowscale rel {rs_err:.2e}")
    assert rs_err <= TOL_SCALE
    dw1 = torch.full((c["hidden"], c["n_items"]), float("nan"), device="cuda")
    got = engine.vae_input_layer_wgrad(dpre, rowscale, csc, pos=_cuda(_pos(c["order"])), lo=ref.LO, b=c["b"], out=dw1, **kw)
    assert got.data_ptr() == dw1.data_ptr()
    g = dw1.cpu().numpy()
    assert np.isfinite(g).all()
    _close(g, c["dw1"], f"case {i} dW1")
    untouched = ~c["xt"].any(axis=0)
    assert untouched[c["n_items"] - 2] and not g[:, untouched].any() and not np.signbit(g[:, untouched]).any()   # exact +0.0
    if ref.ROW_SINGLE in c["rows"] and c["p"] > 0:   # the one-entry row, dropped: its pre is the bias
        assert np.array_equal(pre[list(c["rows"]).index(ref.ROW_SINGLE)].cpu().numpy(), c["b1"])
    engine.feed_status()


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 2, 4])
def test_no_dropout_against_the_dense_expression_on_the_device(engine, cases, i):
    c = cases[i]
    csr, csc = engine.csr_to_device(c["m"]), engine.csc_to_device(c["m"])
    w1, b1, dpre = _cuda(c["w1"]).requires_grad_(), _cuda(c["b1"]), _cuda(c["dpre"])
    x = engine.csr_rows_to_dense(csr, rows=_cuda(c["rows"]))
    want = F.linear(F.normalize(x, p=2, dim=1), w1, b1)
    want.backward(dpre)
    pre, rowscale = engine.vae_input_layer_fwd(w1.detach(), b1, csr, rows=_cuda(c["rows"]), seed=1, step=2, p_drop=0.0)
    dw1 = engine.vae_input_layer_wgrad(dpre, rowscale, csc, pos=_cuda(_pos(c["order"])), lo=ref.LO, b=c["b"], seed=1, step=2, p_drop=0.0)
    _close(pre.cpu().numpy(), want.detach().cpu().numpy(), f"case {i} p = 0 pre vs torch")
    _close(dw1.cpu().numpy(), w1.grad.cpu().numpy(), f"case {i} p = 0 dW1 vs torch")


@pytest.mark.gpu
def test_bit_level_promises(engine, cases):
    c = cases[1]                                        # hidden 200, 1009 items (rows off 16-byte boundaries), ratings with zeros
    csr, csc = engine.csr_to_device(c["m"]), engine.csc_to_device(c["m"])
    w1, b1 = _cuda(c["w1"]), _cuda(c["b1"])
    kw = dict(seed=c["seed"], step=c["step"], p_drop=c["p"])
    everything, rs_all = engine.vae_input_layer_fwd(w1, b1, csr, row0=0, b=ref.FEED_ROWS, **kw)
    rows = _cuda(c["rows"])
    pre, rs = engine.vae_input_layer_fwd(w1, b1, csr, rows=rows, **kw)
    assert torch.equal(pre, everything[rows]) and torch.equal(rs, rs_all[rows])                       # another place, another batch size
    sub = torch.flip(rows[:33], dims=(0,))
    pre_s, rs_s = engine.vae_input_layer_fwd(w1, b1, csr, rows=sub, **kw)
    assert torch.equal(pre_s, everything[sub]) and torch.equal(rs_s, rs_all[sub])
    pre_o, rs_o = engine.vae_input_layer_fwd(w1, b1, csr, row0=123, b=37, **kw)
    assert torch.equal(pre_o, everything[123:160]) and torch.equal(rs_o, rs_all[123:160])             # row0 / b against rows
    pre_1, _ = engine.vae_input_layer_fwd(w1, b1, csr, rows=rows[5:6], **kw)
    assert torch.equal(pre_1[0], pre[5])
    # data = null against explicit ones
    k = cases[2]
    d_none, s_none = engine.csr_to_device(k["m"]), engine.csc_to_device(k["m"])
    assert d_none[2] is None and s_none[2] is None
    d_ones = (d_none[0], d_none[1], torch.ones(k["m"].nnz, device="cuda"), d_none[3])
    s_ones = (s_none[0], s_none[1], torch.ones(k["m"].nnz, device="cuda"), s_none[3])
    kk = dict(seed=k["seed"], step=k["step"], p_drop=k["p"])
    kw1, kb1, kd = _cuda(k["w1"]), _cuda(k["b1"]), _cuda(k["dpre"])
    f_none = engine.vae_input_layer_fwd(kw1, kb1, d_none, rows=_cuda(k["rows"]), **kk)
    f_ones = engine.vae_input_layer_fwd(kw1, kb1, d_ones, rows=_cuda(k["rows"]), **kk)
    assert torch.equal(f_none[0], f_ones[0]) and torch.equal(f_none[1], f_ones[1])
    kpos = _cuda(_pos(k["order"]))
    g_none = engine.vae_input_layer_wgrad(kd, f_none[1], s_none, pos=kpos, lo=ref.LO, b=k["b"], **kk)
    g_ones = engine.vae_input_layer_wgrad(kd, f_none[1], s_ones, pos=kpos, lo=ref.LO, b=k["b"], **kk)
    assert torch.equal(g_none, g_ones)
    # weight gradient: twice the same bits; any order of the batch with its pos; pos = None against the identity map
    dpre = _cuda(c["dpre"])
    pos = _cuda(_pos(c["order"]))
    g_a = engine.vae_input_layer_wgrad(dpre, rs, csc, pos=pos, lo=ref.LO, b=c["b"], **kw)
    g_b = engine.vae_input_layer_wgrad(dpre, rs, csc, pos=pos, lo=ref.LO, b=c["b"], **kw)
    assert torch.equal(g_a, g_b)
    shuffle = np.random.RandomState(6).permutation(c["b"])
    order2 = c["order"].copy()
    order2[ref.LO:ref.LO + c["b"]] = c["rows"][shuffle]
    sh = _cuda(shuffle)
    g_p = engine.vae_input_layer_wgrad(dpre[sh].contiguous(), rs[sh].contiguous(), csc, pos=_cuda(_pos(order2)), lo=ref.LO, b=c["b"], **kw)
    assert torch.equal(g_p, g_a)
    pre_r, rs_r = engine.vae_input_layer_fwd(w1, b1, csr, row0=40, b=c["b"], **kw)
    ident = torch.arange(ref.FEED_ROWS, dtype=torch.int32, device="cuda")
    g_i = engine.vae_input_layer_wgrad(dpre, rs_r, csc, pos=ident, lo=40, b=c["b"], **kw)
    g_n = engine.vae_input_layer_wgrad(dpre, rs_r, csc, pos=None, lo=40, b=c["b"], **kw)
    assert torch.equal(g_i, g_n)
    engine.feed_status()


@pytest.mark.gpu
def test_autograd_function_in_a_small_graph(engine, cases):
    from sdrm_amd.train_SDRM import SparseFeed, sparse_input_linear
    c = cases[2]                                        # hidden 600, batch of 33 with the three special rows, p = 0.3
    feed = SparseFeed(c["m"], engine=engine)
    feed.set_order(c["order"])
    torch.manual_seed(11)
    head = torch.nn.Linear(c["hidden"], 5).cuda()
    w1, b1 = _cuda(c["w1"]).requires_grad_(), _cuda(c["b1"]).requires_grad_()
    loss = head(torch.tanh(sparse_input_linear(w1, b1, feed, ref.LO, ref.LO + c["b"], c["seed"], c["step"], c["p"]))).pow(2).mean()
    loss.backward()
    xt = _cuda(c["xt"], torch.float32)                  # the dense masked input of the restatement
    w2, b2 = w1.detach().clone().requires_grad_(), b1.detach().clone().requires_grad_()
    want = head(torch.tanh(F.linear(xt, w2, b2))).pow(2).mean()
    want.backward()
    print(f"loss {float(loss):.8g} dense {float(want):.8g}")
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    _close(w1.grad.cpu().numpy(), w2.grad.cpu().numpy(), "w1.grad")
    _close(b1.grad.cpu().numpy(), b2.grad.cpu().numpy(), "b1.grad")
    # W1 updated in place between two calls: the second call reads the new weights
    with torch.no_grad():
        first = sparse_input_linear(w1, b1, feed, ref.LO, ref.LO + c["b"], c["seed"], c["step"], c["p"])
        w1.mul_(-2.0)
        second = sparse_input_linear(w1, b1, feed, ref.LO, ref.LO + c["b"], c["seed"], c["step"], c["p"])
    _close((second - b1).detach().cpu().numpy(), (-2.0 * (first - b1)).detach().cpu().numpy(), "after the in-place update")
    # without an order the batch is a contiguous range of the feed
    plain = SparseFeed(c["m"], engine=engine)
    pre = sparse_input_linear(w1.detach(), b1.detach(), plain, 40, 73, c["seed"], c["step"], c["p"])
    want_pre, _ = engine.vae_input_layer_fwd(w1.detach(), b1.detach(), plain.csr, row0=40, b=33, seed=c["seed"], step=c["step"], p_drop=c["p"])
    assert torch.equal(pre, want_pre)
    engine.feed_status()


@pytest.mark.gpu
def test_a_loaded_encoder_is_left_alone(engine, cases):
    c = cases[0]
    rng = np.random.RandomState(31)
    hidden, n_items, latent = 48, c["n_items"], 8
    enc = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in ((hidden, n_items), (hidden,), (2 * latent, hidden), (2 * latent,))]
    engine.vae_encoder_load(*enc)
    csr = engine.csr_to_device(c["m"])
    before = engine.vae_encode_csr(csr, row0=0, b=ref.FEED_ROWS)
    engine.vae_input_layer_fwd(_cuda(c["w1"]), _cuda(c["b1"]), csr, row0=0, b=ref.FEED_ROWS, seed=c["seed"], step=c["step"], p_drop=c["p"])
    after = engine.vae_encode_csr(csr, row0=0, b=ref.FEED_ROWS)
    assert torch.equal(before, after)


@pytest.mark.gpu
def test_range_checks_raise_and_spare_the_rest(engine, cases):
    from sdrm_amd.engine import SdrmError
    c = cases[2]
    m = c["m"]
    csr, csc = engine.csr_to_device(m), engine.csc_to_device(m)
    w1, b1, dpre = _cuda(c["w1"]), _cuda(c["b1"]), _cuda(c["dpre"])
    kw = dict(seed=c["seed"], step=c["step"], p_drop=0.0)      # nothing dropped: the offending entry would have counted
    rows, pos = _cuda(c["rows"]), _cuda(_pos(c["order"]))
    pre_w, rs_w = engine.vae_input_layer_fwd(w1, b1, csr, rows=rows, **kw)
    g_w = engine.vae_input_layer_wgrad(dpre, rs_w, csc, pos=pos, lo=ref.LO, b=c["b"], **kw)
    # forward: one column index == n_items, in the first entry of an ordinary batch row
    counts = np.diff(m.indptr)
    j = next(k for k, r in enumerate(c["rows"]) if 1 < counts[r] < 600)
    victim = int(c["rows"][j])
    p = int(m.indptr[victim])
    bad_idx = csr[1].clone()
    bad_idx[p] = c["n_items"]
    pre, rs = engine.vae_input_layer_fwd(w1, b1, (csr[0], bad_idx, csr[2], csr[3]), rows=rows, check=False, **kw)
    with pytest.raises(SdrmError, match="column index"):
        engine.feed_status()
    engine.feed_status()                                        # raised once, clean afterwards
    keep = torch.ones(c["b"], dtype=torch.bool, device="cuda")
    keep[j] = False
    assert torch.isfinite(pre).all() and torch.isfinite(rs).all()
    assert torch.equal(pre[keep], pre_w[keep]) and torch.equal(rs[keep], rs_w[keep])
    m4 = m.copy().tolil()
    m4[victim, m.indices[p]] = 0
    m4 = m4.tocsr()
    m4.eliminate_zeros()
    assert m4.nnz == m.nnz - 1
    want4, want_rs4, _ = ref.forward(c["w1"], c["b1"], m4, c["rows"], c["seed"], c["step"], 0.0)
    _close(pre[j].cpu().numpy(), want4[j], "the row without its offending entry")
    assert abs(float(rs[j]) / want_rs4[j] - 1) <= TOL_SCALE
    # weight gradient: one row index == n_rows, in the entry (victim, first column)
    col = int(m.indices[p])
    mc = m.tocsc()
    at = int(mc.indptr[col] + np.searchsorted(mc.indices[mc.indptr[col]:mc.indptr[col + 1]], victim))
    assert mc.indices[at] == victim
    bad_row = csc[1].clone()
    bad_row[at] = ref.FEED_ROWS
    g = engine.vae_input_layer_wgrad(dpre, rs_w, (csc[0], bad_row, csc[2], csc[3]), pos=pos, lo=ref.LO, b=c["b"], check=False, **kw)
    with pytest.raises(SdrmError, match="row id"):
        engine.feed_status()
    engine.feed_status()
    others = torch.ones(c["n_items"], dtype=torch.bool, device="cuda")
    others[col] = False
    assert torch.isfinite(g).all() and torch.equal(g[:, others], g_w[:, others])
    xt4 = ref.forward(c["w1"], c["b1"], m, c["rows"], c["seed"], c["step"], 0.0)[2]
    xt4[j, col] = 0.0                                           # the entry is gone, the row's scale is the full row's
    _close(g[:, col].cpu().numpy(), ref.backward(xt4, c["dpre"])[0][:, col], "the column without its offending entry")
    # weight gradient: colptr[col + 1] < colptr[col]: that column counts as empty, no other but its right neighbour changes
    bad_ptr = csc[0].clone()
    bad_ptr[col + 1] = bad_ptr[col] - 1
    g = engine.vae_input_layer_wgrad(dpre, rs_w, (bad_ptr, csc[1], csc[2], csc[3]), pos=pos, lo=ref.LO, b=c["b"], check=False, **kw)
    with pytest.raises(SdrmError, match="not ordered"):
        engine.feed_status()
    engine.feed_status()
    others[col + 1] = False
    assert torch.isfinite(g).all() and not g[:, col].any() and torch.equal(g[:, others], g_w[:, others])
    # host-side refusals, before any launch
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_input_layer_fwd(w1, b1, csr, row0=390, b=33, **kw)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_input_layer_fwd(w1, b1, csr, rows=rows, seed=1, step=1, p_drop=1.0)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_input_layer_wgrad(dpre, rs_w, csc, pos=pos, lo=390, b=c["b"], **kw)
    with pytest.raises(SdrmError):
        engine.vae_input_layer_wgrad(dpre.double(), rs_w, csc, pos=pos, lo=ref.LO, b=c["b"], **kw)
    engine.feed_status()


@pytest.mark.gpu
def test_pre_stage_with_sparse_input(tmp_path, monkeypatch):
    """40 users x 60 items, batch 16, two epochs.  With the flag no train batch is densified; with p_drop = 0 (torch's dropout then
    draws nothing either) the first train batch's loss is that of the `device_feed=True` run from the same seeds.  Nothing behind
    the first Adam step is compared: Adam's first step turns sign-level gradient differences into full-size steps."""
    import inspect
    from sdrm_amd.engine import Engine, utility_engine
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    users, n_items, batch, epochs = 40, 60, 16, 2
    m = synth.synth_feed_csr(users, n_items, 0.2, seed=72, ratings=False)
    calls = {"dense": 0, "dense_train": 0, "first_loss": None, "losses": []}
    orig_dense, orig_backward = Engine.csr_rows_to_dense, torch.Tensor.backward

    def dense(self, *a, **kw):
        calls["dense"] += 1
        calls["dense_train"] += int(torch.is_grad_enabled())     # the evaluation half runs under no_grad
        return orig_dense(self, *a, **kw)

    def backward(self, *a, **kw):
        if calls["first_loss"] is None:
            calls["first_loss"] = self.detach().clone()
        calls["losses"].append(self.detach())
        return orig_backward(self, *a, **kw)

    monkeypatch.setattr(Engine, "csr_rows_to_dense", dense)
    monkeypatch.setattr(torch.Tensor, "backward", backward)
    assert "sparse_input" in inspect.signature(train_variational_autoencoder).parameters

    def run(where, p_drop, **kw):
        calls.update(dense=0, dense_train=0, first_loss=None, losses=[])
        torch.manual_seed(21)
        np.random.seed(22)
        vae = VAE(60, 16, 8, p_drop=p_drop).cuda()
        train_variational_autoencoder(vae, m, m, epochs, batch, 1e-3, "Recall@10", str(where), device_feed=True, **kw)
        files = sorted(f for f in os.listdir(where) if f.startswith("epoch-"))
        return vae, float(calls["first_loss"].cpu()), torch.stack(calls["losses"]).cpu().numpy(), files, dict(calls)

    vae, _, losses, files, seen = run(tmp_path / "a", 0.5, sparse_input=True)
    assert np.isfinite(losses).all() and losses.size == epochs * -(-users // batch)
    assert files and vae.model_is_trained and vae.is_training == 0
    assert seen["dense_train"] == 0 and seen["dense"] == epochs                # one 500-row evaluation slice per epoch, nothing else
    utility_engine().feed_status()
    # p_drop = 0: the same first loss as the dense device feed.  The flagged run draws its seed from numpy first, so its first
    # permutation is the unflagged run's only if that draw is replayed in front of the unflagged run.
    np.random.seed(22)
    np.random.randint(2 ** 63, dtype=np.int64)
    state = np.random.get_state()

    def run_from(where, **kw):
        calls.update(dense=0, dense_train=0, first_loss=None, losses=[])
        torch.manual_seed(21)
        vae = VAE(60, 16, 8, p_drop=0).cuda()
        if kw.get("sparse_input"):
            np.random.seed(22)
        else:
            np.random.set_state(state)
        train_variational_autoencoder(vae, m, m, epochs, batch, 1e-3, "Recall@10", str(where), device_feed=True, **kw)
        return float(calls["first_loss"].cpu()), dict(calls)

    loss_b, seen_b = run_from(tmp_path / "b")
    loss_c, seen_c = run_from(tmp_path / "c", sparse_input=True)
    print(f"first train batch: device feed {loss_b:.8g} sparse input {loss_c:.8g} rel {abs(loss_b - loss_c) / abs(loss_b):.2e}")
    assert seen_b["dense_train"] == epochs * -(-users // batch) and seen_c["dense_train"] == 0
    assert abs(loss_b - loss_c) <= TOL_LOSS * abs(loss_b)
    utility_engine().feed_status()
