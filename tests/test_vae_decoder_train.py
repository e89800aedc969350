"""The VAE decoder and the multinomial loss in train mode on the engine (reference train_SDRM.py:252-254, :141-142 and their share of
:148), csrc/decoder_train.h.

CPU: tests/vae_decoder_ref.py (float64, from the formulas) against torch float64 autograd of `-mean(sum(log_softmax(decoder(z)) * X))`;
the header and the ctypes table; the host-side argument check; `device_decoder=True` ignored on the host.
GPU (-m gpu): both directions against the restatement; the bit-level promises; scratch shared by batches of different sizes; `decoder_nll`
in a small graph; the neighbours left alone; the refusals; the pre-stage with all five flags.

Bars: every tensor rel_max and rel_l2 <= 1e-4 against the float64 restatement and the loss <= 1e-5 relative (the project's fp32 bars,
tests/test_vae_latent.py).  Case numbers count from 0; even cases address their batch through `rows`, odd ones through `row0`."""
import os
import re

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import vae_decoder_ref as ref
from vae_decoder_ref import rel_l2, rel_max
from sdrm_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_LOSS = 1e-4, 1e-5
GRADS = ("dz", "dw3", "db3", "dw4", "db4")


@pytest.fixture(scope="module")
def cases():
    """Inputs and the float64 reference of every case, computed once: case dict + fwd, bwd."""
    out = []
    for i in range(len(ref.CASES)):
        c = ref.case_inputs(i)
        c["fwd"] = ref.forward(c["z"], c["w3"], c["b3"], c["w4"], c["b4"], c["X"])
        c["bwd"] = ref.backward(c["fwd"], c["z"], c["w3"], c["w4"], c["X"], c["scale"])
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- CPU
def test_restatement_matches_torch_float64_autograd(cases):
    for i, c in enumerate(cases[:-1]):
        z, w3, b3, w4, b4 = (torch.from_numpy(c[k].astype(np.float64)).requires_grad_() for k in ("z", "w3", "b3", "w4", "b4"))
        X = torch.from_numpy(c["X"])
        out = F.linear(torch.tanh(F.linear(z, w3, b3)), w4, b4)
        loss = -torch.mean(torch.sum(F.log_softmax(out, dim=1) * X, dim=1))
        (c["scale"] * loss).backward()
        f, g = c["fwd"], c["bwd"]
        err = dict(loss=abs(float(f["loss"]) / float(loss.detach()) - 1), dz=rel_max(g["dz"], z.grad.numpy()), dw3=rel_max(g["dw3"], w3.grad.numpy()),
                   db3=rel_max(g["db3"], b3.grad.numpy()), dw4=rel_max(g["dw4"], w4.grad.numpy()), db4=rel_max(g["db4"], b4.grad.numpy()))
        print(f"case {i}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert max(err.values()) <= 1e-10, (i, err)
    # every feed of more than two rows holds an empty row and a row with every column, and the batches with room for them take both
    for i, c in enumerate(cases):
        nnz = np.diff(c["m"].indptr)
        assert nnz.min() == 0 and nnz.max() == c["n_items"], i
        if c["b"] >= 4:
            per_row = (c["X"] != 0).sum(axis=1)
            assert per_row.min() == 0 and per_row.max() == c["n_items"], i
        assert bool(np.all(c["m"].data == 1)) == (not c["ratings"]), i


def test_header_and_ctypes_table_carry_the_entry_points():
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    debug = open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    from sdrm_amd import _lib
    for text, name, n_args in ((header, "sdrm_vae_decoder_nll_fwd", 15), (header, "sdrm_vae_decoder_nll_bwd", 20),
                               (debug, "sdrm_debug_decoder_nll_args", 7)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    from sdrm_amd import train_SDRM as ts, vae_hooks
    assert ts.decoder_nll is vae_hooks.decoder_nll and vae_hooks.DECODER_HEAD_MAX_HIDDEN == 4096
    from sdrm_amd.engine import Engine
    assert callable(Engine.vae_decoder_nll_fwd) and callable(Engine.vae_decoder_nll_bwd) and callable(vae_hooks.VAE.decode_nll)


def test_host_side_argument_check():
    from sdrm_amd import _lib
    lib = _lib.load()
    ok = dict(latent=83, hidden=600, n_items=1000, b=130, row0=17, n_rows=500, contiguous=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdrm_debug_decoder_nll_args(a["latent"], a["hidden"], a["n_items"], a["b"], a["row0"], a["n_rows"], a["contiguous"])

    assert call() == 0 and lib.sdrm_debug_decoder_nll_args(1, 1, 1, 1, 0, 1, 1) == 0
    assert call(latent=4096) == 0 and call(hidden=4096) == 0 and call(n_items=1 << 20) == 0
    assert call(b=1 << 22, n_rows=1 << 22, row0=0) == 0
    assert call(n_items=(1 << 18) - 1, b=1 << 22, n_rows=1 << 23, row0=0) == 0                       # b x n_items = 2^40 - 2^22
    assert call(row0=370) == 0 and call(row0=0) == 0                                                 # a contiguous range ends at the feed's end
    assert call(row0=10 ** 12, contiguous=0) == 0                                                    # with a `rows` array the range is not formed
    for bad in (dict(latent=0), dict(latent=4097), dict(hidden=0), dict(hidden=4097), dict(n_items=0), dict(n_items=(1 << 20) + 1), dict(b=0),
                dict(b=(1 << 22) + 1, n_rows=1 << 23), dict(n_items=1 << 18, b=1 << 22, n_rows=1 << 23, row0=0), dict(row0=371), dict(row0=-1),
                dict(row0=-1, contiguous=0), dict(n_rows=0, contiguous=0), dict(hidden=-5), dict(b=-1)):
        assert call(**bad) == -2, bad                                                                # SDRM_ERR_SHAPE
    # The weight gradient of W4 reads g [b, Ip] along the batch: the GEMM refuses (K chunk + 64) x Ip x 4 bytes >= 2^32.  At n_items =
    # 2^20 the default chunk of 8192 rows would be refused for every batch of more than 928 + 32 rows; the chunk chosen from Ip keeps it
    # legal, at two slabs and at the envelope's largest b x n_items alike.
    n_items, b = 1 << 20, 8200
    Kb = -(-b // 32) * 32
    assert (min(Kb, 8192) + 64) * n_items * 4 >= 1 << 32
    chosen = min(8192, (((1 << 30) - 1) // n_items - 64) // 32 * 32)
    assert chosen == 928 and (chosen + 64) * n_items * 4 < 1 << 32 and (chosen + 32 + 64) * n_items * 4 >= 1 << 32
    assert call(n_items=n_items, b=b, n_rows=b, row0=0) == 0
    assert call(n_items=n_items, b=(1 << 20) - 1, n_rows=1 << 20, row0=0) == 0
    assert call(n_items=130049, b=8200, n_rows=8200, row0=0) == 0                                    # the first Ip (130080) that needs a smaller chunk


def test_device_decoder_is_ignored_for_a_model_on_the_host(tmp_path, monkeypatch):
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    m = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)
    losses = []
    orig_backward = torch.Tensor.backward

    def backward(self, *a, **kw):
        losses.append(float(self.detach()))
        return orig_backward(self, *a, **kw)

    monkeypatch.setattr(torch.Tensor, "backward", backward)

    def run(where, **kw):
        del losses[:]
        torch.manual_seed(3)
        np.random.seed(4)
        vae = VAE(60, 16, 8)
        train_variational_autoencoder(vae, m, m, 2, 16, 1e-3, "Recall@10", str(where), **kw)
        return vae, list(losses), sorted(f for f in os.listdir(where) if f.startswith("epoch-")), np.random.get_state()

    a, loss_a, best_a, state_a = run(tmp_path / "a")
    b, loss_b, best_b, state_b = run(tmp_path / "b", device_feed=True, sparse_input=True, device_holdout=True, device_latent=True,
                                     device_decoder=True)
    c, loss_c, best_c, state_c = run(tmp_path / "c", device_decoder=True)
    assert len(loss_a) == 2 * 3 and loss_a == loss_b == loss_c
    assert best_a == best_b == best_c and a.model_is_trained and b.model_is_trained and c.model_is_trained
    for st in (state_b, state_c):
        assert np.array_equal(state_a[1], st[1]) and state_a[2:] == st[2:]                         # no extra draw either
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
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    print(f"{what}: rel_max {rel_max(got, want):.2e} rel_l2 {rel_l2(got, want):.2e}")
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    assert rel_max(got, want) <= tol and rel_l2(got, want) <= tol, (what, rel_max(got, want), rel_l2(got, want))


def _dev_inputs(eng, c):
    """The case's five tensors, its feed and its batch keywords on the engine's device."""
    t = tuple(_cuda(c[k]) for k in ("z", "w3", "b3", "w4", "b4"))
    csr = eng.csr_to_device(c["m"])
    assert (csr[2] is not None) == c["ratings"]
    batch = dict(rows=_cuda(c["rows"])) if c["rows"] is not None else dict(row0=c["row0"], b=c["b"])
    return t, csr, batch


def _forward(eng, c, what):
    t, csr, batch = _dev_inputs(eng, c)
    loss, saved = eng.vae_decoder_nll_fwd(*t, csr, **batch)
    f = c["fwd"]
    for name, got in zip(("h3", "logits", "lse"), saved):
        _close(got, f[name], f"{what} {name}")
    err = abs(float(loss) / float(f["loss"]) - 1)
    print(f"{what} loss {float(loss):.8g} rel {err:.2e}")
    assert err <= TOL_LOSS
    return loss, saved


def _saved64(c):
    """The forward's float64 values as the float32 tensors a forward would have left."""
    return tuple(_cuda(c["fwd"][k], torch.float32) for k in ("h3", "logits", "lse"))


def _nan_out(c):
    L, H, I, b = c["latent"], c["hidden"], c["n_items"], c["b"]
    return tuple(torch.full(s, float("nan"), device="cuda") for s in ((b, L), (H, L), (H,), (I, H), (I,)))


def _backward(eng, c, what):
    t, csr, batch = _dev_inputs(eng, c)
    out = _nan_out(c)
    got = eng.vae_decoder_nll_bwd(_saved64(c), *t, csr, **batch, scale=torch.tensor(c["scale"], device="cuda"), out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    for name, g in zip(GRADS, got):
        _close(g, c["bwd"][name], f"{what} {name}")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_hip_forward_vs_fp64(engine, cases, i):
    _forward(engine, cases[i], f"case {i}")
    if i <= 1:                                          # the narrowest case and the one of several row tiles, under every tile shape
        try:
            for tile in range(5):
                engine.debug_set(tile=tile)
                _forward(engine, cases[i], f"case {i} tile {tile}")
        finally:
            engine.debug_set(tile=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_hip_backward_vs_fp64(engine, cases, i):
    c = cases[i]
    full = _backward(engine, c, f"case {i}")
    if i <= 1:
        try:
            for tile in range(5):
                engine.debug_set(tile=tile)
                _backward(engine, c, f"case {i} tile {tile}")
        finally:
            engine.debug_set(tile=-1)
    # need_dz=False: no dz, the other four as before; a null scale is 1
    t, csr, batch = _dev_inputs(engine, c)
    out = _nan_out(c)
    got = engine.vae_decoder_nll_bwd(_saved64(c), *t, csr, **batch, scale=torch.tensor(c["scale"], device="cuda"), need_dz=False, out=out)
    assert got[0] is None and bool(torch.isnan(out[0]).all())
    for name, g, f in zip(GRADS[1:], got[1:], full[1:]):
        assert torch.equal(g, f), name
    unit = engine.vae_decoder_nll_bwd(_saved64(c), *t, csr, **batch)
    for name, g in zip(GRADS, unit):
        _close(g, c["bwd"][name] / c["scale"], f"case {i} scale None {name}")


def _pair(eng, c, t=None, csr=None, batch=None):
    """Forward and backward of a case on `eng`: every output of both directions."""
    if t is None:
        t, csr, batch = _dev_inputs(eng, c)
    loss, saved = eng.vae_decoder_nll_fwd(*t, csr, **batch)
    grads = eng.vae_decoder_nll_bwd(saved, *t, csr, **batch, scale=torch.tensor(c["scale"], device="cuda"))
    return (loss,) + tuple(saved) + tuple(grads)


def _same_bits(xs, ys, what):
    assert len(xs) == len(ys)
    for k, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(x, y), (what, k)


@pytest.mark.gpu
def test_bit_level_promises(engine, cases):
    c = cases[0]                                        # every kernel on its scalar path
    t, csr, batch = _dev_inputs(engine, c)
    n0 = engine.launch_count()
    loss, saved = engine.vae_decoder_nll_fwd(*t, csr, **batch, check=False)
    n1 = engine.launch_count()
    scale = torch.tensor(c["scale"], device="cuda")
    grads = engine.vae_decoder_nll_bwd(saved, *t, csr, **batch, scale=scale)
    n2 = engine.launch_count()
    engine.vae_decoder_nll_bwd(saved, *t, csr, **batch, scale=scale, need_dz=False)
    n3 = engine.launch_count()
    print(f"launches: forward {n1 - n0}, backward {n2 - n1}, backward without dz {n3 - n2}")
    assert n1 - n0 == 6 and n2 - n1 == 7 and n3 - n2 == 6
    first = (loss,) + tuple(saved) + tuple(grads)
    _same_bits(first, _pair(engine, c, t, csr, batch), "second call")
    # two forwards may precede their backwards
    other = cases[2]
    t2, csr2, batch2 = _dev_inputs(engine, other)
    loss2, saved2 = engine.vae_decoder_nll_fwd(*t2, csr2, **batch2)
    _same_bits(grads, engine.vae_decoder_nll_bwd(saved, *t, csr, **batch, scale=scale), "backward behind another forward")
    _close(engine.vae_decoder_nll_bwd(saved2, *t2, csr2, **batch2)[3], other["bwd"]["dw4"] / other["scale"], "the other backward dw4")
    # data == null equals explicit ones (case 2's feed is all ones)
    assert csr2[2] is None
    ones = (csr2[0], csr2[1], torch.ones(csr2[1].numel(), device="cuda"), csr2[3])
    _same_bits(_pair(engine, other, t2, csr2, batch2), _pair(engine, other, t2, ones, batch2), "explicit ones")
    # rows = arange(row0, row0 + b) equals row0 addressing (case 1 is addressed through row0)
    c1 = cases[1]
    t1, csr1, batch1 = _dev_inputs(engine, c1)
    assert "row0" in batch1
    by_rows = dict(rows=torch.arange(c1["row0"], c1["row0"] + c1["b"], device="cuda"))
    _same_bits(_pair(engine, c1, t1, csr1, batch1), _pair(engine, c1, t1, csr1, by_rows), "rows against row0")
    engine.feed_status()


@pytest.mark.gpu
def test_scratch_shared_by_batches_of_different_sizes(cases):
    """Case 1 (b = 300), case 0 (b = 33), case 1 again on ONE engine, each against a fresh engine: the scratch a larger batch left
    behind the smaller one's rows must not reach a reduction over the batch."""
    from sdrm_amd.engine import Engine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    shared = Engine(8, 8, 4, 0, 16)
    try:
        for k, i in enumerate((1, 0, 1)):
            fresh = Engine(8, 8, 4, 0, 16)
            try:
                want = _pair(fresh, cases[i])
            finally:
                fresh.close()
            got = _pair(shared, cases[i])
            _same_bits(got, want, f"call {k} (case {i})")
            for name, g in zip(GRADS, got[4:]):
                _close(g, cases[i]["bwd"][name], f"call {k} (case {i}) {name}")
    finally:
        shared.close()


@pytest.mark.gpu
def test_decoder_nll_in_a_small_graph(engine):
    from sdrm_amd.train_SDRM import VAE, decoder_nll
    users, n_items, hidden, latent, b = 53, 90, 37, 5, 33
    m = synth.synth_feed_csr(users, n_items, 0.2, seed=91, ratings=True)
    csr = engine.csr_to_device(m)
    rows = torch.from_numpy(np.random.RandomState(92).permutation(users)[:b].astype(np.int64)).cuda()
    rows2 = torch.from_numpy(np.random.RandomState(93).permutation(users)[:b].astype(np.int64)).cuda()
    torch.manual_seed(94)
    model = VAE(n_items, hidden, latent).cuda()
    dec = [model.decoder[0].weight, model.decoder[0].bias, model.decoder[2].weight, model.decoder[2].bias]
    z0 = torch.randn(b, latent, device="cuda")
    z1 = torch.randn(b, latent, device="cuda")

    def graph(leaf, fixed, params, nll):
        z = leaf * 1.5                                  # z: a leaf behind a torch op
        first = 0.7 * nll(z, params, rows) + 0.3 * (z ** 2).sum()
        return first + 0.2 * nll(fixed, params, rows2)   # the parameters again, behind a z that needs no gradient: autograd accumulates

    leaf = z0.clone().requires_grad_()
    loss = graph(leaf, z1, dec, lambda z, p, r: decoder_nll(z, *p, csr, rows=r))
    assert loss.dim() == 0 and loss.is_cuda and loss.requires_grad
    loss.backward()
    got = [leaf.grad] + [p.grad for p in dec]
    X = {id(r): torch.from_numpy(m[r.cpu().numpy()].toarray()).double().cuda() for r in (rows, rows2)}

    def torch_nll(z, p, r):
        out = F.linear(torch.tanh(F.linear(z, p[0], p[1])), p[2], p[3])
        return -torch.mean(torch.sum(F.log_softmax(out, dim=1) * X[id(r)], dim=1))

    leaf64 = z0.double().requires_grad_()
    dec64 = [p.detach().double().requires_grad_() for p in dec]
    want = graph(leaf64, z1.double(), dec64, torch_nll)
    want.backward()
    err = abs(float(loss) / float(want) - 1)
    print(f"loss {float(loss):.8g} torch float64 {float(want):.8g} rel {err:.2e}")
    assert err <= TOL_LOSS
    for name, g, w in zip(("z", "w3", "b3", "w4", "b4"), got, [leaf64.grad] + [p.grad for p in dec64]):
        _close(g, w.cpu().numpy(), f"{name}.grad")
    # needs_input_grad is honoured: frozen parameters get no gradient, and the method is the function on the model's own decoder
    model.zero_grad()
    model.decoder[2].weight.requires_grad_(False)
    leaf2 = z0.clone().requires_grad_()
    model.decode_nll(leaf2, csr, rows=rows).backward()
    assert model.decoder[2].weight.grad is None and model.decoder[0].weight.grad is not None and leaf2.grad is not None
    model.decoder[2].weight.requires_grad_(True)
    assert torch.equal(model.decode_nll(z0, csr, rows=rows), decoder_nll(z0, *dec, csr, rows=rows))
    from sdrm_amd.engine import SdrmError
    with pytest.raises(SdrmError, match="no CPU fallback"):
        decoder_nll(z0.cpu(), *[p.cpu() for p in dec], csr, rows=rows)
    engine.feed_status()


@pytest.mark.gpu
def test_neighbours_are_left_alone(engine, cases):
    c = cases[0]
    rng = np.random.RandomState(31)
    hidden, n_items, latent = 48, 70, 8
    enc = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in ((hidden, n_items), (hidden,), (2 * latent, hidden), (2 * latent,))]
    dec = [_cuda(rng.standard_normal(s).astype(np.float32) * 0.1) for s in ((hidden, latent), (hidden,), (n_items, hidden), (n_items,))]
    zs = _cuda(rng.standard_normal((19, latent)).astype(np.float32))
    engine.vae_encoder_load(*enc)
    feed = engine.csr_to_device(synth.synth_feed_csr(64, n_items, 0.2, seed=84, ratings=False))
    before = engine.vae_encode_csr(feed, row0=0, b=64, return_kl=True) + (engine.vae_decode(zs, *dec),)
    t, csr, batch = _dev_inputs(engine, c)
    loss, saved = engine.vae_decoder_nll_fwd(*t, csr, **batch)
    _, lse = engine.multinomial_nll_csr(saved[1], csr, **batch)                                   # interleaved, on the same logits
    engine.vae_decoder_nll_bwd(saved, *t, csr, **batch)
    after = engine.vae_encode_csr(feed, row0=0, b=64, return_kl=True) + (engine.vae_decode(zs, *dec),)
    _same_bits(before, after, "vae_encode_csr / vae_decode")
    _close(lse, saved[2].cpu().numpy().astype(np.float64), "lse of multinomial_nll_csr against the forward's", tol=1e-6)


@pytest.mark.gpu
def test_refusals(engine, cases):
    from sdrm_amd import _lib
    from sdrm_amd.engine import SdrmError, _ptr, _stream
    import ctypes as C
    c = cases[0]
    t, csr, batch = _dev_inputs(engine, c)
    z, w3, b3, w4, b4 = t
    L, H, I, b = c["latent"], c["hidden"], c["n_items"], c["b"]
    n_rows = c["m"].shape[0]
    loss, saved = engine.vae_decoder_nll_fwd(*t, csr, **batch)
    lib, h = engine.lib, engine._h
    dec = _lib.VaeDecoder(w3.data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(), L, H, I)
    rows = batch["rows"]
    raw = torch.empty(b * I + 4, device="cuda")
    outs = dict(h3=torch.empty(b, H, device="cuda"), logits=raw[:b * I], lse=torch.empty(b, device="cuda"), loss=torch.empty((), device="cuda"))
    grads = _nan_out(c)

    def fwd(dec=dec, z=z, indptr=csr[0], indices=csr[1], n_rows=n_rows, rows=rows, row0=0, b=b, **o):
        o = dict(outs, **o)
        return lib.sdrm_vae_decoder_nll_fwd(h, C.byref(dec) if dec is not None else None, _ptr(z), _ptr(indptr), _ptr(indices), _ptr(csr[2]),
                                            n_rows, _ptr(rows), row0, b, _ptr(o["h3"]), _ptr(o["logits"]), _ptr(o["lse"]), _ptr(o["loss"]), _stream())

    def bwd(dec=dec, z=z, h3=saved[0], logits=saved[1], lse=saved[2], indptr=csr[0], indices=csr[1], n_rows=n_rows, rows=rows, row0=0, b=b,
            dz=grads[0], dw3=grads[1], db3=grads[2], dw4=grads[3], db4=grads[4]):
        return lib.sdrm_vae_decoder_nll_bwd(h, C.byref(dec) if dec is not None else None, _ptr(z), _ptr(h3), _ptr(logits), _ptr(lse), _ptr(indptr),
                                            _ptr(indices), _ptr(csr[2]), n_rows, _ptr(rows), row0, b, None, _ptr(dz), _ptr(dw3), _ptr(db3),
                                            _ptr(dw4), _ptr(db4), _stream())

    ARG, SHAPE = -1, -2
    assert _lib.STATUS[ARG] == "SDRM_ERR_ARG" and _lib.STATUS[SHAPE] == "SDRM_ERR_SHAPE"
    assert fwd() == 0 and bwd() == 0 and bwd(dz=None) == 0
    # null pointers
    no_w4 = _lib.VaeDecoder(w3.data_ptr(), b3.data_ptr(), None, b4.data_ptr(), L, H, I)
    for kw in (dict(dec=None), dict(dec=no_w4), dict(z=None), dict(indptr=None), dict(indices=None), dict(h3=None), dict(logits=None),
               dict(lse=None), dict(loss=None)):
        assert fwd(**kw) == ARG, kw
    for kw in (dict(dec=None), dict(dec=no_w4), dict(z=None), dict(h3=None), dict(logits=None), dict(lse=None), dict(indptr=None),
               dict(indices=None), dict(dw3=None), dict(db3=None), dict(dw4=None), dict(db4=None)):
        assert bwd(**kw) == ARG, kw
    # logits off 16 bytes
    assert fwd(logits=raw[1:1 + b * I]) == ARG and bwd(logits=raw[1:1 + b * I]) == ARG
    # each envelope edge through the ABI
    def dims(latent=L, hidden=H, n_items=I):
        return _lib.VaeDecoder(w3.data_ptr(), b3.data_ptr(), w4.data_ptr(), b4.data_ptr(), latent, hidden, n_items)

    for kw in (dict(dec=dims(latent=0)), dict(dec=dims(latent=4097)), dict(dec=dims(hidden=0)), dict(dec=dims(hidden=4097)),
               dict(dec=dims(n_items=0)), dict(dec=dims(n_items=(1 << 20) + 1)), dict(b=0), dict(b=(1 << 22) + 1),
               dict(dec=dims(n_items=1 << 18), b=1 << 22), dict(n_rows=0), dict(rows=None, row0=-1), dict(rows=None, row0=n_rows - b + 1)):
        assert fwd(**kw) == SHAPE, kw
        assert bwd(**kw) == SHAPE, kw
    assert fwd(rows=None, row0=n_rows - b) == 0 and bwd(rows=None, row0=n_rows - b) == 0
    engine.feed_status()
    # the Python surface: wrong shapes and types raise before the call
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_decoder_nll_fwd(z, w3, b3, w4[:-1].contiguous(), b4, csr, **batch)
    with pytest.raises(SdrmError):
        engine.vae_decoder_nll_fwd(z.double(), w3, b3, w4, b4, csr, **batch)
    with pytest.raises(SdrmError):
        engine.vae_decoder_nll_bwd(saved, *t, csr, **batch, scale=torch.ones(2, device="cuda"))
    # a column index out of range: the entry contributes nothing, anywhere
    k = next(k for k in range(b) if 0 < (c["X"][k] != 0).sum() < I)                               # a batch row with some entries
    p = int(c["m"].indptr[int(c["batch_rows"][k])])
    indices = csr[1].clone()
    indices[p] = I
    X = c["X"].copy()
    X[k, int(c["m"].indices[p])] = 0.0
    _refused_entry(engine, c, t, (csr[0], indices, csr[2], csr[3]), batch, X, "column index")
    # a row id out of range: the row counts as empty - its g row is zero, its lse still that of its logits
    bad_rows = rows.clone()
    bad_rows[7] = n_rows
    X = c["X"].copy()
    X[7] = 0.0
    _refused_entry(engine, c, t, csr, dict(rows=bad_rows), X, "row id")
    # a clean call afterwards passes
    engine.vae_decoder_nll_fwd(*t, csr, **batch, check=False)
    engine.vae_decoder_nll_bwd(saved, *t, csr, **batch)
    engine.feed_status()


def _refused_entry(engine, c, t, csr, batch, X, match):
    """Both directions on a feed with one offending entry or row raise at `feed_status()` and give what the restatement gives on `X`,
    the batch with that entry removed or that row emptied."""
    from sdrm_amd.engine import SdrmError
    f = ref.forward(c["z"], c["w3"], c["b3"], c["w4"], c["b4"], X)
    g = ref.backward(f, c["z"], c["w3"], c["w4"], X, c["scale"])
    assert np.array_equal(f["lse"], c["fwd"]["lse"])
    loss, saved = engine.vae_decoder_nll_fwd(*t, csr, **batch, check=False)
    with pytest.raises(SdrmError, match=match):
        engine.feed_status()
    got = engine.vae_decoder_nll_bwd(saved, *t, csr, **batch, scale=torch.tensor(c["scale"], device="cuda"))
    with pytest.raises(SdrmError, match=match):
        engine.feed_status()
    _close(saved[2], f["lse"], f"{match}: lse")
    assert abs(float(loss) / float(f["loss"]) - 1) <= TOL_LOSS
    for name, x in zip(GRADS, got):
        _close(x, g[name], f"{match}: {name}")


@pytest.mark.gpu
def test_pre_stage_with_all_five_flags(tmp_path, monkeypatch):
    """40 users x 60 items, batch 16, two epochs.  With `device_decoder=True` the train half calls neither Linear of the decoder (their
    patched forward raises while autograd records, which is the train half; the evaluation half's `model(...)` under `no_grad` keeps
    them); without the flag the train half calls each once per batch.  With equal seeds the two runs start from equal parameters and
    draw the same randoms, so the first step's losses differ by fp32 rounding alone; later steps are printed, not asserted (Adam's
    first updates are close to lr * sign(g): a gradient element near zero may flip under rounding)."""
    from sdrm_amd.engine import utility_engine
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    users, n_items, batch, epochs = 40, 60, 16, 2
    m = synth.synth_feed_csr(users, n_items, 0.2, seed=72, ratings=False)
    seen = {}
    orig_forward, orig_backward = torch.nn.Linear.forward, torch.Tensor.backward

    def forward(self, x):
        which = seen["decoder"].get(id(self))
        if which is not None and torch.is_grad_enabled():
            seen[which] += 1
            if seen["forbid"]:
                raise AssertionError(f"decoder[{which}] called in the train half")
        return orig_forward(self, x)

    def backward(self, *a, **kw):
        seen["losses"].append(self.detach())
        return orig_backward(self, *a, **kw)

    monkeypatch.setattr(torch.nn.Linear, "forward", forward)
    monkeypatch.setattr(torch.Tensor, "backward", backward)

    def run(where, forbid, **kw):
        torch.manual_seed(21)
        np.random.seed(22)
        vae = VAE(n_items, 16, 8).cuda()
        seen.clear()
        seen.update({0: 0, 2: 0, "losses": [], "forbid": forbid, "decoder": {id(vae.decoder[0]): 0, id(vae.decoder[2]): 2}})
        train_variational_autoencoder(vae, m, m, epochs, batch, 1e-3, "Recall@10", str(where), device_feed=True, sparse_input=True,
                                      device_holdout=True, device_latent=True, **kw)
        files = sorted((f for f in os.listdir(where) if f.startswith("epoch-")), key=lambda f: int(f[6:-4]))
        return vae, torch.stack(seen["losses"]).cpu().numpy(), files, dict(seen)

    steps = epochs * -(-users // batch)
    vae, losses, files, s = run(tmp_path / "a", True, device_decoder=True)
    assert s[0] == 0 and s[2] == 0 and np.isfinite(losses).all() and losses.size == steps
    utility_engine().feed_status()
    assert files and vae.model_is_trained and vae.is_training == 0
    best = torch.load(os.path.join(str(tmp_path / "a"), files[-1]))                          # saved on improvement only: the last is the best
    for name, p in vae.state_dict().items():
        assert torch.equal(p.cpu(), best[name].cpu()), name
    _, losses_b, _, s_b = run(tmp_path / "b", False)
    assert s_b[0] == steps and s_b[2] == steps and np.isfinite(losses_b).all() and losses_b.size == steps
    utility_engine().feed_status()
    rel = np.abs(losses / losses_b - 1)
    print(f"first step: {losses[0]:.8g} against {losses_b[0]:.8g}, rel {rel[0]:.2e}; largest over the other {steps - 1} steps {rel[1:].max():.2e}")
    assert rel[0] <= TOL_LOSS
