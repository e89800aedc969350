"""The VAE encoder behind its first pre-activation in train mode on the engine (reference train_SDRM.py:244-250 with is_training ==
1: tanh, the second Linear, chunk, the KL, the reparameterisation; and their share of :148), csrc/latent.h.

CPU: tests/vae_latent_ref.py (float64, from the formulas) against torch float64 autograd of the module's own expressions; the
restated draw; the header and the ctypes table; the host-side argument check; `device_latent=True` ignored on the host.
GPU (-m gpu): both directions against the restatement; the drawn noise against its numpy restatement; the bit-level promises;
`latent_head` in a small graph; the loaded encoder left alone; the pre-stage with all four flags.

Bars: every tensor rel_max and rel_l2 <= 1e-4 and kl <= 1e-4 relative (the project's fp32 bar; a numpy float32 evaluation of the
formulas stays within 7e-7 of float64 on these inputs).  Drawn eps <= 1e-5 absolute: csrc/philox.h puts the hardware
transcendentals' error at about 1e-6 absolute and the largest Box-Muller radius is sqrt(-2 ln 2^-24) = 5.77.  Loss of the small
graph <= 1e-5 relative.  Case numbers count from 0."""
import os
import re

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import vae_latent_ref as ref
from vae_latent_ref import rel_l2, rel_max
from sdrm_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_EPS, TOL_LOSS = 1e-4, 1e-5, 1e-5
STATS_CASE = 3          # 65 x 830 = 53 950 normals


@pytest.fixture(scope="module")
def cases():
    """Inputs and the float64 reference of every case with the injected eps, computed once: case dict + fwd, bwd."""
    out = []
    for i in range(len(ref.CASES)):
        c = ref.case_inputs(i)
        c["fwd"] = ref.forward(c["pre"], c["w2"], c["b2"], c["eps"])
        c["bwd"] = ref.backward(c["fwd"], c["w2"], c["eps"], c["gz"], c["gkl"])
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- CPU
def test_restatement_matches_torch_float64_autograd(cases):
    for i, c in enumerate(cases):
        pre, w2, b2 = (torch.from_numpy(c[k].astype(np.float64)).requires_grad_() for k in ("pre", "w2", "b2"))
        eps, gz = torch.from_numpy(c["eps"].astype(np.float64)), torch.from_numpy(c["gz"].astype(np.float64))
        h1 = torch.tanh(pre)
        h = F.linear(h1, w2, b2)
        mu, logvar = torch.chunk(h, chunks=2, dim=1)
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        z = mu + eps * torch.exp(0.5 * logvar)
        ((z * gz).sum() + c["gkl"] * kl).backward()
        f, g = c["fwd"], c["bwd"]
        assert np.abs(f["lv"]).max() < 3
        err = dict(h1=rel_max(f["h1"], h1.detach().numpy()), out2=rel_max(f["out2"], h.detach().numpy()), z=rel_max(f["z"], z.detach().numpy()),
                   kl=abs(float(f["kl"]) / float(kl.detach()) - 1), dpre=rel_max(g["dpre"], pre.grad.numpy()), dw2=rel_max(g["dw2"], w2.grad.numpy()),
                   db2=rel_max(g["db2"], b2.grad.numpy()))
        print(f"case {i}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        assert max(err.values()) <= 1e-12, (i, err)
        # a missing upstream gradient is a zero one
        only_z = ref.backward(f, c["w2"], c["eps"], c["gz"], None)
        only_kl = ref.backward(f, c["w2"], c["eps"], None, c["gkl"])
        assert rel_max(only_z["dw2"] + only_kl["dw2"], g["dw2"]) <= 1e-12 and rel_max(only_z["dpre"] + only_kl["dpre"], g["dpre"]) <= 1e-12


def test_restated_draw():
    seed, step = 0x0123_4567_89AB_CDEF, 7
    rows = np.arange(250) * 263
    e = ref.draw_eps(seed, step, rows, 400)
    n = e.size
    assert n == 100_000 and e.dtype == np.float32 and np.isfinite(e).all()
    mean, var = float(e.mean(dtype=np.float64)), float(e.var(dtype=np.float64))
    print(f"mean {mean:+.5f} ({abs(mean) * np.sqrt(n):.2f} sigma) var {var:.5f} ({abs(var - 1) / np.sqrt(2 / n):.2f} sigma)")
    assert abs(mean) <= 4 / np.sqrt(n) and abs(var - 1) <= 4 * np.sqrt(2 / n)
    # a feed row's eps does not change with the batch it is in, nor with the width asked for beyond the last whole quad
    alone = ref.draw_eps(seed, step, [rows[37]], 400)
    among = ref.draw_eps(seed, step, [5, rows[200], rows[37], 0], 400)
    assert np.array_equal(alone[0], e[37]) and np.array_equal(among[2], e[37])
    assert np.array_equal(ref.draw_eps(seed, step, rows[:9], 5), e[:9, :5])      # a quad cut by L
    # eps changes with the seed and with the step
    for other in (ref.draw_eps(seed + 1, step, rows, 400), ref.draw_eps(seed, step + 1, rows, 400)):
        assert not np.array_equal(other, e) and abs(float(np.corrcoef(other.ravel(), e.ravel())[0, 1])) <= 4 / np.sqrt(n)


def test_header_and_ctypes_table_carry_the_entry_points():
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    from sdrm_amd import _lib
    for name, n_args in (("sdrm_vae_latent_fwd", 18), ("sdrm_vae_latent_bwd", 14)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "sdrm_debug_latent_args" in open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    assert "PURPOSE_VAE_EPS = 9" in open(os.path.join(REPO, "sdrm_amd", "csrc", "philox.h")).read()
    from sdrm_amd import train_SDRM as ts, vae_hooks
    assert ts.latent_head is vae_hooks.latent_head
    from sdrm_amd.engine import Engine
    assert callable(Engine.vae_latent_fwd) and callable(Engine.vae_latent_bwd)


def test_host_side_argument_check():
    from sdrm_amd import _lib
    lib = _lib.load()
    ok = dict(hidden=600, latent=83, b=130, row0=17, contiguous=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sdrm_debug_latent_args(a["hidden"], a["latent"], a["b"], a["row0"], a["contiguous"])

    assert call() == 0 and lib.sdrm_debug_latent_args(1, 1, 1, 0, 1) == 0
    assert call(hidden=4096) == 0 and call(latent=4096) == 0 and call(b=1 << 22) == 0
    assert call(row0=(1 << 31) - 130) == 0 and call(row0=0) == 0
    assert call(row0=(1 << 31) - 129, contiguous=0) == 0 and call(row0=-1, contiguous=0) == 0     # with a `rows` array row0 is not read
    for bad in (dict(hidden=0), dict(hidden=4097), dict(latent=0), dict(latent=4097), dict(b=0), dict(b=(1 << 22) + 1), dict(row0=-1),
                dict(row0=(1 << 31) - 129), dict(hidden=-5), dict(b=-1)):
        assert call(**bad) == -2, bad                                                              # SDRM_ERR_SHAPE


def test_device_latent_is_ignored_for_a_model_on_the_host(tmp_path, monkeypatch):
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
    b, loss_b, best_b, state_b = run(tmp_path / "b", device_feed=True, sparse_input=True, device_holdout=True, device_latent=True)
    c, loss_c, best_c, _ = run(tmp_path / "c", device_latent=True)
    assert len(loss_a) == 2 * 3 and loss_a == loss_b == loss_c
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
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    print(f"{what}: rel_max {rel_max(got, want):.2e} rel_l2 {rel_l2(got, want):.2e}")
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    assert rel_max(got, want) <= tol and rel_l2(got, want) <= tol, (what, rel_max(got, want), rel_l2(got, want))


def _forward_injected(engine, c, what):
    eps = _cuda(c["eps"])
    z, kl, saved = engine.vae_latent_fwd(_cuda(c["pre"]), _cuda(c["w2"]), _cuda(c["b2"]), eps=eps)
    f = c["fwd"]
    _close(saved[0], f["h1"], f"{what} h1")
    _close(saved[1], f["out2"], f"{what} out2")
    _close(z, f["z"], f"{what} z")
    kl_err = abs(float(kl) / float(f["kl"]) - 1)
    print(f"{what} kl {float(kl):.8g} rel {kl_err:.2e}")
    assert kl_err <= TOL
    assert saved[2].data_ptr() == eps.data_ptr() and np.array_equal(eps.cpu().numpy().view(np.uint32), c["eps"].view(np.uint32))   # not written
    return z, kl, saved


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_hip_forward_with_injected_eps_vs_fp64(engine, cases, i):
    _forward_injected(engine, cases[i], f"case {i}")
    if i <= 1:                                          # the narrowest case and the one of several row tiles, under every tile shape
        try:
            for tile in range(5):
                engine.debug_set(tile=tile)
                _forward_injected(engine, cases[i], f"case {i} tile {tile}")
        finally:
            engine.debug_set(tile=-1)


def _backward(engine, c, what):
    f = c["fwd"]
    saved = tuple(_cuda(f[k], torch.float32) for k in ("h1", "out2")) + (_cuda(c["eps"]),)     # the forward's float64 values
    H, L, b = c["hidden"], c["latent"], c["b"]
    out = tuple(torch.full(s, float("nan"), device="cuda") for s in ((b, H), (2 * L, H), (2 * L,)))
    got = engine.vae_latent_bwd(saved, _cuda(c["w2"]), _cuda(c["gz"]), torch.tensor(c["gkl"], device="cuda"), out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    for name, g in zip(("dpre", "dw2", "db2"), got):
        _close(g, c["bwd"][name], f"{what} {name}")
    return saved


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_hip_backward_vs_fp64(engine, cases, i):
    c = cases[i]
    saved = _backward(engine, c, f"case {i}")
    if i <= 1:
        try:
            for tile in range(5):
                engine.debug_set(tile=tile)
                _backward(engine, c, f"case {i} tile {tile}")
        finally:
            engine.debug_set(tile=-1)
    # a null upstream gradient is a zero one
    w2 = _cuda(c["w2"])
    for gz, gkl in ((c["gz"], None), (None, c["gkl"])):
        want = ref.backward(c["fwd"], c["w2"], c["eps"], gz, gkl)
        got = engine.vae_latent_bwd(saved, w2, None if gz is None else _cuda(gz), None if gkl is None else torch.tensor(gkl, device="cuda"))
        for name, g in zip(("dpre", "dw2", "db2"), got):
            _close(g, want[name], f"case {i} gz {gz is not None} gkl {gkl is not None} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_hip_drawn_eps(engine, cases, i):
    c = cases[i]
    pre, w2, b2 = _cuda(c["pre"]), _cuda(c["w2"]), _cuda(c["b2"])
    z, kl, saved = engine.vae_latent_fwd(pre, w2, b2, rows=_cuda(c["rows"]), seed=c["seed"], step=c["step"])
    eps = saved[2].cpu().numpy()
    want = ref.draw_eps(c["seed"], c["step"], c["rows"], c["latent"])
    diff = float(np.abs(eps.astype(np.float64) - want).max())
    print(f"case {i}: drawn eps against the restatement, largest absolute difference {diff:.3e} over {eps.size} normals")
    assert eps.shape == want.shape and np.isfinite(eps).all()
    assert diff <= TOL_EPS
    if i == STATS_CASE:
        n = eps.size
        mean, var = float(eps.mean(dtype=np.float64)), float(eps.var(dtype=np.float64))
        print(f"mean {mean:+.5f} ({abs(mean) * np.sqrt(n):.2f} sigma) var {var:.5f} ({abs(var - 1) / np.sqrt(2 / n):.2f} sigma)")
        assert n >= 50_000 and abs(mean) <= 4 / np.sqrt(n) and abs(var - 1) <= 4 * np.sqrt(2 / n)
    f = ref.forward(c["pre"], c["w2"], c["b2"], eps)                                         # the restatement fed the read-back eps
    _close(z, f["z"], f"case {i} z with drawn eps")
    assert abs(float(kl) / float(f["kl"]) - 1) <= TOL
    engine.feed_status()


@pytest.mark.gpu
def test_bit_level_promises(engine, cases):
    c = cases[2]                                        # odd L: every kernel on its scalar path
    pre, w2, b2, rows = _cuda(c["pre"]), _cuda(c["w2"]), _cuda(c["b2"]), _cuda(c["rows"])
    kw = dict(seed=c["seed"], step=c["step"])
    gz, gkl = _cuda(c["gz"]), torch.tensor(c["gkl"], device="cuda")
    n0 = engine.launch_count()
    za, kla, sa = engine.vae_latent_fwd(pre, w2, b2, rows=rows, **kw)
    n1 = engine.launch_count()
    ga = engine.vae_latent_bwd(sa, w2, gz, gkl)
    n2 = engine.launch_count()
    print(f"launches: forward {n1 - n0}, backward {n2 - n1}")
    assert n1 - n0 <= 5 and n2 - n1 <= 6
    zb, klb, sb = engine.vae_latent_fwd(pre, w2, b2, rows=rows, **kw)
    gb = engine.vae_latent_bwd(sb, w2, gz, gkl)
    for x, y in zip((za, kla) + sa + ga, (zb, klb) + sb + gb):
        assert torch.equal(x, y)
    # two forwards may precede their backwards
    c1 = cases[1]
    z1, kl1, s1 = engine.vae_latent_fwd(_cuda(c1["pre"]), _cuda(c1["w2"]), _cuda(c1["b2"]), rows=_cuda(c1["rows"]), seed=1, step=2)
    for x, y in zip(ga, engine.vae_latent_bwd(sa, w2, gz, gkl)):
        assert torch.equal(x, y)
    # eps of a feed row: another place of a batch, a batch of another size, `rows` against `row0`
    eps = sa[2]
    sub = torch.flip(rows[40:57], dims=(0,))
    _, _, ss = engine.vae_latent_fwd(pre[:17].contiguous(), w2, b2, rows=sub, **kw)
    assert torch.equal(ss[2], torch.flip(eps[40:57], dims=(0,)))
    _, _, s_one = engine.vae_latent_fwd(pre[:1].contiguous(), w2, b2, rows=rows[5:6], **kw)
    assert torch.equal(s_one[2][0], eps[5])
    r0 = 70_000
    _, _, s_r0 = engine.vae_latent_fwd(pre, w2, b2, row0=r0, **kw)
    _, _, s_rows = engine.vae_latent_fwd(pre, w2, b2, rows=torch.arange(r0, r0 + c["b"], device="cuda"), **kw)
    assert torch.equal(s_r0[2], s_rows[2]) and not torch.equal(s_r0[2], eps)
    k = int((rows == 0).nonzero()[0])
    _, _, s_zero = engine.vae_latent_fwd(pre[:3].contiguous(), w2, b2, row0=0, **kw)
    assert torch.equal(s_zero[2][0], eps[k])
    # seed and step reach the draw
    for other in (dict(seed=c["seed"] + 1, step=c["step"]), dict(seed=c["seed"], step=c["step"] + 1)):
        assert not torch.equal(engine.vae_latent_fwd(pre, w2, b2, rows=rows, **other)[2][2], eps)
    engine.feed_status()


@pytest.mark.gpu
def test_latent_head_in_a_small_graph(engine):
    from sdrm_amd.train_SDRM import SparseFeed, VAE, latent_head, multinomial_nll, sparse_input_linear
    users, n_items, hidden, latent, lo, hi, anneal = 53, 90, 37, 5, 7, 40, 0.13
    m = synth.synth_feed_csr(users, n_items, 0.2, seed=81, ratings=False)
    feed = SparseFeed(m, engine=engine)
    feed.set_order(np.random.RandomState(82).permutation(users))
    rows = feed.order[lo:hi]
    torch.manual_seed(83)
    model = VAE(n_items, hidden, latent, p_drop=0.5).cuda()
    eps = torch.randn(hi - lo, latent, device="cuda")

    def run(tail, with_kl=True):
        model.zero_grad()
        pre = sparse_input_linear(model.encoder[0].weight, model.encoder[0].bias, feed, lo, hi, 5, 6, 0.5)
        z, kl = tail(pre)
        loss = multinomial_nll(model.decode(z), feed.csr, rows=rows)
        if with_kl:
            loss = loss + anneal * kl
        loss.backward()
        return float(loss), {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()}

    def engine_tail(pre):
        return latent_head(pre, model.encoder[2].weight, model.encoder[2].bias, rows, lo, 0, 0, eps=eps)

    def torch_tail(pre):                                # `VAE.encode_rows`' own lines, with the same eps
        h = model.encoder[1:](pre)
        mu, logvar = torch.chunk(h, chunks=2, dim=1)
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
        return mu + model.is_training * eps * torch.exp(0.5 * logvar), kl

    model.train()
    model.is_training = 1
    for with_kl in (True, False):                       # kl unused: its gradient is None and is passed as null
        loss, grads = run(engine_tail, with_kl)
        want, want_grads = run(torch_tail, with_kl)
        print(f"with kl {with_kl}: loss {loss:.8g} torch {want:.8g} rel {abs(loss - want) / abs(want):.2e}")
        assert abs(loss - want) <= TOL_LOSS * abs(want)
        assert set(grads) == set(want_grads) and len(grads) == 8
        for name in grads:
            _close(grads[name], want_grads[name], f"with kl {with_kl}: {name}.grad")
    # the method: with a latent_seed everything behind the input layer is latent_head, keyed by the feed rows of the order
    z, kl = model.encode_rows(feed, lo, hi, 5, 6, latent_seed=9)
    pre = sparse_input_linear(model.encoder[0].weight, model.encoder[0].bias, feed, lo, hi, 5, 6, 0.5)
    z2, kl2 = latent_head(pre, model.encoder[2].weight, model.encoder[2].bias, rows, lo, 9, 6)
    assert torch.equal(z, z2) and torch.equal(kl, kl2) and z.requires_grad and kl.requires_grad
    engine.feed_status()


@pytest.mark.gpu
def test_a_loaded_encoder_is_left_alone(engine, cases):
    c = cases[0]
    rng = np.random.RandomState(31)
    hidden, n_items, latent = 48, 70, 8
    enc = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in ((hidden, n_items), (hidden,), (2 * latent, hidden), (2 * latent,))]
    engine.vae_encoder_load(*enc)
    csr = engine.csr_to_device(synth.synth_feed_csr(64, n_items, 0.2, seed=84, ratings=False))
    before = engine.vae_encode_csr(csr, row0=0, b=64, return_kl=True)
    z, kl, saved = engine.vae_latent_fwd(_cuda(c["pre"]), _cuda(c["w2"]), _cuda(c["b2"]), rows=_cuda(c["rows"]), seed=c["seed"], step=c["step"])
    engine.vae_latent_bwd(saved, _cuda(c["w2"]), _cuda(c["gz"]), torch.tensor(c["gkl"], device="cuda"))
    after = engine.vae_encode_csr(csr, row0=0, b=64, return_kl=True)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


@pytest.mark.gpu
def test_refusals(engine, cases):
    from sdrm_amd.engine import SdrmError
    c = cases[0]
    pre, w2, b2 = _cuda(c["pre"]), _cuda(c["w2"]), _cuda(c["b2"])
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_latent_fwd(pre, w2, b2, row0=(1 << 31) - 5)
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_latent_fwd(pre, w2[:, :-1].contiguous(), b2)
    with pytest.raises(SdrmError):
        engine.vae_latent_fwd(pre.double(), w2, b2)
    with pytest.raises(SdrmError):
        engine.vae_latent_fwd(pre, w2, b2, eps=torch.zeros(c["b"], c["latent"] + 1, device="cuda"))
    _, _, saved = engine.vae_latent_fwd(pre, w2, b2, eps=_cuda(c["eps"]))
    with pytest.raises(SdrmError):
        engine.vae_latent_bwd(saved, w2, _cuda(c["gz"]), torch.zeros(2, device="cuda"))
    # a feed row of `rows` outside [0, 2^31) raises the feed status word's row bit
    bad = _cuda(c["rows"]).clone()
    bad[3] = 1 << 31
    engine.vae_latent_fwd(pre, w2, b2, rows=bad)
    with pytest.raises(SdrmError, match="row id"):
        engine.feed_status()
    engine.feed_status()


@pytest.mark.gpu
def test_pre_stage_with_all_four_flags(tmp_path, monkeypatch):
    """40 users x 60 items, batch 16, two epochs.  With `device_latent=True` the train half never calls `torch.randn_like` (the patched
    function raises while autograd records, which is the train half; the evaluation half's `VAE.encode` under `no_grad` keeps its
    draw, as in every other path); without the flag the train half calls it once per batch."""
    from sdrm_amd.engine import utility_engine
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    users, n_items, batch, epochs = 40, 60, 16, 2
    m = synth.synth_feed_csr(users, n_items, 0.2, seed=72, ratings=False)
    seen = {"train": 0, "eval": 0, "losses": []}
    orig_randn_like, orig_backward = torch.randn_like, torch.Tensor.backward

    def randn_like(*a, **kw):
        seen["train" if torch.is_grad_enabled() else "eval"] += 1
        if torch.is_grad_enabled() and seen["forbid"]:
            raise AssertionError("torch.randn_like called in the train half")
        return orig_randn_like(*a, **kw)

    def backward(self, *a, **kw):
        seen["losses"].append(self.detach())
        return orig_backward(self, *a, **kw)

    monkeypatch.setattr(torch, "randn_like", randn_like)
    monkeypatch.setattr(torch.Tensor, "backward", backward)

    def run(where, forbid, **kw):
        seen.update(train=0, eval=0, losses=[], forbid=forbid)
        torch.manual_seed(21)
        np.random.seed(22)
        vae = VAE(n_items, 16, 8).cuda()
        train_variational_autoencoder(vae, m, m, epochs, batch, 1e-3, "Recall@10", str(where), device_feed=True, sparse_input=True,
                                      device_holdout=True, **kw)
        files = sorted((f for f in os.listdir(where) if f.startswith("epoch-")), key=lambda f: int(f[6:-4]))
        return vae, torch.stack(seen["losses"]).cpu().numpy(), files, dict(seen)

    steps = epochs * -(-users // batch)
    vae, losses, files, s = run(tmp_path / "a", True, device_latent=True)
    assert s["train"] == 0 and np.isfinite(losses).all() and losses.size == steps
    utility_engine().feed_status()
    assert files and vae.model_is_trained and vae.is_training == 0
    best = torch.load(os.path.join(str(tmp_path / "a"), files[-1]))                          # saved on improvement only: the last is the best
    for name, p in vae.state_dict().items():
        assert torch.equal(p.cpu(), best[name].cpu()), name
    _, losses_b, _, s_b = run(tmp_path / "b", False)
    assert s_b["train"] == steps and np.isfinite(losses_b).all()
    utility_engine().feed_status()
