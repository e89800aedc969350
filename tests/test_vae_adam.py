"""Adam and the L2 term of the VAE pre-stage on the engine, and the train step without autograd (reference train_SDRM.py:126, :143-150,
:262-268), csrc/vae_adam.h.

CPU: tests/vae_adam_ref.py (float64, from the formulas) against `torch.optim.Adam` in float64; the headers and the ctypes table; the
host-side argument check; `DeviceAdam`'s state against `torch.optim.Adam`'s; the new keywords ignored on the host and handed on by
`train_SDRM`.
GPU (-m gpu): one step against the restatement on tensors carved out of guarded arenas; the L2 partials and the loss slot; `DeviceAdam`
against torch's optimizer on the device; the refusals; the direct step against the autograd step, bit for bit; `device_optimizer` against
torch's Adam in the pre-stage; `train_SDRM` with all six keywords; the neighbours left alone.

Bars, against the float64 restatement of the same float32 inputs: m and v rel_max <= 1e-4 (the project's fp32 bar); p elementwise
|p - p_ref| <= 2^-24 |p_ref| + 1e-4 max|p_ref - p_0| - the one final rounding, and the fp32 bar on the update."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import vae_adam_ref as ref
from vae_adam_ref import rel_max
from sdrm_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
LR, EPS = 1e-3, 1e-8
GUARD = 8                                                                                          # floats between neighbouring tensors of an arena
NINE = (1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 7, 4099)                                          # the last one starts one float off a 16-byte boundary
SEVENTEEN = (5,) * 17                                                                              # two launches
SENTINEL = 12345.0


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_restatement_matches_torch_float64_adam(step, wd, betas):
    rng = np.random.RandomState(1000 * step + int(100 * wd) + int(10 * betas[0]))
    shapes = {"a.weight": (7, 5), "a.bias": (7,), "b.weight": (3, 7), "b.bias": (3,)}
    p0 = {k: rng.standard_normal(s) * 0.1 for k, s in shapes.items()}
    g0 = {k: rng.standard_normal(s) * 0.01 for k, s in shapes.items()}
    m0 = {k: (rng.standard_normal(s) * 0.01 if step > 1 else np.zeros(s)) for k, s in shapes.items()}
    v0 = {k: (rng.random_sample(s) * 1e-4 if step > 1 else np.zeros(s)) for k, s in shapes.items()}
    params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in p0.items()}
    opt = torch.optim.Adam(params.values(), lr=LR, betas=betas, eps=EPS)
    if step > 1:
        for k, p in params.items():
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m0[k].copy()),
                            "exp_avg_sq": torch.from_numpy(v0[k].copy())}
    loss = sum((torch.from_numpy(g0[k]) * p).sum() for k, p in params.items())
    loss = loss + wd * sum(torch.norm(p, p=2) ** 2 for k, p in params.items() if k.endswith(".weight"))
    loss.backward()
    opt.step()
    for k, p in params.items():
        got = ref.adam_step(p0[k], g0[k], m0[k], v0[k], step, LR, betas, EPS, l2_coef=wd if k.endswith(".weight") else 0.0)
        want = (p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy())
        assert float(opt.state[p]["step"]) == step
        for name, a, b in zip("pmv", got, want):
            assert rel_max(a, b) <= 1e-12, (k, name, rel_max(a, b))
        assert np.abs(got[0] - p0[k]).max() > 0


def test_headers_and_ctypes_table_carry_the_entry_points():
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    debug = open(os.path.join(REPO, "include", "sdrm_hip_debug.h")).read()
    from sdrm_amd import _lib
    for text, name, n_args in ((header, "sdrm_vae_adam_step", 11), (header, "sdrm_vae_loss_slot", 9), (debug, "sdrm_debug_vae_adam_args", 8)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert "typedef struct sdrm_vae_adam_tensor" in header
    assert [f[0] for f in _lib.VaeAdamTensor._fields_] == ["p", "g", "m", "v", "n", "l2_coef"] and C.sizeof(_lib.VaeAdamTensor) == 48
    from sdrm_amd import train_SDRM as ts, vae_hooks
    assert ts.DeviceAdam is vae_hooks.DeviceAdam and ts.vae_train_step is vae_hooks.vae_train_step
    sig = inspect.signature(ts.train_SDRM).parameters
    for kw in ("vae_sparse_input", "vae_device_latent", "vae_device_decoder", "vae_device_optimizer"):
        assert sig[kw].default is False, kw
    assert inspect.signature(vae_hooks.train_variational_autoencoder).parameters["device_optimizer"].default is False
    from sdrm_amd.engine import Engine
    assert callable(Engine.vae_adam_step) and callable(Engine.vae_loss_slot) and vae_hooks.ADAM_CHUNK == ref.CHUNK == 4096


def _debug_args(spans, step=1, coefs=None, has_partials=0, capacity=0):
    """sdrm_debug_vae_adam_args on tensors given as (p, g, m, v addresses, n): (status, chunk count)."""
    from sdrm_amd import _lib
    lib = _lib.load()
    k = len(spans)
    addr = (C.c_uint64 * max(4 * k, 1))(*[a for s in spans for a in s[:4]])
    n = (C.c_int64 * max(k, 1))(*[s[4] for s in spans])
    coef = (C.c_float * max(k, 1))(*(coefs if coefs is not None else [0.0] * k))
    chunks = C.c_int64(-1)
    rc = lib.sdrm_debug_vae_adam_args(addr, n, coef, k, step, has_partials, capacity, C.byref(chunks))
    return rc, chunks.value


def _spans(ns, base=1 << 20, gap=0):
    """Tensors of ns elements whose 4 x len(ns) ranges follow each other from `base`, `gap` bytes apart."""
    out, at = [], base
    for n in ns:
        four = []
        for _ in range(4):
            four.append(at)
            at += 4 * n + gap
        out.append(tuple(four) + (n,))
    return out


def test_host_side_argument_check():
    ARG, SHAPE = -1, -2
    for n, chunks in ((1, 1), (4095, 1), (4096, 1), (4097, 2)):
        assert _debug_args(_spans([n])) == (0, chunks), n
    ns = [1, 4095, 4096, 4097] * 4
    assert _debug_args(_spans(ns)) == (0, ref.chunk_count(ns)) and ref.chunk_count(ns) == 4 * 5
    assert _debug_args(_spans([5] * 17)) == (0, 17)                                                # more than one launch
    ok = _spans([10, 20])                                                                          # ranges that only touch: accepted
    assert _debug_args(ok) == (0, 2)
    # every refusal
    assert _debug_args([])[0] == SHAPE                                                             # n_tensors <= 0
    assert _debug_args(ok, step=0)[0] == ARG and _debug_args(ok, step=-3)[0] == ARG
    for j in range(4):                                                                             # a null pointer
        bad = [tuple(0 if i == j else a for i, a in enumerate(ok[0][:4])) + (10,), ok[1]]
        assert _debug_args(bad)[0] == ARG, j
    assert _debug_args([ok[0][:4] + (0,), ok[1]])[0] == SHAPE and _debug_args([ok[0][:4] + (-1,), ok[1]])[0] == SHAPE
    assert _debug_args(ok, coefs=[-0.5, 0.0])[0] == ARG
    big = _spans([8192, 4097])                                                                     # 2 + 2 chunks
    assert _debug_args(big, coefs=[0.01, 0.0], has_partials=1, capacity=4) == (0, 4)
    assert _debug_args(big, coefs=[0.01, 0.0], has_partials=1, capacity=3)[0] == SHAPE
    assert _debug_args(big, coefs=[0.0, 0.0], has_partials=1, capacity=0) == (0, 4)                # no coefficient: nothing is summed
    assert _debug_args(big, coefs=[0.01, 0.0], has_partials=0, capacity=0) == (0, 4)               # no buffer: nothing is summed
    # two ranges overlapping by one element: every pair of roles, within a tensor and across tensors
    a = _spans([10], gap=4096)[0]                                                                  # room behind each of a's four ranges
    b = _spans([20], base=1 << 24, gap=4096)[0]
    assert _debug_args([a, b]) == (0, 2)
    for j in range(4):
        for k in range(4):
            moved = list(b[:4])
            moved[k] = a[j] + 4 * (10 - 1)                                                         # starts on the last element of a's range j
            assert _debug_args([a, tuple(moved) + (20,)])[0] == ARG, (j, k)
            assert _debug_args([tuple(moved) + (20,), a])[0] == ARG, (j, k)
            moved[k] += 4                                                                          # ... and only touching
            assert _debug_args([a, tuple(moved) + (20,)])[0] == 0, (j, k)
    same = [a[:1] + a[:1] + a[2:4] + (10,)]                                                        # g aliases p
    assert _debug_args(same)[0] == ARG


def _host_model_run(tmp, **kw):
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    m = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)
    torch.manual_seed(3)
    np.random.seed(4)
    vae = VAE(60, 16, 8)
    train_variational_autoencoder(vae, m, m, 2, 16, 1e-3, "Recall@10", str(tmp), **kw)
    return vae, np.random.get_state()


def test_new_keywords_are_ignored_for_a_model_on_the_host(tmp_path, monkeypatch):
    a, state_a = _host_model_run(tmp_path / "a")
    b, state_b = _host_model_run(tmp_path / "b", device_optimizer=True)
    c, state_c = _host_model_run(tmp_path / "c", device_feed=True, sparse_input=True, device_holdout=True, device_latent=True,
                                 device_decoder=True, device_optimizer=True)
    for st in (state_b, state_c):
        assert np.array_equal(state_a[1], st[1]) and state_a[2:] == st[2:]                         # no extra draw either
    for (name, p), (_, q), (_, r) in zip(a.state_dict().items(), b.state_dict().items(), c.state_dict().items()):
        assert torch.equal(p, q) and torch.equal(p, r), name
    # train_SDRM hands its four new keywords on under train_variational_autoencoder's names, beside the two it had
    from sdrm_amd import train_SDRM as ts

    class Stop(Exception):
        pass

    seen = {}

    def pre_stage(model, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(ts, "train_variational_autoencoder", pre_stage)
    monkeypatch.setattr(ts.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ts, "DEVICE", "cpu")
    for on in (False, True):
        seen.clear()
        with pytest.raises(Stop):
            ts.train_SDRM(None, 60, 16, 8, 16, 1e-3, 8, 1, 1e-3, 1, 5, 1.0, str(tmp_path), None, None, "Recall@10", vae_device_feed=on,
                          vae_device_holdout=on, vae_sparse_input=on, vae_device_latent=on, vae_device_decoder=on, vae_device_optimizer=on)
        for kw in ("device_feed", "device_holdout", "sparse_input", "device_latent", "device_decoder", "device_optimizer"):
            assert seen[kw] is on, kw
    seen.clear()
    with pytest.raises(Stop):
        ts.train_SDRM(None, 60, 16, 8, 16, 1e-3, 8, 1, 1e-3, 1, 5, 1.0, str(tmp_path), None, None, "Recall@10")
    assert not any(seen[kw] for kw in ("sparse_input", "device_latent", "device_decoder", "device_optimizer"))


def _named(shapes, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(name, torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(device))) for name, s in shapes]


SHAPES8 = (("encoder.0.weight", (16, 60)), ("encoder.0.bias", (16,)), ("encoder.2.weight", (16, 16)), ("encoder.2.bias", (16,)),
           ("decoder.0.weight", (16, 8)), ("decoder.0.bias", (16,)), ("decoder.2.weight", (60, 16)), ("decoder.2.bias", (60,)))


def test_state_moves_between_device_adam_and_torch_adam():
    from sdrm_amd.vae_hooks import DeviceAdam
    named = _named(SHAPES8)
    params = [p for _, p in named]
    theirs = torch.optim.Adam(params, lr=LR)
    ours = DeviceAdam(named, lr=LR)
    assert ours.state_dict()["state"] == {} and ours.step_count == 0 and all(not m.any() for m in ours.exp_avg + ours.exp_avg_sq)
    theirs.load_state_dict(ours.state_dict())                                                      # a fresh state loads as a fresh state
    for k in range(3):                                                                             # torch steps on the host ...
        for i, p in enumerate(params):
            p.grad = torch.full_like(p, 0.01 * (i + 1) * (k + 1))
        theirs.step()
    sd = theirs.state_dict()
    moments = [m.data_ptr() for m in ours.exp_avg + ours.exp_avg_sq]
    ours.load_state_dict(sd)                                                                       # ... its state into ours (no launch)
    assert ours.step_count == 3 and moments == [m.data_ptr() for m in ours.exp_avg + ours.exp_avg_sq]
    for i in range(len(params)):
        assert torch.equal(ours.exp_avg[i], sd["state"][i]["exp_avg"]) and torch.equal(ours.exp_avg_sq[i], sd["state"][i]["exp_avg_sq"])
        assert ours.exp_avg[i].abs().max() > 0
    back = torch.optim.Adam(params, lr=5e-2)                                                       # ... and back into a fresh torch.optim.Adam
    back.load_state_dict(ours.state_dict())
    for i, p in enumerate(params):
        st = back.state[p]
        assert float(st["step"]) == 3.0 and torch.equal(st["exp_avg"], ours.exp_avg[i]) and torch.equal(st["exp_avg_sq"], ours.exp_avg_sq[i])
    assert back.param_groups[0]["lr"] == LR and tuple(back.param_groups[0]["betas"]) == (0.9, 0.999) and back.param_groups[0]["weight_decay"] == 0
    for i, p in enumerate(params):                                                                 # the loaded optimizer steps like the one it came from
        p.grad = torch.full_like(p, -0.02 * (i + 1))
    before = [p.detach().clone() for p in params]
    back.step()
    after_back = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, q in zip(params, before):
            p.copy_(q)
    theirs.step()
    for p, q in zip(params, after_back):
        assert torch.equal(p.detach(), q)
    from sdrm_amd.engine import SdrmError
    ours.zero_grad()
    assert all(p.grad is None for p in params)
    with pytest.raises(SdrmError, match="None"):
        ours.step()
    with pytest.raises(SdrmError, match="no CPU fallback"):
        ours.step(grads=[torch.zeros_like(p) for p in params])


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def engine():
    from sdrm_amd.engine import utility_engine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return utility_engine()


def _layout(ns):
    """Offsets of tensors of ns elements in an arena: each on a 16-byte boundary - the nine-tensor case's last one float behind one -,
    GUARD floats or more between neighbours; and the arena's length."""
    offs, at = [], GUARD
    for i, n in enumerate(ns):
        at = -(-at // 4) * 4
        if ns is NINE and i == len(ns) - 1:
            at += 1
        offs.append(at)
        at += n + GUARD
    return offs, at


def _case(ns, step, wd, seed=0):
    """The float32 inputs of one step as four host arenas (guards = SENTINEL) and the float64 expectation per tensor."""
    rng = np.random.RandomState(seed + 7 * step)
    offs, total = _layout(ns)
    arena = {k: np.full(total, SENTINEL, dtype=np.float32) for k in "pgmv"}
    coefs = [wd if i % 2 == 0 else 0.0 for i in range(len(ns))]                                    # weight, bias, weight, ...
    want = []
    for i, (o, n) in enumerate(zip(offs, ns)):
        p = (rng.standard_normal(n) * 0.1).astype(np.float32)
        g = (rng.standard_normal(n) * 0.01).astype(np.float32)
        m = (rng.standard_normal(n) * 0.01).astype(np.float32) if step > 1 else np.zeros(n, dtype=np.float32)
        v = (rng.random_sample(n) * 1e-4).astype(np.float32) if step > 1 else np.zeros(n, dtype=np.float32)
        dead = rng.random_sample(n) < 0.25                                                         # g exactly 0 where m = v = 0
        dead[0] = n > 1
        g[dead] = 0.0; m[dead] = 0.0; v[dead] = 0.0
        for k, a in zip("pgmv", (p, g, m, v)):
            arena[k][o:o + n] = a
        want.append(ref.adam_step(p, g, m, v, step, LR, (0.9, 0.999), EPS, l2_coef=coefs[i]) + (dead,))
    return arena, offs, coefs, want


def _views(dev_arena, offs, ns):
    return [dev_arena[o:o + n] for o, n in zip(offs, ns)]


def _step_on_device(engine, arena, offs, ns, coefs, step, partials=None):
    dev = {k: torch.from_numpy(a.copy()).cuda() for k, a in arena.items()}
    assert all(t.data_ptr() % 16 == 0 for t in dev.values())
    views = {k: _views(dev[k], offs, ns) for k in "pgmv"}
    engine.vae_adam_step(views["p"], views["g"], views["m"], views["v"], step, LR, betas=(0.9, 0.999), eps=EPS,
                         l2_coefs=coefs if any(coefs) else None, l2_partials=partials)
    return {k: t.cpu().numpy() for k, t in dev.items()}


def _check_against(got, arena, offs, ns, want, wd, what):
    worst = dict(p=0.0, m=0.0, v=0.0)
    inside = np.zeros(arena["p"].size, dtype=bool)
    for i, (o, n) in enumerate(zip(offs, ns)):
        inside[o:o + n] = True
        p_ref, m_ref, v_ref, dead = want[i]
        p0 = arena["p"][o:o + n].astype(np.float64)
        p, m, v = (got[k][o:o + n] for k in "pmv")
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all(), (what, i)
        for k, a, r in (("m", m, m_ref), ("v", v, v_ref)):
            if np.abs(r).max() > 0:
                worst[k] = max(worst[k], rel_max(a, r))
                assert rel_max(a, r) <= TOL, (what, i, k, rel_max(a, r))
            else:
                assert not a.any(), (what, i, k)
        bound = 2.0 ** -24 * np.abs(p_ref) + TOL * np.abs(p_ref - p0).max()
        err = np.abs(p.astype(np.float64) - p_ref)
        worst["p"] = max(worst["p"], float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (what, i, float(err.max()), float(bound.min()))
        if wd == 0.0 or i % 2 == 1:                                                                # g = m = v = 0 and no L2 term: nothing moves
            assert np.array_equal(p[dead], arena["p"][o:o + n][dead]) and not m[dead].any() and not v[dead].any(), (what, i)
    print(f"{what}: m rel_max {worst['m']:.2e}, v rel_max {worst['v']:.2e}, p worst error / bound {worst['p']:.2e}")
    assert np.array_equal(got["g"], arena["g"]), what                                              # g and every guard: the bits they had
    for k in "pmv":
        assert np.array_equal(got[k][~inside], arena[k][~inside]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("ns", [NINE, SEVENTEEN], ids=["nine", "seventeen"])
def test_one_step_vs_fp64(engine, ns, step, wd):
    arena, offs, coefs, want = _case(ns, step, wd)
    if ns is NINE:
        assert [o % 4 for o in offs] == [0] * 8 + [1]
    n0 = engine.launch_count()
    got = _step_on_device(engine, arena, offs, ns, coefs, step)
    assert engine.launch_count() - n0 == -(-len(ns) // 16)
    _check_against(got, arena, offs, ns, want, wd, f"{len(ns)} tensors step {step} wd {wd}")
    again = _step_on_device(engine, arena, offs, ns, coefs, step)
    for k in "pgmv":
        assert np.array_equal(got[k], again[k]), k


@pytest.mark.gpu
def test_l2_partials_and_loss_slot(engine):
    wd, step = 0.01, 2
    arena, offs, coefs, want = _case(NINE, step, wd, seed=5)
    chunks = ref.chunk_count(NINE)
    partials = torch.full((chunks + 2,), float("nan"), dtype=torch.float64, device="cuda")
    got = _step_on_device(engine, arena, offs, NINE, coefs, step, partials=partials[:chunks])
    _check_against(got, arena, offs, NINE, want, wd, "with partials")
    part = partials.cpu().numpy()
    assert np.isnan(part[chunks:]).all() and np.isfinite(part[:chunks]).all()
    ps = [arena["p"][o:o + n] for o, n in zip(offs, NINE)]
    c = 0
    for i, n in enumerate(NINE):                                                                   # chunk by chunk: biases are not counted
        for k in range(-(-n // ref.CHUNK)):
            w = ps[i][k * ref.CHUNK:(k + 1) * ref.CHUNK].astype(np.float64)
            exact = float((w ** 2).sum()) if coefs[i] > 0 else 0.0
            assert abs(part[c] - exact) <= 1e-12 * exact, (i, k)
            c += 1
    total = ref.l2_sum(ps, coefs)
    assert c == chunks and abs(part[:chunks].sum() - total) <= 1e-12 * total and total > 0
    # the loss value into its slot
    neg_ll = torch.tensor(431.62537, device="cuda")
    kl = torch.tensor([7.3190207], device="cuda")
    anneal = 0.137
    for trial in range(2):
        out = torch.full((3,), float("nan"), device="cuda")
        engine.vae_loss_slot(neg_ll, kl, anneal, out, 1)
        plain = neg_ll + anneal * kl[0] + torch.zeros((), device="cuda")
        assert torch.equal(out[1], plain) and bool(torch.isnan(out[0])) and bool(torch.isnan(out[2]))
    zero = torch.tensor(-0.0, device="cuda")                                                       # -0 + 0 * kl + 0 = +0, torch's sign
    engine.vae_loss_slot(zero, kl, 0.0, out, 0)
    assert torch.equal(out[0], zero + 0.0 * kl[0] + torch.zeros((), device="cuda")) and not bool(torch.signbit(out[0]))
    out = torch.full((3,), float("nan"), device="cuda")
    engine.vae_loss_slot(neg_ll, kl, anneal, out, 2, l2_partials=partials[:chunks], weight_decay=wd)
    exact = float(neg_ll.double()) + float(np.float32(anneal)) * float(kl.double()) + wd * total
    err = abs(float(out[2]) / exact - 1)
    print(f"loss with L2 {float(out[2]):.8g} float64 {exact:.8g} rel {err:.2e}")
    assert err <= 1e-6 and bool(torch.isnan(out[:2]).all())
    again = torch.full((3,), float("nan"), device="cuda")
    engine.vae_loss_slot(neg_ll, kl, anneal, again, 2, l2_partials=partials[:chunks], weight_decay=wd)
    assert torch.equal(out[2], again[2])


@pytest.mark.gpu
@pytest.mark.parametrize("steps_before", [0, 2])
def test_device_adam_vs_torch_adam_on_the_device(engine, steps_before):
    from sdrm_amd.vae_hooks import DeviceAdam
    shapes = [(f"t{i}.{'weight' if i % 2 == 0 else 'bias'}", (n,)) for i, n in enumerate(NINE[:-1])] + [("t8.weight", (4099,))]
    named = _named(shapes, device="cuda", seed=11)
    params = [p for _, p in named]
    theirs = torch.optim.Adam(params, lr=LR, foreach=False)
    ours = DeviceAdam(named, lr=LR, engine=engine)
    g = torch.Generator().manual_seed(12)
    for _ in range(steps_before):                                                                  # a state with history, made by torch
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g) * 0.01).cuda()
        theirs.step()
    if steps_before:
        ours.load_state_dict(theirs.state_dict())
    for i, p in enumerate(params):
        p.grad = (torch.randn(p.shape, generator=g) * 0.01).cuda()
        p.grad[1::3] = 0.0
    start = [p.detach().clone() for p in params]
    ours.step()
    mine = [p.detach().clone() for p in params]
    assert ours.step_count == steps_before + 1
    with torch.no_grad():
        for p, q in zip(params, start):
            p.copy_(q)
    theirs.step()
    for i, p in enumerate(params):
        st = theirs.state[p]
        assert float(st["step"]) == ours.step_count
        for k, a, r in (("m", ours.exp_avg[i], st["exp_avg"]), ("v", ours.exp_avg_sq[i], st["exp_avg_sq"])):
            assert rel_max(a.cpu().numpy(), r.cpu().numpy()) <= TOL, (i, k)
        p_ref, p0, got = p.detach().double().cpu().numpy(), start[i].double().cpu().numpy(), mine[i].double().cpu().numpy()
        bound = 2.0 ** -24 * np.abs(p_ref) + TOL * np.abs(p_ref - p0).max()
        assert np.abs(p_ref - p0).max() > 0 and (np.abs(got - p_ref) <= bound).all(), (i, float(np.abs(got - p_ref).max()))


@pytest.mark.gpu
def test_refusals(engine):
    from sdrm_amd.engine import SdrmError
    from sdrm_amd.vae_hooks import DeviceAdam
    arena = {k: torch.from_numpy((np.random.RandomState(i).standard_normal(64) * 0.1).astype(np.float32)).cuda().abs() for i, k in enumerate("pgmv")}
    keep = {k: t.clone() for k, t in arena.items()}

    def tensors(k, spans=((0, 5), (8, 13))):
        return [arena[k][a:b] for a, b in spans]

    def call(p=None, g=None, m=None, v=None, step=1, **kw):
        given = dict(p=p, g=g, m=m, v=v)
        engine.vae_adam_step(*[tensors(k) if given[k] is None else given[k] for k in "pgmv"], step, LR, **kw)

    partials = torch.zeros(1, dtype=torch.float64, device="cuda")
    bad = dict(step0=dict(step=0), negative_step=dict(step=-1), empty=dict(**{k: [arena[n][0:0], arena[n][8:13]] for k, n in zip("pgmv", "pgmv")}),
               no_tensor=dict(p=[], g=[], m=[], v=[]),
               capacity=dict(l2_coefs=[0.01, 0.0], l2_partials=partials),                          # two chunks, one slot
               overlap_one_element=dict(g=[arena["p"][4:9], arena["g"][8:13]]),                    # g of tensor 0 starts on p's last element
               overlap_across_tensors=dict(p=[arena["p"][0:5], arena["p"][4:9]]),
               g_is_p=dict(g=tensors("p")), wrong_dtype=dict(m=[t.double() for t in tensors("m")]),
               wrong_length=dict(v=[arena["v"][0:6], arena["v"][8:13]]), not_contiguous=dict(g=[arena["g"][0:10:2], arena["g"][20:25]]),
               negative_coefficient=dict(l2_coefs=[-0.01, 0.0]))
    for name, kw in bad.items():
        with pytest.raises(SdrmError):
            call(**kw)
        for k in "pgmv":
            assert torch.equal(arena[k], keep[k]), (name, k)
    call(p=[arena["p"][0:5], arena["p"][5:10]], g=[arena["g"][0:5], arena["g"][5:10]])             # ranges that only touch: accepted
    assert not torch.equal(arena["p"][:10], keep["p"][:10]) and torch.equal(arena["p"][10:], keep["p"][10:])
    named = _named(SHAPES8, device="cuda")
    opt = DeviceAdam(named, lr=LR, engine=engine)
    for _, p in named[:-1]:
        p.grad = torch.zeros_like(p)
    with pytest.raises(SdrmError, match="decoder.2.bias is None"):
        opt.step()
    named[-1][1].grad = torch.zeros(120, device="cuda")[::2]
    with pytest.raises(SdrmError, match="not contiguous"):
        opt.step()
    assert opt.step_count == 0 and all(not m.any() for m in opt.exp_avg)
    out = torch.zeros(3, device="cuda")
    one = torch.ones((), device="cuda")
    for kw in (dict(slot=3), dict(slot=-1), dict(neg_ll=torch.ones(2, device="cuda")), dict(kl=one.double()), dict(out=out.double())):
        a = dict(dict(neg_ll=one, kl=one, anneal=0.1, out=out, slot=0), **kw)
        with pytest.raises(SdrmError):
            engine.vae_loss_slot(a["neg_ll"], a["kl"], a["anneal"], a["out"], a["slot"])
    assert not out.any()


def _pre_stage(where, monkeypatch, record, **kw):
    """Test 12's pre-stage of tests/test_vae_decoder_train.py - 40 users x 60 items, batch 16, two epochs, equal seeds, the five flags -
    plus `kw`: the model, and every step's loss as a device tensor (what the engine wrote into the epoch's buffer, or what went into
    `backward()` without `device_optimizer`)."""
    from sdrm_amd.engine import Engine
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    users, n_items, batch, epochs = 40, 60, 16, kw.pop("epochs", 2)
    m = synth.synth_feed_csr(kw.pop("users", users), n_items, 0.2, seed=72, ratings=False)
    losses = []
    orig_slot, orig_backward = Engine.vae_loss_slot, torch.Tensor.backward

    def loss_slot(self, neg_ll, kl, anneal, out, slot, **k):
        orig_slot(self, neg_ll, kl, anneal, out, slot, **k)
        losses.append(out[slot].clone())

    def backward(self, *a, **k):
        if record == "backward":
            losses.append(self.detach().clone())
        return orig_backward(self, *a, **k)

    monkeypatch.setattr(Engine, "vae_loss_slot", loss_slot)
    monkeypatch.setattr(torch.Tensor, "backward", backward)
    torch.manual_seed(21)
    np.random.seed(22)
    vae = VAE(n_items, 16, 8).cuda()
    train_variational_autoencoder(vae, m, m, epochs, batch, 1e-3, "Recall@10", str(where), device_feed=True, sparse_input=True,
                                  device_holdout=True, device_latent=True, device_decoder=True, **kw)
    monkeypatch.setattr(Engine, "vae_loss_slot", orig_slot)
    monkeypatch.setattr(torch.Tensor, "backward", orig_backward)
    return vae, torch.stack(losses).cpu().numpy()


@pytest.mark.gpu
def test_direct_step_equals_autograd_step_bit_for_bit(tmp_path, monkeypatch):
    from sdrm_amd import vae_hooks
    from sdrm_amd.engine import utility_engine
    steps = 2 * 3
    monkeypatch.setattr(vae_hooks, "DIRECT_STEP", False)
    calls = []
    orig_step = vae_hooks.vae_train_step
    monkeypatch.setattr(vae_hooks, "vae_train_step", lambda *a, **k: (calls.append(1), orig_step(*a, **k))[1])
    a, loss_a = _pre_stage(tmp_path / "a", monkeypatch, "slot", device_optimizer=True)
    assert not calls and loss_a.size == steps and np.isfinite(loss_a).all()
    monkeypatch.setattr(vae_hooks, "DIRECT_STEP", True)

    def forbidden(what):
        def raiser(*args, **kw):
            raise AssertionError(f"{what} called in the direct step")
        return raiser

    for cls in (vae_hooks._SparseInputLinear, vae_hooks._LatentHead, vae_hooks._DecoderNLL):
        monkeypatch.setattr(cls, "apply", forbidden(cls.__name__ + ".apply"))
    orig_forward = torch.nn.Linear.forward

    def forward(self, x):
        if self.training:                                                                          # the train half; the evaluation half's model(...) keeps its Linears
            raise AssertionError("nn.Linear.forward called in the train half")
        return orig_forward(self, x)

    monkeypatch.setattr(torch.nn.Linear, "forward", forward)
    monkeypatch.setattr(torch.Tensor, "backward", forbidden("Tensor.backward"))
    b, loss_b = _pre_stage(tmp_path / "b", monkeypatch, "slot", device_optimizer=True)
    monkeypatch.setattr(torch.nn.Linear, "forward", orig_forward)
    utility_engine().feed_status()
    assert len(calls) == steps and loss_b.size == steps
    print("losses, autograd:", loss_a, "direct:", loss_b)
    assert np.array_equal(loss_a, loss_b)
    for (name, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(p, q), name
        assert all(x.grad is None for x in b.parameters())
    assert a.model_is_trained and b.model_is_trained


@pytest.mark.gpu
def test_device_optimizer_vs_torch_adam_in_the_pre_stage(tmp_path, monkeypatch):
    from sdrm_amd import vae_hooks
    monkeypatch.setattr(vae_hooks, "DIRECT_STEP", False)                                           # the flag alone: the optimizer and the loss slot
    _, loss_t = _pre_stage(tmp_path / "a", monkeypatch, "backward")
    _, loss_d = _pre_stage(tmp_path / "b", monkeypatch, "slot", device_optimizer=True)
    assert loss_t.size == loss_d.size == 6
    rel = np.abs(loss_d / loss_t - 1)
    print(f"first step {loss_d[0]:.8g} against {loss_t[0]:.8g}; largest relative difference over the later steps {rel[1:].max():.2e}")
    assert loss_d[0].tobytes() == loss_t[0].tobytes()                                              # computed before any update
    assert rel[1:].max() <= TOL
    # one batch, one epoch: the parameters after ONE update, at the one-step bars
    torch.manual_seed(21)
    init = vae_hooks.VAE(60, 16, 8).state_dict()
    t, _ = _pre_stage(tmp_path / "c", monkeypatch, "backward", users=16, epochs=1)
    d, _ = _pre_stage(tmp_path / "d", monkeypatch, "slot", users=16, epochs=1, device_optimizer=True)
    for (name, p), (_, q) in zip(t.state_dict().items(), d.state_dict().items()):
        p_ref, got, p0 = p.double().cpu().numpy(), q.double().cpu().numpy(), init[name].double().numpy()
        bound = 2.0 ** -24 * np.abs(p_ref) + TOL * np.abs(p_ref - p0).max()
        print(f"{name}: largest update {np.abs(p_ref - p0).max():.2e}, largest difference {np.abs(got - p_ref).max():.2e}")
        assert np.abs(p_ref - p0).max() > 0 and (np.abs(got - p_ref) <= bound).all(), name


@pytest.mark.gpu
def test_train_SDRM_with_all_six_keywords(tmp_path, monkeypatch):
    import sdrm_amd.train_SDRM as ts
    from sdrm_amd import vae_hooks
    from sdrm_amd.engine import utility_engine
    from test_reference_surface import make_feed
    data = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)
    dl = make_feed(data, 16)
    calls = []
    orig_step = vae_hooks.vae_train_step
    monkeypatch.setattr(vae_hooks, "vae_train_step", lambda *a, **k: (calls.append(1), orig_step(*a, **k))[1])
    on = dict(vae_device_feed=True, vae_device_holdout=True, vae_sparse_input=True, vae_device_latent=True, vae_device_decoder=True,
              vae_device_optimizer=True)

    def run(where):
        torch.manual_seed(31)
        np.random.seed(32)
        return ts.train_SDRM(dl, 60, 16, 8, 16, 1e-3, 8, 1, 1e-3, 1, 5, 1.0, str(where), data, data, "Recall@10", **on)

    torch.manual_seed(31)
    init = ts.VAE(60, 16, 8).state_dict()
    DIFF, vae = run(tmp_path / "a")
    assert vae.model_is_trained and vae.is_training == 0 and len(calls) >= 3 and len(calls) % 3 == 0
    utility_engine().feed_status()
    moved = 0
    for name, p in vae.state_dict().items():
        assert bool(torch.isfinite(p).all()), name
        moved += int(not torch.equal(p.cpu(), init[name]))
    assert moved == len(init)
    assert np.isfinite(float(DIFF.last_loss.cpu()))

    def broken(*a, **k):
        raise RuntimeError("vae_train_step is what these keywords reach")

    monkeypatch.setattr(vae_hooks, "vae_train_step", broken)
    with pytest.raises(RuntimeError, match="these keywords reach"):
        run(tmp_path / "b")


@pytest.mark.gpu
def test_neighbours_are_left_alone(engine):
    rng = np.random.RandomState(31)
    hidden, n_items, latent = 48, 70, 8
    enc = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in ((hidden, n_items), (hidden,), (2 * latent, hidden), (2 * latent,))]
    dec = [torch.from_numpy(rng.standard_normal(s).astype(np.float32) * 0.1).cuda() for s in ((hidden, latent), (hidden,), (n_items, hidden), (n_items,))]
    zs = torch.from_numpy(rng.standard_normal((19, latent)).astype(np.float32)).cuda()
    engine.vae_encoder_load(*enc)
    feed = engine.csr_to_device(synth.synth_feed_csr(64, n_items, 0.2, seed=84, ratings=False))
    L, W, T, H, B = engine.L, engine.W, engine.T, engine.H, 12
    flat = synth.flatten_params(synth.init_params(L, W, T, H, seed=1), H)
    x0 = synth.synth_latents(B, L, seed=0)
    eps, t, masks = synth.synth_train_randoms(B, L, T, 1.0, seed=2)

    def everything():
        engine.set_params(flat)
        engine.adam_reset()
        loss = engine.train_step(x0, 1e-3, noise=eps, t=t, keep=masks).clone()
        return engine.vae_encode_csr(feed, row0=0, b=64, return_kl=True) + (engine.vae_decode(zs, *dec), loss, engine.get_params().clone())

    before = everything()
    arena, offs, coefs, _ = _case(NINE, 2, 0.01)
    partials = torch.zeros(ref.chunk_count(NINE), dtype=torch.float64, device="cuda")
    _step_on_device(engine, arena, offs, NINE, coefs, 2, partials=partials)
    engine.vae_loss_slot(torch.ones((), device="cuda"), torch.ones((), device="cuda"), 0.1, torch.zeros(2, device="cuda"), 1,
                         l2_partials=partials, weight_decay=0.01)
    after = everything()
    assert len(before) == len(after)
    for k, (x, y) in enumerate(zip(before, after)):
        assert torch.equal(x, y), k
