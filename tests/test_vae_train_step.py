"""The WHOLE train step of the VAE pre-stage, `vae_hooks.vae_train_step`, held to the reference's own arithmetic (reference
train_SDRM.py:132-150, :231-264) through tests/vae_step_ref.py, a float64 statement of the step in plain dense torch autograd.

What pins what: the reference's `train_variational_autoencoder` (fp32, restated randoms injected) -> tests/golden/vae_train_steps.npz
-> the whole-step oracle -> the three piecewise restatements the kernels' own tests use; and the whole-step oracle -> `vae_train_step`
on the device, teacher-forced at five shapes, plus the pre-stage's schedule, seeds, anneal and losses with all seven flags.

CPU: the oracle against the fixture; against the composition of the piecewise restatements; the bars' teeth; the L2 coefficient as the
float32 the engine takes; the schedule replay.
GPU (-m gpu): the direct step against the oracle at S1 .. S5; the pre-stage's schedule and losses; the persistent gradient buffers.

Bars.  Device gradients against the oracle at the read-back parameters: rel_l2 and rel_max <= 1e-4 (the project's fp32 bar); the loss
<= 1e-5 relative; parameters and moments against the float64 Adam fed the device's gradients: |got - want| <= 2^-24 |want| + 1e-4
max|want - before|, the bound of tests/test_vae_adam.py.  Oracle against the fixture: gradients rel_max <= 1e-5 (20 x the 5e-7 between
the fp32 reference and float64 at this shape), loss <= 1e-6 relative, parameters <= 1e-4 max|p_after - p_init| absolute.  Oracle
against the piecewise composition: <= 1e-12 relative (both float64; measured 3e-15 at most)."""
import os

import numpy as np
import pytest
import torch

import vae_step_ref as ref
from vae_step_ref import NAMES, SHORT, rel_l2, rel_max

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_LOSS = 1e-4, 1e-5
TOL_FIXTURE_GRAD, TOL_FIXTURE_LOSS, TOL_FIXTURE_PARAM = 1e-5, 1e-6, 1e-4
TOL_PIECEWISE = 1e-12
TEETH = 1e-3                                  # 10 x the GPU bar: what a wrong anneal, scale, step or L2 coefficient must move
ANNEAL_CYCLE = (0.2, 0.0, 0.07)               # the teacher-forced steps' explicit anneals, then the schedule's own
SENTINEL = 12345.0


def _step_args(s, k=0):
    rows, step, anneal = s["sched"]["steps"][k]
    return dict(tensors=s["tensors"], m=s["m"], rows=rows, drop_seed=s["sched"]["drop_seed"], latent_seed=s["sched"]["latent_seed"],
                step=step, anneal=anneal, p_drop=s["p_drop"], weight_decay=s["weight_decay"])


# ---------------------------------------------------------------------------------------------- CPU
def test_oracle_vs_reference_fixture(golden):
    """The oracle, free-running in float64 from the stored initial state over the stored rows, against the reference's own fp32 run.
    Measured (worst of the six steps): gradients rel_max 3.2e-7 (W1), 3.2e-7 (b1), 3.3e-7 (W2), 2.4e-7 (b2), 3.2e-7 (W3), 3.0e-7 (b3),
    2.8e-7 (W4), 2.0e-7 (b4); loss 8.4e-8 relative; parameters 1.4e-5 (W2) of max|p_after - p_init| at most."""
    g = golden("vae_train_steps")
    s = ref.shape_inputs("S1")
    users, items, hidden, latent, batch, epochs, n_steps = (int(v) for v in g["dims"])
    assert (users, items, hidden, latent, batch, epochs) == (s["users"], s["items"], s["hidden"], s["latent"], s["batch"], ref.EPOCHS)
    np_seed, drop_seed, holdout_seed, latent_seed = (int(v) for v in g["seeds"])
    sched = s["sched"]
    assert (np_seed, drop_seed, holdout_seed, latent_seed) == (s["np_seed"], sched["drop_seed"], sched["holdout_seed"], sched["latent_seed"])
    p_drop, lr = (float(v) for v in g["p_drop_lr"])
    init = [g[f"init_{i}"] for i in range(8)]
    for a, b in zip(init, s["tensors"]):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    steps = [(g[f"s{k}_rows"], k, min(ref.ANNEAL_CAP, k / ref.ANNEAL_STEPS)) for k in range(n_steps)]
    assert n_steps == 6 and [len(r) for r, _, _ in steps] == [32, 32, 1, 32, 32, 1]
    for k in range(3):
        assert np.array_equal(steps[k][0], sched["steps"][k][0])                                  # the first epoch is the replayed one
    for e in range(epochs):
        assert np.array_equal(np.sort(np.concatenate([steps[3 * e + j][0] for j in range(3)])), np.arange(users))
    run = ref.free_run(init, s["m"], steps, drop_seed, latent_seed, p_drop, 0.0, lr=lr)
    worst_g, worst_p, worst_l = [0.0] * 8, [0.0] * 8, 0.0
    for k, res in enumerate(run):
        worst_l = max(worst_l, abs(res["loss"] / float(g[f"s{k}_loss"]) - 1))
        for i in range(8):
            worst_g[i] = max(worst_g[i], rel_max(res["grads"][i], g[f"s{k}_grad_{i}"]))
            want = g[f"s{k}_after_{i}"].astype(np.float64)
            worst_p[i] = max(worst_p[i], np.abs(res["after"][i] - want).max() / np.abs(want - init[i]).max())
    print("oracle vs fixture, worst of", n_steps, "steps: loss", f"{worst_l:.2e}")
    for i in range(8):
        print(f"  {SHORT[i]}: gradient rel_max {worst_g[i]:.2e}, parameters {worst_p[i]:.2e} of the largest movement")
    assert worst_l <= TOL_FIXTURE_LOSS
    assert max(worst_g) <= TOL_FIXTURE_GRAD, worst_g
    assert max(worst_p) <= TOL_FIXTURE_PARAM, worst_p


@pytest.mark.parametrize("name", sorted(ref.SHAPES))
def test_oracle_equals_the_piecewise_restatements(name):
    s = ref.shape_inputs(name)
    for k, anneal in ((0, 0.2), (len(s["sched"]["steps"]) - 1, None)):                            # a full batch; the ragged last one
        args = _step_args(s, k)
        if anneal is not None:
            args["anneal"] = anneal
        got = ref.train_step(**args)
        loss, grads = ref.piecewise_step(**args)
        errs = [rel_max(a, b) for a, b in zip(got["grads"], grads)]
        print(name, "step", k, "loss", abs(got["loss"] / loss - 1), "gradients", max(errs))
        assert abs(got["loss"] / loss - 1) <= TOL_PIECEWISE
        assert max(errs) <= TOL_PIECEWISE, errs
        assert (got["l2"] > 0) == (s["weight_decay"] > 0)


@pytest.mark.parametrize("name", ["S1", "S2"])
def test_the_bars_have_teeth(name):
    """A wrong anneal, a missing 1 / (1 - p), a step counter one off or a lost L2 coefficient moves dW1 and dW2 by at least 10 x the GPU
    bar.  The L2 coefficient reaches no gradient of neg_ll + anneal kl, so its change is measured where the step uses it: in the
    effective gradient g + 2 weight_decay W the optimizer takes, and in the loss."""
    s = ref.shape_inputs(name)
    args = dict(_step_args(s), anneal=0.2)
    base = ref.train_step(**args)
    changes = {"anneal = 0": dict(anneal=0.0), "no 1/(1-p)": dict(drop_scale=1.0), "step + 1": dict(step=args["step"] + 1)}
    for what, kw in changes.items():
        other = ref.train_step(**dict(args, **kw))
        d1, d2 = rel_max(other["grads"][0], base["grads"][0]), rel_max(other["grads"][2], base["grads"][2])
        print(f"{name}, {what}: dW1 {d1:.2e}, dW2 {d2:.2e}")
        assert min(d1, d2) >= TEETH, what
    if s["weight_decay"] > 0:
        wd = s["weight_decay"]
        other = ref.train_step(**dict(args, weight_decay=0.0))
        eff = [b + 2 * wd * np.asarray(s["tensors"][i], np.float64) for i, b in ((0, base["grads"][0]), (2, base["grads"][2]))]
        d1, d2 = rel_max(other["grads"][0], eff[0]), rel_max(other["grads"][2], eff[1])
        print(f"{name}, weight_decay = 0: effective dW1 {d1:.2e}, dW2 {d2:.2e}, loss {abs(other['loss'] / base['loss'] - 1):.2e}")
        assert min(d1, d2) >= TEETH
        assert abs(other["loss"] / base["loss"] - 1) >= 10 * TOL_LOSS
    # at the pre-stage's own anneal of the first steps the KL term is invisible - the reason for the explicit anneals of the GPU test
    low = ref.train_step(**dict(args, anneal=2.5e-4))
    none = ref.train_step(**dict(args, anneal=0.0))
    d1, d2 = rel_max(none["grads"][0], low["grads"][0]), rel_max(none["grads"][2], low["grads"][2])
    print(f"{name}, anneal 2.5e-4 -> 0: dW1 {d1:.2e}, dW2 {d2:.2e}")
    assert max(d1, d2) < TEETH


def test_adam_takes_the_l2_coefficient_as_float32():
    """The engine's call and the reference's fp32 autograd hold `weight_decay` as a float32.  Where 2 c p cancels the gradient to within
    Adam's eps, the 2e-8 between 0.01 and float32(0.01) is more than the bar of a whole update - so the oracle's Adam takes the
    float32 (with 0.01 as a float64, three elements of S2's W1 miss bar (d) by a third at the first step)."""
    wd = ref.SHAPES["S2"][8]
    c32 = float(np.float32(wd))
    assert c32 != wd and ref.l2_coefs(wd) == [c32, 0.0] * 4 and ref.l2_coefs(0.0) == [0.0] * 8
    p = np.asarray([0.05])
    g = -2.0 * c32 * p + 1e-9                                                                     # the effective gradient: 1e-9, a tenth of eps
    zero = np.zeros(1)
    as_f32 = ref.adam(p, g, zero, zero, 1, ref.LR, l2_coef=c32)[0]
    as_f64 = ref.adam(p, g, zero, zero, 1, ref.LR, l2_coef=wd)[0]
    print("update with the float32 coefficient", p - as_f32, "with the float64 one", p - as_f64)
    assert abs(as_f32 - as_f64)[0] > TOL * ref.LR


@pytest.mark.parametrize("name", sorted(ref.SHAPES))
def test_schedule_replay(name):
    s = ref.shape_inputs(name)
    sched, users, batch = s["sched"], s["users"], s["batch"]
    assert len({sched["drop_seed"], sched["holdout_seed"], sched["latent_seed"]}) == 3
    assert all(0 <= v < 2 ** 63 for v in (sched["drop_seed"], sched["holdout_seed"], sched["latent_seed"]))
    per_epoch = -(-users // batch)
    assert len(sched["steps"]) == ref.EPOCHS * per_epoch == len(sched["places"])
    for e in range(ref.EPOCHS):
        seen = np.concatenate([rows for rows, _, _ in sched["steps"][e * per_epoch:(e + 1) * per_epoch]])
        assert np.array_equal(np.sort(seen), np.arange(users))                                    # every user once per epoch
        assert np.array_equal(seen, sched["orders"][e])
    assert not np.array_equal(sched["orders"][0], sched["orders"][1])
    assert [st for _, st, _ in sched["steps"]] == list(range(len(sched["steps"])))
    assert [a for _, _, a in sched["steps"]] == [min(0.2, k / 20000) for k in range(len(sched["steps"]))]
    assert len(sched["steps"][per_epoch - 1][0]) == users - (per_epoch - 1) * batch               # the ragged last batch
    # the replay is numpy's global stream after np.random.seed
    state = np.random.get_state()
    np.random.seed(s["np_seed"])
    seeds = [int(np.random.randint(2 ** 63, dtype=np.int64)) for _ in range(3)]
    first = np.random.permutation(users)
    np.random.set_state(state)
    assert seeds == [sched["drop_seed"], sched["holdout_seed"], sched["latent_seed"]] and np.array_equal(first, sched["orders"][0])
    if ref.SHAPES[name][6]:                                                                       # the empty and the full row: first batch
        nnz = np.diff(s["m"].indptr)[sched["steps"][0][0]]
        assert nnz.min() == 0 and nnz.max() == s["items"]


# ---------------------------------------------------------------------------------------------- GPU
def _device_setup(s):
    """(model in train mode, feed, optimizer, engine) of shape dict `s` on the device: what `train_variational_autoencoder` builds."""
    from sdrm_amd.engine import utility_engine
    from sdrm_amd.vae_hooks import VAE, DeviceAdam, SparseFeed
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    model = VAE(s["items"], s["hidden"], s["latent"], p_drop=s["p_drop"])
    with torch.no_grad():
        for (name, p), t in zip(model.named_parameters(), s["tensors"]):
            assert tuple(p.shape) == t.shape, name
            p.copy_(torch.from_numpy(t))
    model.weight_decay = s["weight_decay"]
    model = model.cuda()
    model.train()
    model.is_training = 1
    assert [n for n, _ in model.named_parameters()] == list(NAMES)
    eng = utility_engine()
    feed = SparseFeed(s["m"], engine=eng)
    opt = DeviceAdam(model.named_parameters(), lr=ref.LR, weight_decay=s["weight_decay"], engine=eng)
    return model, feed, opt, eng


def _read(tensors):
    return [t.detach().double().cpu().numpy() for t in tensors]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ref.SHAPES))
def test_direct_step_vs_fp64(name):
    """Teacher-forced: every step's device gradients and loss against the oracle at the parameters the device held before the step,
    and its update against the float64 Adam fed the device's gradients.  Measured on an MI355X: profiles/vae_train_step_oracle.txt."""
    from sdrm_amd.vae_hooks import vae_train_step
    s = ref.shape_inputs(name)
    sched, m, wd = s["sched"], s["m"], s["weight_decay"]
    model, feed, opt, eng = _device_setup(s)
    params = list(model.parameters())
    n_steps = len(sched["steps"])
    loss_buf = torch.full((n_steps,), SENTINEL, dtype=torch.float32, device="cuda")
    coefs = ref.l2_coefs(wd)
    prev_dw1, prev_losses, fresh_zero_columns = None, None, 0
    worst = [[0.0, 0.0, -1] for _ in range(8)]
    worst_loss = [0.0, -1]
    for k, ((rows, step, own_anneal), (epoch, lo)) in enumerate(zip(sched["steps"], sched["places"])):
        if lo == 0:
            feed.set_order(sched["orders"][epoch])
        anneal = ANNEAL_CYCLE[k] if k < len(ANNEAL_CYCLE) else own_anneal
        before_p, before_m, before_v = _read(params), _read(opt.exp_avg), _read(opt.exp_avg_sq)
        count = opt.step_count
        assert count == k == step
        vae_train_step(model, feed, lo, lo + len(rows), sched["drop_seed"], sched["latent_seed"], step, anneal, opt, loss_buf, k)
        grads = _read(opt.grad_buffers())
        losses = loss_buf.cpu().numpy()
        after_p, after_m, after_v = _read(params), _read(opt.exp_avg), _read(opt.exp_avg_sq)
        want = ref.train_step(before_p, m, rows, sched["drop_seed"], sched["latent_seed"], step, anneal, s["p_drop"], wd)
        # (a) the gradients
        errs = [(rel_l2(g, w), rel_max(g, w)) for g, w in zip(grads, want["grads"])]
        print(f"{name} step {k} (b = {len(rows)}, anneal {anneal:g}): " + ", ".join(f"d{n} {e[0]:.1e}/{e[1]:.1e}" for n, e in zip(SHORT, errs)))
        for i, e in enumerate(errs):
            if e[1] > worst[i][1]:
                worst[i] = [e[0], e[1], k]
        for n, g, e in zip(SHORT, grads, errs):
            assert np.isfinite(g).all(), (n, k)
            assert e[0] <= TOL and e[1] <= TOL, (n, k, e)
        # (b) the columns of dW1 that no kept entry of this batch reaches are exactly zero, whatever the buffer held before
        dead = ~ref.stored_and_kept(m, rows, sched["drop_seed"], step, s["p_drop"]).any(axis=0)
        unstored = np.diff(m[rows].tocsc().indptr) == 0
        assert (dead | ~unstored).all()
        assert dead.any() and (grads[0][:, dead] == 0.0).all(), k
        if prev_dw1 is not None:
            fresh_zero_columns += int((dead & (prev_dw1 != 0.0).any(axis=0)).sum())
        prev_dw1 = grads[0]
        # (c) the loss slot, and no other slot
        rel = abs(float(losses[k]) / want["loss"] - 1)
        print(f"{name} step {k}: loss {losses[k]:.8g} against {want['loss']:.10g} ({rel:.1e}), neg_ll {want['neg_ll']:.6g}, kl {want['kl']:.6g}, "
              f"l2 {want['l2']:.6g}")
        if rel > worst_loss[0]:
            worst_loss = [rel, k]
        assert rel <= TOL_LOSS, k
        assert (losses[k + 1:] == np.float32(SENTINEL)).all() and losses[k] != np.float32(SENTINEL)
        assert prev_losses is None or losses[:k].tobytes() == prev_losses[:k].tobytes()
        prev_losses = losses
        # (d) the update, from the device's own gradients
        assert opt.step_count == count + 1
        for i, n in enumerate(SHORT):
            p_ref, m_ref, v_ref = ref.adam(before_p[i], grads[i], before_m[i], before_v[i], count + 1, ref.LR, l2_coef=coefs[i])
            for what, got, w, b4 in (("p", after_p[i], p_ref, before_p[i]), ("m", after_m[i], m_ref, before_m[i]), ("v", after_v[i], v_ref, before_v[i])):
                moved = np.abs(w - b4).max()
                assert moved > 0, (n, what, k)
                assert (np.abs(got - w) <= 2.0 ** -24 * np.abs(w) + TOL * moved).all(), (n, what, k, np.abs(got - w).max(), moved)
    # (e)
    eng.feed_status()
    print(f"{name} worst: loss {worst_loss[0]:.2e} (step {worst_loss[1]}); " +
          "; ".join(f"d{n} rel_l2 {w[0]:.2e} rel_max {w[1]:.2e} (step {w[2]})" for n, w in zip(SHORT, worst)))
    print(f"{name}: {fresh_zero_columns} column(s) of dW1 exactly zero in a step and not in the step before")
    assert fresh_zero_columns > 0


@pytest.mark.gpu
def test_pre_stage_schedule_and_losses_vs_fp64(tmp_path, monkeypatch):
    """`train_variational_autoencoder` with all seven flags at S1: the rows, seeds, step counters and anneals its steps get are the
    replayed schedule's, and its losses are the free-running oracle's."""
    from sdrm_amd import vae_hooks
    from sdrm_amd.engine import Engine, utility_engine
    s = ref.shape_inputs("S1")
    sched = s["sched"]
    calls, losses, at_eval = [], [], []
    orig_step, orig_slot, orig_eval = vae_hooks.vae_train_step, Engine.vae_loss_slot, vae_hooks.evaluate_holdout

    def train_step(model, feed, lo, hi, drop_seed, latent_seed, step, anneal, opt, loss_out, slot):
        assert isinstance(anneal, tuple)
        calls.append(dict(rows=feed.order[lo:hi].cpu().numpy(), lo=lo, drop_seed=drop_seed, latent_seed=latent_seed, step=step,
                          anneal=anneal[0], anneal_dev=float(anneal[1].cpu().numpy()[0]), slot=slot))
        return orig_step(model, feed, lo, hi, drop_seed, latent_seed, step, anneal, opt, loss_out, slot)

    def loss_slot(self, neg_ll, kl, anneal, out, slot, **kw):
        orig_slot(self, neg_ll, kl, anneal, out, slot, **kw)
        losses.append(out[slot].clone())

    def evaluate_holdout(model, *a, **kw):
        at_eval.append(_read(model.parameters()))
        return orig_eval(model, *a, **kw)

    monkeypatch.setattr(vae_hooks, "vae_train_step", train_step)
    monkeypatch.setattr(Engine, "vae_loss_slot", loss_slot)
    monkeypatch.setattr(vae_hooks, "evaluate_holdout", evaluate_holdout)
    torch.manual_seed(31)
    model = vae_hooks.VAE(s["items"], s["hidden"], s["latent"], p_drop=s["p_drop"])
    with torch.no_grad():
        for p, t in zip(model.parameters(), s["tensors"]):
            p.copy_(torch.from_numpy(t))
    model = model.cuda()
    state = np.random.get_state()
    np.random.seed(s["np_seed"])
    try:
        vae_hooks.train_variational_autoencoder(model, s["m"], s["m"], ref.EPOCHS, s["batch"], ref.LR, "Recall@10", str(tmp_path), device_feed=True,
                                                sparse_input=True, device_holdout=True, device_latent=True, device_decoder=True,
                                                device_optimizer=True, device_eval=True)
    finally:
        np.random.set_state(state)
    utility_engine().feed_status()
    got = torch.stack(losses).cpu().numpy().astype(np.float64)
    assert len(calls) == len(sched["steps"]) == got.size and len(at_eval) == ref.EPOCHS
    per_epoch = len(calls) // ref.EPOCHS
    for k, (c, (rows, step, anneal), (epoch, lo)) in enumerate(zip(calls, sched["steps"], sched["places"])):
        assert np.array_equal(c["rows"], rows), k
        assert (c["lo"], c["step"], c["slot"]) == (lo, step, k % per_epoch) and type(c["step"]) is int, k
        assert (c["drop_seed"], c["latent_seed"]) == (sched["drop_seed"], sched["latent_seed"]), k
        assert c["anneal"] == anneal, k
        assert abs(c["anneal_dev"] - anneal) <= 2.0 ** -24 * anneal, k
    run = ref.free_run(s["tensors"], s["m"], sched["steps"], sched["drop_seed"], sched["latent_seed"], s["p_drop"], s["weight_decay"])
    want = np.asarray([r["loss"] for r in run])
    rel = np.abs(got / want - 1)
    print("losses on the device:", got, "oracle, free-running:", want, "relative difference:", rel)
    init = [np.asarray(t, np.float64) for t in s["tensors"]]
    for n, p, w, p0 in zip(SHORT, at_eval[0], run[per_epoch - 1]["after"], init):                 # printed, not asserted: Adam's update
        print(f"  {n} after the first epoch: rel_l2 of the movement {rel_l2(p - p0, w - p0):.2e}")  # is not Lipschitz near g = 0
    assert rel[0] <= TOL_LOSS
    assert rel[1:].max() <= TOL


@pytest.mark.gpu
def test_grad_buffers_carry_nothing_between_batches():
    """NaN in every element of the optimizer's persistent gradient vector between two steps changes no bit of the second step."""
    from sdrm_amd.vae_hooks import vae_train_step
    s = ref.shape_inputs("S2")
    sched = s["sched"]
    results = []
    for poison in (False, True):
        model, feed, opt, eng = _device_setup(s)
        feed.set_order(sched["orders"][0])
        loss_buf = torch.full((2,), SENTINEL, dtype=torch.float32, device="cuda")
        for k in range(2):
            rows, step, _ = sched["steps"][k]
            _, lo = sched["places"][k]
            if k == 1 and poison:
                views = opt.grad_buffers()
                flat = views[0]._base
                assert flat is not None and flat.dim() == 1 and flat.numel() >= sum(v.numel() for v in views)
                flat.fill_(float("nan"))
                assert all(bool(torch.isnan(v).all()) for v in views)
            vae_train_step(model, feed, lo, lo + len(rows), sched["drop_seed"], sched["latent_seed"], step, ANNEAL_CYCLE[0], opt, loss_buf, k)
        eng.feed_status()
        results.append([t.detach().cpu().numpy() for t in list(opt.grad_buffers()) + list(model.parameters()) + [loss_buf]])
    for n, a, b in zip([f"d{x}" for x in SHORT] + list(SHORT) + ["losses"], *results):
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        assert a.tobytes() == b.tobytes(), n
