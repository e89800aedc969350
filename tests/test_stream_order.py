"""Every entry point of include/sdrm_hip.h that takes a `stream`, on a busy non-blocking side stream (tests/stream_harness.py).

The header says of nearly every entry point that all its work is enqueued on the caller's stream and that nothing synchronises unless
stated.  The rest of the suite calls on the default stream and reads back with `.cpu()` - a device-wide wait - so it cannot see work
that lands on stream 0, a sampler chain that forks before the caller's pending work or is not joined back, or a hidden host wait.  Each
case here makes its call with inputs that arrive late on the side stream and outputs that start as NaN, observes every C call as it
returns, consumes the outputs on the side stream alone, and holds them to the default-stream twin (to the bits wherever the header or
an existing test promises the same bits on every call) and to the family's own reference at the family's own bar.  Each case runs with
the inputs late ("late") and with the default stream kept busy as well ("busy"); utility families run warm and cold (the side-stream
call is the engine's first of the family), and one family per scratch pattern regrows from b = 33 to b = 300 on the side stream.
Needs a real MI355X for everything but the coverage test: `pytest -m gpu`."""
import time

import numpy as np
import pytest
import torch

import stream_harness as sh

_PARAMS = [pytest.param(case, pool, variant, id=f"{case.name}-{pool}-{variant}")
           for case in sh.CASES for pool in case.pools for variant in ("late", "busy")]


def test_every_stream_entry_point_has_a_case():
    """The header's prototypes with a `void* stream` against the case table, the way test_cabi_exports_every_declared_symbol holds the
    exports to the header: an entry point added without a stream-order case fails here, on a machine without a GPU."""
    declared = sh.header_stream_entry_points()
    assert len(declared) >= 57 and len(set(declared)) == len(declared)
    covered = {name for case in sh.CASES for name in case.covers}
    assert not [n for n in declared if n not in covered], "no stream-order case reaches these entry points"
    assert not sorted(covered - set(declared)), "the case table names entry points the header does not declare with a stream"
    # every call the header does not name as synchronising is asserted to return with its inputs pending, in at least one case
    asserted = {name for case in sh.CASES for name in case.nosync}
    silent = [n for n in declared if n not in sh.SYNCHRONISING]
    assert not [n for n in silent if n not in asserted], "no case asserts that these return without waiting"
    for case in sh.CASES:
        assert set(case.nosync) <= set(case.covers) and set(case.syncs) <= set(case.covers) and not set(case.nosync) & set(case.syncs), case.name
    waits = {name for case in sh.CASES for name in case.syncs}
    assert set(sh.SYNCHRONISING) - {"sdrm_feed_status"} <= waits


@pytest.mark.gpu
@pytest.mark.parametrize("case, pool, variant", _PARAMS)
def test_entry_point_on_a_busy_side_stream(engine_cls, case, pool, variant):
    sh.run_case(case, engine_cls, pool, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["late", "busy"])
def test_set_schedule_waits_for_queued_work(engine_cls, variant):
    """sdrm_set_schedule takes no stream: it waits for the device before it rewrites the tables (include/sdrm_hip.h), so a forward
    queued on a side stream behind a delay, and not yet run when the host calls set_schedule(beta2=0.05), still uses the old schedule.
    The queued calls are perturb_input and reverse_step, the two entry points that read the beta tables outside a train step or a
    sampling call: sdrm_forward is the eps-net alone (timestep embedding, no schedule) and could not tell the two schedules apart."""
    from sdrm_amd import synth
    dims, B = (40, 40, 9, 1), 33
    device = torch.device("cuda", torch.cuda.current_device())
    flat = torch.from_numpy(synth.flatten_params(synth.init_params(*dims, seed=1), dims[3])).to(device)
    eps, t, masks = synth.synth_train_randoms(B, dims[0], dims[2], 1.0, seed=2)
    x0, eps, t = torch.from_numpy(synth.synth_latents(B, dims[0], seed=3)).to(device), torch.from_numpy(eps).to(device), torch.from_numpy(t).to(device)
    keep = torch.from_numpy(masks[0]).to(device=device, dtype=torch.uint8)

    def queued(e):
        return e.perturb_input(x0, t, eps), e.reverse_step(x0, 4, eps, keep)

    e = engine_cls(*dims, B)
    e.set_params(flat)
    old = [v.cpu() for v in queued(e)]
    e.set_schedule(beta2=0.05)
    new = [v.cpu() for v in queued(e)]
    e.close()
    assert not torch.equal(old[0], new[0]) and not torch.equal(old[1], new[1])   # the two schedules are told apart by both calls

    e = engine_cls(*dims, B)
    e.set_params(flat)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    if variant == "busy":
        sh.sleep_ms(1.5 * sh.MIN_DELAY_MS)
    with torch.cuda.stream(s):
        sh.sleep_ms(sh.MIN_DELAY_MS)
        got = queued(e)
        late = torch.cuda.Event()
        late.record(s)
        assert not late.query(), "the queued calls waited on the host"
        e.set_schedule(beta2=0.05)
        assert late.query(), "sdrm_set_schedule returned while work was still queued on the device"
        got = [v.clone() for v in got]
        after = [v.clone() for v in queued(e)]
    s.synchronize()
    e.close()
    for g, o, a, n in zip(got, old, after, new):
        assert torch.equal(g.cpu(), o), "work queued before sdrm_set_schedule saw the new schedule"
        assert torch.equal(a.cpu(), n)


# ------------------------------------------------------------------------------------------------ Python layers
def _under_side_stream(run, busy_ms):
    """`run()` under a fresh side stream with the default stream asleep for `busy_ms` - longer than the whole run took on the default
    stream, so it is busy from the first call to the last; everything `run` returns is consumed on the side stream."""
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sh.sleep_ms(busy_ms)
    with torch.cuda.stream(s):
        out = run()
        out = [t.clone() if t.is_cuda else t for t in sh.flatten(out)]
    s.synchronize()
    return [t.cpu() for t in out]


def _same(a, b, what):
    assert len(a) == len(b) and len(a) > 0, what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes(), f"{what}: tensor {i} differs from the default-stream run"


@pytest.mark.gpu
def test_train_sdrm_and_sample_ddpm_under_a_side_stream(tmp_path):
    """sdrm_amd.train_SDRM.train_SDRM for two epochs of two batches behind a frozen VAE, then sample_ddpm in both modes, at
    (40, 40, 9, 1): seeded, so the same bits under `torch.cuda.stream(s)` with the default stream busy as on the default stream."""
    import sdrm_amd.train_SDRM as ts
    from scipy.sparse import csr_matrix
    from test_reference_surface import make_feed
    L, W, T, H = 40, 40, 9, 1
    n_items, hidden, batch = 60, 32, 33
    data = csr_matrix((np.random.RandomState(5).random_sample((2 * batch, n_items)) < 0.25).astype(np.float64))

    def run():
        torch.manual_seed(7)
        vae = ts.VAE(n_items, hidden, L).cuda()
        vae.model_is_trained = True
        torch.manual_seed(1234)
        DIFF, _ = ts.train_SDRM(make_feed(data, batch), n_items, hidden, L, 32, 1e-3, W, H, 1e-3, 2, T, 0.5, str(tmp_path), data, data, "Recall@10",
                                variational_ae=vae)
        eng = DIFF.engine()
        m, v, step = eng.get_adam_state()
        assert step == 4
        outs = [ts.sample_ddpm(2 * batch, DIFF, vae, L, 0.5, timesteps=mode, n_timesteps=T) for mode in ("random", None)]
        return [eng.get_params(), m, v, DIFF.last_loss.clone()] + outs

    _driver_twin(run, "train_SDRM + sample_ddpm")


def _driver_twin(run, what):
    as_tensors = lambda out: [t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t)) for t in sh.flatten_any(out)]
    run()                                   # (warm: kernels loaded, scratch grown - the timed run below is what the side-stream run repeats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    twin = [t.cpu() for t in as_tensors(run())]
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    got = _under_side_stream(lambda: as_tensors(run()), 1.5 * wall_ms)
    _same(got, twin, what)


@pytest.mark.gpu
def test_vae_pre_stage_hook_under_a_side_stream(tmp_path):
    """`train_variational_autoencoder` with every device half on (feed, hold-out, sparse input, latent head, decoder, optimizer, eval),
    two epochs at tests/test_vae_adam.py's smallest shape: the trained weights to the bits of the default-stream run."""
    from sdrm_amd import synth
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    m = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)
    count = iter(range(10))

    def run():
        torch.manual_seed(21)
        np.random.seed(22)
        vae = VAE(60, 16, 8).cuda()
        train_variational_autoencoder(vae, m, m, 2, 16, 1e-3, "Recall@10", str(tmp_path / f"run{next(count)}"), device_feed=True, sparse_input=True,
                                      device_holdout=True, device_latent=True, device_decoder=True, device_optimizer=True, device_eval=True)
        return [v.detach().clone() for v in vae.state_dict().values()]

    _driver_twin(run, "the VAE pre-stage")


@pytest.mark.gpu
def test_mlp_driver_under_a_side_stream(engine_cls):
    """`mlp_eval.compute_mlp_results_device` (train and evaluation on the device) at tests/test_mlp_eval.py's driver shape."""
    from scipy.sparse import csr_matrix
    from sdrm_amd import mlp_eval
    rng = np.random.default_rng(2)
    training = csr_matrix((rng.random((37, 77)) < 0.2).astype(np.float32))
    validation = csr_matrix((rng.random((12, 77)) < 0.3).astype(np.float32))
    engine = engine_cls(8, 8, 4, 0, 16)

    def run():
        h = {}
        rec, ndcg = mlp_eval.compute_mlp_results_device(training, validation, engine, seed=3, epochs=2, history=h)
        return [rec, ndcg, np.asarray(h["val_rmse"]), np.asarray(h["train_loss"])] + [v.detach().clone() for v in h["model"].state_dict().values()]

    try:
        _driver_twin(run, "the MLP evaluator's driver")
    finally:
        engine.close()


@pytest.mark.gpu
def test_neumf_driver_under_a_side_stream(engine_cls):
    """`neumf.compute_neuralcf_results(device_train=True)` at tests/test_neumf_train.py's 40-user toy, two epochs."""
    from sdrm_amd import neumf
    from test_neumf_train import toy
    training, validation = toy()
    engine = engine_cls(8, 8, 4, 0, 16)

    def run():
        h = {}
        rec, ndcg = neumf.compute_neuralcf_results(training, validation, 40, 90, engine=engine, seed=2, epochs=2, eval_recall=False, history=h,
                                                   device_train=True)
        return [rec, ndcg, np.asarray(h["valid_loss"]), np.asarray(h["train_loss"])]

    try:
        _driver_twin(run, "the NeuMF evaluator's driver")
    finally:
        engine.close()
