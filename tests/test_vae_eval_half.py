"""The evaluation half of a VAE pre-stage epoch on the engine (sdrm_vae_eval_holdout, csrc/eval_half.h; `Engine.vae_eval_holdout`,
`evaluate_holdout(device_forward=True)`, `train_variational_autoencoder(device_eval=True)`, `train_SDRM(vae_device_eval=True)`).
Without a GPU: the float64 restatement tests/vae_eval_ref.py against the torch `VAE` in eval mode, the entry points, the host
argument check, and the flags with the model on the host.  On the GPU: the logits at the decode bar, the ranking bit for bit against
`Engine.rank_metrics` and the oracle, every decided user bit for bit against float64 and against the torch path, determinism and
launch counts, refusals and range checks, and a pre-stage that runs no torch `Linear` in either half.

Shapes (the smallest at which the pieces can go wrong): A = 70 users x 97 items, hidden 23, latent 5, batch 32 (three batches, the
last of 6 rows, nothing on a 4- or 32-grid); B = 40 x 301, hidden 36, latent 10, batch 16.  Rows made by hand in both: two empty
users, two with one entry (nan: nothing is held out), one with exactly two; in B one with 290 entries (232 in the train part: more than
one gather chunk of 64).

Decided users: an element error of at most tau cannot change the rank of a held item whose float64 score has no other unmasked
score within 2 tau, so a user all of whose held items are like that must get the float64 metric bit for bit.  tau is the measured
maximum element error of the same run; the tests require that at most 10 % of the users with held items are undecided."""
import contextlib
import ctypes as C
import glob
import inspect
import io
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_ref  # noqa: E402
import vae_eval_ref as ref  # noqa: E402
from oracle import rank_metrics_ref as orc  # noqa: E402
from sdrm_amd import _lib, synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = -2, -1   # SDRM_ERR_SHAPE, SDRM_ERR_ARG
TOL = 1e-4            # the project's decode bar, normwise
K = 10
SHAPES = {"A": dict(users=70, items=97, hidden=23, latent=5, batch=32, density=0.15, seed=81),
          "B": dict(users=40, items=301, hidden=36, latent=10, batch=16, density=0.08, seed=82)}
EMPTY, ONE, TWO, LONG = (3, 11), (5, 17), 8, 20   # the rows made by hand
SHORT = sorted(EMPTY + ONE)                       # fewer than two entries: nothing held out, nan


def _feed(name):
    """The whole test matrix of a shape, all ones, with the hand-made rows."""
    c = SHAPES[name]
    m = synth.synth_feed_csr(c["users"], c["items"], c["density"], seed=c["seed"], ratings=False)
    rs = np.random.RandomState(c["seed"] + 100)
    rows = [m.indices[m.indptr[u]:m.indptr[u + 1]] for u in range(c["users"])]
    for u in EMPTY:
        rows[u] = np.zeros(0, np.int32)
    for u in ONE:
        rows[u] = rs.choice(c["items"], 1).astype(np.int32)
    rows[TWO] = np.sort(rs.choice(c["items"], 2, replace=False)).astype(np.int32)
    if name == "B":
        rows[LONG] = np.sort(rs.choice(c["items"], 290, replace=False)).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    return csr_matrix((np.ones(indices.size, np.float32), indices, indptr), shape=(c["users"], c["items"]))


def _split(m, seed=0x5EED, draw=2):
    """(train, held) scipy matrices of the engine's Philox split, by its host restatement tests/holdout_ref.py."""
    tp, ti, hp, hi = holdout_ref.split(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.shape[1], 0.2, seed=seed, draw=draw)
    return (csr_matrix((np.ones(len(ti), np.float32), ti, tp), shape=m.shape), csr_matrix((np.ones(len(hi), np.float32), hi, hp), shape=m.shape))


def _vae(name):
    from sdrm_amd.vae_hooks import VAE
    c = SHAPES[name]
    torch.manual_seed(c["seed"])
    return VAE(c["items"], c["hidden"], c["latent"])   # xavier weights, as VAE.__init__ draws them


# ------------------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_equals_the_torch_vae_in_eval_mode(name):
    from sdrm_amd import metrics
    m = _feed(name)
    train, held = _split(m)
    n = np.diff(m.indptr)
    assert sorted(np.flatnonzero(n < 2)) == SHORT and n[TWO] == 2 and (name == "A" or n[LONG] == 290)
    assert (np.diff(held.indptr)[n >= 2] >= 1).all() and not np.diff(held.indptr)[n < 2].any()
    vae = _vae(name)
    s = ref.logits(ref.weights_of(vae), train)
    vae = vae.double().eval()
    vae.is_training = 0
    with torch.no_grad():
        want, _ = vae(torch.tensor(train.toarray(), dtype=torch.float64))
    want = want.numpy()
    err = np.abs(s - want).max()
    print(f"{name}: restatement against torch float64: largest difference {err:.2e} at max|s| {np.abs(want).max():.3f}")
    assert err <= 1e-12
    assert np.array_equal(ref.masked(want, train), metrics.mask_training_examples(train, want.copy()), equal_nan=True)
    for k in (K, min(128, SHAPES[name]["items"])):
        rec, ndcg = orc.rank_metrics(want, held, train=train, ks=(k,))                     # (that module ranks float32 scores)
        got = ref.metrics(s.astype(np.float32), train, held, k)
        assert rec[0].tobytes() == got[0].tobytes() and ndcg[0].tobytes() == got[1].tobytes(), k
        assert sorted(np.flatnonzero(np.isnan(got[0]))) == SHORT == sorted(np.flatnonzero(np.isnan(got[1])))


def test_entry_points_are_declared():
    with open(os.path.join(REPO, "include", "sdrm_hip.h")) as f:
        assert re.search(r"\bint sdrm_vae_eval_holdout\(sdrm_engine\* e, const sdrm_vae_encoder\* enc, const sdrm_vae_decoder\* dec,", f.read())
    with open(os.path.join(REPO, "include", "sdrm_hip_debug.h")) as f:
        assert re.search(r"\bint sdrm_debug_vae_eval_args\(int n_items, int hidden, int latent, int64_t n_rows, int batch, int k, int metric\);", f.read())
    assert len(_lib.SIGNATURES["sdrm_vae_eval_holdout"][1]) == 18 and len(_lib.SIGNATURES["sdrm_debug_vae_eval_args"][1]) == 7
    lib = _lib.load()
    assert lib.sdrm_vae_eval_holdout and lib.sdrm_debug_vae_eval_args
    from sdrm_amd import pipeline, train_SDRM, vae_hooks
    from sdrm_amd.engine import Engine
    assert inspect.signature(Engine.vae_eval_holdout).parameters["batch"].default == 500
    assert inspect.signature(vae_hooks.evaluate_holdout).parameters["device_forward"].default is False
    assert inspect.signature(vae_hooks.train_variational_autoencoder).parameters["device_eval"].default is False
    assert inspect.signature(train_SDRM.train_SDRM).parameters["vae_device_eval"].default is False
    assert pipeline.VAE_FLAGS[-1] == "vae_device_eval" and len(pipeline.VAE_FLAGS) == 7


def test_debug_vae_eval_args_envelope():
    check = _lib.load().sdrm_debug_vae_eval_args
    ok = dict(n_items=3125, hidden=600, latent=200, n_rows=6040, batch=500, k=50, metric=1)
    order = ("n_items", "hidden", "latent", "n_rows", "batch", "k", "metric")

    def rc(**kw):
        a = dict(ok, **kw)
        return check(*(a[name] for name in order))
    assert rc() == 0
    corners = (dict(n_items=1, k=1), dict(n_items=36864, k=128), dict(hidden=1), dict(hidden=4096), dict(latent=1), dict(latent=4096),
               dict(n_rows=1), dict(n_rows=(1 << 31) - 1), dict(batch=1), dict(batch=1 << 22), dict(k=1), dict(k=128), dict(n_items=50, k=50),
               dict(metric=0), dict(n_items=36864, hidden=4096, latent=4096, n_rows=(1 << 31) - 1, batch=1 << 22, k=128),
               dict(n_items=1, hidden=1, latent=1, n_rows=1, batch=1, k=1, metric=0))
    for kw in corners:
        assert rc(**kw) == 0, kw
    bad = (dict(n_items=0), dict(n_items=36865), dict(hidden=0), dict(hidden=4097), dict(latent=0), dict(latent=4097), dict(n_rows=0),
           dict(n_rows=1 << 31), dict(n_rows=-1), dict(batch=0), dict(batch=(1 << 22) + 1), dict(k=0), dict(k=129), dict(n_items=49, k=50),
           dict(metric=2), dict(metric=-1))
    for kw in bad:
        assert rc(**kw) == SHAPE, kw


def test_flags_are_ignored_for_a_model_on_the_host(tmp_path, monkeypatch):
    from sdrm_amd.vae_hooks import VAE, train_variational_autoencoder
    m = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)

    def run(where, **kw):
        torch.manual_seed(3)
        np.random.seed(4)
        vae = VAE(60, 16, 8)
        with contextlib.redirect_stdout(io.StringIO()):
            train_variational_autoencoder(vae, m, m, 2, 16, 1e-3, "Recall@10", str(where), **kw)
        return vae.state_dict(), np.random.get_state(), torch.get_rng_state()
    a, na, ta = run(tmp_path / "a")
    b, nb, tb = run(tmp_path / "b", device_eval=True)
    c, nc, tc = run(tmp_path / "c", device_feed=True, sparse_input=True, device_holdout=True, device_latent=True, device_decoder=True,
                    device_optimizer=True, device_eval=True)
    for other, n_state, t_state in ((b, nb, tb), (c, nc, tc)):
        assert np.array_equal(na[1], n_state[1]) and na[2:] == n_state[2:] and torch.equal(ta, t_state)
        for name in a:
            assert torch.equal(a[name], other[name]), name
    # train_SDRM hands the keyword on under train_variational_autoencoder's name
    from sdrm_amd import pipeline
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
            ts.train_SDRM(None, 60, 16, 8, 16, 1e-3, 8, 1, 1e-3, 1, 5, 1.0, str(tmp_path), None, None, "Recall@10", vae_device_eval=on)
        assert seen["device_eval"] is on and not seen["device_holdout"]
    seen.clear()
    with pytest.raises(Stop):
        ts.train_SDRM(None, 60, 16, 8, 16, 1e-3, 8, 1, 1e-3, 1, 5, 1.0, str(tmp_path), None, None, "Recall@10")
    assert seen["device_eval"] is False
    # run_experiment: today's hp makes the call it always made; the seven keys reach train_SDRM under their names
    calls = []
    keywords = set(inspect.signature(ts.train_SDRM).parameters)

    def fake_train_SDRM(*args, **kw):
        calls.append((args, kw))
        raise Stop

    monkeypatch.setattr(ts, "train_SDRM", fake_train_SDRM)
    monkeypatch.setattr(pipeline, "DeviceFeed", lambda *a, **k: "feed")
    import sdrm_amd.engine as engine_mod
    monkeypatch.setattr(engine_mod, "utility_engine", lambda *a, **k: None)
    hp = dict(batch=16, vae_hidden=16, latent=8, vae_batch=16, vae_lr=1e-3, H=1, lr=1e-3, epochs=1, T=5, nd=1.0)
    today = {"N_ITEMS", "VAE_HIDDEN", "VAE_LATENT", "VAE_BATCH_SIZE", "VAE_LR", "DIFF_LATENT", "N_HIDDEN_MLP_LAYERS", "DIFF_LR",
             "DIFF_TRAINING_EPOCHS", "TIMESTEPS", "noise_divider", "VAE_DIR_PATH", "TRAIN_PARTIAL_VALID_DATA", "VALID_DATA",
             "OPTIMIZATION_OBJECTIVE", "verbose", "cache_latents", "engine_encode"}
    for extra in (dict(), {flag: False for flag in pipeline.VAE_FLAGS}):
        calls.clear()
        with pytest.raises(Stop):
            pipeline.run_experiment((m, m, m), dict(hp, **extra), 0, str(tmp_path))
        (args, kw), = calls
        assert args == ("feed",) and set(kw) == today and kw["cache_latents"] is False and kw["engine_encode"] is False
    calls.clear()
    with pytest.raises(Stop):
        pipeline.run_experiment((m, m, m), dict(hp, **{flag: True for flag in pipeline.VAE_FLAGS}), 0, str(tmp_path))
    (args, kw), = calls
    assert set(kw) == today | set(pipeline.VAE_FLAGS) and all(kw[flag] is True for flag in pipeline.VAE_FLAGS)
    assert set(pipeline.VAE_FLAGS) <= keywords


# ------------------------------------------------------------------------------------------------ on the GPU
GUARD = 64
SENTINEL = -12345.0


def _guarded(n, dtype, device):
    """A buffer of n elements with GUARD sentinel elements on both sides: (whole, the n in the middle)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _weights_dev(vae):
    mods = (vae.encoder[0], vae.encoder[2], vae.decoder[0], vae.decoder[2])
    return tuple(t.detach() for mod in mods for t in (mod.weight, mod.bias))


def _run(eng, case, metric, k=K, batch=None, train_dev=None, held_dev=None, with_logits=True):
    """One guarded engine call: (scores [n] float64 numpy, logits [n, items] float32 numpy | None, guards intact)."""
    n, items = case["shape"]
    s_whole, s_mid = _guarded(n, torch.float64, eng.device)
    l_whole = l_mid = None
    if with_logits:
        l_whole, l_flat = _guarded(n * items, torch.float32, eng.device)
        l_mid = l_flat.view(n, items)
    out = eng.vae_eval_holdout(*case["weights"], train_dev or case["train_dev"], held_dev or case["held_dev"], k, metric,
                               batch=batch or case["batch"], out=s_mid, logits=l_mid)
    assert out.data_ptr() == s_mid.data_ptr()
    intact = _guards_intact(s_whole) and (l_whole is None or _guards_intact(l_whole))
    return s_mid.cpu().numpy().copy(), None if l_mid is None else l_mid.cpu().numpy().copy(), intact


def _same_bits(a, b):
    """Equal nan pattern and equal bits everywhere else (a nan's sign and payload say nothing: the device's 0/0 and numpy's differ)."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


_CASES = {}


def _case(name):
    """A shape's inputs, its float64 reference and ONE engine run per metric with the logits asked for: computed once, shared."""
    if name in _CASES:
        return _CASES[name]
    from sdrm_amd.engine import utility_engine
    eng = utility_engine()
    c = SHAPES[name]
    m = _feed(name)
    train, held = _split(m)
    vae = _vae(name)
    case = dict(shape=m.shape, batch=c["batch"], train=train, held=held, vae=vae.cuda(), s64=ref.logits(ref.weights_of(vae), train))
    case["weights"] = _weights_dev(case["vae"])
    case["train_dev"], case["held_dev"] = eng.csr_to_device(train), eng.csr_to_device(held)
    before = eng.launch_count()
    rec, logits, ok0 = _run(eng, case, "recall")
    case["launches"] = eng.launch_count() - before
    ndcg, logits1, ok1 = _run(eng, case, "ndcg")
    eng.feed_status()
    case.update(scores=(rec, ndcg), logits=logits, logits_again=logits1, intact=ok0 and ok1)
    case["tau"] = float(np.abs(logits.astype(np.float64) - case["s64"]).max())
    _CASES[name] = case
    return case


def _decided_equal(got, want, dec, what):
    """Every decided user bit for bit; at most 10 % of the users with held items undecided."""
    with_held = ~np.isnan(want)
    undecided = int((with_held & ~dec).sum())
    print(f"{what}: {undecided} of {int(with_held.sum())} users with held items undecided")
    assert undecided <= 0.1 * with_held.sum(), what
    assert got[dec].tobytes() == want[dec].tobytes(), (what, np.flatnonzero(dec & (got != want)))
    assert np.array_equal(np.isnan(got), np.isnan(want)), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_logits_against_float64(name):
    case = _case(name)
    got, want = case["logits"].astype(np.float64), case["s64"]
    b = case["batch"]
    for lo in range(0, got.shape[0], b):
        err = np.linalg.norm(got[lo:lo + b] - want[lo:lo + b]) / np.linalg.norm(want[lo:lo + b])
        print(f"{name} rows {lo}..: normwise error {err:.2e}")
        assert err <= TOL, (lo, err)
    print(f"{name}: tau = largest element error {case['tau']:.3e}, tau / max|s| = {case['tau'] / np.abs(want).max():.3e}")
    assert case["intact"]                                             # nothing behind n_rows or round the outputs is written
    assert np.array_equal(case["logits"], case["logits_again"])       # the metric does not change the forward


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_ranking_is_rank_metrics_on_the_same_logits(name):
    from sdrm_amd.engine import utility_engine
    eng = utility_engine()
    case = _case(name)
    logits = torch.from_numpy(case["logits"]).to(eng.device)
    for k in (K, min(128, case["shape"][1])):
        scores = case["scores"] if k == K else tuple(_run(eng, case, metric, k=k, with_logits=False)[0] for metric in (0, 1))
        dev = eng.rank_metrics(logits, case["held_dev"], train=case["train_dev"], ks=(k,))
        host = orc.rank_metrics(case["logits"], case["held"], train=case["train"], ks=(k,))
        for metric in (0, 1):
            got = scores[metric]
            assert _same_bits(got, dev[metric][0].cpu().numpy()), (k, metric)
            assert _same_bits(got, host[metric][0]), (k, metric)
            assert sorted(np.flatnonzero(np.isnan(got))) == SHORT, (k, metric)
    eng.feed_status()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_decided_users_match_float64_bit_for_bit(name):
    case = _case(name)
    dec = ref.decided(case["s64"], case["train"], case["held"], case["tau"])
    want = ref.metrics(case["s64"], case["train"], case["held"], K)
    for metric in (0, 1):
        _decided_equal(case["scores"][metric], want[metric], dec, f"{name} metric {metric}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_evaluate_holdout_both_ways(name):
    """`evaluate_holdout` with the torch forward and with the engine's, on equal weights, seed and draw."""
    from sdrm_amd.engine import utility_engine
    from sdrm_amd.vae_hooks import evaluate_holdout
    eng = utility_engine()
    case = _case(name)
    vae, b = case["vae"], case["batch"]
    test_dev = eng.csr_to_device(_feed(name))
    seed, draw = 0xABCDE, 3
    train_dev, held_dev = eng.holdout_split(test_dev, seed=seed, draw=draw)
    n, items = case["shape"]
    vae.eval()
    vae.is_training = 0
    with torch.no_grad():
        torch_logits = torch.cat([vae(eng.csr_rows_to_dense(train_dev, row0=lo, b=min(b, n - lo)))[0] for lo in range(0, n, b)])
    eng_logits = torch.empty(n, items, dtype=torch.float32, device=eng.device)
    eng.vae_eval_holdout(*case["weights"], train_dev, held_dev, K, 0, batch=b, logits=eng_logits)
    tau = float((torch_logits.double() - eng_logits.double()).abs().max())
    print(f"{name}: torch logits against the engine's: largest difference {tau:.3e}")
    end = int(train_dev[0][-1]), int(held_dev[0][-1])
    train = csr_matrix((np.ones(end[0], np.float32), train_dev[1][:end[0]].cpu().numpy(), train_dev[0].cpu().numpy()), shape=(n, items))
    held = csr_matrix((np.ones(end[1], np.float32), held_dev[1][:end[1]].cpu().numpy(), held_dev[0].cpu().numpy()), shape=(n, items))
    dec = ref.decided(torch_logits.double().cpu().numpy(), train, held, tau)
    for metric in ("Recall@10", "NDCG@10"):
        a = evaluate_holdout(vae, eng, test_dev, seed, draw, metric, batch=b).cpu().numpy()
        d = evaluate_holdout(vae, eng, test_dev, seed, draw, metric, batch=b, device_forward=True).cpu().numpy()
        _decided_equal(d, a, dec, f"{name} {metric}")
        assert sorted(np.flatnonzero(np.isnan(d))) == SHORT
    eng.feed_status()


@pytest.mark.gpu
def test_determinism_launch_count_batches_and_the_loaded_encoder():
    from sdrm_amd.engine import utility_engine
    eng = utility_engine()
    case = _case("A")
    n, items = case["shape"]
    batches = -(-n // case["batch"])
    print(f"launches of one call: {case['launches']} = staging + 5 x {batches} batches")
    assert batches == 3 and case["launches"] <= 2 + 5 * batches
    again, _, intact = _run(eng, case, "recall", with_logits=False)
    assert intact and _same_bits(again, case["scores"][0])
    # one batch, and a one-row tail: the same decided users, the same bits
    dec = ref.decided(case["s64"], case["train"], case["held"], case["tau"])
    want = ref.metrics(case["s64"], case["train"], case["held"], K)
    for batch in (n, n + 50, n - 1, 1 << 22):
        for metric in (0, 1):
            got, logits, intact = _run(eng, case, metric, batch=batch)
            assert intact
            tau_b = float(np.abs(logits.astype(np.float64) - case["s64"]).max())   # (this run's own error, should it be larger)
            dec_b = dec if tau_b <= case["tau"] else ref.decided(case["s64"], case["train"], case["held"], tau_b)
            _decided_equal(got, want[metric], dec_b, f"batch {batch} metric {metric}")
    # an encoder staged by vae_encoder_load is not touched by a call with other weights
    torch.manual_seed(5)
    loaded = [torch.randn(s, device=eng.device) * 0.1 for s in ((19, items), (19,), (2 * 7, 19), (2 * 7,))]
    eng.vae_encoder_load(*loaded)
    z0 = eng.vae_encode_csr(case["train_dev"], row0=0, b=n)
    _run(eng, case, "ndcg")
    caseB = _case("B")
    _run(eng, caseB, "ndcg")
    z1 = eng.vae_encode_csr(case["train_dev"], row0=0, b=n)
    assert torch.equal(z0, z1) and bool(torch.isfinite(z0).all())
    eng.feed_status()


@pytest.mark.gpu
def test_widest_item_row_ranks_under_the_raised_lds_limit():
    """36864 items, the envelope's end: the ranking's score row is 144 KB of LDS, above the 48 KB a kernel gets unasked."""
    from sdrm_amd.engine import utility_engine
    from sdrm_amd.vae_hooks import VAE
    eng = utility_engine()
    users, items, k = 5, 36864, 128
    rs = np.random.RandomState(9)
    rows = [np.sort(rs.choice(items, size=c, replace=False)).astype(np.int32) for c in (40, 300, 2, 1, 77)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    m = csr_matrix((np.ones(indptr[-1], np.float32), np.concatenate(rows), indptr), shape=(users, items))
    train, held = _split(m)
    torch.manual_seed(9)
    vae = VAE(items, 6, 3)
    s64 = ref.logits(ref.weights_of(vae), train)
    case = dict(shape=m.shape, batch=3, weights=_weights_dev(vae.cuda()), train_dev=eng.csr_to_device(train), held_dev=eng.csr_to_device(held))
    for metric in (0, 1):
        got, logits, intact = _run(eng, case, metric, k=k)
        err = np.linalg.norm(logits - s64) / np.linalg.norm(s64)
        print(f"36864 items, metric {metric}: normwise error {err:.2e}")
        assert intact and err <= TOL
        dev = eng.rank_metrics(torch.from_numpy(logits).to(eng.device), case["held_dev"], train=case["train_dev"], ks=(k,))
        assert _same_bits(got, dev[metric][0].cpu().numpy())
        assert list(np.flatnonzero(np.isnan(got))) == [3]
    eng.feed_status()


def _c_call(eng, case, k=K, metric=0, batch=None, **kw):
    """sdrm_vae_eval_holdout through ctypes with one argument replaced: its status, and the launches it made."""
    n, items = case["shape"]
    w = case["weights"]
    hidden, latent = w[4].shape
    enc = dict(w1=w[0].data_ptr(), b1=w[1].data_ptr(), w2=w[2].data_ptr(), b2=w[3].data_ptr(), n_items=items, hidden=hidden, latent=latent)
    dec = dict(w1=w[4].data_ptr(), b1=w[5].data_ptr(), w2=w[6].data_ptr(), b2=w[7].data_ptr(), latent=latent, hidden=hidden, n_items=items)
    enc.update(kw.pop("enc", {}))
    dec.update(kw.pop("dec", {}))
    _, tp, idcg = eng._rank_tables((K,))
    scores = torch.zeros(n, dtype=torch.float64, device=eng.device)
    (tr_ptr, tr_idx, _, _), (he_ptr, he_idx, _, _) = case["train_dev"], case["held_dev"]
    a = dict(train_indptr=tr_ptr.data_ptr(), train_indices=tr_idx.data_ptr(), train_nnz=tr_idx.numel(), held_indptr=he_ptr.data_ptr(),
             held_indices=he_idx.data_ptr(), held_nnz=he_idx.numel(), n_rows=n, batch=case["batch"] if batch is None else batch, k=k, tp=tp.data_ptr(),
             idcg=idcg.data_ptr(), metric=metric, scores=scores.data_ptr(), logits=None)
    a.update(kw)
    e = _lib.VaeEncoder(enc["w1"], enc["b1"], enc["w2"], enc["b2"], enc["n_items"], enc["hidden"], enc["latent"])
    d = _lib.VaeDecoder(dec["w1"], dec["b1"], dec["w2"], dec["b2"], dec["latent"], dec["hidden"], dec["n_items"])
    before = eng.launch_count()
    rc = eng.lib.sdrm_vae_eval_holdout(eng._h, C.byref(e) if a.get("enc_struct", True) else None, C.byref(d) if a.get("dec_struct", True) else None,
                                       a["train_indptr"], a["train_indices"], a["train_nnz"], a["held_indptr"], a["held_indices"], a["held_nnz"],
                                       a["n_rows"], a["batch"], a["k"], a["tp"], a["idcg"], a["metric"], a["scores"], a["logits"], None)
    torch.cuda.synchronize()
    return rc, eng.launch_count() - before


@pytest.mark.gpu
def test_refusals_make_no_launch():
    from sdrm_amd.engine import SdrmError, utility_engine
    eng = utility_engine()
    case = _case("A")
    n, items = case["shape"]
    assert _c_call(eng, case) == (0, 2 + 5 * 3)
    nulls = [dict(enc={name: None}) for name in ("w1", "b1", "w2", "b2")] + [dict(dec={name: None}) for name in ("w1", "b1", "w2", "b2")]
    nulls += [{name: None} for name in ("train_indptr", "train_indices", "held_indptr", "held_indices", "tp", "idcg", "scores")]
    nulls += [dict(enc_struct=False), dict(dec_struct=False)]
    for kw in nulls:
        assert _c_call(eng, case, **kw) == (ARG, 0), kw
    both = lambda **kw: dict(enc=dict(kw), dec=dict(kw))   # noqa: E731
    shapes = [both(n_items=0), both(n_items=36865), both(hidden=0), both(hidden=4097), both(latent=0), both(latent=4097), dict(n_rows=0),
              dict(n_rows=1 << 31), dict(batch=0), dict(batch=(1 << 22) + 1), dict(k=0), dict(k=129), dict(k=items + 1), dict(metric=2),
              dict(metric=-1), dict(enc=dict(hidden=24)), dict(dec=dict(latent=6)), dict(dec=dict(n_items=96)), dict(train_nnz=-1), dict(held_nnz=-1)]
    for kw in shapes:
        assert _c_call(eng, case, **kw) == (SHAPE, 0), kw
    with pytest.raises(SdrmError):
        eng.vae_eval_holdout(*case["weights"], case["train_dev"], case["held_dev"], 0, "recall")
    before = eng.launch_count()
    for metric in ("mrr", "", True, 2, -1, 1.0, None):
        with pytest.raises(SdrmError):
            eng.vae_eval_holdout(*case["weights"], case["train_dev"], case["held_dev"], K, metric)
    assert eng.launch_count() == before
    with pytest.raises(SdrmError):
        eng.vae_eval_holdout(*case["weights"][:7], case["weights"][7].double(), case["train_dev"], case["held_dev"], K, "recall")
    eng.feed_status()


@pytest.mark.gpu
def test_range_checks_raise_the_feed_status_and_spare_the_others():
    from sdrm_amd.engine import SdrmError, utility_engine
    eng = utility_engine()
    case = _case("A")
    n, items = case["shape"]
    tr_ptr, tr_idx = case["train"].indptr.astype(np.int64).copy(), case["train"].indices.astype(np.int32).copy()
    he_ptr, he_idx = case["held"].indptr.astype(np.int64).copy(), case["held"].indices.astype(np.int32).copy()
    a, b, c = 20, 30, 40   # a: a train column out of range; b: a held column out of range; c: an unordered train indptr pair (and c + 1 with it)
    assert tr_ptr[a + 1] - tr_ptr[a] >= 2 and he_ptr[b + 1] > he_ptr[b] and tr_ptr[c] >= 1 and tr_ptr[c + 1] > tr_ptr[c]
    tr_idx[tr_ptr[a]] = items
    he_idx[he_ptr[b]] = -1
    tr_ptr[c + 1] = tr_ptr[c] - 1
    dev = lambda ptr, idx: (torch.from_numpy(ptr).to(eng.device), torch.from_numpy(idx).to(eng.device), None, (n, items))   # noqa: E731
    spared = np.setdiff1d(np.arange(n), [a, b, c, c + 1])
    for metric in (0, 1):
        got, logits, intact = _run(eng, case, metric, train_dev=dev(tr_ptr, tr_idx), held_dev=dev(he_ptr, he_idx))
        with pytest.raises(SdrmError) as err:
            eng.feed_status()
        assert "column index" in str(err.value) and "indptr pair" in str(err.value)
        assert intact
        assert _same_bits(got[spared], case["scores"][metric][spared])
        assert np.array_equal(logits[spared], case["logits"][spared]) and np.isfinite(logits).all()
    eng.feed_status()   # read and cleared
    # each kind alone raises too
    for ptr, idx, held in ((tr_ptr, case["train"].indices.astype(np.int32), False), (case["held"].indptr.astype(np.int64), he_idx, True)):
        kw = dict(held_dev=dev(ptr, idx)) if held else dict(train_dev=dev(ptr, idx))
        _run(eng, case, 0, with_logits=False, **kw)
        with pytest.raises(SdrmError):
            eng.feed_status()
    # a train indptr pair that is ordered but ends behind the index array (train_nnz): the gather reads nothing of it and the ranking
    # masks nothing - the user is one without train entries in both, and everybody else is spared
    d = n - 1
    tr_ptr = case["train"].indptr.astype(np.int64).copy()
    assert tr_ptr[d + 1] - tr_ptr[d] >= 1 and tr_ptr[d + 1] == case["train"].nnz
    emptied = csr_matrix((case["train"].data[:tr_ptr[d]], case["train"].indices[:tr_ptr[d]], np.append(tr_ptr[:d + 1], tr_ptr[d])), shape=(n, items))
    tr_ptr[d + 1] += 3
    spared = np.arange(d)
    for metric in (0, 1):
        got, logits, intact = _run(eng, case, metric, train_dev=dev(tr_ptr, case["train"].indices.astype(np.int32)))
        with pytest.raises(SdrmError) as err:
            eng.feed_status()
        assert "indptr pair" in str(err.value) and "column index" not in str(err.value)
        assert intact
        assert _same_bits(got[spared], case["scores"][metric][spared]) and np.array_equal(logits[spared], case["logits"][spared])
        want = case["s64"][EMPTY[0]]   # the float64 logits of a user without train entries
        assert np.linalg.norm(logits[d] - want) / np.linalg.norm(want) <= TOL
        assert _same_bits(got, orc.rank_metrics(logits, case["held"], train=emptied, ks=(K,))[metric][0])
    eng.feed_status()


def _pre_stage(where, monkeypatch, **kw):
    """The pre-stage of tests/test_vae_adam.py - 40 users x 60 items, batch 16, two epochs, its seeds, the six flags - plus `kw`: the
    model, every step's loss as the engine wrote it, and every epoch's mean metric."""
    from sdrm_amd import vae_hooks
    from sdrm_amd.engine import Engine
    m = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)
    losses, means = [], []
    orig_slot, orig_eval = Engine.vae_loss_slot, vae_hooks.evaluate_holdout

    def loss_slot(self, neg_ll, kl, anneal, out, slot, **k):
        orig_slot(self, neg_ll, kl, anneal, out, slot, **k)
        losses.append(out[slot].clone())

    def evaluate(*a, **k):
        scores = orig_eval(*a, **k)
        means.append(scores.clone())
        return scores

    with monkeypatch.context() as mp:
        mp.setattr(Engine, "vae_loss_slot", loss_slot)
        mp.setattr(vae_hooks, "evaluate_holdout", evaluate)
        torch.manual_seed(21)
        np.random.seed(22)
        vae = vae_hooks.VAE(60, 16, 8).cuda()
        vae_hooks.train_variational_autoencoder(vae, m, m, 2, 16, 1e-3, "Recall@10", str(where), device_feed=True, sparse_input=True,
                                                device_holdout=True, device_latent=True, device_decoder=True, device_optimizer=True, **kw)
    return vae, torch.stack(losses).cpu().numpy(), [float(np.nanmean(s.cpu().numpy())) for s in means]


def _forbid_torch_forward(mp):
    """`nn.Linear.forward`, `VAE.forward`, `VAE.encode` and `Engine.csr_rows_to_dense` raise: neither half may call them."""
    from sdrm_amd import vae_hooks
    from sdrm_amd.engine import Engine

    def forbidden(what):
        def raiser(*args, **kw):
            raise AssertionError(f"{what} called in a pre-stage with device_eval")
        return raiser

    mp.setattr(torch.nn.Linear, "forward", forbidden("nn.Linear.forward"))
    mp.setattr(vae_hooks.VAE, "forward", forbidden("VAE.forward"))
    mp.setattr(vae_hooks.VAE, "encode", forbidden("VAE.encode"))
    mp.setattr(Engine, "csr_rows_to_dense", forbidden("Engine.csr_rows_to_dense"))


@pytest.mark.gpu
def test_pre_stage_without_a_torch_linear_in_either_half(tmp_path, monkeypatch):
    from sdrm_amd.engine import Engine, utility_engine
    a, loss_a, mean_a = _pre_stage(tmp_path / "a", monkeypatch)
    calls = []
    orig = Engine.vae_eval_holdout
    with monkeypatch.context() as mp:
        _forbid_torch_forward(mp)
        mp.setattr(Engine, "vae_eval_holdout", lambda *args, **kw: (calls.append(1), orig(*args, **kw))[1])
        b, loss_b, mean_b = _pre_stage(tmp_path / "b", monkeypatch, device_eval=True)
    utility_engine().feed_status()
    print("losses without / with device_eval:", loss_a, loss_b, "epoch means:", mean_a, mean_b)
    assert len(calls) == 2 and loss_a.size == loss_b.size == 6
    assert loss_a.tobytes() == loss_b.tobytes()                       # the evaluation half does not feed the train half
    assert len(mean_b) == 2 and np.isfinite(mean_b).all() and np.isfinite(mean_a).all()
    assert b.model_is_trained and b.is_training == 0
    final = {name: p.cpu() for name, p in b.state_dict().items()}
    saved = [torch.load(path, map_location="cpu") for path in sorted(glob.glob(str(tmp_path / "b" / "epoch-*.pth")))]
    assert 1 <= len(saved) <= 2
    assert any(all(torch.equal(final[name], sd[name]) for name in final) for sd in saved)


@pytest.mark.gpu
def test_train_SDRM_with_vae_device_eval(tmp_path, monkeypatch):
    import sdrm_amd.train_SDRM as ts
    from sdrm_amd.engine import Engine, utility_engine
    from test_reference_surface import make_feed
    data = synth.synth_feed_csr(40, 60, 0.2, seed=72, ratings=False)
    dl = make_feed(data, 16)
    calls = []
    orig_eval, orig_pre = Engine.vae_eval_holdout, ts.train_variational_autoencoder

    def pre_stage(*args, **kw):   # the torch forward is forbidden for the whole pre-stage (the eps-net's stage encodes with the module)
        with monkeypatch.context() as mp:
            _forbid_torch_forward(mp)
            return orig_pre(*args, **kw)

    monkeypatch.setattr(ts, "train_variational_autoencoder", pre_stage)
    monkeypatch.setattr(Engine, "vae_eval_holdout", lambda *args, **kw: (calls.append(1), orig_eval(*args, **kw))[1])
    torch.manual_seed(31)
    np.random.seed(32)
    DIFF, vae = ts.train_SDRM(dl, 60, 16, 8, 16, 1e-3, 8, 1, 1e-3, 1, 5, 1.0, str(tmp_path), data, data, "Recall@10", vae_device_feed=True,
                              vae_device_holdout=True, vae_sparse_input=True, vae_device_latent=True, vae_device_decoder=True,
                              vae_device_optimizer=True, vae_device_eval=True)
    utility_engine().feed_status()
    assert vae.model_is_trained and vae.is_training == 0 and len(calls) >= 1
    assert all(bool(torch.isfinite(p).all()) for p in vae.state_dict().values())
    assert np.isfinite(float(DIFF.last_loss.cpu()))
