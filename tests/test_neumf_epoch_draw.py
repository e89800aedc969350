"""The NeuMF evaluator's epoch draw on the device (csrc/neumf_draw.h; sdrm_neumf_epoch_draw; `Engine.neumf_epoch_draw`;
`neumf.compute_neuralcf_results(device_draw=True)`) against its numpy restatement tests/neumf_draw_ref.py: integer work, so every
comparison is exact.  Sizes: one lane, around a wave, around a work-group, many work-groups inside one chunk of `k_draw_scan` (70001 rows:
219 of a chunk's 2048), both parities of the bit length - and one case of 700000 part rows, 2735 work-groups, where the scan's carry
runs from its first chunk into a second one with 420 k label-0 rows placed by it (the path of the ML-1M shape; the fault could show at
no smaller size: a chunk is 2048 work-groups = 524288 rows).  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import neumf_draw_ref as ref
import stream_harness as sh
from test_neumf_train import toy
from sdrm_amd import neumf
from sdrm_amd.engine import Engine, SdrmError

SHAPE, ARG = -2, -1
N_USERS, N_ITEMS = 50, 300
SEED, EPOCH = 11, 3
SENTINEL = -77
SIZES = (2, 3, 7, 255, 256, 257, 4097, 70001)
PATTERNS = ("ones", "zeros", "single-zero", "label-2")


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def default_hold(n):
    return int(math.ceil(0.2 * n))


_TRIPLES, _REF = {}, {}


def triples(n, pattern="mixed"):
    if (n, pattern) not in _TRIPLES:
        rng = np.random.default_rng(1000 + n)
        label = (rng.random(n) < 0.4).astype(np.int64)
        if pattern == "ones":
            label[:] = 1
        elif pattern == "zeros":
            label[:] = 0
        elif pattern == "single-zero":
            label[:] = 1
            label[n // 3] = 0
        elif pattern == "label-2":
            label[n // 2] = 2
        t = np.stack([rng.integers(0, N_USERS, n), rng.integers(0, N_ITEMS, n), label], axis=1).astype(np.int32)
        t.setflags(write=False)
        _TRIPLES[(n, pattern)] = t
    return _TRIPLES[(n, pattern)]


def restated(n, pattern, n_hold, seed=SEED, epoch=EPOCH):
    """The restatement's (hold, out, counts, present), computed once per case and shared."""
    key = (n, pattern, n_hold, seed, epoch)
    if key not in _REF:
        _REF[key] = ref.epoch_draw(triples(n, pattern), n_hold, seed=seed, epoch=epoch, n_users=N_USERS)
    return _REF[key]


def sentinel_bufs(engine, n, n_hold):
    return (torch.full((n_hold, 3), SENTINEL, dtype=torch.int32, device=engine.device),
            torch.full((2 * (n - n_hold), 3), SENTINEL, dtype=torch.int32, device=engine.device))


def check_against(engine, t_dev, want, n_hold, seed=SEED, epoch=EPOCH):
    n = t_dev.shape[0]
    bufs = sentinel_bufs(engine, n, n_hold)
    hold, part, counts, present = engine.neumf_epoch_draw(t_dev, n_hold, seed=seed, epoch=epoch, n_users=N_USERS, out=bufs)
    w_hold, w_out, w_counts, w_present = want
    print("n", n, "n_hold", n_hold, "counts", counts, "restated", w_counts)
    assert counts == w_counts and part.shape == (w_counts[2], 3) and hold.data_ptr() == bufs[0].data_ptr() and part.data_ptr() == bufs[1].data_ptr()
    assert np.array_equal(hold.cpu().numpy(), w_hold)
    assert np.array_equal(part.cpu().numpy(), w_out)
    assert np.array_equal(present.cpu().numpy(), w_present)
    assert bool((bufs[1][counts[2]:] == SENTINEL).all())          # rows behind m are left as they were
    return hold, part, counts, present


TWO_CHUNKS = 700001     # n_hold = 1: 700000 part rows > 524288, the rows of one chunk of k_draw_scan (256 x DRAW_SCAN_PER work-groups of 256)
_CASES = ([(n, "mixed", h) for n in SIZES for h in sorted({default_hold(n), 1, n - 1})] + [(n, p, default_hold(n)) for n in (257, 70001) for p in PATTERNS]
          + [(TWO_CHUNKS, "mixed", 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("n, pattern, n_hold", _CASES, ids=[f"{n}-{p}-hold{h}" for n, p, h in _CASES])
def test_draw_is_the_restatement(engine, n, pattern, n_hold):
    t_dev = torch.from_numpy(triples(n, pattern).copy()).to(engine.device)
    _, _, counts, _ = check_against(engine, t_dev, restated(n, pattern, n_hold), n_hold)
    assert np.array_equal(t_dev.cpu().numpy(), triples(n, pattern))                      # the triples are left as they are
    if n == TWO_CHUNKS:
        assert n - n_hold > 256 * 8 * 256 and counts[1] > 300000 and counts[0] > 200000  # two chunks, and negatives drawn from both
    engine.feed_status()


@pytest.mark.gpu
def test_default_n_hold_and_no_present(engine):
    n = 257
    t_dev = torch.from_numpy(triples(n).copy()).to(engine.device)
    hold, part, counts, present = engine.neumf_epoch_draw(t_dev, seed=SEED, epoch=EPOCH)
    want = restated(n, "mixed", default_hold(n))
    assert present is None and counts == want[2] and np.array_equal(hold.cpu().numpy(), want[0]) and np.array_equal(part.cpu().numpy(), want[1])
    assert part._base is not None and part._base.shape == (2 * (n - default_hold(n)), 3)


@pytest.mark.gpu
def test_same_bits_twice_and_another_epoch_differs(engine):
    n, n_hold = 4097, default_hold(4097)
    t_dev = torch.from_numpy(triples(n).copy()).to(engine.device)
    a = engine.neumf_epoch_draw(t_dev, n_hold, seed=SEED, epoch=EPOCH, n_users=N_USERS)
    b = engine.neumf_epoch_draw(t_dev, n_hold, seed=SEED, epoch=EPOCH, n_users=N_USERS)
    c = engine.neumf_epoch_draw(t_dev, n_hold, seed=SEED, epoch=EPOCH + 1, n_users=N_USERS)
    d = engine.neumf_epoch_draw(t_dev, n_hold, seed=SEED + 1, epoch=EPOCH, n_users=N_USERS)
    assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for other in (c, d):
        assert not torch.equal(a[0], other[0]) and (a[1].shape != other[1].shape or not torch.equal(a[1], other[1]))


@pytest.mark.gpu
def test_out_reuse_shows_no_stale_row(engine):
    """One pair of buffers across calls whose m shrinks and grows again: mixed labels (m = n_part + n_pos), all ones (m = n_part), mixed."""
    n, n_hold = 257, default_hold(257)
    bufs = sentinel_bufs(engine, n, n_hold)
    ms = []
    for pattern, epoch in (("mixed", EPOCH), ("ones", EPOCH), ("mixed", EPOCH + 1)):
        t_dev = torch.from_numpy(triples(n, pattern).copy()).to(engine.device)
        hold, part, counts, _ = engine.neumf_epoch_draw(t_dev, n_hold, seed=SEED, epoch=epoch, n_users=N_USERS, out=bufs)
        want = restated(n, pattern, n_hold, epoch=epoch)
        assert counts == want[2] and part.shape[0] == counts[2]
        assert np.array_equal(hold.cpu().numpy(), want[0]) and np.array_equal(part.cpu().numpy(), want[1])
        ms.append(counts[2])
    assert ms[1] == n - n_hold < ms[0] and ms[2] > ms[1]


@pytest.mark.gpu
def test_bad_user_ids_in_hold(engine):
    n, n_hold = 257, default_hold(257)
    p0 = ref.perm(n, SEED, EPOCH, 0)
    t = triples(n).copy()
    t[p0[0], 0], t[p0[n_hold - 1], 0] = -1, N_USERS               # both land in hold: its first and its last row
    want = ref.epoch_draw(t, n_hold, seed=SEED, epoch=EPOCH, n_users=N_USERS)
    assert want[0][0, 0] == -1 and want[0][-1, 0] == N_USERS
    engine.feed_status()
    t_dev = torch.from_numpy(t).to(engine.device)
    hold, part, counts, present = engine.neumf_epoch_draw(t_dev, n_hold, seed=SEED, epoch=EPOCH, n_users=N_USERS)
    with pytest.raises(SdrmError, match="row id outside"):
        engine.feed_status()
    assert np.array_equal(hold.cpu().numpy(), want[0]) and np.array_equal(part.cpu().numpy(), want[1]) and counts == want[2]   # copied verbatim
    assert np.array_equal(present.cpu().numpy(), want[3])
    engine.feed_status()                                          # (reading the word cleared it)
    check_against(engine, torch.from_numpy(triples(n).copy()).to(engine.device), restated(n, "mixed", n_hold), n_hold)
    engine.feed_status()


@pytest.mark.gpu
def test_refusals_write_nothing(engine):
    n, n_hold = 257, default_hold(257)
    t_dev = torch.from_numpy(triples(n).copy()).to(engine.device)
    hold, buf = sentinel_bufs(engine, n, n_hold)
    present = torch.full((N_USERS,), 200, dtype=torch.uint8, device=engine.device)
    counts = (C.c_int64 * 3)(-5, -5, -5)

    def raw(triples=t_dev, n=n, n_hold=n_hold, hold=hold, out=buf, capacity=None, present=present, n_users=N_USERS, counts=counts, handle=True):
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
        return engine.lib.sdrm_neumf_epoch_draw(engine._h if handle else None, ptr(triples), n, n_hold, SEED, EPOCH, ptr(hold), ptr(out),
                                                buf.shape[0] if capacity is None else capacity, ptr(present), n_users, counts)

    def untouched():
        torch.cuda.synchronize()
        return bool((hold == SENTINEL).all()) and bool((buf == SENTINEL).all()) and bool((present == 200).all()) and list(counts) == [-5, -5, -5]

    for kw in (dict(n=1, n_hold=1), dict(n=1, n_hold=0), dict(n_hold=0), dict(n_hold=n), dict(capacity=2 * (n - n_hold) - 1), dict(n=2 ** 30 + 1),
               dict(n_users=0)):
        assert raw(**kw) == SHAPE and untouched(), kw
    for kw in (dict(triples=None), dict(hold=None), dict(out=None), dict(counts=None), dict(handle=False)):
        assert raw(**kw) == ARG and untouched(), kw
    # the Python surface
    wide = torch.zeros(n, 4, dtype=torch.int32, device=engine.device)
    for bad, text in ((t_dev.to(torch.int64), "contiguous int32"), (t_dev.cpu(), "engine's device"), (wide[:, :3], "contiguous"), (t_dev[:1], "SDRM_ERR_SHAPE"),
                      (t_dev.reshape(-1), "contiguous int32")):
        with pytest.raises(SdrmError, match=text):
            engine.neumf_epoch_draw(bad, seed=SEED, epoch=EPOCH, n_users=N_USERS, out=(hold, buf))
    for kw, text in ((dict(n_hold=0), "SDRM_ERR_SHAPE"), (dict(n_hold=n), "SDRM_ERR_SHAPE"), (dict(n_users=0), "SDRM_ERR_SHAPE"),
                     (dict(out=(hold, buf[:-1])), r"out\[1\]"), (dict(out=(hold[:-1], buf)), r"out\[0\]"), (dict(out=(hold, buf.to(torch.int64))), r"out\[1\]")):
        with pytest.raises(SdrmError, match=text):
            engine.neumf_epoch_draw(t_dev, **{**dict(n_hold=n_hold, seed=SEED, epoch=EPOCH, n_users=N_USERS, out=(hold, buf)), **kw})
    assert untouched()
    assert raw(present=None, n_users=0) == 0 and not untouched()                                    # ... and the accepted call does write
    want = restated(n, "mixed", n_hold)
    assert tuple(counts) == want[2] and np.array_equal(hold.cpu().numpy(), want[0]) and bool((present == 200).all())


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["late", "busy"])
def test_draw_waits_for_queued_work(engine, variant):
    """sdrm_neumf_epoch_draw takes no stream and is device-synchronous (include/sdrm_hip.h): the real triples are copied into its input
    on a non-blocking side stream behind a delay, not yet there when the host makes the call - and the call, made without waiting,
    still draws from them.  "busy": the default stream is asleep as well."""
    n, n_hold = 4097, default_hold(4097)
    real = torch.from_numpy(triples(n).copy()).to(engine.device)
    buf = torch.zeros(n, 3, dtype=torch.int32, device=engine.device)       # (in-range triples, whatever the call would read too early)
    sh.cycles_per_ms()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    if variant == "busy":
        sh.sleep_ms(1.5 * sh.MIN_DELAY_MS)
    with torch.cuda.stream(s):
        sh.sleep_ms(sh.MIN_DELAY_MS)
        buf.copy_(real, non_blocking=True)
        late = torch.cuda.Event()
        late.record(s)
    assert not late.query(), "the queued copy waited on the host"
    bufs = sentinel_bufs(engine, n, n_hold)
    got = engine.neumf_epoch_draw(buf, n_hold, seed=SEED, epoch=EPOCH, n_users=N_USERS, out=bufs)
    assert late.query(), "sdrm_neumf_epoch_draw returned while work was still queued on the device"
    want = restated(n, "mixed", n_hold)
    assert got[2] == want[2] and np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(got[3].cpu().numpy(), want[3])
    s.synchronize()


def replay(engine, training, validation, seed, epochs, eval_recall, device_draw):
    """The driver's epochs made by hand: the restatement's draws (or, for the host-draw path, numpy's as the driver orders them), a second
    model of the same seed, `neumf_train_steps` and `validation_loss` called as the driver calls them, the ranking WITHOUT the cache."""
    dev = engine.device
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = neumf.NCF(40, 90, factor=8, layers=3, dropout=0.5).to(dev)
    live = model.engine_weights()
    m, v = [torch.zeros_like(t) for t in live], [torch.zeros_like(t) for t in live]
    n_hold = int(math.ceil(0.2 * training.shape[0]))
    out = dict(train_loss=[], valid_loss=[], recall10=[], draw_counts=[], after=[])
    step0 = 0
    for epoch in range(epochs):
        if device_draw:
            hold, part, counts, present = ref.epoch_draw(training.astype(np.int32), n_hold, seed=seed, epoch=epoch, n_users=40)
            out["draw_counts"].append(counts)
            hold_arg, users = torch.from_numpy(hold).to(dev), np.flatnonzero(present)
        else:
            perm = rng.permutation(training.shape[0])
            hold, part = training[perm[:n_hold]], training[perm[n_hold:]]
            negatives = part[part[:, 2] == 0]
            part = np.concatenate([part, negatives[rng.integers(0, negatives.shape[0], size=int((part[:, 2] == 1).sum()))]])
            part = part[rng.permutation(part.shape[0])]
            hold_arg, users = hold, hold[:, 0]
        losses = engine.neumf_train_steps(live, m, v, torch.from_numpy(np.ascontiguousarray(part, dtype=np.int32)).to(dev), 256, step0, lr=1e-3, p_drop=0.5,
                                          seed=seed, call_id=epoch, check=False)
        step0 += int(losses.numel())
        out["train_loss"].extend(losses.cpu().tolist())
        out["valid_loss"].append(neumf.validation_loss(model, hold_arg, engine))
        if eval_recall:
            rec, _ = neumf.rank_all_items(model, training, validation, users, engine)
            out["recall10"].append(float(np.nanmean(rec[neumf.K_LIST.index(10)])))
        out["after"].append({k: t.clone() for k, t in model.state_dict().items()})
    if eval_recall:
        best = 0 if out["recall10"][0] > 0 else epochs - 1
    else:
        best = int(np.argmin(out["valid_loss"]))
    model.load_state_dict(out["after"][best])
    out["best_epoch"] = best
    out["per_user"] = neumf.rank_all_items(model, training, validation, validation[:, 0], engine)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("eval_recall", [False, True])
@pytest.mark.parametrize("device_draw", [True, False])
def test_driver_replay(engine, eval_recall, device_draw):
    """`compute_neuralcf_results(device_train=True, device_draw=...)` on the toy against the epochs made by hand, bit for bit (the header
    promises the same bits on every run for the same array).  device_draw=False: the parent's host draws, and a ranking without the
    cached problem - the cache moves no number."""
    training, validation = toy()
    seed, epochs = 2, 2
    h = {}
    got = neumf.compute_neuralcf_results(training, validation, 40, 90, engine=engine, seed=seed, epochs=epochs, eval_recall=eval_recall, history=h,
                                         device_train=True, device_draw=device_draw)
    want = replay(engine, training, validation, seed, epochs, eval_recall, device_draw)
    print("train loss", h["train_loss"][:2], "valid", h["valid_loss"], "recall10", h["recall10"], "counts", h.get("draw_counts"))
    assert h["epochs_run"] == epochs and h["train_loss"] == want["train_loss"] and h["valid_loss"] == want["valid_loss"]
    assert np.array_equal(np.asarray(h["recall10"]), np.asarray(want["recall10"]), equal_nan=True)
    assert h["best_epoch"] == want["best_epoch"]
    if device_draw:
        n_part = training.shape[0] - int(math.ceil(0.2 * training.shape[0]))
        assert h["draw_counts"] == want["draw_counts"] and all(c[2] == n_part + c[0] for c in h["draw_counts"])
    else:
        assert "draw_counts" not in h
    for a, b in zip(h["per_user"], want["per_user"]):
        assert np.array_equal(a, b, equal_nan=True)
    with np.errstate(invalid="ignore"):
        for a, b in zip(got, want["per_user"]):
            assert np.array_equal(a, np.array([np.round(np.nanmean(b[q]), 4) for q in range(6)]), equal_nan=True)
