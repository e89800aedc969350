"""Stream-order harness: one engine call on a busy, non-blocking side stream, with inputs that arrive late and outputs that start
poisoned (tests/test_stream_order.py drives it; the case table at the bottom is what its coverage test reads).

include/sdrm_hip.h promises that every entry point enqueues all its work on the caller's `stream` and does not synchronise unless it
says so.  Every other GPU test calls on the default stream and reads back with `.cpu()`, so a launch on the wrong stream, a chain
that forks too early or is not joined, or a hidden host wait cannot show there.  Here, per case (`run_case`):

  1. every device input and output of the call exists up front, while the device is idle: float inputs and outputs hold NaN,
     integer inputs hold ZEROS (an in-range value everywhere: empty rows, column 0, id 0, t = 0), so a call that runs ahead of its
     inputs computes a wrong number and never an out-of-range address.  The outputs a wrapper makes itself with `torch.empty` are
     caught too: the twin's run records their shapes, and the side-stream run hands out pre-poisoned tensors in the same order;
  2. on the side stream `s` a delay (`torch.cuda._sleep`) is queued, then the copies that write the real inputs, then an event `late`;
  3. the call is made under `torch.cuda.stream(s)`;
  4. every C entry point the call reaches is observed as it returns (`_LibSpy`): `late.query()` must still be false for those the
     header says do not synchronise (`Case.nosync`), and true for those it says do (`Case.syncs`).  The delay is 20 x the call's own
     warm host time (at least 20 ms, at most 200 ms); a case that meets the cap and still finds `late` done fails - it would be vacuous;
  5. still on `s`, every output is copied into a fresh tensor; then `s.synchronize()` and nothing else, and the copies are compared;
  6. the "busy" variant also keeps the default stream asleep for 1.5 x as long, so work that landed there by mistake ends late.

The result is compared with the twin: the same call on a fresh engine on the default stream, everything synchronised - bit for bit
wherever the header or an existing test promises the same bits on every call, and through `Case.anchor` (the family's own reference at
the family's own bar, no new tolerance) for the twin and for everything that has no such promise.

The range check of the CSR entry points (`check=True` of the wrappers, one `sdrm_feed_status`) synchronises the stream by contract, so
the cases pass check=False and the harness makes the same check itself, once the call's return has been observed: `Case.feed`.  Every
case is therefore still range-checked, one call later than the wrapper would.

What the poisoning does not reach: an output a wrapper makes with `torch.zeros` (the loss sum of neumf_pair_logits, nmf_fit's violation
tail: the C contract wants them zero on entry) starts as zeros, not NaN; `_TorchProxy` replaces `empty` and `empty_like` only.

Pool states (utility families): "warm" - the same call ran before on this engine, nothing grows, the no-wait assertion holds;
"cold" - the side-stream call is the engine's first of that family, so the zeroing of new scratch and the first launch meet on
different streams (result only: a growing call may synchronise); "regrow" - b = 33 on the default stream, then b = 300 on `s`."""
from __future__ import annotations

import contextlib
import dataclasses
import os
import re
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "sdrm_hip.h")

MIN_DELAY_MS, MAX_DELAY_MS, HOST_FACTOR = 20.0, 200.0, 20.0

# Entry points whose header text says they synchronise `stream` (or the device): sdrm_feed_status ("Synchronises `stream`"),
# sdrm_equal_sparsity_csr_begin ("synchronises `stream` ONCE"), sdrm_svd_fit ("The call synchronises `stream`"), sdrm_profile_end
# ("synchronises the stream").  sdrm_sample / sdrm_sample_begin wait only for a caller's Tj (EXPLICIT mode, multi-resolution).
SYNCHRONISING = ("sdrm_feed_status", "sdrm_equal_sparsity_csr_begin", "sdrm_svd_fit", "sdrm_profile_end")


def header_stream_entry_points(path=HEADER):
    """Names of the prototypes of include/sdrm_hip.h that take a `void* stream`, in header order."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    names = []
    for m in re.finditer(r"\b(sdrm_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"void\s*\*\s*stream\b", m.group(2)):
            names.append(m.group(1))
    return names


# ------------------------------------------------------------------------------------------------ the delay
_RATE = {}
OBSERVED = {}     # entry point -> {"pending" / "arrived": warm returns that found the stream's work pending / done, "host_ms": longest warm host time}
STATS = {"cycles_per_ms": None, "max_host_ms": 0.0, "max_host_case": None, "capped": []}


def cycles_per_ms():
    """`torch.cuda._sleep` cycles per millisecond, measured once per process with two events around one sleep."""
    if "rate" not in _RATE:
        torch.cuda.synchronize()
        torch.cuda._sleep(1_000_000)   # (the first launch loads the kernel)
        rates = []
        for cycles in (20_000_000, 40_000_000):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            torch.cuda.synchronize()
            rates.append(cycles / a.elapsed_time(b))
        _RATE["rate"] = min(rates)
        STATS["cycles_per_ms"] = _RATE["rate"]
    return _RATE["rate"]


def sleep_ms(ms):
    torch.cuda._sleep(int(ms * cycles_per_ms()))


# ------------------------------------------------------------------------------------------------ spies
class _LibSpy:
    """Stands in for `engine.lib`: every sdrm_* call is made as it is, and `late.query()` is noted the moment it returns."""

    def __init__(self, lib, late, log):
        self.__dict__.update(_lib=lib, _late=late, _log=log)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("sdrm_") or name.startswith("sdrm_debug") or name in ("sdrm_last_error", "sdrm_sample_remaining"):
            return fn

        def spied(*args):
            rc = fn(*args)
            self._log.append((name, not self._late.query()))
            return rc
        return spied


class _Alloc:
    """`torch.empty` / `torch.empty_like` of the wrappers (and `alloc` of a case): "record" notes shape and dtype of every output the
    call makes, "replay" hands out the tensors poisoned beforehand in the same order."""

    def __init__(self, device, record=None, prepared=None):
        self.device, self.record, self.prepared, self.i = device, record, prepared, 0
        self.delay_again = lambda: None   # (side-stream run: a new delay on the stream, behind a call that had to wait for the first)

    def __call__(self, *shape, dtype=torch.float32, device=None, **_):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        shape = tuple(int(v) for v in shape)
        if self.prepared is None:
            if self.record is not None:
                self.record.append((shape, dtype))
            # (poisoned like the side-stream run's: what a call leaves untouched - the tail of an index array - is then the same)
            return torch.full(shape, float("nan"), dtype=dtype, device=self.device) if dtype.is_floating_point else torch.zeros(shape, dtype=dtype, device=self.device)
        assert self.i < len(self.prepared), "the side-stream call allocates more outputs than its twin did"
        t = self.prepared[self.i]
        self.i += 1
        assert tuple(t.shape) == shape and t.dtype == dtype, f"output {self.i - 1}: the twin made {tuple(t.shape)} {t.dtype}, this call {shape} {dtype}"
        return t


class _TorchProxy:
    """`torch` as sdrm_amd/engine.py sees it while a case runs: only `empty` and `empty_like` are replaced."""

    def __init__(self, alloc):
        self._alloc = alloc

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, **kw):
        return self._alloc(*shape, **kw)

    def empty_like(self, t, **kw):
        return self._alloc(tuple(t.shape), dtype=kw.get("dtype", t.dtype))


@contextlib.contextmanager
def _allocating(alloc):
    from sdrm_amd import engine as engine_mod
    saved = engine_mod.torch
    engine_mod.torch = _TorchProxy(alloc)
    try:
        yield
    finally:
        engine_mod.torch = saved


def poison_like(t):
    """NaN for floating point, zero for every integer type (zeros are in range wherever an index, an id or a timestep is read)."""
    return torch.full_like(t, float("nan")) if t.is_floating_point() else torch.zeros_like(t)


def flatten(x, out=None):
    """The tensors of a nested result, in order; None and host values are skipped."""
    out = [] if out is None else out
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, (tuple, list)):
        for y in x:
            flatten(y, out)
    elif isinstance(x, dict):
        for y in x.values():
            flatten(y, out)
    return out


def flatten_any(x, out=None):
    """Tensors and host arrays / numbers of a nested result, in order (the Python-layer tests compare both)."""
    out = [] if out is None else out
    if isinstance(x, (tuple, list)):
        for y in x:
            flatten_any(y, out)
    elif x is not None:
        out.append(x)
    return out


def host_values(x, out=None):
    """Everything of a nested result that is not a tensor (counts, shapes, numpy arrays read back by a synchronising call)."""
    out = [] if out is None else out
    if isinstance(x, (tuple, list)):
        for y in x:
            host_values(y, out)
    elif isinstance(x, dict):
        for y in x.values():
            host_values(y, out)
    elif isinstance(x, np.ndarray):
        out.append(x.tobytes())
    elif x is not None and not isinstance(x, torch.Tensor):
        out.append(repr(x))
    return out


# ------------------------------------------------------------------------------------------------ a case
@dataclasses.dataclass
class Case:
    name: str
    covers: tuple                 # C entry points the call reaches (checked against what the spy saw)
    make: object                  # (device) -> {name: staging tensor on the device}: the real inputs
    engine: object                # (engine_cls) -> a fresh engine
    call: object                  # (e, bufs, alloc) -> nested result; idempotent: it sets whatever engine state it depends on
    nosync: tuple = ()            # of `covers`: must return with the inputs pending (warm pool only)
    syncs: tuple = ()             # of `covers`: documented to wait - must return with the inputs there
    anchor: object = None         # (staging on the host, result on the host) -> asserts against the family's reference at its bar
    bitwise: bool = True          # the side-stream result equals the twin's to the bits (else: `anchor` judges it too)
    twin_call: object = None      # the twin's own call where the reference order differs from the side-stream call's (same result shape)
    feed: bool = False            # ask sdrm_feed_status after the call (the wrappers' check=True, made once its return was observed)
    pools: tuple = ("warm",)      # utility families: ("warm", "cold")
    prepare: object = None        # (e, staging) for pool "regrow": the smaller call made first on the default stream


def _to_host(tensors):
    return [t.detach().cpu() for t in tensors]


def _invoke(case, e, bufs, alloc, twin=False):
    with _allocating(alloc):
        out = (case.twin_call if twin and case.twin_call is not None else case.call)(e, bufs, alloc)
    return out


def run_twin(case, engine_cls, staging):
    """The call on a fresh engine on the default stream, everything synchronised.  Returns (tensors on the host, host values, the
    shapes of what it allocated, its warm host time in ms)."""
    e = case.engine(engine_cls)
    try:
        record = []
        bufs = {k: v.clone() for k, v in staging.items()}
        torch.cuda.synchronize()
        out = _invoke(case, e, bufs, _Alloc(e.device, record=record), twin=True)
        if case.feed:
            e.feed_status()
        torch.cuda.synchronize()
        result = (_to_host(flatten(out)), host_values(out), record)
        # the same call once more, warm, for its host time (the calls are idempotent)
        bufs = {k: v.clone() for k, v in staging.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _invoke(case, e, bufs, _Alloc(e.device))
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if case.feed:
            e.feed_status()
        return result + (host_ms,)
    finally:
        e.close()


def run_case(case, engine_cls, pool="warm", variant="late"):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    device = torch.device("cuda", torch.cuda.current_device())
    staging = case.make(device)
    twin, twin_host, shapes, host_ms = run_twin(case, engine_cls, staging)
    host_staging = {k: v.cpu() for k, v in staging.items()}
    if case.anchor is not None:
        case.anchor(host_staging, twin)

    e = case.engine(engine_cls)
    try:
        if pool == "warm":
            for _ in range(2):   # the second one is timed: nothing grows any more
                bufs = {k: v.clone() for k, v in staging.items()}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _invoke(case, e, bufs, _Alloc(device))
                host_ms = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                if case.feed:
                    e.feed_status()
        elif pool == "regrow":
            case.prepare(e, staging)
            torch.cuda.synchronize()
        delay_ms = min(MAX_DELAY_MS, max(MIN_DELAY_MS, HOST_FACTOR * host_ms))
        capped = HOST_FACTOR * host_ms > MAX_DELAY_MS
        if host_ms > STATS["max_host_ms"]:
            STATS["max_host_ms"], STATS["max_host_case"] = host_ms, case.name
        if capped:
            STATS["capped"].append(case.name)

        # 1. everything exists and is poisoned while the device is idle
        bufs = {k: poison_like(v) for k, v in staging.items()}
        prepared = [torch.full(shape, float("nan"), dtype=dtype, device=device) if dtype.is_floating_point
                    else torch.zeros(shape, dtype=dtype, device=device) for shape, dtype in shapes]
        cycles_per_ms()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        log = []
        if variant == "busy":
            sleep_ms(1.5 * delay_ms)                      # 6. the default stream is busy for longer than `s`
        with torch.cuda.stream(s):
            sleep_ms(delay_ms)                            # 2. the delay, then the inputs
            for k, v in staging.items():
                bufs[k].copy_(v, non_blocking=True)
            late = torch.cuda.Event()
            late.record(s)
            lib = e.lib
            e.lib = spy = _LibSpy(lib, late, log)
            alloc = _Alloc(device, prepared=prepared)

            def delay_again():
                sleep_ms(delay_ms)
                ev = torch.cuda.Event()
                ev.record(s)
                spy.__dict__["_late"] = ev
                log.append(("delay_again", True))
            alloc.delay_again = delay_again
            try:
                out = _invoke(case, e, bufs, alloc)   # 3. the call
            finally:
                e.lib = lib
            if case.feed:
                e.feed_status()
            got = [t.clone() for t in flatten(out)]       # 5. consumed on `s`
            got_host = host_values(out)
        s.synchronize()
        result = _to_host(got)
        torch.cuda.synchronize()
    finally:
        e.close()

    # 4. what the spy saw
    seen = {}
    waited = False   # a documented wait has returned: what follows it in this case cannot find the inputs pending
    for name, pending in log:
        if name == "delay_again":
            waited = False
            continue
        seen.setdefault(name, []).append(pending)
        if pool == "warm" and not waited:   # (behind a documented wait of the same case a return says nothing)
            rec = OBSERVED.setdefault(name, {"pending": 0, "arrived": 0, "host_ms": 0.0})
            rec["pending" if pending else "arrived"] += 1
            rec["host_ms"] = max(rec["host_ms"], host_ms)
        if name in case.syncs:
            waited = True
    missing = [n for n in case.covers if n not in seen and n != "sdrm_feed_status"]
    assert not missing, f"{case.name}: the call never reached {missing}"
    if pool == "warm":
        for name in case.nosync:
            if not all(seen[name]):
                if capped:
                    raise AssertionError(f"{case.name}: {name} returned after its inputs had arrived, and the call's warm host time "
                                         f"({host_ms:.1f} ms) x {HOST_FACTOR:.0f} exceeds the {MAX_DELAY_MS:.0f} ms cap of the delay: the case "
                                         f"cannot tell a wait from a slow call")
                raise AssertionError(f"{case.name}: {name} waited on the host: its inputs, queued behind a {delay_ms:.0f} ms delay on the "
                                     f"caller's stream, had arrived when it returned (warm host time {host_ms:.2f} ms); the header says it "
                                     f"does not synchronise")
        for name in case.syncs:
            assert not any(seen[name]), f"{case.name}: {name} is documented to synchronise, but returned with the stream's work pending"

    # the comparison
    assert len(result) == len(twin), f"{case.name}: {len(result)} result tensors, the twin has {len(twin)}"
    assert got_host == twin_host, f"{case.name}: host values {got_host} differ from the twin's {twin_host}"
    if case.bitwise:
        for i, (a, b) in enumerate(zip(result, twin)):
            assert a.shape == b.shape and a.dtype == b.dtype, (case.name, i, a.shape, b.shape)
            same = a.contiguous().reshape(-1).view(torch.uint8).equal(b.contiguous().reshape(-1).view(torch.uint8)) if a.numel() else True
            if not same:
                bad = (a != b) | (a.isnan() != b.isnan()) if a.is_floating_point() else (a != b)
                raise AssertionError(f"{case.name} [{pool}, {variant}]: result tensor {i} {tuple(a.shape)} differs from the default-stream "
                                     f"twin in {int(bad.sum())} of {a.numel()} elements ({int(a.isnan().sum()) if a.is_floating_point() else 0} "
                                     f"of them still the NaN it was poisoned with)")
    else:
        assert case.anchor is not None, f"{case.name}: neither a bit promise nor a reference"
        case.anchor(host_staging, result)
    return result


# ================================================================================================ the case table
# Shapes are the smallest of the existing tests of each path (tests/test_scratch_pool.py, test_sampler_chains.py, test_hip_parity.py,
# test_sample_persist.py).  Every call below is idempotent: it first sets the engine state it depends on - from late inputs too.
ITEMS, HIDDEN, LATENT = 70, 36, 12
SEED, STEP, P_DROP = 0xC0FFEE, 3, 0.5
FACTOR, NEUMF_USERS = 8, 310
LR = 1e-4            # (what tests/test_hip_parity.py compares with the oracle at: at 1e-3 a parameter whose gradient cancels moves 2 lr either way)
UTIL_LR = 1e-3       # the optimizer families at their own tests' rate (tests/neumf_train_ref.py, tests/mlp_eval_ref.py LR): their bound on p,
                     # 2^-24 |p| + 1e-4 max|p - p_0|, takes the fp32 rounding of p in EVERY step of a chain out of its second term
CORE_TOL = 1e-4   # the engine's bar against the fp64 oracle (tests/test_hip_parity.py TOL, __graft_entry__.smoke)


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def _rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------------ core engine
def _core_engine(dims, max_rows, **debug):
    def make(engine_cls):
        e = engine_cls(*dims, max_rows)
        if debug:
            e.debug_set(**debug)
        return e
    return make


def _core_inputs(dims, B, seed=1):
    from sdrm_amd import synth
    L, W, T, H = dims

    def make(device):
        eps, t, masks = synth.synth_train_randoms(B, L, T, 1.0, seed=seed + 1)
        zeros = np.zeros(synth.param_count(L, W, T, H), np.float32)
        return dict(flat=_dev(synth.flatten_params(synth.init_params(L, W, T, H, seed=seed), H), device), m0=_dev(zeros, device), v0=_dev(zeros, device),
                    x0=_dev(synth.synth_latents(B, L, seed=seed + 2), device), eps=_dev(eps, device), t=_dev(t, device, torch.int64),
                    keep=_dev(np.stack(masks), device, torch.uint8))
    return make


def _reset(e, b):
    e.set_params(b["flat"])
    e.set_adam_state(b["m0"], b["v0"], 0)


def _randoms(b, mode, k):
    """Keyword arguments of one train step: the caller's randoms (EXPLICIT) or Philox keys of step k."""
    return dict(noise=b["eps"], t=b["t"], keep=b["keep"]) if mode == "explicit" else dict(seed=7, step=k)


def _state(e):
    return [e.get_params(), *e.get_adam_state()[:2]]



def _train_randoms(dims, B, mode, inp, k):
    """(eps, t, keeps) of train step k: the caller's (EXPLICIT) or oracle/philox_ref.py's restatement of the device generator for the
    keys `_randoms` passes (PHILOX; integer draws bit for bit, tests/test_hip_parity.py::test_philox_mode_train)."""
    if mode == "explicit":
        return inp["eps"].numpy(), inp["t"].numpy(), list(inp["keep"].numpy())
    from oracle import philox_ref as pr
    eps, t, keep = pr.train_randoms(7, k, 0, B, dims[0], dims[2], 1.0)
    return eps, t, list(keep)


class _Preacts:
    """What tests/test_hip_parity.py::engine_branch_masks reads from an engine, from the pre-activations a case brought back."""

    def __init__(self, layers):
        self.layers = layers

    def preacts(self, layer, B):
        return self.layers[layer]


def _oracle_train(dims, B, mode, steps, phases):
    """The anchor of a train case, tests/test_hip_parity.py::train_step_vs_oracle restated on what the case returns: the last loss and
    the parameters after `steps` steps against the fp64 oracle at CORE_TOL; for a three-phase case also P / S / Q and, per tensor, the
    gradient of the FIRST step, the oracle's backward evaluated with the engine's own PReLU branch choice (checked to differ only at
    pre-activations that are zero within rounding)."""
    def anchor(inp, res):
        from oracle import sdrm_oracle as orc
        from sdrm_amd import synth
        import test_hip_parity as hp
        L, W, T, H = dims
        o = orc.Oracle(L, W, T, H, synth.unflatten_params(inp["flat"].numpy(), L, W, T, H))
        x0 = inp["x0"].numpy()
        if phases:
            eps, t, keeps = _train_randoms(dims, B, mode, inp, 0)
            caches = []
            o.loss_and_grads(x0, eps, t, keeps, caches=caches)
            branch, flips = hp.engine_branch_masks(_Preacts(res[6:6 + H + 1]), o, caches, B)
            _, grads_ref, outs_ref, _ = o.loss_and_grads(x0, eps, t, keeps, neg_override=branch)
            for j in range(3):
                assert hp.close(res[5][j].numpy(), outs_ref[j].numpy(), CORE_TOL)
            for name, got in hp.per_tensor(res[4].numpy(), dims):
                ref = grads_ref[name].numpy().ravel()
                assert _rel_l2(got, ref) <= CORE_TOL and _rel_max(got, ref) <= CORE_TOL, (name, flips, _rel_l2(got, ref), _rel_max(got, ref))
        for k in range(steps):
            loss_ref, _, _ = o.train_step(x0, *_train_randoms(dims, B, mode, inp, k), LR)
        losses, params = res[0].numpy(), res[1].numpy()
        assert abs(float(losses[-1]) - loss_ref) <= CORE_TOL * abs(loss_ref), (float(losses[-1]), loss_ref)
        assert _rel_l2(params, o.flat(synth.param_names(H))) <= CORE_TOL
    return anchor


def case_params_roundtrip():
    dims = (40, 40, 9, 1)

    def make(device):
        g = torch.Generator().manual_seed(5)
        from sdrm_amd import synth
        P = synth.param_count(*dims)
        return dict(flat=torch.randn(P, generator=g).to(device), m=torch.randn(P, generator=g).to(device), v=torch.rand(P, generator=g).to(device))

    def call(e, b, alloc):
        e.set_params(b["flat"])
        e.set_adam_state(b["m"], b["v"], 11)
        p = e.get_params()
        m, v, step = e.get_adam_state()
        e.adam_reset()
        m0, v0, step0 = e.get_adam_state()
        return p, m, v, step, m0, v0, step0

    def anchor(inp, res):
        assert torch.equal(res[0], inp["flat"]) and torch.equal(res[1], inp["m"]) and torch.equal(res[2], inp["v"])
        assert not res[3].any() and not res[4].any()

    names = ("sdrm_set_params", "sdrm_get_params", "sdrm_set_adam_state", "sdrm_get_adam_state", "sdrm_adam_reset")
    return Case("params-roundtrip", names, make, _core_engine(dims, 33), call, nosync=names, anchor=anchor)



def case_train(tag, dims, B, mode, one_call, **debug):
    """Two train steps, as three phases or as sdrm_train_step: the losses and the state after them; the three-phase form also brings
    back the first step's gradient, P / S / Q and every layer's pre-activations, which the anchor needs for the gradient."""
    H = dims[3]

    def call(e, b, alloc):
        _reset(e, b)
        losses = []
        for k in range(2):
            if one_call:
                losses.append(e.train_step(b["x0"], LR, **_randoms(b, mode, k)).clone())
            else:
                e.train_forward(b["x0"], **_randoms(b, mode, k))
                losses.append(e.train_backward().clone())
                if k == 0:
                    first = [e.get_grads(), e.train_outputs(B)] + [e.preacts(layer, B) for layer in range(H + 1)]
                e.adam_step(LR)
        out = [torch.cat(losses), *_state(e)]
        return out + [e.get_grads()] if one_call else out + first

    names = ("sdrm_train_step", "sdrm_get_grads") if one_call else (
        "sdrm_train_forward", "sdrm_train_backward", "sdrm_adam_step", "sdrm_get_train_outputs", "sdrm_get_preacts", "sdrm_get_grads")
    return Case(f"train-{tag}-{mode}-{'step' if one_call else 'phases'}", names, _core_inputs(dims, B), _core_engine(dims, B, **debug), call,
                nosync=names, anchor=_oracle_train(dims, B, mode, 2, not one_call))


def case_backward_buckets():
    """sdrm_train_backward_begin leaves the FIRST bucket of the caller's gradient buffer final in stream order: it is consumed on the
    stream between begin and finish."""
    dims, B = (136, 136, 12, 2), 75

    def call(e, b, alloc):
        _reset(e, b)
        (o1, n1), (o2, n2) = e.grad_buckets()
        grad = alloc(e.P)
        e.train_forward(b["x0"], **_randoms(b, "explicit", 0))
        e.train_backward_begin(grad=grad)
        first = grad[o1:o1 + n1].clone()
        e.train_backward_finish(grad=grad)
        e.adam_step(LR, grad=grad)
        return first, grad, e.get_params()

    def anchor(inp, res):
        first, grad = res[0], res[1]
        assert torch.equal(first, grad[:first.numel()]) and not grad.isnan().any()
        # ... and the step that gradient made, against the fp64 oracle (losses are not part of this case's result)
        from oracle import sdrm_oracle as orc
        from sdrm_amd import synth
        o = orc.Oracle(*dims, synth.unflatten_params(inp["flat"].numpy(), *dims))
        o.train_step(inp["x0"].numpy(), *_train_randoms(dims, B, "explicit", inp, 0), LR)
        assert _rel_l2(res[2].numpy(), o.flat(synth.param_names(dims[3]))) <= CORE_TOL

    names = ("sdrm_train_forward", "sdrm_train_backward_begin", "sdrm_train_backward_finish", "sdrm_adam_step")
    return Case("backward-buckets", names, _core_inputs(dims, B), _core_engine(dims, B, tile="row"), call, nosync=names, anchor=anchor)


def case_inference():
    """sdrm_forward (both modes), sdrm_perturb_input, sdrm_reverse_step on a caller's state."""
    dims, B = (40, 40, 9, 1), 33

    def call(e, b, alloc):
        _reset(e, b)
        y = e.forward(b["x0"], b["t"], keep=b["keep"][0])
        y2 = e.forward(b["x0"], b["t"], seed=3, step=1, row0=5)
        xp = e.perturb_input(b["x0"], b["t"], b["eps"])
        x1 = e.reverse_step(b["x0"], 4, b["eps"], b["keep"][1])
        return y, y2, xp, x1

    def anchor(inp, res):
        from oracle import sdrm_oracle as orc
        from sdrm_amd import synth
        o = orc.Oracle(*dims, synth.unflatten_params(inp["flat"].numpy(), *dims))
        want = o.forward(torch.from_numpy(inp["x0"].numpy()), inp["t"], torch.from_numpy(inp["keep"][0].numpy().astype(np.float32))).numpy()
        assert _rel_max(res[0].numpy(), want) <= CORE_TOL

    names = ("sdrm_forward", "sdrm_perturb_input", "sdrm_reverse_step")
    return Case("inference", names, _core_inputs(dims, B), _core_engine(dims, B), call, nosync=names, anchor=anchor)



def _sample_randoms(dims, n, mode, multires, inp, seed=17, call_id=3, row0=1358, nd=0.9):
    """(xT, z, keep, Tj | None): the caller's, or oracle/philox_ref.py's restatement of the device draws for the PHILOX keys."""
    if mode == "explicit":
        return inp["xT"].numpy(), inp["z"].numpy(), inp["keep"].numpy(), inp["Tj"].numpy() if multires else None
    from oracle import philox_ref as pr
    xT, z, keep, Tj = pr.sample_randoms(seed, call_id, row0, n, dims[0], dims[2], nd, multires)
    return xT, z, keep, Tj if multires else None


def _oracle_sample(dims, inp, randoms, got):
    """The latents against the fp64 oracle's reverse loop at tests/test_hip_parity.py's `close` (rel_l2 and rel_max <= TOL)."""
    from oracle import sdrm_oracle as orc
    from sdrm_amd import synth
    import test_hip_parity as hp
    want = orc.Oracle(*dims, synth.unflatten_params(inp["flat"].numpy(), *dims)).sample(*randoms).numpy()
    assert hp.close(got.numpy(), want, CORE_TOL), (_rel_l2(got.numpy(), want), _rel_max(got.numpy(), want))


def case_sample(tag, dims, n, mode, multires, chains=None, resumable=False, **debug):
    """sdrm_sample - or, `resumable`, the same call as sdrm_sample_begin + sdrm_sample_steps + sdrm_sample_end with the caller's
    randoms (the C call directly: the Python wrapper of the resumable form is PHILOX only)."""
    import ctypes as C
    from sdrm_amd import synth
    L, W, T, H = dims
    if chains:
        debug["chains"] = chains

    def make(device):
        d = dict(flat=_dev(synth.flatten_params(synth.init_params(L, W, T, H, seed=4), H), device))
        if mode == "explicit":
            xT, z, keep, Tj = synth.synth_sample_randoms(n, L, T, 0.9, seed=6, multires=multires)
            d.update(xT=_dev(xT, device), z=_dev(z, device), keep=_dev(keep, device, torch.uint8))
            if multires:
                d["Tj"] = _dev(Tj, device, torch.int64)
        return d

    def call(e, b, alloc):
        e.set_params(b["flat"])
        if resumable:
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            e._check(e.lib.sdrm_sample_begin(e._h, n, 0.9, int(multires), 0, ptr(b["xT"]), ptr(b["z"]), ptr(b["keep"]), ptr(b.get("Tj")), 0, 0, 0, None,
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sdrm_sample_begin")
            e._sample_n = n
            while e.sample_steps(5) > 0:
                pass
            out = e.sample_end()
        elif mode == "explicit":
            out = e.sample(n, nd=0.9, multires=multires, xT=b["xT"], z=b["z"], keep=b["keep"], Tj=b.get("Tj"))
        else:
            out = e.sample(n, nd=0.9, multires=multires, seed=17, call_id=3, row0=1358, return_Tj=multires)
        if chains:
            assert e.sampler_chains == chains, (e.sampler_chains, chains)
        return out

    def anchor(inp, res):
        randoms = _sample_randoms(dims, n, mode, multires, inp)
        if mode == "philox" and multires:
            assert np.array_equal(res[1].numpy(), randoms[3])   # the drawn start steps, exactly
        _oracle_sample(dims, inp, randoms, res[0])

    # a caller's Tj is read back by the call (it orders the rows on the host): that one form waits for the stream, see the header
    waits = mode == "explicit" and multires
    entry = "sdrm_sample_begin" if resumable else "sdrm_sample"
    names = ("sdrm_set_params", entry) + (("sdrm_sample_steps", "sdrm_sample_end") if resumable else ())
    return Case(f"sample-{tag}-{mode}-{'multires' if multires else 'full'}", names, make, _core_engine(dims, n, **debug), call,
                nosync=("sdrm_set_params",) if waits else names, syncs=(entry,) if waits else (), anchor=anchor)



def case_sample_resumable(tag, train_tile, chains):
    """sdrm_sample_begin, sdrm_sample_steps in chunks of 1, 5 and the rest with train steps of 64 users queued between them on the same
    side stream, sdrm_sample_end, with the caller's stream still pending: with one chain the detach-armed path (a small call's chain
    leaves the caller's stream beside the train step), with two forced chains the forked-chain path and, behind a row-owned step, the
    hold event.  The twin is the SEQUENTIAL order on the default stream - the sampling call uninterrupted, then the train steps - and
    both halves are held to the fp64 oracle."""
    from sdrm_amd import synth
    dims, n, B = (136, 136, 40, 2), 400, 64
    L, W, T, H = dims

    def make(device):
        return dict(flat=_dev(synth.flatten_params(synth.init_params(L, W, T, H, seed=41), H), device), x0=_dev(synth.synth_latents(B, L, seed=12), device),
                    m0=torch.zeros(synth.param_count(*dims), device=device), v0=torch.zeros(synth.param_count(*dims), device=device))

    def engine(engine_cls):
        return engine_cls(*dims, n).debug_set(sample_persist=0, chains=chains)

    def start(e, b):
        if train_tile == "per-layer":
            e.debug_set(rowchain=0, rows48=0)
        else:
            e.debug_set(tile=train_tile)
        _reset(e, b)

    def call(e, b, alloc):
        start(e, b)
        e.sample_begin(n, nd=0.9, seed=17, call_id=3, row0=1358)
        e.sample_steps(1)
        e.train_step(b["x0"], LR, seed=7, step=0)
        e.sample_steps(5)
        e.train_step(b["x0"], LR, seed=7, step=1)
        e.train_step(b["x0"], LR, seed=7, step=2)
        while e.sample_steps(1000) > 0:
            pass
        out = e.sample_end()
        assert e.sampler_chains == chains, (e.sampler_chains, chains)
        return out, e.get_params()

    def sequential(e, b, alloc):
        start(e, b)
        out = e.sample(n, nd=0.9, seed=17, call_id=3, row0=1358)
        for k in range(3):
            e.train_step(b["x0"], LR, seed=7, step=k)
        return out, e.get_params()

    def anchor(inp, res):
        from oracle import sdrm_oracle as orc
        _oracle_sample(dims, inp, _sample_randoms(dims, n, "philox", False, inp), res[0])
        o = orc.Oracle(L, W, T, H, synth.unflatten_params(inp["flat"].numpy(), L, W, T, H))
        for k in range(3):
            o.train_step(inp["x0"].numpy(), *_train_randoms(dims, B, "philox", inp, k), LR)
        assert _rel_l2(res[1].numpy(), o.flat(synth.param_names(H))) <= CORE_TOL

    names = ("sdrm_sample_begin", "sdrm_sample_steps", "sdrm_sample_end", "sdrm_train_step")
    return Case(f"sample-resumable-{tag}", names, make, engine, call, nosync=names, anchor=anchor, twin_call=sequential)


def case_sharded():
    dims, B = (40, 40, 9, 1), 33

    def engine(engine_cls):
        import pytest
        if not engine_cls.comm_available():
            pytest.skip("librccl does not resolve in this process")
        e = engine_cls(*dims, B)
        e.comm_init_rank(1, 0, engine_cls.comm_unique_id())
        return e

    def call(e, b, alloc):
        _reset(e, b)
        losses = [e.train_step_sharded(b["x0"], LR, **_randoms(b, "explicit", k)).clone() for k in range(2)]
        return [torch.cat(losses), *_state(e)]

    return Case("train-sharded-one-rank", ("sdrm_train_step_sharded",), _core_inputs(dims, B), engine, call, nosync=("sdrm_train_step_sharded",),
                anchor=_oracle_train(dims, B, "explicit", 2, False))


def case_profile():
    dims, B = (40, 40, 9, 1), 33

    def call(e, b, alloc):
        _reset(e, b)
        e.profile_begin(capacity=64)
        loss = e.train_step(b["x0"], LR, **_randoms(b, "explicit", 0)).clone()
        e.profile_end()
        return loss, e.get_params()

    return Case("profile-end", ("sdrm_train_step", "sdrm_profile_end"), _core_inputs(dims, B), _core_engine(dims, B), call,
                nosync=("sdrm_train_step",), syncs=("sdrm_profile_end",), anchor=_oracle_train(dims, B, "explicit", 1, False))


# ------------------------------------------------------------------------------------------------ utility families
def _util_engine(engine_cls):
    return engine_cls(8, 8, 4, 0, 16)


def _vae(device, seed=20261):
    rng = np.random.default_rng(seed)
    t = lambda *shape: _dev((rng.standard_normal(shape) * 0.2).astype(np.float32), device)
    return dict(w1=t(HIDDEN, ITEMS), b1=t(HIDDEN), w2=t(2 * LATENT, HIDDEN), b2=t(2 * LATENT), w3=t(HIDDEN, LATENT), b3=t(HIDDEN), w4=t(ITEMS, HIDDEN),
                b4=t(ITEMS))


def _feed(b):
    import vae_input_layer_ref as ilr
    return ilr.case_feed(ITEMS, "ones", SEED, STEP, P_DROP)[:b].tocsr()


def _csr_inputs(m, device, prefix="csr"):
    m = m.tocsr().copy()
    m.sort_indices()
    return {f"{prefix}_indptr": _dev(m.indptr.astype(np.int64), device), f"{prefix}_indices": _dev(m.indices.astype(np.int32), device)}


def _csc_inputs(m, device):
    c = m.tocsc().copy()
    c.sort_indices()
    return dict(csc_indptr=_dev(c.indptr.astype(np.int64), device), csc_indices=_dev(c.indices.astype(np.int32), device))


def _csr(b_, shape, prefix="csr"):
    return b_[f"{prefix}_indptr"], b_[f"{prefix}_indices"], None, shape


def _rnd(device, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(device)


def _util(name, covers, make, call, nosync=None, syncs=(), anchor=None, bitwise=True, pools=("warm", "cold"), prepare=None, feed=True):
    covers = tuple(covers) + (("sdrm_feed_status",) if feed else ())
    nosync = tuple(n for n in covers if n not in SYNCHRONISING and n not in syncs) if nosync is None else nosync
    return Case(name, covers, make, _util_engine, call, nosync=nosync, syncs=tuple(syncs), anchor=anchor, bitwise=bitwise, feed=feed, pools=pools,
                prepare=prepare)


def case_csr_rows_to_dense(b=33):
    m = _feed(b)

    def make(device):
        return dict(_csr_inputs(m, device), rows=_dev(np.random.default_rng(3).permutation(b).astype(np.int64), device))

    def call(e, x, alloc):
        return e.csr_rows_to_dense(_csr(x, m.shape), rows=x["rows"], check=False), e.csr_rows_to_dense(_csr(x, m.shape), row0=2, b=b - 2, check=False)

    def anchor(inp, res):   # the family's bar: the dense rows, exactly (tests/test_device_feed.py)
        dense = m.toarray().astype(np.float32)
        assert np.array_equal(res[0].numpy(), dense[inp["rows"].numpy()]) and np.array_equal(res[1].numpy(), dense[2:])

    return _util("csr-rows-to-dense", ("sdrm_csr_rows_to_dense",), make, call, anchor=anchor, bitwise=False)


def case_equal_sparsity():
    def make(device):
        return dict(raw=_dev(np.random.default_rng(20261).random((33, ITEMS), dtype=np.float32), device))

    def call(e, x, alloc):
        return e.equal_sparsity(x["raw"], 0.8, return_threshold=True)

    def anchor(inp, res):   # exactly numpy's quantile and comparison (tests/test_equal_sparsity.py)
        raw = inp["raw"].numpy()
        thr = np.quantile(raw.flatten(), 0.8)
        assert np.float32(res[1].numpy()) == np.float32(thr) and np.array_equal(res[0].numpy().astype(bool), raw >= thr)

    return _util("equal-sparsity", ("sdrm_equal_sparsity",), make, call, anchor=anchor, bitwise=False, feed=False)


def case_equal_sparsity_csr():
    def make(device):
        return dict(raw=_dev(np.random.default_rng(20261).random((33, ITEMS), dtype=np.float32), device))

    def call(e, x, alloc):
        indptr, nnz, thr = e.equal_sparsity_csr_begin(x["raw"], 0.8)
        alloc.delay_again()   # begin has waited for the stream: `end` is observed behind a delay of its own
        indices = e.equal_sparsity_csr_end(alloc(max(nnz, 1), dtype=torch.int32))
        return indptr, nnz, thr, indices[:nnz]

    def anchor(inp, res):
        import scipy.sparse as sp
        raw = inp["raw"].numpy()
        want = sp.csr_matrix(raw >= np.quantile(raw.flatten(), 0.8))
        want.sort_indices()
        assert np.array_equal(res[0].numpy(), want.indptr) and np.array_equal(res[2].numpy(), want.indices)

    return _util("equal-sparsity-csr", ("sdrm_equal_sparsity_csr_begin", "sdrm_equal_sparsity_csr_end"), make, call,
                 nosync=("sdrm_equal_sparsity_csr_end",), syncs=("sdrm_equal_sparsity_csr_begin",), anchor=anchor, feed=False)


def case_csr_transpose_vstack(b=33):
    m = _feed(b)

    def make(device):
        return _csr_inputs(m, device)

    def call(e, x, alloc):
        csr = _csr(x, m.shape)
        colptr, rowidx, _, _ = e.csr_transpose(csr, check=False)
        indptr, indices, _, _ = e.csr_vstack([csr, csr], check=False)
        return colptr, rowidx, indptr, indices

    def anchor(inp, res):   # scipy's tocsc() + sort_indices() / vstack, byte for byte (tests/test_csr_transpose.py)
        import scipy.sparse as sp
        c = m.tocsc()
        c.sort_indices()
        v = sp.vstack([m, m]).tocsr()
        assert np.array_equal(res[0].numpy(), c.indptr) and np.array_equal(res[1].numpy()[:c.nnz], c.indices)
        assert np.array_equal(res[2].numpy(), v.indptr) and np.array_equal(res[3].numpy()[:v.nnz], v.indices)

    def prepare(e, staging):
        small = _feed(33)
        d = _csr_inputs(small, e.device)
        e.csr_transpose(_csr(d, small.shape))
        e.csr_vstack([_csr(d, small.shape)] * 2)

    return _util(f"csr-transpose-vstack-{b}", ("sdrm_csr_transpose", "sdrm_csr_vstack"), make, call, anchor=anchor,
                 pools=("warm", "cold") if b == 33 else ("regrow",), prepare=prepare)


def case_vae_decode(b=33):
    def make(device):
        v = _vae(device)
        return dict(z=_rnd(device, b, b, LATENT), **{k: v[k] for k in ("w3", "b3", "w4", "b4")})

    def call(e, x, alloc):
        return e.vae_decode(x["z"], x["w3"], x["b3"], x["w4"], x["b4"])

    def anchor(inp, res):   # oracle/vae_decode_ref.py in fp64 at tests/test_vae_decode.py's TOL
        from oracle import vae_decode_ref
        want = vae_decode_ref.decode(*(inp[k].numpy() for k in ("z", "w3", "b3", "w4", "b4")))
        assert _rel_max(res[0].numpy(), want) <= 1e-4 and _rel_l2(res[0].numpy(), want) <= 1e-4

    def prepare(e, staging):
        e.vae_decode(_rnd(e.device, 1, 33, LATENT), *(staging[k] for k in ("w3", "b3", "w4", "b4")))

    return _util(f"vae-decode-{b}", ("sdrm_vae_decode",), make, call, anchor=anchor, feed=False, pools=("warm", "cold") if b == 33 else ("regrow",),
                 prepare=prepare)


def case_vae_encode(b=33):
    m = _feed(b)

    def make(device):
        v = _vae(device)
        return dict(_csr_inputs(m, device), x=_dev(m.toarray().astype(np.float32), device), **{k: v[k] for k in ("w1", "b1", "w2", "b2")})

    def call(e, x, alloc):
        e.vae_encoder_load(x["w1"], x["b1"], x["w2"], x["b2"])
        return e.vae_encode(x["x"], return_kl=True), e.vae_encode_csr(_csr(x, m.shape), row0=0, b=b, return_kl=True, check=False)

    def anchor(inp, res):   # tests/vae_encode_ref.py in fp64 at tests/test_vae_encode.py's TOL = 1e-4 (both forms)
        import vae_encode_ref as ver
        z, kl = ver.encode(inp["x"].numpy(), *(inp[k].numpy() for k in ("w1", "b1", "w2", "b2")))
        for got_z, got_kl in ((res[0], res[1]), (res[2], res[3])):
            assert _rel_max(got_z.numpy(), z) <= 1e-4 and _rel_l2(got_z.numpy(), z) <= 1e-4 and abs(float(got_kl) - float(kl)) <= 1e-4 * abs(float(kl))

    return _util("vae-encode", ("sdrm_vae_encoder_load", "sdrm_vae_encode", "sdrm_vae_encode_csr"), make, call, anchor=anchor, bitwise=False)


def case_multinomial_nll(b=33):
    m = _feed(b)

    def make(device):
        return dict(_csr_inputs(m, device), logits=_rnd(device, 2, b, ITEMS), scale=torch.full((1,), 0.7, device=device))

    def call(e, x, alloc):
        loss, lse = e.multinomial_nll_csr(x["logits"], _csr(x, m.shape), row0=0, b=b, check=False)
        return loss, lse, e.multinomial_nll_csr_grad(x["logits"], lse, _csr(x, m.shape), row0=0, b=b, scale=x["scale"])

    def anchor(inp, res):   # tests/multinomial_nll_ref.py in fp64 at tests/test_multinomial_nll.py's TOL_LOSS and TOL_GRAD
        import multinomial_nll_ref as mn
        loss, lse, grad = mn.nll(inp["logits"].numpy(), m, scale=float(inp["scale"][0]))
        assert abs(float(res[0]) - loss) <= 1e-5 * abs(loss) and _rel_max(res[1].numpy(), lse) <= 1e-5
        assert _rel_max(res[2].numpy(), grad) <= 1e-4 and _rel_l2(res[2].numpy(), grad) <= 1e-4

    return _util("multinomial-nll", ("sdrm_multinomial_nll_csr", "sdrm_multinomial_nll_csr_grad"), make, call, anchor=anchor)


def case_input_layer(b=33):
    m = _feed(b)

    def make(device):
        v = _vae(device)
        return dict(_csr_inputs(m, device), **_csc_inputs(m, device), w1=v["w1"], b1=v["b1"], dpre=_rnd(device, 3, b, HIDDEN))

    def call(e, x, alloc):
        pre, rowscale = e.vae_input_layer_fwd(x["w1"], x["b1"], _csr(x, m.shape), row0=0, b=b, seed=SEED, step=STEP, p_drop=P_DROP, check=False)
        return pre, rowscale, e.vae_input_layer_wgrad(x["dpre"], rowscale, _csr(x, m.shape, "csc"), lo=0, b=b, seed=SEED, step=STEP, p_drop=P_DROP, check=False)

    def anchor(inp, res):   # tests/vae_input_layer_ref.py in fp64 at tests/test_vae_input_layer.py's TOL (pre, dW1) and TOL_SCALE (rowscale)
        import vae_input_layer_ref as ilr
        pre, rowscale, xt = ilr.forward(inp["w1"].numpy(), inp["b1"].numpy(), m, np.arange(b), SEED, STEP, P_DROP)
        dw1 = ilr.backward(xt, inp["dpre"].numpy())[0]
        assert _rel_max(res[0].numpy(), pre) <= 1e-4 and _rel_l2(res[0].numpy(), pre) <= 1e-4
        assert np.abs(res[1].numpy() / rowscale - 1).max() <= 1e-5
        assert _rel_max(res[2].numpy(), dw1) <= 1e-4 and _rel_l2(res[2].numpy(), dw1) <= 1e-4

    def prepare(e, staging):
        small = _feed(33)
        e.vae_input_layer_fwd(staging["w1"], staging["b1"], e.csr_to_device(small), row0=0, b=33, seed=SEED, step=STEP, p_drop=P_DROP)

    return _util(f"vae-input-layer-{b}", ("sdrm_vae_input_layer_fwd", "sdrm_vae_input_layer_wgrad"), make, call, anchor=anchor,
                 pools=("warm", "cold") if b == 33 else ("regrow",), prepare=prepare)


def case_latent(b=33):
    def make(device):
        v = _vae(device)
        return dict(pre=_rnd(device, 4, b, HIDDEN), w2=v["w2"], b2=v["b2"], gz=_rnd(device, 5, b, LATENT), gkl=_rnd(device, 6, 1))

    def call(e, x, alloc):
        z, kl, saved = e.vae_latent_fwd(x["pre"], x["w2"], x["b2"], row0=0, seed=SEED, step=STEP)
        return z, kl, saved, e.vae_latent_bwd(saved, x["w2"], x["gz"], x["gkl"])

    def anchor(inp, res):   # tests/vae_latent_ref.py in fp64 at tests/test_vae_latent.py's TOL, TOL_EPS and TOL_LOSS
        import vae_latent_ref as lr
        z, kl, h1, out2, eps, dpre, dw2, db2 = (t.numpy() for t in res)
        assert _rel_max(eps, lr.draw_eps(SEED, STEP, np.arange(b), LATENT)) <= 1e-5
        fwd = lr.forward(inp["pre"].numpy(), inp["w2"].numpy(), inp["b2"].numpy(), eps)
        assert _rel_max(z, fwd["z"]) <= 1e-4 and _rel_max(out2, fwd["out2"]) <= 1e-4 and abs(float(kl) - float(fwd["kl"])) <= 1e-5 * abs(float(fwd["kl"]))
        bwd = lr.backward(fwd, inp["w2"].numpy(), eps, inp["gz"].numpy(), float(inp["gkl"][0]))
        for got, name in ((dpre, "dpre"), (dw2, "dw2"), (db2, "db2")):
            assert _rel_max(got, bwd[name]) <= 1e-4 and _rel_l2(got, bwd[name]) <= 1e-4, name

    return _util("vae-latent", ("sdrm_vae_latent_fwd", "sdrm_vae_latent_bwd"), make, call, anchor=anchor, feed=False)


def case_decoder_nll(b=33):
    m = _feed(b)

    def make(device):
        v = _vae(device)
        return dict(_csr_inputs(m, device), z=_rnd(device, 7, b, LATENT), **{k: v[k] for k in ("w3", "b3", "w4", "b4")})

    def call(e, x, alloc):
        w = [x[k] for k in ("w3", "b3", "w4", "b4")]
        loss, saved = e.vae_decoder_nll_fwd(x["z"], *w, _csr(x, m.shape), row0=0, b=b, check=False)
        return loss, saved, e.vae_decoder_nll_bwd(saved, x["z"], *w, _csr(x, m.shape), row0=0, b=b)

    def prepare(e, staging):
        small = _feed(33)
        e.vae_decoder_nll_fwd(_rnd(e.device, 7, 33, LATENT), *(staging[k] for k in ("w3", "b3", "w4", "b4")), e.csr_to_device(small), row0=0, b=33)

    def anchor(inp, res):   # tests/vae_decoder_ref.py in fp64 at tests/test_vae_decoder_train.py's TOL and TOL_LOSS
        import vae_decoder_ref as dr
        w = [inp[k].numpy() for k in ("w3", "b3", "w4", "b4")]
        X = m.toarray()
        fwd = dr.forward(inp["z"].numpy(), *w, X)
        bwd = dr.backward(fwd, inp["z"].numpy(), w[0], w[2], X)
        loss, h3, logits, lse = (t.numpy() for t in res[:4])
        assert abs(float(loss) - float(fwd["loss"])) <= 1e-5 * abs(float(fwd["loss"])) and _rel_max(logits, fwd["logits"]) <= 1e-4
        for got, name in zip(res[4:], ("dz", "dw3", "db3", "dw4", "db4")):
            assert _rel_max(got.numpy(), bwd[name]) <= 1e-4 and _rel_l2(got.numpy(), bwd[name]) <= 1e-4, name

    return _util(f"vae-decoder-nll-{b}", ("sdrm_vae_decoder_nll_fwd", "sdrm_vae_decoder_nll_bwd"), make, call, anchor=anchor,
                 pools=("warm", "cold") if b == 33 else ("regrow",), prepare=prepare)


def _adam_bars(p, m, v, p0, want, what):
    """tests/test_vae_adam.py's bars for one tensor (as tests/test_neumf_train.py and tests/test_mlp_train.py restate them): m and v
    rel_max <= 1e-4 (exactly zero where the expectation is), |p - p_ref| <= 2^-24 |p_ref| + 1e-4 max|p_ref - p_0|."""
    p_ref, m_ref, v_ref = want
    for key, a, r in (("m", m, m_ref), ("v", v, v_ref)):
        if np.abs(r).max() > 0:
            assert _rel_max(a, r) <= 1e-4, (what, key, _rel_max(a, r))
        else:
            assert not np.asarray(a).any(), (what, key)
    bound = 2.0 ** -24 * np.abs(p_ref) + 1e-4 * np.abs(p_ref - np.asarray(p0, dtype=np.float64)).max()
    err = np.abs(np.asarray(p, dtype=np.float64) - p_ref)
    assert (err <= bound).all(), (what, float(err.max()), float(bound.min()))


def case_vae_adam():
    sizes = (ITEMS * HIDDEN, HIDDEN, 5000)

    def make(device):
        d = {}
        for i, n in enumerate(sizes):
            d.update({f"p{i}": _rnd(device, 10 + i, n), f"g{i}": _rnd(device, 20 + i, n), f"m{i}": _rnd(device, 30 + i, n) * 0.1,
                      f"v{i}": _rnd(device, 40 + i, n).abs() * 0.01})
        d.update(neg_ll=_rnd(device, 50, 1), kl=_rnd(device, 51, 1))
        return d

    def call(e, x, alloc):
        k = range(len(sizes))
        partials = alloc(sum(-(-n // 4096) for n in sizes), dtype=torch.float64)
        slots = alloc(4)
        e.vae_adam_step([x[f"p{i}"] for i in k], [x[f"g{i}"] for i in k], [x[f"m{i}"] for i in k], [x[f"v{i}"] for i in k], step=3, lr=UTIL_LR,
                        l2_coefs=[1e-4, 0.0, 1e-4], l2_partials=partials)
        e.vae_loss_slot(x["neg_ll"], x["kl"], 0.2, slots, 2, l2_partials=partials, weight_decay=1e-4)
        return [x[f"{t}{i}"] for t in "pmv" for i in k], partials, slots[2:3]

    def anchor(inp, res):   # tests/vae_adam_ref.py in fp64 at tests/test_vae_adam.py's bars for p, m and v
        import vae_adam_ref as var
        for i, coef in enumerate((1e-4, 0.0, 1e-4)):
            want = var.adam_step(*(inp[f"{t}{i}"].numpy() for t in "pgmv"), 3, UTIL_LR, l2_coef=coef)
            _adam_bars(res[i].numpy(), res[3 + i].numpy(), res[6 + i].numpy(), inp[f"p{i}"].numpy(), want, f"tensor {i}")

    return _util("vae-adam", ("sdrm_vae_adam_step", "sdrm_vae_loss_slot"), make, call, anchor=anchor, feed=False)


def case_holdout_split(b=33):
    m = _feed(b)

    def make(device):
        return _csr_inputs(m, device)

    def call(e, x, alloc):
        (tp, ti, _, _), (hp, hi, _, _) = e.holdout_split(_csr(x, m.shape), test_prop=0.2, seed=5, draw=1, check=False)
        return tp, ti, hp, hi

    def anchor(inp, res):   # tests/holdout_ref.py, the split restated on the host: the same entries, exactly
        import holdout_ref as hr
        want = hr.split(inp["csr_indptr"].numpy(), inp["csr_indices"].numpy(), ITEMS, 0.2, 5, 1)
        flat = flatten_np(want)
        got = [res[0].numpy(), res[1].numpy()[:int(res[0][-1])], res[2].numpy(), res[3].numpy()[:int(res[2][-1])]]
        assert len(flat) == 4 and all(np.array_equal(g, w) for g, w in zip(got, flat)), "holdout_split differs from tests/holdout_ref.split"

    return _util("holdout-split", ("sdrm_holdout_split",), make, call, anchor=anchor)


def flatten_np(x, out=None):
    out = [] if out is None else out
    if isinstance(x, np.ndarray):
        out.append(x)
    elif isinstance(x, (tuple, list)):
        for y in x:
            flatten_np(y, out)
    return out


def _split_on_host(m):
    import holdout_ref as hr
    return flatten_np(hr.split(m.indptr.astype(np.int64), m.indices.astype(np.int32), ITEMS, 0.2, 5, 1))


def case_rank_metrics(b=33):
    m = _feed(b)
    ks = (1, 5, 10)

    def make(device):
        tp, ti, hp, hi = _split_on_host(m)
        return dict(scores=_rnd(device, 8, b, ITEMS), tr_indptr=_dev(tp, device, torch.int64), tr_indices=_dev(ti, device, torch.int32),
                    he_indptr=_dev(hp, device, torch.int64), he_indices=_dev(hi, device, torch.int32))

    def call(e, x, alloc):
        e._rank_tables(ks)   # (the discount tables are cached per engine: made before the call, as an epoch loop has them)
        return e.rank_metrics(x["scores"], _csr(x, m.shape, "he"), _csr(x, m.shape, "tr"), ks=ks)

    def anchor(inp, res):   # oracle/rank_metrics_ref.py, exactly (tests/test_rank_metrics.py: nan pattern and values equal)
        import scipy.sparse as sp
        from oracle import rank_metrics_ref
        mk = lambda p: sp.csr_matrix((np.ones(len(inp[p + "_indices"]), np.float64), inp[p + "_indices"].numpy(), inp[p + "_indptr"].numpy()), shape=m.shape)
        rec, ndcg = rank_metrics_ref.rank_metrics(inp["scores"].numpy(), mk("he"), mk("tr"), ks=ks)
        for got, want in ((res[0].numpy(), rec), (res[1].numpy(), ndcg)):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])

    return _util("rank-metrics", ("sdrm_rank_metrics",), make, call, anchor=anchor, bitwise=False, feed=False)


def case_eval_holdout(b=33):
    m = _feed(b)

    def make(device):
        tp, ti, hp, hi = _split_on_host(m)
        return dict(_vae(device), tr_indptr=_dev(tp, device, torch.int64), tr_indices=_dev(ti, device, torch.int32),
                    he_indptr=_dev(hp, device, torch.int64), he_indices=_dev(hi, device, torch.int32))

    def call(e, x, alloc):
        e._rank_tables((5,))
        logits = alloc(b, ITEMS)
        scores = e.vae_eval_holdout(*(x[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")), _csr(x, m.shape, "tr"), _csr(x, m.shape, "he"), 5,
                                    "ndcg", batch=max(1, b // 2), logits=logits)
        return scores, logits

    def anchor(inp, res):   # tests/vae_eval_ref.py: the eval-mode logits in fp64, normwise at tests/test_vae_eval_half.py's TOL
        import scipy.sparse as sp
        import vae_eval_ref as er
        train = sp.csr_matrix((np.ones(len(inp["tr_indices"])), inp["tr_indices"].numpy(), inp["tr_indptr"].numpy()), shape=m.shape)
        want = er.logits([inp[k].numpy() for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")], train)
        assert float(np.linalg.norm(res[1].numpy() - want) / np.linalg.norm(want)) <= 1e-4

    return _util("vae-eval-holdout", ("sdrm_vae_eval_holdout",), make, call, anchor=anchor)


def case_svd(b=33):
    m = _feed(b)

    def make(device):
        import svd_eval_ref as ser
        return dict(_csr_inputs(m, device), **_csc_inputs(m, device), q0=_dev(ser.start_panel(ITEMS, 7), device))

    def call(e, x, alloc):
        comps, sigma = e.svd_fit(_csr(x, m.shape), _csr(x, m.shape, "csc"), n_components=4, n_iter=2, q0=x["q0"])
        alloc.delay_again()
        return comps, sigma, e.svd_scores(_csr(x, m.shape), comps, row0=0, b=b, check=False)

    def anchor(inp, res):   # tests/svd_eval_ref.py: the same iteration restated, at tests/test_svd_eval.py's BAR on the reconstruction
        import svd_eval_ref as ser
        v_ref, s_ref = ser.fit(m, 4, 2, inp["q0"].numpy())
        a = m.toarray().astype(np.float64)
        assert ser.normwise(ser.scores(a, res[0].numpy()), ser.scores(a, v_ref).astype(np.float64)) <= 1e-4
        assert ser.normwise(res[1].numpy(), ser.scores(a, v_ref).astype(np.float64)) <= 1e-4

    return _util("svd", ("sdrm_svd_fit", "sdrm_svd_scores"), make, call, nosync=("sdrm_svd_scores",), syncs=("sdrm_svd_fit",), anchor=anchor)


def case_svd_scores(b=33):
    m = _feed(b)

    def make(device):
        return dict(_csr_inputs(m, device), comps=_rnd(device, 9, 4, ITEMS))

    def call(e, x, alloc):
        return e.svd_scores(_csr(x, m.shape), x["comps"], row0=0, b=b, check=False)

    def anchor(inp, res):   # tests/svd_eval_ref.py: (A V^T) V in fp64, normwise at tests/test_svd_eval.py's fp32 bar
        import svd_eval_ref as ser
        assert ser.normwise(res[0].numpy(), ser.scores(m.toarray().astype(np.float64), inp["comps"].numpy().astype(np.float64))) <= 1e-5

    return _util("svd-scores", ("sdrm_svd_scores",), make, call, anchor=anchor)


def case_nmf(b=33, k=5):
    import ctypes as C
    m = _feed(b)

    def make(device):
        rng = np.random.default_rng(11)
        return dict(_csr_inputs(m, device), **_csc_inputs(m, device), w0=_dev(rng.random((b, k)), device), h0=_dev(rng.random((k, ITEMS)), device),
                    comps=_dev(rng.standard_normal((k, ITEMS)).astype(np.float32), device))

    def call(e, x, alloc):
        csr, csc = _csr(x, m.shape), _csr(x, m.shape, "csc")
        # sdrm_nmf_init on its own (the wrapper makes it behind a synchronising svd_fit): components from the caller, sigma on the host
        sigma = np.linspace(3.0, 1.0, k)
        w_init, ht_init = alloc(b, 16, dtype=torch.float64), alloc(ITEMS, 16, dtype=torch.float64)
        w_init[:, k:] = 0    # (the contract: columns k .. 15 are zero on entry; the k result columns stay poisoned)
        ht_init[:, k:] = 0
        e._check(e.lib.sdrm_nmf_init(e._h, C.c_void_p(csr[0].data_ptr()), C.c_void_p(csr[1].data_ptr()), None, b, ITEMS, int(csr[1].numel()), k,
                                     C.c_void_p(x["comps"].data_ptr()), sigma.ctypes.data_as(C.c_void_p), C.c_void_p(w_init.data_ptr()),
                                     C.c_void_p(ht_init.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sdrm_nmf_init")
        w, h, n_iter, viol = e.nmf_fit(csr, csc, n_components=k, max_iter=4, tol=0.0, init=(x["w0"], x["h0"]), check=False)
        alloc.delay_again()   # (the Python wrapper of nmf_fit reads n_iter back: the C call had returned before that)
        return w_init, ht_init, w, h, n_iter, viol, e.nmf_scores(w, h, row0=0, b=b, check=False)

    def anchor(inp, res):   # tests/nmf_ref.py: the same coordinate descent in fp64, normwise at tests/test_nmf_eval.py's SOLVER_BAR
        import nmf_ref
        w, h = nmf_ref.fit(m.astype(np.float64), inp["w0"].numpy(), inp["h0"].numpy(), max_iter=4, tol=0.0)[:2]
        bar = min(100 * 1.81e-13, 1e-10)
        assert nmf_ref.normwise(res[2].numpy(), w) <= bar and nmf_ref.normwise(res[3].numpy(), h) <= bar

    return _util("nmf", ("sdrm_nmf_init", "sdrm_nmf_fit", "sdrm_nmf_scores"), make, call, anchor=anchor)


def case_nmf_scores(b=33, k=5):
    def make(device):
        rng = np.random.default_rng(12)
        return dict(w=_dev(rng.random((b, k)), device), h=_dev(rng.random((k, ITEMS)), device))

    def call(e, x, alloc):
        return e.nmf_scores(x["w"], x["h"], row0=0, b=b, check=False)

    def anchor(inp, res):   # W H in fp64, rounded once: within one ulp of numpy's product (tests/test_nmf_eval.py)
        want = (inp["w"].numpy() @ inp["h"].numpy()).astype(np.float32)
        assert (np.abs(res[0].numpy() - want) <= np.spacing(np.abs(want))).all()

    return _util("nmf-scores", ("sdrm_nmf_scores",), make, call, anchor=anchor)


def _neumf_inputs(device):
    import neumf_ref as nr
    return {f"w{i:02d}": _dev(v, device) for i, v in enumerate(nr.weights(FACTOR, NEUMF_USERS, ITEMS, 99).values())}


def _neumf_list(x, prefix="w"):
    return [x[f"{prefix}{i:02d}"] for i in range(12)]


def case_neumf_eval(b=33):
    def make(device):
        users = np.arange(b, dtype=np.int32) * 9 % NEUMF_USERS
        return dict(_neumf_inputs(device), users=_dev(users, device), items=_dev((users * 7 % ITEMS).astype(np.int32), device),
                    labels=_dev((users % 2).astype(np.float32), device))

    def call(e, x, alloc):
        w = _neumf_list(x)
        return e.neumf_scores(w, x["users"], check=False), e.neumf_pair_logits(w, x["users"], x["items"], labels=x["labels"], check=False)

    def anchor(inp, res):   # tests/neumf_ref.py forward in fp64, normwise at the project's fp32 bar
        import neumf_ref as nr
        w = {n: inp[f"w{i:02d}"].numpy() for i, n in enumerate(nr.NAMES)}
        assert nr.normwise(res[0].numpy(), nr.scores64(w, inp["users"].numpy(), np.arange(ITEMS))) <= 1e-4
        assert nr.normwise(res[1].numpy(), nr.forward64(w, inp["users"].numpy(), inp["items"].numpy())) <= 1e-4

    def prepare(e, staging):
        e.neumf_scores(_neumf_list(staging), torch.arange(33, dtype=torch.int32, device=e.device))

    return _util(f"neumf-eval-{b}", ("sdrm_neumf_scores", "sdrm_neumf_pair_loss"), make, call, anchor=anchor,
                 pools=("warm", "cold") if b == 33 else ("regrow",), prepare=prepare)


def case_neumf_train(n=40, batch=16):
    def make(device):
        import neumf_train_ref as ntr
        d = _neumf_inputs(device)
        for i in range(12):
            d[f"m{i:02d}"], d[f"v{i:02d}"] = torch.zeros_like(d[f"w{i:02d}"]), torch.zeros_like(d[f"w{i:02d}"])
        d["triples"] = _dev(ntr.triples(NEUMF_USERS, ITEMS, n, 3), device)
        return d

    def call(e, x, alloc):
        w, m, v = _neumf_list(x), _neumf_list(x, "m"), _neumf_list(x, "v")
        losses = e.neumf_train_steps(w, m, v, x["triples"], batch, 0, lr=UTIL_LR, p_drop=P_DROP, seed=SEED, call_id=2, check=False)
        return losses, w, m, v

    def anchor(inp, res):
        """tests/neumf_train_ref.py::step64 with the engine's Philox keep masks restated, chained through tests/vae_adam_ref.py::adam_step:
        every step's loss at tests/test_neumf_train.py's TOL, the final weights and moments at its Adam bars."""
        import neumf_train_ref as ntr
        import vae_adam_ref as var
        p0 = {name: inp[f"w{i:02d}"].numpy() for i, name in enumerate(ntr.NAMES)}
        p = {k: a.astype(np.float64) for k, a in p0.items()}
        mm, vv = ({k: np.zeros_like(a) for k, a in p.items()} for _ in range(2))
        tri = inp["triples"].numpy()
        for step, lo in enumerate(range(0, n, batch)):
            hi = min(n, lo + batch)
            r = ntr.step64(p, tri[lo:hi], ntr.philox_keep(SEED, 2, lo, hi - lo, FACTOR, P_DROP), p_drop=P_DROP)
            assert abs(float(res[0][step]) - r["loss"]) <= 1e-4 * abs(r["loss"]), (step, float(res[0][step]), r["loss"])
            for name in ntr.NAMES:
                p[name], mm[name], vv[name] = var.adam_step(p[name], r["grads"][name], mm[name], vv[name], step + 1, UTIL_LR)
        for i, name in enumerate(ntr.NAMES):
            _adam_bars(res[1 + i].numpy(), res[13 + i].numpy(), res[25 + i].numpy(), p0[name], (p[name], mm[name], vv[name]), name)

    return _util("neumf-train", ("sdrm_neumf_train_steps",), make, call, anchor=anchor)


def case_mlp(n_users=20, n=20, batch=16):
    from sdrm_amd.engine import Engine
    m = _feed(n_users)
    shapes = Engine.mlp_shapes(n_users, ITEMS)

    def make(device):
        rng = np.random.default_rng(13)
        d = _csr_inputs(m, device)
        for i, shape in enumerate(shapes):
            d[f"w{i}"] = _dev((rng.standard_normal(shape) * 0.05).astype(np.float32), device)
            d[f"m{i}"], d[f"v{i}"] = torch.zeros_like(d[f"w{i}"]), torch.zeros_like(d[f"w{i}"])
        d["rows"] = _dev(rng.permutation(n_users)[:n].astype(np.int64), device)
        return d

    def call(e, x, alloc):
        w, mm, v = ([x[f"{t}{i}"] for i in range(9)] for t in "wmv")
        losses = e.mlp_train_steps(w, mm, v, _csr(x, m.shape), x["rows"], batch=batch, step0=0, lr=UTIL_LR, p_drop=P_DROP, seed=SEED, call_id=1, check=False)
        out, sse = e.mlp_eval(w, _csr(x, m.shape), rows=x["rows"], batch=8, sse=True, check=False)
        return losses, w, mm, v, out, sse

    def anchor(inp, res):
        """tests/mlp_eval_ref.py::step64 with the engine's Philox keep masks restated, chained through its keras_adam: every step's loss at
        tests/test_mlp_train.py's TOL, the final tensors and moments at its Adam bars; then tests/mlp_eval_fwd_ref.py's oracle of the
        eval-mode forward (step64 with every unit kept, its sigmoid64) on the weights the device trained: probabilities normwise and the
        SSE relative at tests/test_mlp_eval.py's TOL."""
        import mlp_eval_fwd_ref as fr
        import mlp_eval_ref as mr
        p0 = {name: inp[f"w{i}"].numpy() for i, name in enumerate(mr.NAMES)}
        p = {k: a.astype(np.float64) for k, a in p0.items()}
        mm, vv = ({k: np.zeros_like(a) for k, a in p.items()} for _ in range(2))
        x, rows = m.toarray(), inp["rows"].numpy()
        for step, lo in enumerate(range(0, n, batch)):
            hi = min(n, lo + batch)
            r = mr.step64(p, x[rows[lo:hi]], mr.philox_keep(SEED, 1, lo, hi - lo, P_DROP), p_drop=P_DROP)
            assert abs(float(res[0][step]) - r["loss"]) <= 1e-4 * abs(r["loss"]), (step, float(res[0][step]), r["loss"])
            for name in mr.NAMES:
                p[name], mm[name], vv[name] = mr.keras_adam(p[name], r["grads"][name], mm[name], vv[name], step + 1, lr=UTIL_LR, eps=1e-7)
        for i, name in enumerate(mr.NAMES):
            _adam_bars(res[1 + i].numpy(), res[10 + i].numpy(), res[19 + i].numpy(), p0[name], (p[name], mm[name], vv[name]), name)
        trained = {name: res[1 + i].numpy() for i, name in enumerate(mr.NAMES)}
        xe = x[rows]
        y = mr.step64(trained, xe, np.ones((len(rows), mr.KEEP_COLS)), p_drop=0.0)["y"]
        prob = fr.sigmoid64(y)
        assert mr.normwise(res[28].numpy(), prob) <= 1e-4
        sse = float(((prob - xe) ** 2).sum())
        assert abs(float(res[29][0]) - sse) <= 1e-4 * sse

    return _util("mlp", ("sdrm_mlp_train_steps", "sdrm_mlp_eval"), make, call, anchor=anchor)


def build_cases():
    row = (136, 136, 12, 2)
    cases = [case_params_roundtrip()]
    for mode in ("explicit", "philox"):
        for one_call in (False, True):
            cases += [case_train("narrow", (40, 40, 9, 1), 33, mode, one_call),
                      case_train("tile0", (96, 80, 7, 1), 70, mode, one_call, tile=0), case_train("tile4", (96, 80, 7, 1), 70, mode, one_call, tile=4),
                      case_train("row", row, 75, mode, one_call, tile="row"), case_train("row-layers", row, 75, mode, one_call, tile="row-layers"),
                      case_train("row48", row, 75, mode, one_call, tile="row48"), case_train("row48x2", row, 333, mode, one_call, tile="row48x2")]
        for multires in (False, True):
            cases += [case_sample("narrow", (20, 64, 11, 0), 70, mode, multires),
                      case_sample("gemm", row, 400, mode, multires, sample_persist=0),
                      case_sample("chains2", row, 403, mode, multires, chains=2, sample_persist=0),
                      case_sample("chains4", row, 403, mode, multires, chains=4, sample_persist=0),
                      case_sample("persist19", row, 19, mode, multires), case_sample("persist352", row, 352, mode, multires)]
    # the resumable form with the caller's randoms: with a caller's Tj sdrm_sample_begin is the call that waits (include/sdrm_hip.h)
    cases += [case_sample("begin-chains2", row, 403, "explicit", multires, chains=2, resumable=True, sample_persist=0) for multires in (False, True)]
    cases += [case_backward_buckets(), case_inference(), case_sharded(), case_profile()]
    cases += [case_sample_resumable("per-layer-detach", "per-layer", 1), case_sample_resumable("per-layer-chains2", "per-layer", 2),
              case_sample_resumable("row48-detach", "row48", 1), case_sample_resumable("row48-chains2", "row48", 2)]
    cases += [case_csr_rows_to_dense(), case_equal_sparsity(), case_equal_sparsity_csr(), case_csr_transpose_vstack(), case_vae_decode(),
              case_vae_encode(), case_multinomial_nll(), case_input_layer(), case_latent(), case_decoder_nll(), case_vae_adam(), case_holdout_split(),
              case_rank_metrics(), case_eval_holdout(), case_svd(), case_svd_scores(), case_nmf(), case_nmf_scores(), case_neumf_eval(),
              case_neumf_train(), case_mlp()]
    # regrow: b = 33 on the default stream, then b = 300 on the side stream - padded operand buffers (vae_decode, decoder head), split-K slabs
    # (input layer), integer workspaces (csr_transpose / csr_vstack, the NeuMF id lists)
    cases += [case_vae_decode(300), case_decoder_nll(300), case_input_layer(300), case_csr_transpose_vstack(300), case_neumf_eval(300)]
    return cases


CASES = build_cases()
