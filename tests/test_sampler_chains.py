"""Every transition of the sampler's row-chain scheduling (csrc/sdrm_hip.hip: ChainSched) in one resumable sampling call, at the
smallest shapes that take them: a net of padded width 160 (L = W = 136, inside the row-owned kernels' envelope), 400 sampled rows
(above the persistent sampler's 352: one launch per layer) as one, two and three chains - 448, 256 + 144 and 192 + 192 + 16 rows,
the last chain ragged - and train steps of 64 users between its steps.  Whatever the chains wait for, and whichever stream they run
on, the call reads its own snapshot of the net and the generator is keyed by row: the latents are those of the uninterrupted call
and the parameters those of the same train steps with no sampling call, bit for bit.  Needs a real MI355X: `pytest -m gpu`."""
import itertools

import pytest
import torch

from sdrm_amd import synth

pytestmark = pytest.mark.gpu

L, W, T, H = 136, 136, 40, 2
N, B = 400, 64
ND = 0.9
LR = 1e-3


def _walk(e, x0, lr, chunk, stop_after=7):
    """The events of the walk, `chunk()` between them (sampling steps; nothing at all for the run without a sampling call)."""
    def step(k):
        e.train_step(x0, lr, seed=3, step=k)

    chunk()
    e.debug_set(rowchain=0, rows48=0)       # 1: a per-layer train step (a small call's chain: detach armed)
    step(0)
    chunk()
    step(1)                                 # 2: two train steps in a row
    step(2)
    chunk()
    e.debug_set(rowchain=2)                 # 3: a row-owned step (the chains wait for its weight gradients)
    step(3)
    if stop_after == 3:
        return
    chunk()
    step(4)                                 # 4: a row-owned step followed at once by a per-layer one
    e.debug_set(rowchain=0)
    step(5)
    chunk()
    e.profile_begin(capacity=256)           # 5: an event profile (the chains one after the other on the caller's stream)
    chunk()
    e.profile_end()
    chunk()
    e.get_params()                          # 6: a join by an unrelated entry point
    chunk()
    e.debug_set(rowchain=2)                 # 7: a row-owned step, one call per phase
    e.train_forward(x0, seed=3, step=6)
    e.train_backward_begin()
    e.train_backward_finish()
    e.adam_step(lr)


@pytest.fixture(scope="module")
def case(engine_cls):
    """Start parameters, the train batch, and the parameters after the walk's train steps on an engine with no sampling call."""
    flat = synth.flatten_params(synth.init_params(L, W, T, H, seed=41), H)
    x0 = synth.synth_latents(B, L, seed=12)
    e = engine_cls(L, W, T, H, N)
    e.set_params(flat)
    _walk(e, x0, LR, lambda: None)
    params = e.get_params().cpu()
    e.close()
    return dict(flat=flat, x0=x0, params=params)


@pytest.mark.parametrize("chains", [1, 2, 3])
@pytest.mark.parametrize("multires", [False, True])
def test_every_chain_transition_changes_no_bit(engine_cls, case, multires, chains):
    """One call driven by sample_steps(k), k cycling through 1, 2, 3, with the events of `_walk` between the chunks: several train
    steps in a row, row-owned steps beside a detached chain and beside forked ones, a row-owned step followed by a per-layer one, an
    event profile, a join by sdrm_get_params, a three-call train step.  Then the same call abandoned by a new sdrm_sample_begin after
    event 3 (train steps at lr = 0: the net stays what it is), with a row-owned step beside an armed detach, a profile that begins
    while the detach is armed, and the detach armed again behind it."""
    flat, x0 = case["flat"], case["x0"]
    kw = dict(nd=ND, multires=multires, seed=17, call_id=3, row0=1358)
    e = engine_cls(L, W, T, H, N).debug_set(chains=chains)
    e.set_params(flat)
    ref = e.sample(N, **kw).cpu()
    assert e.sampler_chains == chains
    e.close()

    e = engine_cls(L, W, T, H, N).debug_set(chains=chains)
    e.set_params(flat)
    ks = itertools.cycle((1, 2, 3))

    def chunk():
        return e.sample_steps(next(ks))

    e.sample_begin(N, **kw)
    _walk(e, x0, LR, chunk)
    tail = 0
    while chunk() > 0:
        tail += 1
    assert tail >= 1                        # the walk ended inside the call
    out = e.sample_end().cpu()
    assert e.sampler_chains == chains
    assert torch.equal(out, ref)
    assert torch.equal(e.get_params().cpu(), case["params"])

    # the second walk
    e.set_params(flat)
    e.sample_begin(N, **kw)
    _walk(e, x0, 0.0, chunk, stop_after=3)
    e.sample_begin(N, **kw)                 # abandons the call above, its chains in flight
    e.train_step(x0, 0.0, seed=3, step=7)   # row-owned, beside a call still on the caller's stream
    e.profile_begin(capacity=256)
    chunk()
    e.profile_end()
    e.train_step(x0, 0.0, seed=3, step=8)
    while chunk() > 0:
        pass
    assert torch.equal(e.sample_end().cpu(), ref)
    assert e.sampler_chains == chains
    e.close()
