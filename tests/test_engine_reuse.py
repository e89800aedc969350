"""One long-lived engine across batch sizes that cross the automatic path thresholds (csrc/sdrm_hip.hip: plan_step, chains_for,
sample_persist_fits) - what a production epoch does every time its short last batch arrives.  Needs a real MI355X.

The paths of the train step share U, pre, act, Y, dY, dA, the weight-gradient slabs and the loss partials, in three stacked-row orders
and with different row counts; the column-split hand-shake counters and the persistent sampler's row-tile counters count on from
launch to launch.  Every other test creates an engine for ONE batch size; here engine `A` lives through a walk of sizes, and before
every checked call a fresh TWIN of the same max_rows is given A's parameters and Adam state and runs the same call: same device, same
plan, same arithmetic, no history - so everything the call returns must be equal BIT FOR BIT.  Between the checked calls A alone runs a
"loud" call (a full-size forward of inputs scaled by 1e3) so that whatever a path leaves behind is far above any bar.  `Engine.last_plan()`
pins which kernels each size really took: a retuned threshold fails these tests instead of quietly moving what they cover.  At the first
visit of every plan the step is also held to the CPU oracle (the bars of test_hip_parity.train_step_vs_oracle), so that the twin cannot
share a fault with A.

sdrm_get_preacts is answered until the parameters change and refused (SDRM_ERR_STATE) afterwards (include/sdrm_hip.h,
test_preactivations_after_a_whole_step): behind a fused step or an Adam step the walks require the SAME outcome of A and the twin -
the same bits where the read is answered, a refusal of every layer on both where it is not.

The padding rows behind a row-owned step's last group are read by the 64-row-tile weight gradients only, and behind a row-owned forward
those run in the two-call backward (sdrm_train_backward_begin / _finish: what every sharded step takes); a one-call backward takes the
strip-owned launch, which does not read them.  test_batch_size_walk_two_call_backward is the walk that sees such rows: a build without the
48-row chain's pad-row sweep (csrc/rows48.h) passes the fused walk and fails that one at its first column-split step (B = 1300:
nearly every gradient element differs).  On the per-layer path the padding rows are guarded twice - k_stage zero-fills them in U and
k_loss_seed zero-fills dY's tail rows, so every product a weight gradient forms with such a row has an exact zero in it: a build without
k_stage's zero-fill passes every walk, whose leftovers are finite, and fails test_per_layer_step_behind_non_finite_rows (0 x inf)."""
import numpy as np
import pytest
import torch

from sdrm_amd import synth
from test_hip_parity import TOL, close, engine_branch_masks, per_tensor, rel_l2, rel_max

gpu = pytest.mark.gpu        # per test: the host arithmetic below runs in the CPU suite

WIDE = (148, 148, 7, 1)      # padded width 160 = ten column tiles of 16: the 48-row kernels' shared-tile form; 148 = 9 x 16 + 4: the compact
WIDE_ROWS = 4928             # last K-step (rc_light_klast) - the smallest kind of net that reaches both, inside the row-owned envelope
NARROW = (40, 40, 93, 5)
NARROW_ROWS = 850
LR, ND = 1e-3, 0.9

WALK = [4928, 1300, 4096, 2049, 2048, 33, 2545, 1281, 1, 4897, 700, 3000, 4928,
        4097, 4896]          # ... and the two edges of the per-layer band between the 48-row and the 96-row groups
TRAJECTORY_STEPS = 13        # the oracle follows the walk this far (an oracle step of ~4900 users is a second of CPU time)
WALK_THREE_PHASE = [4928, 1281, 2545, 33, 4897]
TWO_CALL_ROWS = 4992         # 156 groups of 32 users: room for 4960 users = 155 groups, whose 14880 stacked rows are no multiple of 64
WALK_TWO_CALL = [4960, 1300, 2577, 2049, 1281, 4960, 33, 4897]   # every row-owned size here but the last leaves padding rows
WALK_NARROW = [850, 5, 129, 16, 17, 850]
SAMPLE_WALK = [7040, 19, 353, 352, 4097, 339, 7040]

PER_LAYER, SKINNY = ("per_layer", 1, "tiles"), ("skinny", 1, "skinny_own")


def expected_train_plan(B, split_ok):
    """(train_path, parts, dgrad) of a step of B users on the WIDE net, from the documented size rules (include/sdrm_hip_debug.h:
    sdrm_debug_set_rowchain / _rows48 / _rows48_split; the row-owned dgrad chain follows every row-owned forward of such a net)."""
    if B >= 4897:                       # 96-row groups: one round of the chip from 154 groups of 32 users on; their dgrad chain wants
        rows = 96 * -(-B // 32)         # the stacked rows, padded to the 64-row granule, to be whole 96-row groups (else: tile dgrads)
        return ("row96", 1, "chain" if (-(-rows // 64) * 64) % 96 == 0 else "tiles")
    if 2545 <= B <= 4096:               # 48-row groups: 160 .. 256 groups of 16 users
        return ("row48", 1, "chain")
    if 1281 <= B <= 2048:               # two work-groups per 48-row group
        return ("row48", 2, "chain") if split_ok else PER_LAYER
    return PER_LAYER                    # up to 1280, 2049 .. 2544, 4097 .. 4896


def test_walks_cover_every_path_and_both_sides_of_every_threshold():
    """The walks are what this module says they are (host arithmetic only; kept beside the GPU tests that use it).  Every checked
    step follows a loud call of max_rows users (96-row groups, grouped by 32) or of 3 max_rows plain rows: more rows than any step."""
    for lo in (1280, 2048, 2544, 4096, 4896):                                            # the documented thresholds ...
        assert expected_train_plan(lo, True)[:2] != expected_train_plan(lo + 1, True)[:2]
        below = [B for B in WALK if B <= lo and expected_train_plan(B, True) == expected_train_plan(lo, True)]
        above = [B for B in WALK if B > lo and expected_train_plan(B, True) == expected_train_plan(lo + 1, True)]
        assert below and above, (lo, below, above)                                       # ... each with a step on both of its sides
    assert {1281, 2048, 2049, 2545, 4096, 4097, 4896, 4897} <= set(WALK) and max(WALK) == WIDE_ROWS   # the exact edges, but for 1280 / 2544
    every = {("row96", 1), ("row48", 2), ("row48", 1), ("per_layer", 1)}
    assert {expected_train_plan(B, True)[:2] for B in WALK} == every
    assert {expected_train_plan(B, True)[:2] for B in WALK_THREE_PHASE} == every
    # the column-split geometry (row groups of the launch) changes and comes back: 1300 -> 2048 -> 1281
    assert [-(-B // 16) for B in WALK if expected_train_plan(B, True)[1] == 2] == [82, 128, 81]
    # without the block -> XCD mapping the column-split sizes take the per-layer path
    assert expected_train_plan(1300, False) == PER_LAYER
    # the two-call walk: every path, and padding rows (stacked rows short of the 64-row granule) behind each kind of row-owned step
    assert {expected_train_plan(B, True)[:2] for B in WALK_TWO_CALL} == every and max(WALK_TWO_CALL) < TWO_CALL_ROWS
    padded = {expected_train_plan(B, True)[:2] for B in WALK_TWO_CALL
              if expected_train_plan(B, True)[0] != "per_layer" and ({"row96": 96 * -(-B // 32), "row48": 48 * -(-B // 16)}[expected_train_plan(B, True)[0]]) % 64}
    assert padded == {("row96", 1), ("row48", 1), ("row48", 2)}, padded
    assert expected_train_plan(4960, True) == ("row96", 1, "tiles") and expected_train_plan(4897, True) == ("row96", 1, "chain")
    # the ranges above are the ones the header documents (the table is not only checked against itself)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrm_hip_debug.h")).read()
    for text in ("at least 154 groups of 32 users", "160..256 groups: 2545..4096 users", "1281..2048 users: 2 work-groups per group"):
        assert text in header, text


# ------------------------------------------------------------------------------------------------ helpers
def same_bits(a, b, what):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    if not torch.equal(a, b):
        d = (a != b).reshape(-1)
        first = int(torch.nonzero(d)[0])
        worst = float((a.double() - b.double()).abs().reshape(-1)[d].nan_to_num(nan=float("inf")).max())
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ from the fresh twin's, the first at flat index "
                             f"{first} (of shape {tuple(a.shape)}); largest difference {worst:.3e}")
    assert bool(torch.isfinite(a).all()), (what, "not finite")


def read_preacts(e, B):
    """Every layer's pre-activations, or "refused" when the library refuses them - then for every layer."""
    from sdrm_amd.engine import SdrmError
    got = []
    try:
        for k in range(e.H + 1):
            got.append(e.preacts(k, B))
    except SdrmError as err:
        assert not got and "SDRM_ERR_STATE" in str(err), (len(got), str(err))
        for k in range(e.H + 1):
            with pytest.raises(SdrmError):
                e.preacts(k, B)
        return "refused"
    return got


def same_preacts(pa, pf, what):
    if isinstance(pa, str) or isinstance(pf, str):
        assert pa == pf, (what, "one engine answered the read, the other refused it")
        return
    for k, (x, y) in enumerate(zip(pa, pf)):
        same_bits(x, y, f"{what}: pre-activations of layer {k}")


def make_twin(engine_cls, a, dims, max_rows, **debug):
    f = engine_cls(*dims, max_rows).debug_set(**debug)
    f.set_params(a.get_params())
    f.set_adam_state(*a.get_adam_state())
    return f


def same_state(a, f, what):
    same_bits(a.get_params(), f.get_params(), what + ": parameters")
    (ma, va, sa), (mf, vf, sf) = a.get_adam_state(), f.get_adam_state()
    assert sa == sf, (what, sa, sf)
    same_bits(ma, mf, what + ": Adam first moments")
    same_bits(va, vf, what + ": Adam second moments")


class Loud:
    """The calls engine A alone makes between the checked ones: a train forward that is never back-propagated, at max_rows users, of
    an x0 scaled by 1e3 (a pending forward is dropped by whatever comes next), alternating with a plain forward of 3 max_rows rows."""

    def __init__(self, dims, max_rows):
        L, T = dims[0], dims[2]
        self.x = torch.from_numpy(synth.synth_latents(3 * max_rows, L, seed=900)).cuda() * 1e3
        self.t = torch.from_numpy(np.random.RandomState(901).randint(1, T + 1, size=3 * max_rows)).cuda()
        self.rows = max_rows

    def __call__(self, a, k):
        if k % 2 == 0:
            a.train_forward(self.x[:self.rows], seed=77, step=k, nd=ND)
        else:
            a.forward(self.x, self.t, seed=77, step=k)


def step_inputs(dims, B, k):
    L, _, T, _ = dims
    x0 = synth.synth_latents(B, L, seed=1000 + k)
    eps, t, keep = synth.synth_train_randoms(B, L, T, ND, seed=2000 + k)
    return x0, eps, t, keep


def oracle_of(a, dims):
    from oracle import sdrm_oracle as orc
    L, W, T, H = dims
    return orc.Oracle(L, W, T, H, synth.unflatten_params(a.get_params().cpu().numpy(), L, W, T, H))


def oracle_anchor(engine_cls, a, dims, max_rows, inputs, want_plan, what, **debug):
    """The step `inputs` on the parameters A holds now, against the CPU oracle - as test_hip_parity.train_step_vs_oracle does it:
    three-phase form on a twin, the oracle's backward on the engine's own PReLU branch choice, TOL normwise.  Returns the oracle's
    (loss, gradients, outputs) for the caller to hold A's fused step to as well."""
    x0, eps, t, keep = inputs
    B = x0.shape[0]
    f = make_twin(engine_cls, a, dims, max_rows, **debug)
    o = oracle_of(a, dims)
    f.train_forward(x0, noise=eps, t=t, keep=keep)
    assert tuple(f.last_plan()[:3]) == want_plan, (what, f.last_plan())
    caches = []
    o.loss_and_grads(x0, eps, t, list(keep), caches=caches)
    branch, flips = engine_branch_masks(f, o, caches, B)
    loss_ref, grads_ref, outs_ref, _ = o.loss_and_grads(x0, eps, t, list(keep), neg_override=branch)
    loss = float(f.train_backward().cpu())
    ref = (float(loss_ref), grads_ref, outs_ref)
    against_oracle(loss, f.train_outputs(B), f.get_grads(), ref, dims, what + " (three phases on a twin)")
    f.close()
    return ref


def against_oracle(loss, psq, grads, ref, dims, what):
    loss_ref, grads_ref, outs_ref = ref
    print(f"    oracle {what}: loss {loss:.7f} against {loss_ref:.7f}")
    assert abs(loss - loss_ref) <= TOL * abs(loss_ref), (what, loss, loss_ref)
    psq = psq.cpu().numpy()
    for j, tag in enumerate("PSQ"):
        assert close(psq[j], outs_ref[j].numpy()), (what, tag, rel_l2(psq[j], outs_ref[j].numpy()), rel_max(psq[j], outs_ref[j].numpy()))
    for n, got in per_tensor(grads.cpu().numpy(), dims):
        want = grads_ref[n].numpy().ravel()
        assert rel_l2(got, want) <= TOL and rel_max(got, want) <= TOL, (what, n, rel_l2(got, want), rel_max(got, want))


def fused_walk(engine_cls, dims, max_rows, sizes, want_plan_of, anchor_at, trajectory=False, **debug):
    """Fused train steps of `sizes` users on one engine, each against a fresh twin; want_plan_of(B) names the plan, anchor_at(k, plan,
    seen) says whether step k is held to the oracle."""
    from oracle import sdrm_oracle as orc
    L, W, T, H = dims
    init = synth.init_params(L, W, T, H, seed=61)
    a = engine_cls(*dims, max_rows).debug_set(**debug)
    a.set_params(synth.flatten_params(init, H))
    loud = Loud(dims, max_rows)
    o_traj = orc.Oracle(L, W, T, H, init) if trajectory else None
    seen = []
    for k, B in enumerate(sizes):
        what = f"step {k} (B = {B})"
        inputs = step_inputs(dims, B, k)
        x0, eps, t, keep = inputs
        want = want_plan_of(B)
        loud(a, k)
        ref = oracle_anchor(engine_cls, a, dims, max_rows, inputs, want, what, **debug) if anchor_at(k, B, want, seen) else None
        f = make_twin(engine_cls, a, dims, max_rows, **debug)
        loss_a = float(a.train_step(x0, LR, noise=eps, t=t, keep=keep).cpu())
        loss_f = float(f.train_step(x0, LR, noise=eps, t=t, keep=keep).cpu())
        plan = a.last_plan()
        print(f"  {what}: {plan.train_path} parts {plan.parts} dgrad {plan.dgrad}" + ("  [oracle]" if ref else ""))
        assert tuple(plan[:3]) == want and tuple(f.last_plan()[:3]) == want, (what, plan, f.last_plan(), want)
        assert loss_a == loss_f and np.isfinite(loss_a), (what, loss_a, loss_f)
        grads_a, psq_a = a.get_grads(), a.train_outputs(B)
        same_bits(grads_a, f.get_grads(), what + ": gradients")
        same_bits(psq_a, f.train_outputs(B), what + ": P / S / Q")
        same_preacts(read_preacts(a, B), read_preacts(f, B), what)
        same_state(a, f, what)
        if ref:
            against_oracle(loss_a, psq_a, grads_a, ref, dims, what + " (the long-lived engine's fused step)")
        if o_traj is not None and k < TRAJECTORY_STEPS:
            o_traj.train_step(x0, eps, t, list(keep), LR)
            if k == TRAJECTORY_STEPS - 1:   # informational: Adam's lr / eps slope at a zero gradient makes a many-step trajectory a non-smooth measure
                print(f"  parameters after {k + 1} steps against the oracle's: rel_l2 "
                      f"{rel_l2(a.get_params().cpu().numpy(), o_traj.flat(synth.param_names(H))):.3e} (not asserted)")
        seen.append(want)
        f.close()
    a.close()
    return seen


# ------------------------------------------------------------------------------------------------ the walks
@gpu
def test_batch_size_walk(engine_cls):
    """Fifteen fused steps on one engine: every automatic path entered behind more rows in another row order, every size threshold
    hit on both of its sides, the column-split geometry changed and brought back."""
    probe = engine_cls(*WIDE, 64)
    split_ok = probe.rows48_split_available
    assert probe.rowchain_available
    probe.close()
    seen = fused_walk(engine_cls, WIDE, WIDE_ROWS, WALK, lambda B: expected_train_plan(B, split_ok),
                      lambda k, B, want, seen: want not in seen, trajectory=True)
    assert {p[0] for p in seen} == {"row96", "row48", "per_layer"}
    assert not split_ok or ("row48", 2, "chain") in seen


@gpu
def test_batch_size_walk_three_phase(engine_cls):
    """The same walk through train_forward, train_backward, adam_step: the forward's sums, the pre-activations while they are the
    forward's, and the reads behind the Adam step."""
    dims, sizes = WIDE, WALK_THREE_PHASE
    L, W, T, H = dims
    a = engine_cls(*dims, WIDE_ROWS)
    split_ok = a.rows48_split_available
    a.set_params(synth.flatten_params(synth.init_params(L, W, T, H, seed=62), H))
    loud = Loud(dims, WIDE_ROWS)
    for k, B in enumerate(sizes):
        what = f"step {k} (B = {B})"
        x0, eps, t, keep = step_inputs(dims, B, 50 + k)
        want = expected_train_plan(B, split_ok)
        loud(a, k)
        f = make_twin(engine_cls, a, dims, WIDE_ROWS)
        sums_a = a.train_forward(x0, noise=eps, t=t, keep=keep).clone()
        sums_f = f.train_forward(x0, noise=eps, t=t, keep=keep).clone()
        plan = a.last_plan()
        print(f"  {what}: {plan.train_path} parts {plan.parts} dgrad {plan.dgrad}")
        assert tuple(plan[:3]) == want and tuple(f.last_plan()[:3]) == want, (what, plan, f.last_plan(), want)
        same_bits(sums_a, sums_f, what + ": loss sums of the forward")
        pre_a, pre_f = read_preacts(a, B), read_preacts(f, B)
        assert not isinstance(pre_a, str), (what, "the forward's pre-activations were refused")
        same_preacts(pre_a, pre_f, what + ", behind the forward")
        same_bits(a.train_outputs(B), f.train_outputs(B), what + ": P / S / Q behind the forward")
        loss_a, loss_f = float(a.train_backward().cpu()), float(f.train_backward().cpu())
        assert loss_a == loss_f and np.isfinite(loss_a), (what, loss_a, loss_f)
        same_bits(a.get_grads(), f.get_grads(), what + ": gradients")
        same_preacts(read_preacts(a, B), pre_a, what + ", behind the backward (against the forward's own)")
        a.adam_step(LR)
        f.adam_step(LR)
        same_state(a, f, what)
        same_bits(a.train_outputs(B), f.train_outputs(B), what + ": P / S / Q behind the Adam step")
        same_preacts(read_preacts(a, B), read_preacts(f, B), what + ", behind the Adam step")
        f.close()
    a.close()


@gpu
def test_batch_size_walk_two_call_backward(engine_cls):
    """The walk through train_forward, train_backward_begin, train_backward_finish, adam_step - the backward of every sharded step
    (sdrm_amd/parallel.py).  Behind a row-owned forward its weight gradients are the 64-row-tile launches, which sum over the stacked
    rows PADDED to the tile: the rows behind the last group, which each path clears in its own code (the 48-row chain's pad-row sweep,
    k_loss_seed's tail rows behind the 96-row forward and on the per-layer path).  Each row-owned size comes behind a loud call of more
    rows in another row order, and behind a checked step whose gradients still lie in those rows."""
    dims, sizes, max_rows = WIDE, WALK_TWO_CALL, TWO_CALL_ROWS
    L, W, T, H = dims
    a = engine_cls(*dims, max_rows)
    split_ok = a.rows48_split_available
    a.set_params(synth.flatten_params(synth.init_params(L, W, T, H, seed=66), H))
    loud = Loud(dims, max_rows)
    for k, B in enumerate(sizes):
        what = f"step {k} (B = {B})"
        x0, eps, t, keep = step_inputs(dims, B, 80 + k)
        want = expected_train_plan(B, split_ok)
        loud(a, k)
        f = make_twin(engine_cls, a, dims, max_rows)
        got = []
        for e in (a, f):
            sums = e.train_forward(x0, noise=eps, t=t, keep=keep).clone()
            loss = float(e.train_backward_begin().cpu())
            e.train_backward_finish()
            got.append((sums, loss, e.get_grads(), e.train_outputs(B)))
            e.adam_step(LR)
        plan = a.last_plan()
        print(f"  {what}: {plan.train_path} parts {plan.parts} dgrad {plan.dgrad}")
        assert tuple(plan[:3]) == want and tuple(f.last_plan()[:3]) == want, (what, plan, f.last_plan(), want)
        same_bits(got[0][0], got[1][0], what + ": loss sums of the forward")
        assert got[0][1] == got[1][1] and np.isfinite(got[0][1]), (what, got[0][1], got[1][1])
        same_bits(got[0][2], got[1][2], what + ": gradients of the two-call backward")
        same_bits(got[0][3], got[1][3], what + ": P / S / Q")
        same_state(a, f, what)
        f.close()
    a.close()


@gpu
@pytest.mark.parametrize("B", [33, 700])
def test_per_layer_step_behind_non_finite_rows(engine_cls, B):
    """What k_stage's zero-fill of U's padding rows is for.  Finite leftovers there are harmless - k_loss_seed zero-fills dY's tail rows,
    so they only ever meet exact zeros - but 0 x inf is NaN: a plain forward of rows of +inf leaves non-finite values in the rows of U,
    pre and Y behind the next train step's 3 B stacked rows, up to its padded row count and beyond.  The per-layer step that follows
    must be the fresh twin's, bit for bit, and finite."""
    dims, max_rows = WIDE, 704
    L, W, T, H = dims
    a = engine_cls(*dims, max_rows)
    a.set_params(synth.flatten_params(synth.init_params(L, W, T, H, seed=67), H))
    n = 3 * max_rows
    x = torch.from_numpy(synth.synth_latents(n, L, seed=902)).cuda()
    x[3 * B:] = float("inf")
    a.forward(x, torch.from_numpy(np.random.RandomState(903).randint(1, T + 1, size=n)).cuda(), seed=78, step=0)
    x0, eps, t, keep = step_inputs(dims, B, 90)
    f = make_twin(engine_cls, a, dims, max_rows)
    loss_a = float(a.train_step(x0, LR, noise=eps, t=t, keep=keep).cpu())
    loss_f = float(f.train_step(x0, LR, noise=eps, t=t, keep=keep).cpu())
    assert tuple(a.last_plan()[:3]) == PER_LAYER, a.last_plan()
    assert loss_a == loss_f and np.isfinite(loss_a), (loss_a, loss_f)
    same_bits(a.get_grads(), f.get_grads(), "gradients")
    same_bits(a.train_outputs(B), f.train_outputs(B), "P / S / Q")
    same_state(a, f, "behind the step")
    f.close()
    a.close()


@gpu
@pytest.mark.parametrize("skinny", [1, 2], ids=["fwd4", "fwd16"])
def test_narrow_net_batch_walk(engine_cls, skinny):
    """The narrow nets' step (csrc/skinny_fwd4.h: 4 users per work-group; csrc/skinny_step.h: 16) across batch sizes on one engine:
    more user groups than slab sets, one group, a ragged second one."""
    seen = fused_walk(engine_cls, NARROW, NARROW_ROWS, WALK_NARROW, lambda B: SKINNY, lambda k, B, want, seen: B == 17, skinny=skinny)
    assert seen == [SKINNY] * len(WALK_NARROW)


@gpu
def test_sampling_size_walk(engine_cls):
    """Sampling calls of different sizes on one engine: two row chains from 2560 x 352 elements per layer on, the persistent kernel
    up to 352 rows (its row-tile counters carry on from call to call), the fused reverse update up to 4096 rows; a multi-resolution
    call and a row-owned train step in between."""
    from oracle import philox_ref as pr
    dims = WIDE
    L, W, T, H = dims
    a = engine_cls(*dims, WIDE_ROWS)
    xcd_ok = a.rows48_split_available
    a.set_params(synth.flatten_params(synth.init_params(L, W, T, H, seed=63), H))
    seed, row0 = 0x5EED5EED77, 1000
    big = synth.synth_sample_randoms(7040, L, T, ND, seed=64)

    def checked(what, want_path, want_chains, oracle_randoms=None, **call):
        f = make_twin(engine_cls, a, dims, WIDE_ROWS)
        before = a.launch_count()
        out_a, out_f = a.sample(nd=ND, **call), f.sample(nd=ND, **call)
        launches = a.launch_count() - before
        got = (a.last_plan().sample_path, a.sampler_chains)
        print(f"  {what}: {got[0]}, {got[1]} chain(s), {launches} launches" + ("  [oracle]" if oracle_randoms else ""))
        # sample_path is what sdrm_sample_begin decided: a call that fell back to a launch per layer behind a timed-out hand-shake
        # still reads "persist" - on A and on a twin alike.  The launches tell them apart: a layer per launch is (H + 2) T at the least
        assert got[0] != "persist" or launches < (H + 2) * T, (what, launches)
        assert got == (want_path, want_chains) and (f.last_plan().sample_path, f.sampler_chains) == got, (what, got, want_path, want_chains)
        same_bits(out_a, out_f, what + ": latents")
        if oracle_randoms:
            xT, z, keep, Tj = oracle_randoms
            ref = oracle_of(a, dims).sample(xT, z, keep, Tj).numpy()
            assert close(out_a, ref), (what, rel_l2(out_a.cpu().numpy(), ref), rel_max(out_a.cpu().numpy(), ref))
        f.close()

    for k, n in enumerate(SAMPLE_WALK):
        want_chains = 2 if n * 160 >= 2560 * 352 else 1
        want_path = "persist" if (n <= 352 and want_chains == 1 and xcd_ok) else "per_layer"
        randoms = pr.sample_randoms(seed, k, row0, n, L, T, ND, False)[:3] + (None,) if n in (19, 339) else None
        checked(f"call {k} (n = {n}, Philox)", want_path, want_chains, randoms, n=n, seed=seed, call_id=k, row0=row0)
        if n == 7040:      # the oracle's part of the two-chain calls: explicit randoms (never the persistent kernel)
            xT, z, keep, _ = big
            checked(f"call {k} (n = {n}, explicit randoms)", "per_layer", 2, (xT, z, keep, None) if k == 0 else None, n=n, xT=xT, z=z, keep=keep)
        if n == 353:       # one multi-resolution call between the persistent kernel's neighbours
            xT, z, keep, Tj = synth.synth_sample_randoms(700, L, T, ND, seed=65, multires=True)
            checked("a multi-resolution call of 700 rows", "per_layer", 1, (xT, z, keep, Tj), n=700, multires=True, xT=xT, z=z, keep=keep, Tj=Tj)
        if n == 4097:      # one row-owned train step: the next twins get the parameters it leaves
            x0, eps, t, keep = step_inputs(dims, 4096, 70)
            a.train_step(x0, LR, noise=eps, t=t, keep=keep)
            assert tuple(a.last_plan()[:3]) == ("row48", 1, "chain"), a.last_plan()
    a.close()


@gpu
def test_short_last_batch_through_train_SDRM(engine_cls, tmp_path):
    """The call surface: a loader of 4096 + 1333 users in batches of 4096, two epochs - the 48-row path, the column-split path, and
    again - leaves the parameters of four Engine.train_step calls on fresh twins fed the same latents and Philox keys, bit for bit."""
    import sdrm_amd.train_SDRM as ts
    from scipy.sparse import csr_matrix
    from test_reference_surface import make_feed
    L, W, T, H = WIDE
    n_items, hidden, batch, epochs, lr0, nd, seed = 60, 32, 4096, 2, 1e-3, 0.5, 1234
    rs = np.random.RandomState(5)
    data = csr_matrix((rs.random_sample((4096 + 1333, n_items)) < 0.25).astype(np.float64))
    torch.manual_seed(7)
    vae = ts.VAE(n_items, hidden, L).cuda()       # the frozen stub of test_cache_latents_matches_per_batch_encoding
    vae.model_is_trained = True
    feed = make_feed(data, batch)
    assert [x.shape[0] for x, _ in feed] == [4096, 1333]
    torch.manual_seed(seed)
    # train_SDRM makes its own SDRM and hands out neither its initial parameters nor its Philox key (the reference's signature has no
    # place for them): both are read from the private state of an SDRM built at the same torch seed
    init = ts.SDRM(L, T, W, H)._pending.clone()
    torch.manual_seed(seed)
    DIFF, _ = ts.train_SDRM(feed, n_items, hidden, L, 32, 1e-3, W, H, lr0, epochs, T, nd, str(tmp_path), data, data, "Recall@10",
                            variational_ae=vae)
    eng = DIFF.engine()
    assert DIFF._seed == seed and eng.max_rows == batch and eng.get_adam_state()[2] == 4
    split_ok = eng.rows48_split_available
    assert tuple(eng.last_plan()[:3]) == expected_train_plan(1333, split_ok), eng.last_plan()
    with torch.no_grad():
        zs = [vae.encode(x.to_dense())[0].float().contiguous() for x, _ in feed]
    params, adam = init, None
    for step in range(2 * epochs):
        f = engine_cls(L, W, T, H, batch)
        f.set_params(params)
        if adam is not None:
            f.set_adam_state(*adam)
        f.train_step(zs[step % 2], lr0 * (1 - (step // 2) / epochs), seed=seed, step=step, nd=nd)
        assert tuple(f.last_plan()[:3]) == expected_train_plan(zs[step % 2].shape[0], split_ok), (step, f.last_plan())
        print(f"  step {step} (B = {zs[step % 2].shape[0]}): {f.last_plan().train_path} parts {f.last_plan().parts}")
        params, adam = f.get_params(), f.get_adam_state()
        f.close()
    same_bits(eng.get_params(), params, "parameters after train_SDRM's two epochs")
    same_bits(eng.get_adam_state()[0], adam[0], "Adam first moments after train_SDRM's two epochs")
    same_bits(eng.get_adam_state()[1], adam[1], "Adam second moments after train_SDRM's two epochs")
