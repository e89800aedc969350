"""The persistent sampler (csrc/sample_persist.h: k_sample_persist) - on by default for PHILOX, full-resolution calls of a mid-width
net with L == W, one row chain and n <= 352 rows (csrc/sdrm_hip.hip: sample_persist_fits), and for larger calls when forced.  It runs
`count` reverse steps in ONE launch and hands the activations of a row tile from layer to layer through one XCD's L2 (sc1 loads of
the A operand, work-group-scope counters that carry from one sdrm_sample_steps call to the next).

Every case is compared three ways:
  * with the per-layer path, BIT FOR BIT: a second engine with debug_set(sample_persist=0, tile=4, fused_reverse=2) runs the same
    tile body (gemm_body<Cfg4>) with the same K order (kchunk = K, one split) and the same EPI_TANH_REV epilogue; only the cache
    policy of the A loads differs.  A stale line, a hand-shake that lets a tile start early, a wrong loop count all change bits;
  * with the CPU oracle fed the numpy restatement of the device generator (oracle/philox_ref.py), at the project's bar
    (test_hip_parity.close: 1e-4 in both norms - what the per-layer sampler meets at n = 5429 on the headline net);
  * proof of path: every sdrm_sample_steps call that had steps left is exactly ONE kernel launch (the per-layer path issues three or
    more per reverse step), the event profile shows the class "sample: k_sample_persist ..." with that many launches and no
    "sample: gemm_kernel..." class - and the reverse on the reference engine.

Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

from sdrm_amd import synth
from test_hip_parity import close, rel_l2, rel_max

pytestmark = pytest.mark.gpu

SEED, CALL_ID, ROW0 = 0x5DEECE66D1234, 7, 2715      # a 64-bit seed, non-zero call id and shard offset
HEADLINE, DEEP, FLAT, FULLW, NARROW = (340, 340, 78, 1), (136, 136, 12, 2), (308, 308, 8, 0), (352, 352, 9, 3), (97, 97, 9, 1)

# (net, n, sdrm_debug_set_sample_persist mode, noise divider)
CASES = [(HEADLINE, 19, 1, 0.9), (HEADLINE, 339, 1, 1.0), (HEADLINE, 352, 1, 0.9),       # 2 and 12 row tiles of 32 (MP = round_up(n, 64)): a wholly
                                                                                        # padded row tile; two row tiles on XCDs 0 .. 3
         (DEEP, 19, 1, 1.0), (DEEP, 339, 1, 0.9), (DEEP, 352, 1, 1.0),                   # H = 2: the hidden loop more than once; 5 column tiles
         (FLAT, 33, 1, 0.9), (FLAT, 200, 1, 1.0),                                        # H = 0: zero-trip hidden loop, the out layer reads layer 0's buffer
         (FULLW, 97, 1, 0.9),                                                            # no padded columns
         (NARROW, 64, 1, 1.0), (NARROW, 65, 1, 0.9),                                     # WP = 128, L no multiple of 4, n on both sides of a row granule
         (HEADLINE, 679, 2, 1.0), (HEADLINE, 1280, 2, 0.9)]                              # the 8-GPU shard; the largest n with ceil(tiles_m / 8) * 11 <= 64


def case_id(c):
    (L, W, T, H), n, mode, nd = c
    return f"{L}-{T}-{H}-n{n}-m{mode}"


def init_of(dims, seed=21):
    return synth.init_params(*dims, seed=seed)


_ORACLE = {}


def oracle_latents(dims, n, nd, init_seed=21, multires=False):
    """The oracle's latents of the call (SEED, CALL_ID, ROW0) on the net init_of(dims, init_seed); computed once per module run."""
    key = (dims, n, nd, init_seed, multires)
    if key not in _ORACLE:
        from oracle import philox_ref as pr
        from oracle import sdrm_oracle as orc
        L, W, T, H = dims
        xT, z, keep, Tj = pr.sample_randoms(SEED, CALL_ID, ROW0, n, L, T, nd, multires)
        _ORACLE[key] = orc.Oracle(L, W, T, H, init_of(dims, init_seed)).sample(xT, z, keep, Tj).numpy()
    return _ORACLE[key]


def make(engine_cls, dims, max_rows, init_seed=21, **debug):
    e = engine_cls(*dims, max_rows)
    if debug:
        e.debug_set(**debug)
    e.set_params(synth.flatten_params(init_of(dims, init_seed), dims[3]))
    return e


def need_xcd_mapping(e):
    """The one skip this file knows: a device whose work-groups do not land on XCD (block & 7) - never an MI355X."""
    if not e.rows48_split_available:
        e.close()
        pytest.skip("no block -> XCD mapping on this device: the persistent sampler is never taken")


def reference_engine(engine_cls, dims, max_rows, init_seed=21):
    """The per-layer path on the persistent kernel's tile, its K order and its epilogue."""
    return make(engine_cls, dims, max_rows, init_seed, sample_persist=0, tile=4, fused_reverse=2)


def drive(e, n, nd, chunks=None, multires=False, between=None):
    """One sampling call (SEED, CALL_ID, ROW0) under an event profile.  `chunks`: the counts given to sample_steps one after the other
    (None: the one-call form, sample()); `between`: {index: callable} run after that chunk.  Returns the latents (numpy), the number
    of k_sample_persist launches and of per-layer sampler GEMM launches the profile saw, and the launch-count increments of the
    sample_steps calls that had steps left."""
    kw = dict(nd=nd, multires=multires, seed=SEED, call_id=CALL_ID, row0=ROW0)
    deltas, profs = [], []
    if chunks is None:
        e.profile_begin(capacity=4096)
        out = e.sample(n, **kw)
    else:
        e.sample_begin(n, **kw)
        e.profile_begin(capacity=4096)
        left = e.T
        for k, count in enumerate(chunks):
            before = e.launch_count()
            had = left >= 1 and count > 0
            left = e.sample_steps(count)
            if had:
                deltas.append(e.launch_count() - before)
            if between and k in between:
                profs.append(e.profile_end())
                between[k]()
                e.profile_begin(capacity=4096)
        assert left == 0
        out = e.sample_end()
    profs.append(e.profile_end())
    persist = sum(v[1] for prof in profs for name, v in prof.items() if name.startswith("sample: k_sample_persist"))
    layers = sum(v[1] for prof in profs for name, v in prof.items() if name.startswith("sample: gemm_kernel"))
    return out.cpu().numpy(), persist, layers, deltas


def assert_oracle(out, ref, what):
    assert np.isfinite(out).all(), what
    print(what, "vs oracle: rel_l2 %.3e rel_max %.3e" % (rel_l2(out, ref), rel_max(out, ref)))
    assert close(out, ref), (what, rel_l2(out, ref), rel_max(out, ref))


def assert_same_bits(a, b, what):
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ, rows {bad[:, 0].min()}..{bad[:, 0].max()}, first at "
                             f"({r}, {c}): {a[r, c]!r} against {b[r, c]!r}")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_persistent_sampler_vs_per_layer_path_and_oracle(engine_cls, case):
    dims, n, mode, nd = case
    T = dims[2]
    e = make(engine_cls, dims, n, sample_persist=mode)
    need_xcd_mapping(e)
    out, persist, layers, _ = drive(e, n, nd)
    assert (persist, layers) == (1, 0), ("the call did not run in one k_sample_persist launch", persist, layers)
    # the same call as three sample_steps calls: one launch each
    out3, persist3, layers3, deltas = drive(e, n, nd, chunks=[T // 2, T - T // 2 - 1, 1])
    assert (persist3, layers3, deltas) == (3, 0, [1, 1, 1]), (persist3, layers3, deltas)
    e.close()
    r = reference_engine(engine_cls, dims, n)
    ref, rpersist, rlayers, _ = drive(r, n, nd)
    assert rpersist == 0 and rlayers >= 2 * T, ("reference engine: not the per-layer path", rpersist, rlayers)
    r.close()
    assert_oracle(ref, oracle_latents(dims, n, nd), "per-layer path")
    # all three comparisons are made before any of them fails the test: a wrong kernel shows in which of them it is wrong
    wrong = []
    for check, args in ((assert_oracle, (out, oracle_latents(dims, n, nd), "persistent sampler")),
                        (assert_same_bits, (out, ref, "persistent sampler against the per-layer path")),
                        (assert_same_bits, (out3, ref, "persistent sampler in three launches against the per-layer path"))):
        try:
            check(*args)
        except AssertionError as err:
            wrong.append(str(err).split("\n")[0])
    assert not wrong, "\n".join(wrong)


def test_persistent_sampler_refuses_what_is_not_resident_at_once(engine_cls):
    """n = 1281 on the headline net: 41 row tiles, ceil(41 / 8) * 11 = 66 work-groups on the fullest XCD - more than the 64 that are
    resident at once, so even the forced mode must take the per-layer path (a launch whose work-groups wait for ones that cannot
    start would sit out its time limit)."""
    dims, n, nd = HEADLINE, 1281, 1.0
    e = make(engine_cls, dims, n, sample_persist=2)
    need_xcd_mapping(e)
    out, persist, layers, _ = drive(e, n, nd)
    e.close()
    assert persist == 0 and layers >= 2 * dims[2], (persist, layers)
    assert_oracle(out, oracle_latents(dims, n, nd), "n = 1281, forced mode")


@pytest.mark.parametrize("dims,n", [(HEADLINE, 339), (DEEP, 352)], ids=["340-n339", "136-n352"])
def test_chunking_changes_no_bit(engine_cls, dims, n):
    """The same call as sample(), one step per sdrm_sample_steps, chunks of 7, one call of T steps, and a request for more steps than
    remain: the counters' base (P.base from xphaseS), the `count > 1` loop and the clamp at step 1 - all the same bits, every
    sdrm_sample_steps call one launch."""
    T, nd = dims[2], 0.9
    e = make(engine_cls, dims, n)        # the default mode
    need_xcd_mapping(e)
    whole, persist, layers, _ = drive(e, n, nd)
    assert (persist, layers) == (1, 0)
    sevens = [7] * ((T + 6) // 7)
    for name, chunks in (("one step per call", [1] * T), ("chunks of 7", sevens), ("one call of T steps", [T]), ("T + 5 steps asked", [T + 5]),
                         ("3, then more than remain", [3, T + 5])):
        out, persist, layers, deltas = drive(e, n, nd, chunks=chunks)
        assert persist == len(chunks) and layers == 0 and deltas == [1] * len(chunks), (name, persist, layers, deltas)
        assert_same_bits(out, whole, name)
    e.close()
    assert_oracle(whole, oracle_latents(dims, n, nd), "whole call")


@pytest.mark.parametrize("dims,n", [(HEADLINE, 339), (DEEP, 352)], ids=["340-n339", "136-n352"])
def test_train_steps_between_chunks(engine_cls, dims, n):
    """A call is a function of the parameters at sdrm_sample_begin, on this kernel too (test_sampling_call_uses_the_parameters_of_its_begin
    runs EXPLICIT randoms and never reaches it): a train step whose Adam moves every parameter and a set_params with another net between
    its chunks change no bit of it, and the next call sees the new net."""
    L, W, T, H = dims
    nd = 1.0
    fresh = make(engine_cls, dims, n)
    need_xcd_mapping(fresh)
    ref_a, persist, _, _ = drive(fresh, n, nd)
    assert persist == 1
    fresh.close()
    fresh = make(engine_cls, dims, n, init_seed=22)
    ref_b, persist, _, _ = drive(fresh, n, nd)
    assert persist == 1
    fresh.close()
    assert not np.array_equal(ref_a, ref_b)
    x0 = synth.synth_latents(n, L, seed=45)
    eps, t, masks = synth.synth_train_randoms(n, L, T, 1.0, seed=44)
    e = make(engine_cls, dims, n)
    before = e.get_params().cpu().numpy()

    def train():
        e.train_step(x0, 1e-2, noise=eps, t=t, keep=masks)
        moved = e.get_params().cpu().numpy() != before
        assert moved.mean() > 0.9, "Adam at lr = 1e-2 was to move every parameter"

    def replace():
        e.set_params(synth.flatten_params(init_of(dims, 22), H))

    cut = T // 3
    out, persist, layers, deltas = drive(e, n, nd, chunks=[cut, cut, T - 2 * cut], between={0: train, 1: replace})
    assert (persist, layers, deltas) == (3, 0, [1, 1, 1]), (persist, layers, deltas)
    assert_same_bits(out, ref_a, "call interleaved with a train step and set_params")
    nxt, persist, layers, _ = drive(e, n, nd)
    assert (persist, layers) == (1, 0)
    assert_same_bits(nxt, ref_b, "the next call, on the replaced parameters")
    e.close()
    assert_oracle(ref_a, oracle_latents(dims, n, nd), "parameters of the begin")
    assert_oracle(ref_b, oracle_latents(dims, n, nd, init_seed=22), "replaced parameters")


@pytest.mark.parametrize("dims", [HEADLINE, DEEP], ids=["340", "136"])
def test_consecutive_calls_with_different_row_counts(engine_cls, dims):
    """352, then 19, then 339 rows on one engine created for 352: the row tiles - and with them the counters in use and what they count up
    to - differ from call to call, so sdrm_sample_begin clears them; each call equals a fresh engine's."""
    nd = 0.9
    e = make(engine_cls, dims, 352)
    need_xcd_mapping(e)
    for n in (352, 19, 339):
        out, persist, layers, _ = drive(e, n, nd, chunks=[5, dims[2]])
        assert (persist, layers) == (2, 0), (n, persist, layers)
        f = make(engine_cls, dims, n)
        ref, persist, layers, _ = drive(f, n, nd)
        assert (persist, layers) == (1, 0), (n, persist, layers)
        f.close()
        assert_same_bits(out, ref, f"n = {n} behind the earlier calls")
        assert_oracle(out, oracle_latents(dims, n, nd), f"n = {n}")
    e.close()


GATES = [("n353", dict(), 353, False, False), ("multires", dict(), 339, True, False), ("chains2", dict(chains=2), 339, False, False),
         ("tile0", dict(tile=0), 339, False, False), ("fused_reverse0", dict(fused_reverse=0), 339, False, False),
         ("tile4", dict(tile=4), 339, False, True)]


@pytest.mark.parametrize("gate", GATES, ids=[g[0] for g in GATES])
def test_gates_of_the_size_rule(engine_cls, gate):
    """sample_persist_fits with the default mode (1, by size) on the headline net: one row more than 352, a multi-resolution call, two row
    chains, a forced tile other than 32x32 and the stand-alone reverse update each take the per-layer path - and still give the
    oracle's latents; the forced 32x32 tile keeps the persistent kernel."""
    name, debug, n, multires, want_persist = gate
    dims, nd = HEADLINE, 0.9
    T = dims[2]
    e = make(engine_cls, dims, n, sample_persist=1, **debug)
    need_xcd_mapping(e)
    out, persist, layers, _ = drive(e, n, nd, multires=multires)
    e.close()
    if want_persist:
        assert (persist, layers) == (1, 0), (name, persist, layers)
    else:
        assert persist == 0 and layers >= (2 if multires else 2 * T), (name, persist, layers)
    assert_oracle(out, oracle_latents(dims, n, nd, multires=multires), name)
