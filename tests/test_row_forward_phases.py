"""The phases around the K loops of the 96-row train forward (csrc/rowchain.h): its staging - the x0 requests, the timestep draw, the
time-embedding columns, the randoms and the three staged inputs, four columns wide - and what a K-step holds beside its MFMAs.

The kernel is two: k_row_fwd<CT, LIGHT> draws its randoms itself (PHILOX), k_row_fwd_explicit<CT, LIGHT> reads the step's noise / t /
keep arrays.  The first test reads the generated code of both (no GPU needed); the others run them - forced on at batches the size rule
would never give them (debug_set(tile="row") of the test engine: sdrm_debug_set_rowchain(e, 2)) - against the per-layer path of the same
engine, against oracle/philox_ref.py and against themselves."""
import re

import numpy as np
import pytest
import torch

import test_isa_lint as lint
from sdrm_amd import synth
from test_hip_parity import CT_LR, close, per_tensor, rel_l2, rel_max, row_group_steps_are_reproducible

# VALU instructions (everything v_* but the MFMAs) in the K-loop block that streams the tile - a pair of K-steps - per (CT, LIGHT), as
# generated at this commit; the ceiling is this count + 0: three v_add for the LDS addresses of the stream's three chunks and two that
# advance the running fragment offsets, once per trip.  At the parent commit the same block held 12 (CT = 11) and 10 (CT = 4): per
# pair a v_subrev for the odd K-step's fragment address, per K-step three v_mov (the opaque by-value offset was a copy per read) and,
# at CT = 11, a v_add for the third row tile, whose offset does not fit the 16-bit field; the stream's three; one v_add for the trip.
STREAM_LOOP_VALU = {(11, True): 5, (4, False): 5}

# RowChainArgs: x0 at byte 0 of the kernel arguments, then noise, t and keep (three pointers: bytes 8 .. 31)
EXPLICIT_ARG_BYTES = range(8, 32)


def _forward_kernels(ct, light):
    targs = "%d, %s" % (ct, str(light).lower())
    asm = lint._compile("template __global__ void sdrm::k_row_fwd<%s>(const sdrm::RowChainArgs);\n"
                        "template __global__ void sdrm::k_row_fwd_explicit<%s>(const sdrm::RowChainArgs);\n" % (targs, targs), "rowchain.h")
    ks = lint._kernels(asm)
    (philox,) = [n for n in ks if re.search(r"\d+k_row_fwdI", n)]
    (explicit,) = [n for n in ks if "k_row_fwd_explicitI" in n]
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\w+)[\s\S]*?\.amdhsa_private_segment_fixed_size (\d+)", asm)}
    return ks, philox, explicit, scratch


def _kernarg_bytes(ins):
    """Bytes of the kernel-argument segment (s[0:1]) the kernel loads."""
    got = set()
    for x in ins:
        m = re.match(r"s_load_dword(x(\d+))? s\[?[\d:]+\]?, s\[0:1\], (0x[0-9a-f]+|\d+)", x)
        if m:
            off = int(m.group(3), 0)
            got.update(range(off, off + 4 * int(m.group(2) or 1)))
    return got


@pytest.mark.parametrize("ct, light", [(11, True), (4, False)])
def test_forward_kernels_generated_code(ct, light):
    """Both RNG instantiations of the headline width and of the narrowest one: no scratch, no accumulator copies in a K-loop block, no
    more VALU in the streamed K-loop block than at this commit - and the kernel that draws its randoms does not even load the pointers
    of the explicit ones (the other one does: the check sees what it looks for)."""
    ks, philox, explicit, scratch = _forward_kernels(ct, light)
    for name in (philox, explicit):
        ins = ks[name]
        assert scratch[name] == 0 and not [x for x in ins if x.startswith("scratch_")], name
        loops = lint._loops(ins)
        inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
        kloops = [(a, b) for a, b in inner if sum(1 for x in ins[a:b] if x.startswith("v_mfma")) >= 24 and "s_barrier" not in ins[a:b]]
        assert kloops, name
        streamed = [(a, b) for a, b in kloops if any(x.startswith("buffer_store") for x in ins[a:b])]
        assert len(streamed) == 1, (name, streamed)
        for a, b in kloops:
            assert not [x for x in ins[a:b] if x.startswith("v_accvgpr")], (name, "accumulator copies inside a K loop")
        (a, b), = streamed
        valu = [x for x in ins[a:b] if x.startswith("v_") and not x.startswith("v_mfma")]
        print(name, "VALU in the streamed K-loop block:", len(valu), valu)
        assert len(valu) <= STREAM_LOOP_VALU[(ct, light)], (name, len(valu), valu)
    assert not _kernarg_bytes(ks[philox]) & set(EXPLICIT_ARG_BYTES), sorted(_kernarg_bytes(ks[philox]) & set(EXPLICIT_ARG_BYTES))
    assert set(EXPLICIT_ARG_BYTES) <= _kernarg_bytes(ks[explicit])


# ---------------------------------------------------------------------------------------------------------------- on the device
WIDTHS = [(100, 1), (116, 0), (340, 1), (352, 2)]   # 4 and 11 column tiles, the compact and the plain last K-step of each
BATCHES = [33, 370]                                 # two groups of 32 users with ONE user in the second; twelve, the last one ragged
T = 7
SEED, STEP, ROW0, ND = 0x1234ABCD5678, 11, 1000, 0.8


def _engine(engine_cls, dims, row, init):
    L, W, T_, H, B = dims
    e = engine_cls(L, W, T_, H, B)
    e.debug_set(tile="row") if row else e.debug_set(rowchain=0, rows48=0)
    e.set_params(init)
    return e


def _shifted(x0, off):
    """x0 as a view `off` floats into a larger buffer (off = 1: rows no longer 16-byte aligned)."""
    B, L = x0.shape
    big = torch.zeros(B * L + off + 8, device="cuda")
    big[off:off + B * L] = x0.reshape(-1)
    return big[off:off + B * L].view(B, L)


def _one_step(engine_cls, dims, row, init, x0, randoms):
    """One train forward + backward; (loss, P / S / Q outputs, gradients, staged inputs, timesteps, path taken)."""
    e = _engine(engine_cls, dims, row, init)
    if randoms is None:
        e.train_forward(x0, seed=SEED, step=STEP, nd=ND, row0=ROW0)
    else:
        e.train_forward(x0, noise=randoms[0], t=randoms[1], keep=randoms[2])
    staged, t = e.staged(dims[4])
    staged, t = staged.cpu().numpy(), t.cpu().numpy()
    loss = float(e.train_backward().cpu())
    out = (loss, e.train_outputs(dims[4]).cpu().numpy(), e.get_grads().cpu().numpy(), staged, t, e.last_plan().train_path)
    e.close()
    return out


@pytest.fixture(scope="module")
def reference_draws():
    """oracle/philox_ref.py's randoms of (SEED, STEP, ROW0) per (B, L): drawn once, shared, never written."""
    from oracle import philox_ref as pr
    cache = {}

    def get(B, L):
        if (B, L) not in cache:
            cache[(B, L)] = pr.train_randoms(SEED, STEP, ROW0, B, L, T, ND)
        return cache[(B, L)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: f"W{w[0]}-H{w[1]}")
def test_both_rng_kernels_against_the_per_layer_path(engine_cls, reference_draws, width, B):
    """One PHILOX step and one EXPLICIT step through each kernel: the row-owned path was taken, loss, outputs and gradients are the
    per-layer path's to fp32 summation order (the bars of the existing path comparisons), the same bits come out twice and from an x0
    view shifted by one float; and four fused PHILOX steps hold the assertions of test_row_group_steps_are_reproducible."""
    W, H = width
    dims = (W, W, T, H, B)
    init = synth.flatten_params(synth.init_params(W, W, T, H, seed=6), H)
    x0 = torch.from_numpy(synth.synth_latents(B, W, seed=7)).cuda()
    for randoms in (None, reference_draws(B, W)):
        a = _one_step(engine_cls, dims, True, init, x0, randoms)
        b = _one_step(engine_cls, dims, True, init, x0, randoms)
        c = _one_step(engine_cls, dims, True, init, _shifted(x0, 1), randoms)
        ref = _one_step(engine_cls, dims, False, init, x0, randoms)
        assert a[5] == "row96" and ref[5] == "per_layer", (a[5], ref[5])
        for other in (b, c):
            assert a[0] == other[0] and all(np.array_equal(u, v) for u, v in zip(a[1:5], other[1:5]))
        assert abs(a[0] - ref[0]) <= 2e-5 * abs(ref[0]), (a[0], ref[0])
        assert close(a[1], ref[1], 2e-5), rel_max(a[1], ref[1])
        for (n, g), (_, g0) in zip(per_tensor(a[2], dims[:4]), per_tensor(ref[2], dims[:4])):
            assert rel_l2(g, g0) <= 2e-5 and rel_max(g, g0) <= 2e-5, (n, rel_l2(g, g0), rel_max(g, g0))
    row_group_steps_are_reproducible(engine_cls, dims, "row", lr=CT_LR)


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
def test_timesteps_are_the_reference_draw(engine_cls, reference_draws, B):
    """Every thread of the staging draws its user's timestep itself: tdev after a PHILOX step is oracle/philox_ref.py's draw of the same
    (seed, step, row0), user for user - in the full groups and in the ragged last one."""
    W, H = 340, 1
    init = synth.flatten_params(synth.init_params(W, W, T, H, seed=6), H)
    x0 = torch.from_numpy(synth.synth_latents(B, W, seed=7)).cuda()
    got = _one_step(engine_cls, (W, W, T, H, B), True, init, x0, None)
    assert got[5] == "row96"
    _, t, _ = reference_draws(B, W)
    assert np.array_equal(got[4].astype(np.int64), np.asarray(t).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [100, 340])
def test_staged_inputs_against_the_per_layer_staging(engine_cls, W):
    """The layer-0 input the row-owned forward stages (B = 33) against k_prep_train's image of the same PHILOX keys, element for element
    over the real columns: the S and Q inputs to the bit at both widths, the P input to the bit at W = 100.  At W = 340 (eleven column
    tiles) the row kernel has always computed column 0 of every quad of P as 2 fma(sa, x, om e) where k_prep_train - and the kernel's
    other columns, and every column at the other widths - round sa x first (csrc/rowchain.h: rc_stage_quad): there the two differ by the
    rounding of that product and by nothing else, 2 (ulp(sa x) / 2 + ulp(P / 2)) at most; every other element is the same bits."""
    H, B = 1, 33
    init = synth.flatten_params(synth.init_params(W, W, T, H, seed=6), H)
    x0 = torch.from_numpy(synth.synth_latents(B, W, seed=7)).cuda()
    row = _one_step(engine_cls, (W, W, T, H, B), True, init, x0, None)
    ref = _one_step(engine_cls, (W, W, T, H, B), False, init, x0, None)
    assert row[5] == "row96" and ref[5] == "per_layer"
    assert np.array_equal(row[4], ref[4])
    assert np.array_equal(row[3][1:], ref[3][1:])
    fused = np.zeros(W, bool)
    if W == 340:
        fused[0::4] = True
    assert np.array_equal(row[3][0][:, ~fused], ref[3][0][:, ~fused])
    if fused.any():
        p, p0 = row[3][0][:, fused].astype(np.float64), ref[3][0][:, fused].astype(np.float64)
        x = x0.cpu().numpy()[:, fused]
        bound = 2.0 * (0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64) + np.spacing((np.abs(p0) / 2).astype(np.float32)).astype(np.float64))
        # (sa <= 1: ulp(sa x) <= ulp(x))
        print("P column 0 of a quad, W = 340: elements that differ", int((p != p0).sum()), "of", p.size, "largest |difference| / bound",
              float((np.abs(p - p0) / bound).max()))
        assert (np.abs(p - p0) <= bound).all()
