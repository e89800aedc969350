"""The frozen, eval-mode VAE encode hook (reference train_SDRM.py:210-212, :241-250, called at :323) on the engine.

CPU: tests/vae_encode_ref.py (float64, and float32 summed in CSR order) against golden outputs of the reference's own VAE class
(tests/golden/vae_encode.npz, made by tests/golden/make_vae_encode_golden.py); the header declares the entry points;
`encoder_tensors` takes the reference-shaped encoder only frozen and in eval mode.
GPU (-m gpu): sdrm_vae_encode / sdrm_vae_encode_csr through the C ABI against those goldens, the float64 restatement and the
PyTorch module on the device at the project's fp32 bar (1e-4, rel_max and rel_l2), at the fixture's cases and at the BASELINE
shapes; the bit-level promises of the CSR form; its range checks; the call-order statuses; `train_SDRM(engine_encode=True)`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vae_encode_ref as ver
from sdrm_amd import synth
from vae_encode_ref import rel_l2, rel_max

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "vae_encode.npz")
TOL = 1e-4


def golden_cases():
    g = np.load(GOLD)
    assert int(g["n_cases"]) == len(ver.CASES)
    for i in range(int(g["n_cases"])):
        tensors, m = ver.case_inputs(i)
        n_items, hidden, latent, n = (int(v) for v in g[f"c{i}_dims"][:4])
        assert (n_items, hidden, latent, n) == ver.CASES[i][1:5] and m.shape == (n, n_items) and m.nnz == int(g[f"c{i}_nnz"])
        yield i, tensors, m, g[f"c{i}_z"], float(g[f"c{i}_kl"])


# ---------------------------------------------------------------------------------------------- CPU
def test_restatement_matches_reference_goldens():
    for i, tensors, m, z_want, kl_want in golden_cases():
        z, kl = ver.encode(m, *tensors)
        print(f"case {i}: fp64 rel_max {rel_max(z, z_want):.2e} rel_l2 {rel_l2(z, z_want):.2e} kl rel {abs(kl - kl_want) / abs(kl_want):.2e}")
        assert z.shape == z_want.shape
        assert rel_max(z, z_want) <= 2e-6 and rel_l2(z, z_want) <= 2e-6, (i, rel_max(z, z_want), rel_l2(z, z_want))
        assert abs(kl - kl_want) <= 2e-6 * abs(kl_want), (i, kl, kl_want)
        z32, kl32 = ver.encode_csr_order32(m, *tensors)
        print(f"case {i}: fp32 CSR order rel_max {rel_max(z32, z_want):.2e} rel_l2 {rel_l2(z32, z_want):.2e} kl rel {abs(kl32 - kl_want) / abs(kl_want):.2e}")
        assert rel_max(z32, z_want) <= 2e-6 and rel_l2(z32, z_want) <= 2e-6, (i, rel_max(z32, z_want), rel_l2(z32, z_want))


def test_fixture_covers_the_cases_the_kernels_branch_on():
    """Real rows with stored zeros, an empty row, n = 1, widths that are not multiples of 4, every kernel form, the 8582-item case."""
    kinds = [c[0] for c in ver.CASES]
    assert "ml100k" in kinds
    _, m0 = ver.case_inputs(kinds.index("ml100k"))
    per_row = np.diff(m0.indptr)
    assert (m0.data == 0).any() and per_row.min() >= 18 and per_row.max() <= 550
    assert any(c[7] >= 0 for c in ver.CASES) and any(c[4] == 1 for c in ver.CASES)
    assert any(c[1] % 4 and c[2] % 4 for c in ver.CASES) and any(c[1] == 8582 for c in ver.CASES)
    q = [(c[2] + 3) // 4 for c in ver.CASES]
    assert min(q) <= 64 and any(64 < v <= 256 for v in q) and any(256 < v <= 512 for v in q) and any(512 < v <= 1024 for v in q) and max(q) > 1024
    for i, c in enumerate(ver.CASES):
        if c[7] >= 0:
            _, m = ver.case_inputs(i)
            assert m.indptr[c[7]] == m.indptr[c[7] + 1]
    assert os.path.getsize(GOLD) < 100_000


def test_header_declares_the_entry_points():
    header = open(os.path.join(REPO, "include", "sdrm_hip.h")).read()
    for name in ("sdrm_vae_encoder_load", "sdrm_vae_encode", "sdrm_vae_encode_csr"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "typedef struct sdrm_vae_encoder" in header
    from sdrm_amd import _lib
    assert {"sdrm_vae_encoder_load", "sdrm_vae_encode", "sdrm_vae_encode_csr"} <= set(_lib.SIGNATURES)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on a ROCm device: `encoder_tensors` only looks."""
    is_cuda = True


def _as_cuda(vae):
    for lin in (vae.encoder[0], vae.encoder[2]):
        lin.weight = torch.nn.Parameter(lin.weight.data.as_subclass(_FakeCuda), requires_grad=False)
        lin.bias = torch.nn.Parameter(lin.bias.data.as_subclass(_FakeCuda), requires_grad=False)
    return vae


def test_encoder_tensors_takes_the_frozen_eval_encoder_only():
    from sdrm_amd.train_SDRM import VAE, encoder_tensors
    vae = _as_cuda(VAE(50, 20, 6)).eval()
    if not all(t.is_cuda for t in (vae.encoder[0].weight, vae.encoder[0].bias)):
        pytest.fail("the stand-in device tensors did not survive nn.Parameter")
    ts = encoder_tensors(vae)
    assert ts is not None and tuple(ts[0].shape) == (20, 50) and tuple(ts[2].shape) == (12, 20)
    vae.train()
    assert encoder_tensors(vae) is None                       # train mode: dropout is live
    vae.eval()
    vae.is_training = 1
    assert encoder_tensors(vae) is None                       # the reparameterisation draw is live
    vae.is_training = 0
    assert encoder_tensors(vae) is not None
    assert encoder_tensors(VAE(50, 20, 6).eval()) is None     # on the host

    class Foreign(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = torch.nn.Sequential(torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 12))
            self.is_training = 0
    assert encoder_tensors(_as_cuda(Foreign()).eval()) is None
    assert encoder_tensors(object()) is None


def test_routing_agrees_with_the_measurement():
    """`encode_csr_pays` / `engine_encode_pays` return, at every shape of profiles/vae_encode_bench.txt, the variant that file
    shows fastest (the engine where the module is within the file's own spread)."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import encode_bench
    from sdrm_amd import train_SDRM as ts
    text = open(os.path.join(REPO, "profiles", "vae_encode_bench.txt")).read()
    seen = 0
    for name, n_rows, n_items, density, _, hidden, latent, batch in encode_bench.SHAPES:
        row = re.search(re.escape(name) + r"\s+(\d+)" + r"\s+([\d.]+) \(([\d.]+) \.\. ([\d.]+)\)" * 3, text)
        assert row, name
        nnz_row = float(row.group(1))
        (mod, mod_lo, _), (dense, _, dense_hi), (csr, _, csr_hi) = [tuple(float(v) for v in row.groups()[1 + 3 * k:4 + 3 * k]) for k in range(3)]
        dens = nnz_row / n_items if density is None else density
        assert ts.encode_csr_pays(dens, n_items, hidden) == (csr < dense), (name, dense, csr)
        engine_best_hi = csr_hi if csr < dense else dense_hi
        assert ts.engine_encode_pays(batch, n_items, hidden, latent) == (min(dense, csr) < mod or engine_best_hi >= mod_lo), name
        seen += 1
    assert seen == 4


# ---------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def engine():
    from sdrm_amd.engine import Engine
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


def _close(got, want, what):
    print(f"{what}: rel_max {rel_max(got, want):.2e} rel_l2 {rel_l2(got, want):.2e}")
    assert got.shape == want.shape, what
    assert rel_max(got, want) <= TOL and rel_l2(got, want) <= TOL, (what, rel_max(got, want), rel_l2(got, want))


@pytest.mark.gpu
def test_status_before_a_load_and_wrong_width():
    """(Runs first on a fresh engine.)  No encoder loaded: SDRM_ERR_STATE from both calls; a dense x of another width: SdrmError
    (SDRM_ERR_SHAPE) from the Python handle - the C call takes no width."""
    from sdrm_amd.engine import Engine, SdrmError, _stream
    e = Engine(8, 8, 4, 0, 16)
    try:
        x = torch.zeros(3, 10, device="cuda")
        z = torch.zeros(3, 4, device="cuda")
        ip = torch.zeros(4, dtype=torch.int64, device="cuda")
        ix = torch.zeros(1, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        assert e.lib.sdrm_vae_encode(e._h, p(x), 3, p(z), None, _stream()) == -4
        assert b"no encoder loaded" in e.lib.sdrm_last_error(e._h)
        assert e.lib.sdrm_vae_encode_csr(e._h, p(ip), p(ix), None, 3, None, 0, 3, p(z), None, _stream()) == -4
        with pytest.raises(SdrmError, match="SDRM_ERR_STATE"):
            e.vae_encode(x)
        e.vae_encoder_load(*synth.synth_vae_encoder(10, 6, 4, seed=1))
        assert tuple(e.vae_encode(x).shape) == (3, 4)
        with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
            e.vae_encode(torch.zeros(3, 11, device="cuda"))
        enc = synth.synth_vae_encoder(10, 6, 4, seed=1)
        from sdrm_amd import _lib
        bad = _lib.VaeEncoder(None, None, None, None, 10, 6, 4)
        assert e.lib.sdrm_vae_encoder_load(e._h, C.byref(bad), _stream()) == -1
        w = [torch.from_numpy(t).cuda() for t in enc]
        big = _lib.VaeEncoder(*[t.data_ptr() for t in w], 10, 20000, 4)
        assert e.lib.sdrm_vae_encoder_load(e._h, C.byref(big), _stream()) == -2
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [-1, 0, 4])
def test_hip_encode_matches_goldens(engine, tile):
    engine.debug_set(tile=tile)
    try:
        for i, tensors, m, z_want, kl_want in golden_cases():
            engine.vae_encoder_load(*tensors)
            csr = engine.csr_to_device(m)
            if ver.CASES[i][0] == "ml100k":   # stored zeros: csr_to_device keeps them (it does not eliminate zeros)
                assert csr[1].numel() == m.nnz
            z64, kl64 = ver.encode(m, *tensors)
            dense = torch.from_numpy(m.toarray().astype(np.float32))
            for form in ("dense", "csr"):
                if form == "dense":
                    z = engine.vae_encode(dense)
                    z2, kl = engine.vae_encode(dense, return_kl=True)
                else:
                    z = engine.vae_encode_csr(csr, row0=0, b=m.shape[0])
                    z2, kl = engine.vae_encode_csr(csr, row0=0, b=m.shape[0], return_kl=True)
                _close(z.cpu().numpy(), z_want, f"case {i} {form} vs fixture")
                _close(z.cpu().numpy(), z64, f"case {i} {form} vs fp64")
                assert torch.equal(z, z2), (i, form, "z differs with and without kl")
                kl = float(kl.cpu())
                print(f"case {i} {form}: kl {kl:.8g} fixture {kl_want:.8g} rel {abs(kl - kl_want) / abs(kl_want):.2e}")
                assert abs(kl - kl_want) <= TOL * abs(kl_want), (i, form, kl, kl_want)
                assert abs(kl - kl64) <= TOL * abs(kl64), (i, form, kl, kl64)
    finally:
        engine.debug_set(tile=-1)


def _baseline_inputs(name):
    """(encoder tensors, scipy CSR) at a BASELINE shape: ML-100k's 843 real rows with 930/830, ML-1M 8192 x 3125 at about 5 % with
    600/340, ADM 2000 x 8582 with 200/40."""
    if name == "ml100k":
        m = ver.ml100k_train()
        assert m.shape == (843, 1008)
        return synth.synth_vae_encoder(1008, 930, 830, seed=11), m
    if name == "ml1m":
        return synth.synth_vae_encoder(3125, 600, 340, seed=12), synth.synth_feed_csr(8192, 3125, 0.05, seed=13)
    return synth.synth_vae_encoder(8582, 200, 40, seed=14), synth.synth_feed_csr(2000, 8582, 0.004, seed=15, ratings=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ml100k", "ml1m", "adm"])
def test_hip_encode_vs_fp64_and_torch_at_baseline_shapes(engine, name):
    from sdrm_amd.train_SDRM import VAE, encoder_tensors
    tensors, m = _baseline_inputs(name)
    n, n_items = m.shape
    hidden, latent = tensors[0].shape[0], tensors[2].shape[0] // 2
    z64, kl64 = ver.encode(m, *tensors)
    engine.vae_encoder_load(*tensors)
    csr = engine.csr_to_device(m)
    x = engine.csr_rows_to_dense(csr, row0=0, b=n)
    vae = VAE(n_items, hidden, latent).cuda().eval()
    with torch.no_grad():
        for p, t in zip((vae.encoder[0].weight, vae.encoder[0].bias, vae.encoder[2].weight, vae.encoder[2].bias), tensors):
            p.copy_(torch.from_numpy(t))
        z_mod, kl_mod = vae.encode(x)
    assert encoder_tensors(vae) is not None
    z_mod, kl_mod = z_mod.cpu().numpy(), float(kl_mod.cpu())
    for form in ("dense", "csr"):
        z, kl = engine.vae_encode(x, return_kl=True) if form == "dense" else engine.vae_encode_csr(csr, row0=0, b=n, return_kl=True)
        z_nokl = engine.vae_encode(x) if form == "dense" else engine.vae_encode_csr(csr, row0=0, b=n)
        assert torch.equal(z, z_nokl)
        z, kl = z.cpu().numpy(), float(kl.cpu())
        _close(z, z64, f"{name} {form} vs fp64")
        _close(z, z_mod, f"{name} {form} vs the module")
        print(f"{name} {form}: kl {kl:.8g} fp64 {kl64:.8g} module {kl_mod:.8g}")
        assert abs(kl - kl64) <= TOL * abs(kl64) and abs(kl - kl_mod) <= TOL * abs(kl_mod)


@pytest.mark.gpu
def test_csr_form_is_a_function_of_the_row(engine):
    """Twice the same call: the same bits.  Permuted `rows`: z permuted, bit for bit.  data=None: as explicit ones."""
    tensors = synth.synth_vae_encoder(3125, 600, 34, seed=21)
    m = synth.synth_feed_csr(700, 3125, 0.05, seed=22)
    engine.vae_encoder_load(*tensors)
    csr = engine.csr_to_device(m)
    a = engine.vae_encode_csr(csr, row0=0, b=700)
    b = engine.vae_encode_csr(csr, row0=0, b=700)
    assert torch.equal(a, b)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(700))
    c = engine.vae_encode_csr(csr, rows=perm)
    assert torch.equal(c, a[perm.cuda()])
    sub = engine.vae_encode_csr(csr, rows=perm[:37])      # another batch size, another place in the batch
    assert torch.equal(sub, a[perm[:37].cuda()])
    off = engine.vae_encode_csr(csr, row0=123, b=50)
    assert torch.equal(off, a[123:173])
    # all ones: one wave per row (hidden 200) and one work-group per row (hidden 600)
    for hidden in (200, 600):
        t1 = synth.synth_vae_encoder(8582, hidden, 40, seed=23)
        ones = synth.synth_feed_csr(300, 8582, 0.004, seed=24, ratings=False)
        engine.vae_encoder_load(*t1)
        d_none = engine.csr_to_device(ones)
        assert d_none[2] is None
        d_ones = (d_none[0], d_none[1], torch.ones(ones.nnz, dtype=torch.float32, device="cuda"), d_none[3])
        z_none, z_ones = engine.vae_encode_csr(d_none, row0=0, b=300), engine.vae_encode_csr(d_ones, row0=0, b=300)
        assert torch.equal(z_none, z_ones)
        _close(z_none.cpu().numpy(), ver.encode(ones, *t1)[0], f"all ones, hidden {hidden}")


@pytest.mark.gpu
def test_empty_row_is_the_bias_path(engine):
    w1, b1, w2, b2 = tensors = synth.synth_vae_encoder(257, 61, 17, seed=31)
    from scipy.sparse import csr_matrix
    m = csr_matrix((np.asarray([2.0, 3.0], np.float32), np.asarray([5, 200], np.int32), np.asarray([0, 0, 2, 2], np.int64)), shape=(3, 257))
    engine.vae_encoder_load(*tensors)
    want = (w2[:17].astype(np.float64) @ np.tanh(b1.astype(np.float64)) + b2[:17]).astype(np.float64)
    for z in (engine.vae_encode_csr(engine.csr_to_device(m), row0=0, b=3), engine.vae_encode(torch.from_numpy(m.toarray()))):
        z = z.cpu().numpy()
        _close(z[0], want, "empty row")
        _close(z[2], want, "empty row")
        _close(z, ver.encode(m, *tensors)[0], "batch with empty rows")


@pytest.mark.gpu
def test_range_checks_raise_and_spare_the_other_rows(engine):
    from sdrm_amd.engine import SdrmError
    tensors = synth.synth_vae_encoder(500, 120, 9, seed=41)
    m = synth.synth_feed_csr(40, 500, 0.05, seed=42)
    engine.vae_encoder_load(*tensors)
    good = engine.csr_to_device(m)
    want = engine.vae_encode_csr(good, row0=0, b=40)
    # a column index >= n_items in row 7: raises through feed_status; every other row is still right, and row 7 is the row without it
    bad_idx = good[1].clone()
    p = int(m.indptr[7])
    bad_idx[p] = 500
    bad = (good[0], bad_idx, good[2], good[3])
    with pytest.raises(SdrmError, match="column index"):
        engine.vae_encode_csr(bad, row0=0, b=40)
    z = engine.vae_encode_csr(bad, row0=0, b=40, check=False)
    with pytest.raises(SdrmError, match="column index"):
        engine.feed_status()
    engine.feed_status()   # cleared
    keep = np.ones(40, bool)
    keep[7] = False
    assert torch.equal(z[torch.from_numpy(keep).cuda()], want[torch.from_numpy(keep).cuda()])
    m7 = m.copy().tolil()
    m7[7, m.indices[p]] = 0
    m7 = m7.tocsr()
    m7.eliminate_zeros()
    _close(z[7].cpu().numpy(), ver.encode(m7, *tensors)[0][7], "row with the offending entry dropped")
    # a row id >= n_rows: encoded as an empty row, raises; the others are right
    rows = torch.arange(40)
    rows[11] = 40
    z = engine.vae_encode_csr(good, rows=rows, check=False)
    with pytest.raises(SdrmError, match="row id"):
        engine.feed_status()
    keep = np.ones(40, bool)
    keep[11] = False
    assert torch.equal(z[torch.from_numpy(keep).cuda()], want[torch.from_numpy(keep).cuda()])
    w1, b1, w2, b2 = tensors
    _close(z[11].cpu().numpy(), w2[:9].astype(np.float64) @ np.tanh(b1.astype(np.float64)) + b2[:9], "row outside the matrix = empty row")
    # host-side: a contiguous range behind the matrix is refused before any launch
    with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
        engine.vae_encode_csr(good, row0=30, b=20)


@pytest.mark.gpu
def test_second_load_replaces_the_first(engine):
    m = synth.synth_feed_csr(50, 700, 0.05, seed=51)
    csr = engine.csr_to_device(m)
    first, second = synth.synth_vae_encoder(700, 300, 20, seed=52), synth.synth_vae_encoder(700, 90, 33, seed=53)
    engine.vae_encoder_load(*first)
    _close(engine.vae_encode_csr(csr, row0=0, b=50).cpu().numpy(), ver.encode(m, *first)[0], "first encoder")
    engine.vae_encoder_load(*second)
    x = torch.from_numpy(m.toarray())
    for z in (engine.vae_encode_csr(csr, row0=0, b=50), engine.vae_encode(x)):
        assert tuple(z.shape) == (50, 33)
        _close(z.cpu().numpy(), ver.encode(m, *second)[0], "second encoder")
    engine.vae_encoder_load(*first)   # and back, into the buffers that shrank and grew
    _close(engine.vae_encode(x).cpu().numpy(), ver.encode(m, *first)[0], "first encoder again")


@pytest.mark.gpu
@pytest.mark.parametrize("feed", ["device", "dense"])
def test_train_sdrm_engine_encode(feed):
    """`train_SDRM(engine_encode=True)` with a supplied VAE: the first step's loss within 1e-4 of the module path, torch's device
    generator left where the module path leaves it, and with a DeviceFeed not one `csr_rows_to_dense`."""
    from sdrm_amd import pipeline, train_SDRM as ts
    from sdrm_amd.engine import Engine, utility_engine
    n_items, hidden, latent, users, batch = 300, 70, 48, 64, 64
    m = synth.synth_feed_csr(users, n_items, 0.06, seed=61)
    torch.manual_seed(5)
    vae = ts.VAE(n_items, hidden, latent).cuda()
    with torch.no_grad():
        for prm, t in zip((vae.encoder[0].weight, vae.encoder[0].bias, vae.encoder[2].weight, vae.encoder[2].bias),
                          synth.synth_vae_encoder(n_items, hidden, latent, seed=62)):
            prm.copy_(torch.from_numpy(t))
    vae.model_is_trained = True
    calls = {"dense": 0, "csr": 0, "enc": 0}
    orig_dense, orig_csr, orig_enc = Engine.csr_rows_to_dense, Engine.vae_encode_csr, Engine.vae_encode

    def counted(name, fn):
        def wrapper(self, *a, **kw):
            calls[name] += 1
            return fn(self, *a, **kw)
        return wrapper

    def run(engine_encode):
        for k in calls:
            calls[k] = 0
        torch.manual_seed(17)
        if feed == "device":
            dl = pipeline.DeviceFeed(m, batch, utility_engine(), seed=9)
        else:
            dl = [(torch.from_numpy(m.toarray().astype(np.float32)).cuda(),) * 2]
        net, _ = ts.train_SDRM(dl, n_items, hidden, latent, 32, 1e-3, latent, 1, 1e-3, 1, 9, 1.0, "/nonexistent", None, None, "Recall@10",
                               variational_ae=vae, engine_encode=engine_encode)
        loss = float(net.last_loss.cpu())
        state = torch.cuda.get_rng_state().clone()
        net.engine().close()
        return loss, state, dict(calls)

    Engine.csr_rows_to_dense, Engine.vae_encode_csr, Engine.vae_encode = (counted("dense", orig_dense), counted("csr", orig_csr),
                                                                            counted("enc", orig_enc))
    try:
        loss_mod, rng_mod, calls_mod = run(False)
        loss_eng, rng_eng, calls_eng = run(True)
    finally:
        Engine.csr_rows_to_dense, Engine.vae_encode_csr, Engine.vae_encode = orig_dense, orig_csr, orig_enc
    print(f"{feed}: first-step loss module {loss_mod:.8g} engine {loss_eng:.8g} rel {abs(loss_eng - loss_mod) / abs(loss_mod):.2e}; calls {calls_mod} -> {calls_eng}")
    assert abs(loss_eng - loss_mod) <= 1e-4 * abs(loss_mod), (loss_eng, loss_mod)
    assert torch.equal(rng_mod, rng_eng)
    assert calls_mod["csr"] == 0 and calls_mod["enc"] == 0
    if feed == "device":
        assert calls_mod["dense"] == 1
        assert ts.encode_csr_pays(m.nnz / (users * n_items), n_items, hidden), "this shape is routed to the gather"
        assert calls_eng == {"dense": 0, "csr": 1, "enc": 0}
    else:
        assert calls_eng == {"dense": 0, "csr": 0, "enc": 1}
