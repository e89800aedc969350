"""The MLP evaluator's eval-mode forward, validation SSE and predict on the device (csrc/mlp_eval.h; sdrm_mlp_eval; `Engine.mlp_eval`;
`mlp_eval.compute_mlp_results_device`).  Every test needs the GPU; tests/test_mlp_eval_host.py holds what does not.

The oracle is tests/mlp_eval_ref.py's float64 step in inference mode (tests/mlp_eval_fwd_ref.py), and the bar the house rule: BAR_FACTOR
(4) times the deviation of the FLOAT32 torch module on the CPU from that oracle for the same quantity, measured here and printed; nothing
may exceed 1e-4.  The LOGITS are held as well as the probabilities: with p near 0.5 the module's deviation on p is float32's own
rounding, and a bar on p alone would pass a wrong forward.  Outputs sit in guarded arenas and the weights are checked unchanged after
every call.

Measured on an MI355X (device / float32 module on the CPU, normwise unless said otherwise) - the figures are in DESIGN.md section 4z."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import mlp_eval_fwd_ref as fr
import mlp_eval_ref as mr
from sdrm_amd import _lib, mlp_eval
from sdrm_amd.engine import Engine, SdrmError

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # the project's fp32 bar
GUARD, SENTINEL = 8, 12345.0
SHAPE, ARG = -2, -1
CALL_LAUNCHES, SSE_LAUNCHES, BATCH_LAUNCHES = 7, 1, 5   # include/sdrm_hip.h: per call, one more with sse, per batch


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    e = Engine(8, 8, 4, 0, 16)
    yield e
    e.close()


class Arena:
    """float32 arrays carved out of one device buffer, GUARD sentinel elements or more between neighbours and at both ends, every array
    on a 64-element boundary (so on the 16-byte grid)."""

    def __init__(self, arrays):
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        self.offs, at = [], GUARD
        for a in arrays:
            at = -(-at // 64) * 64
            self.offs.append(at)
            at += a.size + GUARD
        self.host = np.full(at, SENTINEL, dtype=np.float32)
        self.inside = np.zeros(at, dtype=bool)
        for o, a in zip(self.offs, arrays):
            self.host[o:o + a.size] = a.ravel()
            self.inside[o:o + a.size] = True
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.views = [self.dev[o:o + a.size].view(a.shape) for o, a in zip(self.offs, arrays)]
        self.shapes = [a.shape for a in arrays]

    def arrays(self):
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[~self.inside], self.host[~self.inside]), "a guard was written"
        return [got[o:o + int(np.prod(s))].reshape(s) for o, s in zip(self.offs, self.shapes)]

    def unchanged(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.host)


def csr_of(engine, name):
    return fr.cached(("csr", name), lambda: engine.csr_to_device(csr_matrix(mr.matrix(name).astype(np.float32))))


def weights_of(name):
    return fr.cached(("arena", name), lambda: Arena([mr.weights(name)[0][t] for t in mr.NAMES]))


def run(engine, name, csr_dev=None, n_out=None, out=True, **kw):
    """One `mlp_eval` call of the case's weights: (out [n, I] float32 numpy | None, sse float | None, launches).  The output sits in a
    guarded arena pre-filled with a sentinel; the weights are checked unchanged."""
    W = weights_of(name)
    n_items = mr.CASES[name][0]
    A = Arena([np.full((n_out, n_items), 777.0, dtype=np.float32)]) if out else None
    n0 = engine.launch_count()
    got = engine.mlp_eval(W.views, csr_of(engine, name) if csr_dev is None else csr_dev, out=A.views[0] if out else False, **kw)
    launches = engine.launch_count() - n0
    W.unchanged()
    sse = None
    if kw.get("sse"):
        sse_t = got[1] if out else got
        assert sse_t.dtype == torch.float64 and sse_t.numel() == 1
        sse = float(sse_t.cpu().numpy()[0])
    return (A.arrays()[0] if out else None), sse, launches


def all_rows(engine, name, batch, logits=False, sse=False):
    return fr.cached(("all", name, batch, logits, sse), lambda: run(engine, name, n_out=mr.CASES[name][1], batch=batch, logits=logits, sse=sse))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ================================================================================================ the forward
@pytest.mark.parametrize("name", list(mr.CASES))
def test_logits_and_probabilities(engine, name):
    o = fr.oracle(name)
    bar, ref = fr.bars(name)
    y, _, _ = all_rows(engine, name, 1024, logits=True)
    p, _, _ = all_rows(engine, name, 1024)
    dev = dict(y=mr.normwise(y, o["y"]), p=mr.normwise(p, o["p"]), p_max=float(np.abs(p.astype(np.float64) - o["p"]).max()))
    for k in ("y", "p", "p_max"):
        print(f"case {name} {k}: device {dev[k]:.3e} reference {ref[k]:.3e} bar {bar[k]:.3e}")
    assert np.isfinite(y).all() and ((p > 0) & (p < 1)).all()
    for k in ("y", "p", "p_max"):
        assert dev[k] <= bar[k] <= TOL, (name, k, dev[k], bar[k])


def test_ragged_calls_give_the_rows_bits(engine):
    name = "B"
    n_items, n_rows, seed = mr.CASES[name]
    assert n_rows == 22
    for logits in (False, True):
        full8, _, launches = all_rows(engine, name, 8, logits=logits)                              # 8 + 8 + 6: the last batch is partial
        assert launches == CALL_LAUNCHES + 3 * BATCH_LAUNCHES
        assert mr.normwise(full8, fr.oracle(name)["y" if logits else "p"]) <= fr.bars(name)[0]["y" if logits else "p"]
        one, _, _ = run(engine, name, n_out=1, row0=13, n=1, batch=8, logits=logits)
        assert np.array_equal(bits(one[0]), bits(full8[13]))
        # a list of 70 ids with repeats, shuffled, in ONE batch: it crosses the 64-row tile
        ids = np.random.default_rng(seed + 11).integers(0, n_rows, size=70).astype(np.int64)
        assert len(set(ids.tolist())) < 70 and len(set(ids.tolist())) > 15
        full70, _, _ = all_rows(engine, name, 70, logits=logits)
        listed, _, launches = run(engine, name, n_out=70, rows=torch.from_numpy(ids).cuda(), batch=70, logits=logits)
        assert launches == CALL_LAUNCHES + BATCH_LAUNCHES
        assert np.array_equal(bits(listed), bits(full70[ids]))
        # row0 / n against the same rows as a list
        ranged, _, _ = run(engine, name, n_out=9, row0=5, n=9, batch=8, logits=logits)
        as_list, _, _ = run(engine, name, n_out=9, rows=torch.arange(5, 14, dtype=torch.int64).cuda(), batch=8, logits=logits)
        assert np.array_equal(bits(ranged), bits(as_list)) and np.array_equal(bits(ranged), bits(full8[5:14]))


# ================================================================================================ the sum of squared errors
@pytest.mark.parametrize("name", list(mr.CASES))
def test_sse(engine, name):
    o = fr.oracle(name)
    bar, ref = fr.bars(name)
    x = mr.matrix(name).astype(np.float64)
    n_rows = mr.CASES[name][1]
    plain, _, _ = all_rows(engine, name, 16)
    out, sse, launches = all_rows(engine, name, 16, sse=True)
    assert launches == CALL_LAUNCHES + SSE_LAUNCHES + -(-n_rows // 16) * BATCH_LAUNCHES
    dev = abs(sse - o["sse"]) / o["sse"]
    print(f"case {name} sse: device {dev:.3e} reference {ref['sse']:.3e} bar {bar['sse']:.3e}")
    assert dev <= bar["sse"] <= TOL
    own = float(((out.astype(np.float64) - x) ** 2).sum())                                         # the identity and the entry walk, apart from the forward
    assert abs(sse - own) <= 1e-12 * own
    assert np.array_equal(bits(out), bits(plain))                                                  # out with sse = out without
    _, again, _ = run(engine, name, n_out=n_rows, batch=16, sse=True)
    assert np.float64(again).view(np.uint64) == np.float64(sse).view(np.uint64)                    # two runs: the same bits
    _, alone, launches = run(engine, name, out=False, batch=16, sse=True)
    assert np.float64(alone).view(np.uint64) == np.float64(sse).view(np.uint64) and launches == CALL_LAUNCHES + SSE_LAUNCHES + -(-n_rows // 16) * BATCH_LAUNCHES
    _, with_logits, _ = run(engine, name, n_out=n_rows, batch=16, sse=True, logits=True)           # sse counts probabilities whatever `logits` says
    assert np.float64(with_logits).view(np.uint64) == np.float64(sse).view(np.uint64)
    # a row range: the validation rows of the fit
    n_fit = mr.n_fit(name)
    part, sse_part, _ = run(engine, name, n_out=n_rows - n_fit, row0=n_fit, batch=16, sse=True)
    own = float(((part.astype(np.float64) - x[n_fit:]) ** 2).sum())
    assert abs(sse_part - own) <= 1e-12 * own and np.array_equal(bits(part), bits(out[n_fit:]))


# ================================================================================================ ranking
@pytest.mark.parametrize("name", ["B", "C"])
def test_ranking_equals_the_oracles(engine, name):
    x, held = mr.matrix(name), fr.held_pattern(name)
    left = fr.users_left_out(name)
    assert not left.any()                                                                          # the rule leaves out NO user (held on the CPU too)
    p, _, _ = all_rows(engine, name, 1024)
    train_dev, held_dev = csr_of(engine, name), engine.csr_to_device(csr_matrix(held.astype(np.float32)))
    got = engine.rank_metrics(torch.from_numpy(p).cuda(), held_dev, train_dev, ks=fr.KS)
    want = engine.rank_metrics(torch.from_numpy(fr.oracle(name)["p"].astype(np.float32)).cuda(), held_dev, train_dev, ks=fr.KS)
    for g, w in zip(got, want):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        assert g.shape == (len(fr.KS), x.shape[0]) and np.array_equal(g, w, equal_nan=True)
        assert np.nanmax(w) > 0


# ================================================================================================ faults in the feed, as data
def test_faults_in_the_feed(engine):
    name = "B"
    n_items, n_rows, _ = mr.CASES[name]
    x = mr.matrix(name)
    clean, clean_sse, _ = all_rows(engine, name, 8, sse=True)
    xd = x.astype(np.float64)

    def own_sse(out, xx):
        return float(((out.astype(np.float64) - xx) ** 2).sum())

    # a row id outside the matrix
    for bad_id in (n_rows, -1):
        ids = np.arange(n_rows, dtype=np.int64)
        ids[4] = bad_id
        out, sse, _ = run(engine, name, n_out=n_rows, rows=torch.from_numpy(ids).cuda(), batch=8, sse=True, check=False)
        with pytest.raises(SdrmError, match="row id outside"):
            engine.feed_status()
        live = np.delete(np.arange(n_rows), 4)
        assert not out[4].any() and np.array_equal(bits(out[live]), bits(clean[live]))
        want = own_sse(out[live], xd[live])
        assert abs(sse - want) <= 1e-12 * want
    # an indptr pair out of order: row v is dead; row v + 1 then starts inside row v and is left out of the call
    m = csr_matrix(x.astype(np.float32))
    m.sort_indices()
    v = 9
    assert m.indptr[v] >= 1 and m.indptr[v + 1] > m.indptr[v]
    indptr = m.indptr.astype(np.int64).copy()
    indptr[v + 1] = indptr[v] - 1
    broken = (torch.from_numpy(indptr).cuda(), torch.from_numpy(m.indices.astype(np.int32)).cuda(), None, m.shape)
    ids = np.delete(np.arange(n_rows, dtype=np.int64), v + 1)
    out, sse, _ = run(engine, name, csr_dev=broken, n_out=n_rows - 1, rows=torch.from_numpy(ids).cuda(), batch=8, sse=True, check=False)
    with pytest.raises(SdrmError, match="indptr pair"):
        engine.feed_status()
    ref8, _, _ = run(engine, name, n_out=n_rows - 1, rows=torch.from_numpy(ids).cuda(), batch=8)   # the clean call over the same list
    at = int(np.flatnonzero(ids == v)[0])
    live = np.delete(np.arange(n_rows - 1), at)
    assert not out[at].any() and np.array_equal(bits(out[live]), bits(ref8[live]))
    want = own_sse(out[live], xd[ids[live]])
    assert abs(sse - want) <= 1e-12 * want
    # ... and one that reaches behind nnz (the last row's)
    indptr = m.indptr.astype(np.int64).copy()
    indptr[-1] += 5
    behind = (torch.from_numpy(indptr).cuda(), torch.from_numpy(np.concatenate([m.indices, np.zeros(5)]).astype(np.int32)).cuda()[:m.nnz], None, m.shape)
    out, sse, _ = run(engine, name, csr_dev=behind, n_out=n_rows, batch=8, sse=True, check=False)
    with pytest.raises(SdrmError, match="indptr pair"):
        engine.feed_status()
    assert not out[-1].any() and np.array_equal(bits(out[:-1]), bits(clean[:-1]))
    want = own_sse(out[:-1], xd[:-1])
    assert abs(sse - want) <= 1e-12 * want
    # a column index outside [0, n_items): that entry is skipped, by the first layer and by the sum
    victim = 2
    assert m.indptr[victim + 1] - m.indptr[victim] >= 2
    at = int(m.indptr[victim])
    lost = int(m.indices[at])
    for bad_col in (n_items + 3, -2):
        indices = m.indices.astype(np.int32).copy()
        indices[at] = bad_col
        csr_dev = (torch.from_numpy(m.indptr.astype(np.int64)).cuda(), torch.from_numpy(indices).cuda(), None, m.shape)
        out, sse, _ = run(engine, name, csr_dev=csr_dev, n_out=n_rows, batch=8, sse=True, check=False)
        with pytest.raises(SdrmError, match="column index outside"):
            engine.feed_status()
        others = np.delete(np.arange(n_rows), victim)
        assert np.array_equal(bits(out[others]), bits(clean[others]))
        xb = x.copy()
        xb[victim, lost] = 0
        y = mr.step64(mr.weights(name)[0], xb[victim:victim + 1], np.ones((1, mr.KEEP_COLS)), p_drop=0.0)["y"]
        assert mr.normwise(out[victim], fr.sigmoid64(y)[0]) <= fr.bars(name)[0]["p"]
        assert not np.array_equal(bits(out[victim]), bits(clean[victim]))
        want = own_sse(out, xb.astype(np.float64))
        assert abs(sse - want) <= 1e-12 * want
    engine.feed_status()                                                                           # the word was cleared
    assert clean_sse > 0


# ================================================================================================ the envelope
def test_refused_calls_launch_nothing_and_accepted_ones_count(engine):
    name = "B"
    n_items, n_rows, _ = mr.CASES[name]
    indptr, indices, _, _ = csr_of(engine, name)
    nnz = int(indices.numel())
    W = weights_of(name)
    O = Arena([np.full((n_rows, n_items), 777.0, dtype=np.float32)])
    sse = torch.full((1,), -5.0, dtype=torch.float64, device="cuda")
    ids = torch.arange(n_rows, dtype=torch.int64).cuda()
    n0 = engine.launch_count()

    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def call(p=None, rows_t=None, row0=0, n=n_rows, batch=8, kind=0, out_t=O.views[0], sse_t=None, nnz_=nnz, m_rows=n_rows, n_users=n_rows, items=n_items,
             ip=indptr, ix=indices):
        rec = _lib.MlpEvalW()
        addrs = p if p is not None else [t.data_ptr() for t in W.views]
        for i in range(9):
            rec.p[i] = addrs[i]
        rec.n_users, rec.n_items = n_users, items
        return engine.lib.sdrm_mlp_eval(engine._h, C.byref(rec), ptr(ip), ptr(ix), nnz_, m_rows, ptr(rows_t), row0, n, batch, kind, ptr(out_t), ptr(sse_t), None)

    for kw in (dict(batch=0), dict(batch=4097), dict(n=0), dict(n=n_rows + 1), dict(row0=-1), dict(row0=n_rows, n=1), dict(row0=3, n=n_rows - 2),
               dict(nnz_=-1), dict(m_rows=0), dict(n_users=1), dict(items=0), dict(items=36865), dict(out_t=None, sse_t=None)):
        assert call(**kw) == SHAPE, kw
    off = [t.data_ptr() for t in W.views]
    off[2] += 4
    assert call(p=off) == SHAPE                                                                    # b1 off the 16-byte grid
    null = [t.data_ptr() for t in W.views]
    null[7] = None
    assert call(p=null) == ARG and call(kind=2) == ARG and call(ip=None) == ARG and call(ix=None) == ARG
    for kw in (dict(batch=0), dict(batch=4097), dict(n=0), dict(row0=20, n=3), dict(out=False)):
        with pytest.raises(SdrmError, match="SDRM_ERR_SHAPE"):
            engine.mlp_eval(W.views, csr_of(engine, name), **kw)
    assert engine.launch_count() == n0
    O.unchanged()
    W.unchanged()
    assert float(sse.cpu()[0]) == -5.0
    assert call() == 0                                                                             # 22 rows in batches of 8: three batches
    torch.cuda.synchronize()
    assert engine.launch_count() == n0 + CALL_LAUNCHES + 3 * BATCH_LAUNCHES
    assert call(rows_t=ids, n=n_rows, batch=4096, sse_t=sse, out_t=None) == 0                      # one batch, the sum alone
    torch.cuda.synchronize()
    assert engine.launch_count() == n0 + 2 * CALL_LAUNCHES + 4 * BATCH_LAUNCHES + SSE_LAUNCHES
    assert float(sse.cpu()[0]) > 0
    W.unchanged()
    assert np.array_equal(bits(O.arrays()[0]), bits(all_rows(engine, name, 8)[0]))
    engine.feed_status()


# ================================================================================================ the driver
def test_driver_evaluates_on_the_device(engine, monkeypatch):
    """`compute_mlp_results_device` at the train driver test's shape (case A's row counts at 77 items), 3 epochs: with the
    torch train loop the trajectory is that of the `compute_mlp_results` run from the same seed - the validation RMSE per epoch within the
    SSE bar, the same best epoch -; then with `device_train=True` as well, `MLP.forward` never runs."""
    seed, n_rows, n_items = 3, 37, 77
    rng = np.random.default_rng(2)
    x = (rng.random((n_rows, n_items)) < 0.2).astype(np.float32)
    training, validation = csr_matrix(x), csr_matrix((rng.random((12, n_items)) < 0.3).astype(np.float32))
    h_t, h_d = {}, {}
    torch_rec = mlp_eval.compute_mlp_results(training, validation, engine=engine, seed=seed, epochs=3, history=h_t)
    dev_rec = mlp_eval.compute_mlp_results_device(training, validation, engine, seed=seed, epochs=3, history=h_d, device_train=False)
    assert h_t["train_loss"] == h_d["train_loss"]                                                  # the same train trajectory
    bar = mr.BAR_FACTOR * fr.sse_level()
    for a, b in zip(h_t["val_rmse"], h_d["val_rmse"]):
        print(f"driver val_rmse: torch {a:.12f} device {b:.12f} relative {abs(a - b) / a:.3e} bar {bar:.3e}")
    assert len(h_d["val_rmse"]) == 3 and all(abs(a - b) <= bar * a for a, b in zip(h_t["val_rmse"], h_d["val_rmse"]))
    assert h_d["best_epoch"] == h_t["best_epoch"] and h_d["epochs_run"] == h_t["epochs_run"] == 3
    assert all(r.shape == (6,) and np.isfinite(r).all() for r in dev_rec) and h_d["per_user"][0].shape == h_t["per_user"][0].shape
    engine.feed_status()

    def forbidden(self, *a, **k):
        raise AssertionError("MLP.forward was called")
    monkeypatch.setattr(mlp_eval.MLP, "forward", forbidden)
    h = {}
    rec, ndcg = mlp_eval.compute_mlp_results_device(training, validation, engine, seed=seed, epochs=3, history=h)
    assert rec.shape == (6,) and ndcg.shape == (6,) and np.isfinite(rec).all() and np.isfinite(ndcg).all()
    assert ((0 <= rec) & (rec <= 1)).all() and ((0 <= ndcg) & (ndcg <= 1)).all()
    assert h["epochs_run"] == 3 and len(h["val_rmse"]) == 3 and all(np.isfinite(h["val_rmse"])) and all(0.3 < r < 0.7 for r in h["val_rmse"])
    engine.feed_status()
