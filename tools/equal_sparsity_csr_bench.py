#!/usr/bin/env python3
"""Equal-sparsity output as CSR (csrc/compact.h) against the dense entry point (csrc/select.h), at the BASELINE shapes, in ONE process:
  (a) device time per call, HIP events around windows of back-to-back calls: sdrm_equal_sparsity_csr_begin + _end (threshold, bit
      mask + row counts, scan, fill - and the one 8-byte readback in the middle, which is part of the call) against
      sdrm_equal_sparsity (threshold + binarise); the threshold alone (out = null) is timed beside them, so that the part behind
      it can be read off either one;
  (b) wall time from device scores to a host object, a device synchronise before the clock starts and the object in hand when it
      stops: pipeline.equal_sparsity_csr (a csr_matrix) against pipeline.equal_sparsity (the dense int array) and against
      csr_matrix(pipeline.equal_sparsity(...)) - what a consumer of the dense result pays today for the same object.
The versions alternate inside every repeat (other work shares the host); medians and the spread (min .. max) over the repeats.
Algorithmic bytes behind the threshold: mask sweep 4 + 1/8 B per element (+ the fill: the mask again and 4 B per index) against 5 B
per element of the binarise."""
import ctypes as C
import json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scipy.sparse import csr_matrix
from sdrm_amd import pipeline, synth
from sdrm_amd.engine import Engine, _ptr, _stream

SHAPES = {"ML-100k": (843, 1008, 0.937), "ML-1M": (5429, 3125, 0.9553), "ADM": (9558, 8582, 0.9877)}
WINDOWS, HOST_REPS = 7, 5


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    ms = (time.perf_counter() - t) * 1e3
    return ms, out


def summary(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


e = Engine(8, 8, 4, 0, 16)
res = {}
for name, (users, items, q) in SHAPES.items():
    n = users * items
    M = synth.synth_scores(users, items, seed=3)
    x = torch.from_numpy(M).cuda()
    thr = torch.empty((), dtype=torch.float32, device="cuda")

    def threshold_only():
        e._check(e.lib.sdrm_equal_sparsity(e._h, _ptr(x), n, q, None, _ptr(thr), _stream()), "sdrm_equal_sparsity")
    fns = {"threshold_only": threshold_only, "dense": lambda: e.equal_sparsity(x, q), "csr": lambda: e.equal_sparsity_csr(x, q)}
    reps = max(20, int(0.3 / (n * 17 / 4e12 + 60e-6)))        # windows of about 0.3 s and more
    for fn in fns.values():                                    # warm-up: every kernel of every version, the workspace grown
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dev = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            dev[k].append(window_us(fn, reps))
    indptr, indices, _ = e.equal_sparsity_csr(x, q)
    nnz = int(indices.numel())
    host = {"pipeline.equal_sparsity_csr": [], "pipeline.equal_sparsity": [], "csr_matrix(pipeline.equal_sparsity)": []}
    for _ in range(HOST_REPS):
        ms, got = wall_ms(lambda: pipeline.equal_sparsity_csr(x, q, e))
        host["pipeline.equal_sparsity_csr"].append(ms)
        ms, dense = wall_ms(lambda: pipeline.equal_sparsity(x, q, e))
        host["pipeline.equal_sparsity"].append(ms)
        ms, want = wall_ms(lambda: csr_matrix(pipeline.equal_sparsity(x, q, e)))
        host["csr_matrix(pipeline.equal_sparsity)"].append(ms)
    want.sort_indices()
    assert got.nnz == want.nnz == nnz and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(dense, (M >= np.quantile(M.flatten(), q)).astype(int))
    d = {k: summary(v) for k, v in dev.items()}
    behind_csr = d["csr"]["median"] - d["threshold_only"]["median"]
    behind_dense = d["dense"]["median"] - d["threshold_only"]["median"]
    res[name] = {"users": users, "items": items, "q": q, "nnz": nnz, "calls_per_window": reps, "windows": WINDOWS,
                 "device_us": d,
                 "behind_threshold_us": {"csr (mask + scan + readback + fill)": round(behind_csr, 1), "dense (binarise)": round(behind_dense, 1)},
                 "algorithmic_MB_behind_threshold": {"csr": round((n * 4.125 + n / 8 + nnz * 4 + users * 20) / 1e6, 1), "dense": round(n * 5 / 1e6, 1)},
                 "host_object_ms": {k: summary(v, 2) for k, v in host.items()},
                 "bytes_to_host": {"csr": int(nnz * 4 + (users + 1) * 8), "dense": n}}
    print(name, json.dumps(res[name]), flush=True)
print(json.dumps(res))
