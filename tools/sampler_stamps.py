#!/usr/bin/env python3
"""Diagnostic (stamped build, never benchmarked): where a work-group of the sampler's GEMM launches spends its cycles - the
engine's own launches inside a PHILOX sampling call, one row chain so that a launch is stamped alone.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -DSDRM_STAMPS=2 -DSDRM_SOURCE_HASH='"stamps"' -o tools/libsdrm_stamps.so sdrm_amd/csrc/sdrm_hip.hip -ldl
    python tools/sampler_stamps.py          (env N rows of the call, L, T, H; STAMPLIB another stamped build)

Per launch class (layer 0, hidden, out + fused reverse update) the LAST launch of the call is kept: a work-group's lifetime in
shader cycles = prologue (entry -> first K-step's fragments read; with the split of -DSDRM_STAMPS=2: -> first loads issued
-> first K-step in LDS ->) + K loop + epilogue (behind the last MFMA -> the work-group's stores acknowledged)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STAMPLIB = os.path.abspath(os.environ.get("STAMPLIB", "tools/libsdrm_stamps.so"))
os.environ["SDRM_LIB"] = STAMPLIB   # (sdrm_amd/_lib.py: another build of the same ABI, loaded as it is)
from sdrm_amd import _lib, synth  # noqa: E402
from sdrm_amd.engine import Engine  # noqa: E402

N, L, T, H = (int(os.environ.get(k, d)) for k, d in (("N", 2715), ("L", 340), ("T", 78), ("H", 1)))
lib = _lib.load()
lib.sdrm_debug_wgrad_stamps_read.restype = C.c_int
e = Engine(L, L, T, H, int(os.environ.get("B", 8192)))
e.set_params(synth.flatten_params(synth.init_params(L, L, T, H, seed=1), H))
e.debug_set(chains=1)
for k in range(int(os.environ.get("WARM", 40))):   # ~ 2 s of launches: the clock the chip holds under this load
    e.sample(N, seed=3, call_id=k)
torch.cuda.synchronize()
mb = 8192
print(f"{STAMPLIB}: sampling call of {N} rows, L={L} T={T} H={H}, one chain")
for cls, name in ((6, "layer 0"), (7, "hidden"), (8, "out + reverse update")):
    lib.sdrm_debug_stamp_class(cls)
    assert lib.sdrm_debug_wgrad_stamps_begin(mb) == 0
    e.sample(N, seed=3, call_id=1000 + cls)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * (8 * mb))()
    nb = lib.sdrm_debug_wgrad_stamps_read(buf, mb)
    if nb <= 0:
        print(f"  class {cls} ({name}): no stamps ({nb})")
        continue
    a = np.frombuffer(buf, dtype=np.uint64).reshape(mb, 8)[:nb].astype(np.int64)
    a = a[a[:, 3] > 0]
    pro, loop, epi = a[:, 1] - a[:, 0], a[:, 2] - a[:, 1], a[:, 3] - a[:, 2]
    life, real = a[:, 3] - a[:, 0], a[:, 5] - a[:, 4]
    clk = np.median(life[real > 0] / real[real > 0]) * 0.1
    wall_us = (a[:, 5].max() - a[:, 4].min()) / 100.0
    p = lambda v, q: np.percentile(v, q)  # noqa: E731
    print(f"  class {cls} ({name}): grid {nb}; launch wall {wall_us:.1f} us; clock {clk:.3f} GHz; lifetime med {np.median(life):.0f} cyc = "
          f"prologue {np.median(pro):.0f} + loop {np.median(loop):.0f} + epilogue {np.median(epi):.0f} (p10 {p(epi, 10):.0f}, p90 {p(epi, 90):.0f}; "
          f"{np.median(epi) / clk / 1e3:.2f} us)")
    if (a[:, 6] > a[:, 0]).all() and (a[:, 7] >= a[:, 6]).all():   # -DSDRM_STAMPS=2: slots 6 / 7 are cycle stamps inside the prologue
        print(f"      prologue: entry -> first loads issued {np.median(a[:, 6] - a[:, 0]):.0f}, -> first K-step in LDS {np.median(a[:, 7] - a[:, 6]):.0f}, "
              f"-> fragments read {np.median(a[:, 1] - a[:, 7]):.0f}")
e.close()
