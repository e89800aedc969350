#!/usr/bin/env python3
"""The NeuMF arm's training triples, assembled on the device and on the host, at the ML-1M shape: both tails of a 6040 x 3706 matrix of
scores at the training sparsity (1 - 1000209 / (6040 x 3706)) and the training half, 80 % of the entries, of 604 validation users.

In one process, alternating, WARM warm-ups and REPS timed repeats each:

  device   ONE sdrm_neumf_triples call (csrc/neumf_triples.h) on the three device-resident CSR parts into a reused buffer, with
           item_present: two device events around the call, nothing read back inside the window (the event pair's own cost, measured around
           nothing, stands beside it); and `Engine.neumf_triples` as the route calls it, buffers allocated and the 32-byte counts read
           back, on the host clock around a device synchronise;
  host     what it replaces: `neumf.assemble_triples` on the three host-resident scipy parts, then the int32 cast and the upload that
           `compute_neuralcf_results(device_draw=True)` makes of its `training` array; host clock, ends in a device synchronise.  The
           copy of the two tails from the device to the host, which a caller of the host form pays first, is timed separately.

The byte counts are the algorithm's, from the shapes: per triple 4 B of indices read and 12 B written, per row two 8-byte indptr reads in
each of the two passes, a 4-byte length and two 8-byte bases written and one of each read again, and n_items bytes of item_present.
`--out FILE` appends the table to FILE (profiles/neumf_triples_bench.txt is such a file)."""
import argparse
import os
import sys
import time

import numpy as np
import torch
from scipy.sparse import csr_matrix

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import neumf  # noqa: E402
from sdrm_amd.engine import utility_engine  # noqa: E402

USERS, ITEMS, RATINGS, VALID_USERS = 6040, 3706, 1000209, 604
WARM, REPS, INNER = 3, 20, 20


def spread(v, unit=1.0, digits=3):
    v = np.asarray(v) * unit
    return f"{np.median(v):.{digits}f} ({v.min():.{digits}f} .. {v.max():.{digits}f})"


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, inner):
    """Device time of `inner` consecutive calls of fn between two events, per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "neumf_triples_bench needs the GPU"
    eng = utility_engine()
    dev = eng.device
    sparsity = 1.0 - RATINGS / (USERS * ITEMS)
    raw = torch.randn(USERS, ITEMS, generator=torch.Generator().manual_seed(0)).to(dev)
    ones_dev = eng.equal_sparsity_csr(raw, sparsity, side=">=")
    zeros_dev = eng.equal_sparsity_csr(raw, 1.0 - sparsity, side="<=")
    rng = np.random.default_rng(0)
    valid = (rng.random((VALID_USERS, ITEMS)) < RATINGS / (USERS * ITEMS)).astype(np.float64)
    valid[:, :2] = 1.0
    parts_host, _ = neumf.synthetic_parts_host((USERS, ITEMS), csr_matrix(valid), csr_matrix((USERS, ITEMS)), csr_matrix((USERS, ITEMS)))
    valid_train, offset, _ = parts_host[2]
    valid_dev = eng.csr_to_device(valid_train)
    device_parts = [(zeros_dev, 0, 0), (ones_dev, 0, 1), (valid_dev, offset, 1)]

    def to_host(d):
        return csr_matrix((np.ones(d[1].numel(), dtype=np.float32), d[1].cpu().numpy(), d[0].cpu().numpy()), shape=d[2])
    pull_ms = [host_ms(lambda: (to_host(zeros_dev), to_host(ones_dev))) for _ in range(WARM + 5)][WARM:]
    host_parts = [(to_host(zeros_dev), 0, 0), (to_host(ones_dev), 0, 1), (valid_train, offset, 1)]
    rows = sum(p[0].shape[0] for p in host_parts)
    m = sum(p[0].nnz for p in host_parts)

    out = torch.empty(m, 3, dtype=torch.int32, device=dev)
    triples, counts, present = eng.neumf_triples(device_parts, ITEMS, out=out)
    want, dims = neumf.assemble_triples(host_parts)
    assert counts == (m, host_parts[1][0].nnz + valid_train.nnz) + dims and np.array_equal(triples.cpu().numpy(), want.astype(np.int32))
    assert np.array_equal(np.flatnonzero(present.cpu().numpy()), np.unique(want[:, 1]))

    # the C call alone, buffers reused, nothing read back: Engine.neumf_triples' own launch path with the readback taken out
    import ctypes as C
    from sdrm_amd import _lib
    desc = (_lib.TriplePart * 3)()
    for d, (csr, user0, label) in zip(desc, device_parts):
        d.indptr, d.indices, d.n_rows, d.capacity, d.user0, d.label = csr[0].data_ptr(), csr[1].data_ptr(), int(csr[-1][0]), csr[1].numel(), user0, label
    counts_dev = torch.empty(4, dtype=torch.int64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = eng.lib.sdrm_neumf_triples(eng._h, desc, 3, ITEMS, C.c_void_p(out.data_ptr()), m, C.c_void_p(present.data_ptr()), C.c_void_p(counts_dev.data_ptr()),
                                        stream)
        assert rc == 0

    def host_form():
        t, _ = neumf.assemble_triples(host_parts)
        return torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(dev)

    ev, empty, wrapped, hosted = [], [], [], []
    for rep in range(WARM + REPS):
        e0 = event_ms(lambda: None, INNER)
        e1 = event_ms(call, INNER)
        w = host_ms(lambda: eng.neumf_triples(device_parts, ITEMS, check=False))
        h = host_ms(host_form)
        if rep >= WARM:
            empty.append(e0); ev.append(e1); wrapped.append(w); hosted.append(h)
    eng.feed_status()
    eng.profile_begin(capacity=64)
    for _ in range(5):
        call()
    prof = {k: val[0] / val[1] for k, val in eng.profile_end().items() if k.startswith("neumf triples")}

    read_b = 4 * m + rows * (2 * 16 + 4 + 8)
    write_b = 12 * m + rows * (4 + 16) + ITEMS + 32
    call_us = float(np.median(ev)) * 1e3
    lines = [f"ML-1M shape: {USERS} x {ITEMS}, sparsity {sparsity:.4f}; parts (rows, entries): " + ", ".join(f"({p[0].shape[0]}, {p[0].nnz})" for p in host_parts)
             + f"; {rows} rows, m = {m} triples",
             f"bytes of one call, from the shapes: {read_b} read + {write_b} written = {(read_b + write_b) / 1e6:.1f} MB (the triples alone: {16 * m / 1e6:.1f} MB)",
             f"{'':<66}{'median (min .. max)':>34}",
             f"{'sdrm_neumf_triples, device events, us per call (' + str(INNER) + ' calls per window)':<66}{spread(ev, 1e3, 1):>34}",
             f"{'  the same window around nothing, us per call':<66}{spread(empty, 1e3, 1):>34}",
             f"{'  the call as ONE profile interval (3 memsets + 3 launches), us':<66}{', '.join(f'{v * 1e3:.1f}' for v in prof.values()):>34}",
             f"{'  achieved, the bytes above over the event time':<66}{(read_b + write_b) / (call_us * 1e-6) / 1e12:>30.2f} TB/s",
             f"{'Engine.neumf_triples (allocations, call, 32-byte readback), host ms':<66}{spread(wrapped):>34}",
             f"{'host: assemble_triples + int32 cast + upload, host ms':<66}{spread(hosted):>34}",
             f"{'  (before it, both tails device -> host as scipy CSR, host ms)':<66}{spread(pull_ms):>34}",
             f"{'host form / Engine.neumf_triples':<66}{np.median(hosted) / np.median(wrapped):>33.1f}x",
             f"{'gap beyond both spreads':<66}{'yes' if min(hosted) - max(wrapped) > max(max(hosted) - min(hosted), max(wrapped) - min(wrapped)) else 'NO':>34}"]
    text = "\n".join(lines) + "\n\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
