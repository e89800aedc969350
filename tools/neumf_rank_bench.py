#!/usr/bin/env python3
"""The NeuMF arm's ranking problem, built and selected on the device and on the host, at the ML-1M shape of tools/neumf_triples_bench.py:
both tails of a 6040 x 3706 matrix of scores at the training sparsity and the training half of 604 validation users; the validation
triples are the other half.

In one process, alternating, WARM warm-ups and REPS timed repeats each, two legs:

  (a) build, once per driver call
      device  `neumf.DeviceRankingProblem.build` as the route calls it (validation triples uploaded, ONE sdrm_neumf_rank_problem call, the
              32-byte counts read back), host clock around a device synchronise; and the C call alone into reused buffers between two
              device events, nothing read back inside the window;
      host    what it replaces: both tails' indptr / indices to the host, `item_present` to the host, `RankingProblem.from_parts`;
  (b) one epoch's ranking, `present` -> per-user recall on the host
      device  `rank_all_items(model, ..., present, engine, problem=<DeviceRankingProblem>)`: the mask compacted on the device, one
              neumf_scores call, sdrm_rank_metrics_rows with the footing, the metrics read back;
      host    what it replaces: `np.flatnonzero(present.cpu())`, `RankingProblem.select`, two `csr_to_device` uploads, the same neumf_scores
              call, `rank_metrics`, the metrics read back, the footing on the host.
      Both legs of (b) hold the same neumf_scores call; it is timed alone beside them.

`--trace-loop N` runs only N device builds and N device rankings (for a run under a kernel trace); `--out FILE` appends the table to FILE
(profiles/neumf_rank_bench.txt is such a file)."""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch
from scipy.sparse import csr_matrix

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdrm_amd import _lib, neumf  # noqa: E402
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


def beyond(slow, fast):
    return "yes" if min(slow) - max(fast) > max(max(slow) - min(slow), max(fast) - min(fast)) else "NO"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-loop", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "neumf_rank_bench needs the GPU"
    eng = utility_engine()
    dev = eng.device
    sparsity = 1.0 - RATINGS / (USERS * ITEMS)
    raw = torch.randn(USERS, ITEMS, generator=torch.Generator().manual_seed(0)).to(dev)
    ones_dev = eng.equal_sparsity_csr(raw, sparsity, side=">=")
    zeros_dev = eng.equal_sparsity_csr(raw, 1.0 - sparsity, side="<=")
    rng = np.random.default_rng(0)
    valid = (rng.random((VALID_USERS, ITEMS)) < RATINGS / (USERS * ITEMS)).astype(np.float64)
    valid[:, :2] = 1.0
    parts_host, validation = neumf.synthetic_parts_host((USERS, ITEMS), csr_matrix(valid), csr_matrix((USERS, ITEMS)), csr_matrix((USERS, ITEMS)))
    valid_train, offset, _ = parts_host[2]
    device_parts = [(zeros_dev, 0, 0), (ones_dev, 0, 1), (eng.csr_to_device(valid_train), offset, 1)]
    training_dev, counts, item_present = eng.neumf_triples(device_parts, ITEMS)
    n_users, n_items = counts[2], counts[3]

    def host_pattern(d):
        indptr, indices = d[0].cpu().numpy(), d[1].cpu().numpy()
        return csr_matrix((np.ones(indices.shape[0], dtype=np.float32), indices, indptr), shape=d[2])

    def build_host():
        host_parts = [(host_pattern(zeros_dev), 0, 0), (host_pattern(ones_dev), 0, 1), (valid_train, offset, 1)]
        return neumf.RankingProblem.from_parts(host_parts, np.flatnonzero(item_present.cpu().numpy()), validation)

    def build_device():
        return neumf.DeviceRankingProblem.build(eng, device_parts, ITEMS, item_present, validation, n_users)

    host_problem, device_problem = build_host(), build_device()
    check = device_problem.to_host()
    assert np.array_equal(check.cols, host_problem.cols)
    for x, y in zip(check._relevant + check._seen, host_problem._relevant + host_problem._seen):
        assert x.dtype == y.dtype and np.array_equal(x, y)

    # the C call alone, buffers reused, nothing read back
    desc = (_lib.TriplePart * 3)()
    for d, (csr, user0, label) in zip(desc, device_parts):
        d.indptr, d.indices, d.n_rows, d.capacity, d.user0, d.label = csr[0].data_ptr(), csr[1].data_ptr(), int(csr[-1][0]), csr[1].numel(), user0, label
    cap = sum(p[0][1].numel() for p in device_parts)
    val_dev = torch.from_numpy(np.ascontiguousarray(validation, dtype=np.int32)).to(dev)
    bufs = [torch.empty(ITEMS, dtype=torch.int32, device=dev), torch.empty(n_users + 1, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
            torch.empty(n_users + 1, dtype=torch.int64, device=dev), torch.empty(val_dev.shape[0], dtype=torch.int32, device=dev),
            torch.empty(4, dtype=torch.int64, device=dev)]
    p = [C.c_void_p(b.data_ptr()) for b in bufs]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = eng.lib.sdrm_neumf_rank_problem(eng._h, desc, 3, ITEMS, C.c_void_p(item_present.data_ptr()), C.c_void_p(val_dev.data_ptr()), val_dev.shape[0],
                                             n_users, p[0], ITEMS, p[1], p[2], cap, p[3], p[4], val_dev.shape[0], p[5], stream)
        assert rc == 0

    # an epoch's mask and a model
    n_train = int(training_dev.shape[0])
    _, _, _, present = eng.neumf_epoch_draw(training_dev, int(math.ceil(0.2 * n_train)), seed=0, epoch=0, n_users=n_users)
    torch.manual_seed(0)
    model = neumf.NCF(n_users, n_items).to(dev).eval()

    def rank_device():
        return neumf.rank_all_items(model, None, None, present, eng, problem=device_problem)

    def rank_host():
        return neumf.rank_all_items(model, None, None, np.flatnonzero(present.cpu().numpy()), eng, problem=host_problem)

    got, want = rank_device(), rank_host()
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True)
    n_ranked = got[0].shape[1]

    if args.trace_loop:
        for _ in range(args.trace_loop):
            call()
            rank_device()
        torch.cuda.synchronize()
        return

    users_dev = eng.neumf_rank_users(present)
    weights = model.engine_weights(dev)

    def scores_only():
        eng.neumf_scores(weights, users_dev, device_problem.cols, check=False)

    ev, empty, b_dev, b_host, r_dev, r_host, sc = [], [], [], [], [], [], []
    for rep in range(WARM + REPS):
        e0 = event_ms(lambda: None, INNER)
        e1 = event_ms(call, INNER)
        t = [host_ms(build_device), host_ms(build_host), host_ms(rank_device), host_ms(rank_host), host_ms(scores_only)]
        if rep >= WARM:
            empty.append(e0); ev.append(e1)
            for lst, v in zip((b_dev, b_host, r_dev, r_host, sc), t):
                lst.append(v)
    eng.feed_status()

    wpr = -(-ITEMS // 64)
    table_b = n_users * wpr * 8
    rows = sum(int(p_[0][-1][0]) for p_ in device_parts)
    lines = [f"ML-1M shape: {USERS} x {ITEMS}, sparsity {sparsity:.4f}; {rows} part rows, {cap} entries, {val_dev.shape[0]} validation triples; n_users {n_users}, "
             f"C = {device_problem.counts[0]} columns, seen {device_problem.counts[1]} entries, relevant {device_problem.counts[2]}; one bit table {table_b / 1e6:.2f} MB",
             f"an epoch's mask names {n_ranked} users: a score matrix of {n_ranked} x {device_problem.counts[0]} float32, {n_ranked * device_problem.counts[0] * 4 / 1e6:.1f} MB",
             f"{'':<86}{'median (min .. max)':>34}",
             f"{'(a) sdrm_neumf_rank_problem, device events, us per call (' + str(INNER) + ' calls per window)':<86}{spread(ev, 1e3, 1):>34}",
             f"{'    the same window around nothing, us per call':<86}{spread(empty, 1e3, 1):>34}",
             f"{'(a) device: DeviceRankingProblem.build (upload, call, 32-byte readback), host ms':<86}{spread(b_dev):>34}",
             f"{'(a) host: both tails + item_present to the host, RankingProblem.from_parts, host ms':<86}{spread(b_host):>34}",
             f"{'    host / device':<86}{np.median(b_host) / np.median(b_dev):>33.1f}x",
             f"{'    gap beyond both spreads':<86}{beyond(b_host, b_dev):>34}",
             f"{'(b) device: present -> recall on the host through the device problem, host ms':<86}{spread(r_dev):>34}",
             f"{'(b) host: flatnonzero + select + 2 csr_to_device + rank_metrics + host footing, host ms':<86}{spread(r_host):>34}",
             f"{'    (in both: the one neumf_scores call, host ms)':<86}{spread(sc):>34}",
             f"{'    host / device':<86}{np.median(r_host) / np.median(r_dev):>33.1f}x",
             f"{'    gap beyond both spreads':<86}{beyond(r_host, r_dev):>34}"]
    text = "\n".join(lines) + "\n\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
