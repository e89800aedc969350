"""Float64 restatement of the optimizer step of the VAE pre-stage (reference train_SDRM.py:126 `torch.optim.Adam(model.parameters(), lr)`,
:143-150), from the formulas, for tests/test_vae_adam.py.  The L2 term of the loss, `wd * sum ||W||^2` over the weights (:262-268), is
folded into the gradient as `g + 2 wd p`; biases carry no coefficient."""
import numpy as np

CHUNK = 4096   # elements per work-group of csrc/vae_adam.h


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, l2_coef=0.0):
    """One Adam update of one tensor in float64: returns (p, m, v) after the step `step` >= 1 (the count after this update)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    g = g + 2.0 * float(l2_coef) * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def chunk_count(ns):
    return sum(-(-int(n) // CHUNK) for n in ns)


def l2_sum(ps, l2_coefs):
    """sum(p^2) in float64 over the tensors with a coefficient."""
    return float(sum((np.asarray(p, dtype=np.float64) ** 2).sum() for p, c in zip(ps, l2_coefs) if c > 0))


def rel_max(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))
