"""float64 statement of ONE whole train step of the VAE pre-stage (reference train_SDRM.py:132-150, :231-264), in plain dense form with
torch's float64 autograd, for tests/test_vae_train_step.py:

    x      = dropout(F.normalize(X, p=2, dim=1))          dropout = keep(R, c) * scale, the restated Philox bits of (drop_seed, step)
    h      = Linear2(tanh(Linear1(x))) ;  mu, logvar = chunk(h, 2, dim=1)
    kl     = -0.5 mean_r(sum_j(1 + logvar - mu^2 - exp(logvar)))
    z      = mu + eps exp(0.5 logvar)                      eps = the restated normals of (latent_seed, step)
    neg_ll = -mean_r(sum_i(log_softmax(Linear4(tanh(Linear3(z))))_i X_i))
    l2     = weight_decay sum_W ||W||^2                    over the four .weight tensors; 0 when weight_decay <= 0
    loss   = neg_ll + anneal kl + l2 ;  the eight gradients are those of neg_ll + anneal kl (the optimizer folds in 2 weight_decay W)

It shares no arithmetic with the piecewise restatements (vae_input_layer_ref, vae_latent_ref, vae_decoder_ref): it takes from them the
randoms alone - `keep_mask`, `scale`, `draw_eps` -, which are held to the kernels' draws by their own tests.  Beside it: the float64
Adam, the replay of what `train_variational_autoencoder` draws from `np.random` with all flags on, and the shapes S1 .. S5 made from
seeds."""
import functools

import numpy as np
import torch
from torch.nn import functional as F

import vae_adam_ref
import vae_decoder_ref
import vae_input_layer_ref as vil
import vae_latent_ref as vlr
from sdrm_amd import synth
from vae_encode_ref import rel_l2, rel_max  # noqa: F401  (the tests take the error measures from here)

NAMES = ("encoder.0.weight", "encoder.0.bias", "encoder.2.weight", "encoder.2.bias",
         "decoder.0.weight", "decoder.0.bias", "decoder.2.weight", "decoder.2.bias")     # `VAE.named_parameters()`'s order
SHORT = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")
ANNEAL_CAP, ANNEAL_STEPS = 0.2, 20_000
LR = 1e-3
EPOCHS = 2

# name: (users, items, hidden, latent, batch, ratings (values 1..5; else all ones), an empty and a full row, p_drop, weight_decay)
SHAPES = {
    "S1": (65, 131, 37, 5, 32, False, False, 0.5, 0.0),     # no width on any grid; a last batch of ONE row
    "S2": (150, 1283, 200, 40, 64, True, True, 0.5, 0.01),  # ADM's widths, odd items > 1024, several row tiles, L2 in loss and update
    "S3": (70, 1009, 600, 83, 33, False, False, 0.3, 0.0),  # odd latent (the mu | logvar boundary off 16 bytes), p_drop != 0.5
    "S4": (40, 70, 2052, 16, 16, True, False, 0.5, 0.0),    # hidden above 2048: the input layer's second pass
    "S5": (40, 70, 48, 8, 16, False, False, 0.0, 0.0),      # no dropout: every bit kept, scale 1
}


def schedule(np_seed, users, batch, epochs=EPOCHS):
    """What `train_variational_autoencoder` draws from `np.random` after `np.random.seed(np_seed)` with all flags on: three
    `randint(2**63, dtype=int64)` - the drop, hold-out and latent seeds, in that order - and then one `permutation(users)` per epoch,
    applied cumulatively.  dict of the three seeds, `orders` (one int64 [users] per epoch), `steps`: per step (rows = order[lo:lo + batch],
    step = the running count, anneal = min(0.2, count / 20000)), and `places`: per step (the epoch, lo)."""
    rs = np.random.RandomState(np_seed)
    drop_seed, holdout_seed, latent_seed = (int(rs.randint(2 ** 63, dtype=np.int64)) for _ in range(3))
    order, orders, steps, places, count = np.arange(users), [], [], [], 0
    for epoch in range(epochs):
        order = order[rs.permutation(users)]
        orders.append(order.astype(np.int64))
        for lo in range(0, users, batch):
            steps.append((orders[-1][lo:lo + batch].copy(), count, min(ANNEAL_CAP, 1.0 * count / ANNEAL_STEPS)))
            places.append((epoch, lo))
            count += 1
    return dict(drop_seed=drop_seed, holdout_seed=holdout_seed, latent_seed=latent_seed, orders=orders, steps=steps, places=places)


@functools.lru_cache(maxsize=None)
def shape_inputs(name):
    """dict of shape `name`: `tensors` (the eight float32 arrays in NAMES' order), `m` (the scipy feed [users, items]), the dims,
    p_drop, weight_decay, np_seed and `sched` = schedule(np_seed, users, batch).  A feed with an empty and a full row holds both in
    the first epoch's first batch.  Shared by the tests: nobody writes into it."""
    users, items, hidden, latent, batch, ratings, special, p_drop, weight_decay = SHAPES[name]
    k = sorted(SHAPES).index(name)
    np_seed = 2200 + k
    sched = schedule(np_seed, users, batch)
    if special:
        first = sched["steps"][0][0]
        m = vae_decoder_ref.feed_of(users, items, 2300 + k, ratings, int(first[1]), int(first[-2]))
    else:
        m = synth.synth_feed_csr(users, items, 0.1, seed=2300 + k, ratings=ratings)
    tensors = synth.synth_vae_encoder(items, hidden, latent, seed=2400 + k) + synth.synth_vae_decoder(latent, hidden, items, seed=2500 + k)
    return dict(name=name, tensors=tuple(tensors), m=m, users=users, items=items, hidden=hidden, latent=latent, batch=batch,
                p_drop=p_drop, weight_decay=weight_decay, np_seed=np_seed, sched=sched)


def stored_and_kept(m, rows, drop_seed, step, p_drop):
    """bool [len(rows), items]: the entries of the feed rows `rows` that are stored AND kept by the restated dropout bits."""
    pattern = m[np.asarray(rows)].copy()
    pattern.data = np.ones_like(pattern.data)
    return (np.asarray(pattern.toarray()) != 0) & vil.keep_mask(drop_seed, step, rows, m.shape[1], p_drop)


def train_step(tensors, m, rows, drop_seed, latent_seed, step, anneal, p_drop, weight_decay, drop_scale=None):
    """One train step at the eight tensors (any float dtype, used as float64) for the feed rows `rows` of the scipy matrix `m`:
    dict of neg_ll, kl, l2, loss (floats) and `grads`, the eight float64 arrays of d(neg_ll + anneal kl).  `drop_scale`: the factor of
    a kept entry, default the reference's 1 / (1 - p) as `vae_input_layer_ref.scale` rounds it (another value only to show that a bar
    notices it)."""
    rows = np.asarray(rows, np.int64)
    params = [torch.tensor(np.asarray(t, dtype=np.float64), dtype=torch.float64, requires_grad=True) for t in tensors]
    w1, b1, w2, b2, w3, b3, w4, b4 = params
    X = torch.from_numpy(np.asarray(m[rows].toarray(), np.float64))
    keep = torch.from_numpy(vil.keep_mask(drop_seed, step, rows, m.shape[1], p_drop).astype(np.float64))
    drop_scale = float(vil.scale(p_drop)) if drop_scale is None else float(drop_scale)
    x = F.normalize(X, p=2, dim=1) * keep * drop_scale
    h = F.linear(torch.tanh(F.linear(x, w1, b1)), w2, b2)
    mu, logvar = torch.chunk(h, chunks=2, dim=1)
    kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
    eps = torch.from_numpy(np.asarray(vlr.draw_eps(latent_seed, step, rows, mu.shape[1]), np.float64))
    z = mu + eps * torch.exp(0.5 * logvar)
    out = F.linear(torch.tanh(F.linear(z, w3, b3)), w4, b4)
    neg_ll = -torch.mean(torch.sum(F.log_softmax(out, dim=1) * X, dim=1))
    grads = torch.autograd.grad(neg_ll + float(anneal) * kl, params)
    l2 = 0.0
    if weight_decay > 0:
        l2 = float(weight_decay) * float(sum((p.detach() ** 2).sum() for p, n in zip(params, NAMES) if n.endswith(".weight")))
    neg_ll, kl = float(neg_ll.detach()), float(kl.detach())
    return dict(neg_ll=neg_ll, kl=kl, l2=l2, loss=neg_ll + float(anneal) * kl + l2, grads=[g.numpy() for g in grads])


def l2_coefs(weight_decay):
    """Per tensor the coefficient c of the loss term c sum(p^2) that the optimizer folds into the gradient as 2 c p: `weight_decay` for
    the weights, rounded to float32 - the type in which the engine's call takes it, and in which the reference's fp32 autograd
    multiplies by it.  The rounding is an INPUT, not noise: where 2 c p cancels g to within Adam's eps the update
    lr g' / (|g'| + eps) turns the 2e-8 between 0.01 and float32(0.01) into 1e-4 of a whole update (tests/test_vae_train_step.py
    shows it on the CPU)."""
    c = float(np.float32(weight_decay))
    return [c if (n.endswith(".weight") and weight_decay > 0) else 0.0 for n in NAMES]


def adam(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, l2_coef=0.0):
    """float64 Adam of one tensor with g + 2 l2_coef p as the effective gradient: (p, m, v) after the step `step` >= 1."""
    return vae_adam_ref.adam_step(p, g, m, v, step, lr, betas=betas, eps=eps, l2_coef=l2_coef)


def free_run(tensors, m, steps, drop_seed, latent_seed, p_drop, weight_decay, lr=LR):
    """The oracle running on its own float64 state from `tensors` through `steps` ((rows, step, anneal) each): per step a dict of
    `train_step`'s result plus `after`, the eight float64 parameters after the update."""
    ps = [np.asarray(t, np.float64) for t in tensors]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    coefs, out = l2_coefs(weight_decay), []
    for k, (rows, step, anneal) in enumerate(steps):
        res = train_step(ps, m, rows, drop_seed, latent_seed, step, anneal, p_drop, weight_decay)
        upd = [adam(p, g, mm, v, k + 1, lr, l2_coef=c) for p, g, mm, v, c in zip(ps, res["grads"], ms, vs, coefs)]
        ps, ms, vs = [u[0] for u in upd], [u[1] for u in upd], [u[2] for u in upd]
        res["after"] = ps
        out.append(res)
    return out


def piecewise_step(tensors, m, rows, drop_seed, latent_seed, step, anneal, p_drop, weight_decay):
    """The same step as the composition the kernels' own tests pin: vae_input_layer_ref -> vae_latent_ref -> vae_decoder_ref, backward
    with scale 1, gz = dz, gkl = anneal.  (loss, the eight gradients)."""
    w1, b1, w2, b2, w3, b3, w4, b4 = tensors
    rows = np.asarray(rows, np.int64)
    X = np.asarray(m[rows].toarray(), np.float64)
    pre, _, xt = vil.forward(w1, b1, m, rows, drop_seed, step, p_drop)
    eps = vlr.draw_eps(latent_seed, step, rows, np.asarray(w2).shape[0] // 2)
    lat = vlr.forward(pre, w2, b2, eps)
    dec = vae_decoder_ref.forward(lat["z"], w3, b3, w4, b4, X)
    dback = vae_decoder_ref.backward(dec, lat["z"], w3, w4, X, scale=1.0)
    lback = vlr.backward(lat, w2, eps, dback["dz"], anneal)
    dw1, db1 = vil.backward(xt, lback["dpre"])
    l2 = weight_decay * vae_adam_ref.l2_sum(tensors, l2_coefs(weight_decay)) if weight_decay > 0 else 0.0
    loss = float(dec["loss"]) + float(anneal) * float(lat["kl"]) + l2
    return loss, [dw1, db1, lback["dw2"], lback["db2"], dback["dw3"], dback["db3"], dback["dw4"], dback["db4"]]
