"""The feature-table optimizers restated in numpy float32: one function per kind, the touched rule, the `lazy` flag.

The sequence of operations is the contract (include/svoxt.h): every + - * / sqrt below is one correctly
rounded float32 operation, in the kernel's order, so the results are the kernel's bits.  Scalars with a hat are computed
in double precision and rounded to float32 once; t is the 1-based count of steps.

  sgd           p = p + (-lr)^ g
  sgd_momentum  b = mu^ b + g;  p = p + (-lr)^ b                              (b starts at zero)
  rmsprop       v = alpha^ v + (1 - alpha)^ (g g);  p = p + (-lr)^ (g / (sqrt(v) + eps^))
  adam          m = m + (g - m) (1 - b1)^;  v = b2^ v + (1 - b2)^ (g g)
                d = sqrt(v) / (sqrt(1 - b2^t))^ + eps^;  p = p + (-lr / (1 - b1^t))^ (m / d)

A row is touched iff some element of its gradient row compares != 0 (-0.0 does not touch, NaN does).  lazy: untouched
rows keep every bit of p and of the state.  Dense: every row is updated.
"""
import math

import numpy as np

KINDS = ("sgd", "sgd_momentum", "rmsprop", "adam")
STATE_KEYS = {"sgd": (), "sgd_momentum": ("momentum_buffer",), "rmsprop": ("square_avg",), "adam": ("exp_avg", "exp_avg_sq")}
f32 = np.float32


def touched_rows(g):
    """bool [M]: rows with an element != 0."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(g, np.float32) != 0).any(axis=1)


def _rows(g, lazy):
    return touched_rows(g) if lazy else np.ones(g.shape[0], bool)


def sgd(p, g, lr, lazy=True):
    """Returns the new p."""
    p = np.array(p, np.float32, copy=True)
    r = _rows(g, lazy)
    with np.errstate(all="ignore"):
        p[r] = p[r] + f32(-float(lr)) * g[r]
    return p


def sgd_momentum(p, g, buf, lr, momentum, lazy=True):
    """Returns (p, momentum_buffer)."""
    p, buf = np.array(p, np.float32, copy=True), np.array(buf, np.float32, copy=True)
    r = _rows(g, lazy)
    with np.errstate(all="ignore"):
        b = f32(float(momentum)) * buf[r] + g[r]
        p[r] = p[r] + f32(-float(lr)) * b
    buf[r] = b
    return p, buf


def rmsprop(p, g, v, lr, alpha=0.99, eps=1e-8, lazy=True):
    """Returns (p, square_avg)."""
    p, v = np.array(p, np.float32, copy=True), np.array(v, np.float32, copy=True)
    r = _rows(g, lazy)
    alpha = float(alpha)
    with np.errstate(all="ignore"):
        gr = g[r]
        vr = f32(alpha) * v[r] + f32(1.0 - alpha) * (gr * gr)
        p[r] = p[r] + f32(-float(lr)) * (gr / (np.sqrt(vr) + f32(float(eps))))
    v[r] = vr
    return p, v


def adam(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, lazy=True):
    """Returns (p, exp_avg, exp_avg_sq); t: the 1-based step count."""
    p, m, v = (np.array(x, np.float32, copy=True) for x in (p, m, v))
    r = _rows(g, lazy)
    b1, b2 = float(betas[0]), float(betas[1])
    neg_step = f32(-float(lr) / (1.0 - b1 ** t))
    bias2_sqrt = f32(math.sqrt(1.0 - b2 ** t))
    with np.errstate(all="ignore"):
        gr = g[r]
        mr = m[r] + (gr - m[r]) * f32(1.0 - b1)
        vr = f32(b2) * v[r] + f32(1.0 - b2) * (gr * gr)
        d = np.sqrt(vr) / bias2_sqrt + f32(float(eps))
        p[r] = p[r] + neg_step * (mr / d)
    m[r], v[r] = mr, vr
    return p, m, v


def step(kind, p, g, state, t, lazy=True, **hp):
    """One step of `kind`: (new p, new state dict keyed as torch.optim's).  state: {} at first (zeros)."""
    g = np.ascontiguousarray(g, np.float32)
    zeros = lambda k: np.array(state[k], np.float32) if k in state else np.zeros_like(g)   # noqa: E731
    if kind == "sgd":
        return sgd(p, g, hp["lr"], lazy), {}
    if kind == "sgd_momentum":
        p, b = sgd_momentum(p, g, zeros("momentum_buffer"), hp["lr"], hp["momentum"], lazy)
        return p, {"momentum_buffer": b}
    if kind == "rmsprop":
        p, v = rmsprop(p, g, zeros("square_avg"), hp["lr"], hp.get("alpha", 0.99), hp.get("eps", 1e-8), lazy)
        return p, {"square_avg": v}
    if kind == "adam":
        p, m, v = adam(p, g, zeros("exp_avg"), zeros("exp_avg_sq"), t, hp["lr"], hp.get("betas", (0.9, 0.999)),
                       hp.get("eps", 1e-8), lazy)
        return p, {"exp_avg": m, "exp_avg_sq": v}
    raise ValueError(kind)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
