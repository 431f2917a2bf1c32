"""NumPy restatement of the RealNVP log-density and its first two time derivatives (helper, not a test).

Second-order forward mode in t through the whole model of oracle.numpy_ref.realnvp_logdensity: every
t-dependent quantity is a triple (value, d/dt, d2/dt2); dense layers act on the three streams alike
(the bias on the value only), an activation y = g(z) maps them by
    y' = g'(z) z',   y'' = g''(z) z'^2 + g'(z) z'',
products by Leibniz. Kinks: relu g' = [z > 0], g'' = 0; celu / elu g' = g'' = e^z for z <= 0 and
(1, 0) for z > 0. `dtype` selects the arithmetic (float64: the reference; float32: the same rule at the
HIP kernel's precision, which the GPU tests use to size their tolerance). `margin` is the smallest
|pre-activation| the sample meets (how close it comes to a kink).
"""
import numpy as np

from oracle import numpy_ref as nr


def act3(name, z, z1, z2):
    """(g(z), its first and second t-derivative) from the three streams of z."""
    one = z.dtype.type(1)
    if name in ("celu", "elu"):
        e = np.exp(np.minimum(z, 0))
        pos = z > 0
        y = np.where(pos, z, np.expm1(np.minimum(z, 0)))
        g1 = np.where(pos, one, e)
        g2 = np.where(pos, 0 * e, e)
    elif name == "relu":
        pos = z > 0
        y = np.maximum(z, 0)
        g1 = np.where(pos, one, 0 * z)
        g2 = 0 * z
    elif name == "tanh":
        y = np.tanh(z)
        g1 = one - y * y
        g2 = -2 * y * g1
    elif name == "silu":
        s = one / (one + np.exp(-z))
        y = z * s
        g1 = s + z * s * (one - s)
        g2 = s * (one - s) * (2 + z * (one - 2 * s))
    elif name == "softplus":
        s = one / (one + np.exp(-z))
        y = np.logaddexp(z, 0 * z)
        g1 = s
        g2 = s * (one - s)
    elif name == "gelu":  # tanh approximation
        c, a = z.dtype.type(np.sqrt(2 / np.pi)), z.dtype.type(0.044715)
        u = c * (z + a * z ** 3)
        u1 = c * (one + 3 * a * z * z)
        u2 = 6 * c * a * z
        th = np.tanh(u)
        th1 = (one - th * th) * u1
        th2 = (one - th * th) * u2 - 2 * th * (one - th * th) * u1 * u1
        half = z.dtype.type(0.5)
        y = half * z * (one + th)
        g1 = half * (one + th) + half * z * th1
        g2 = th1 + half * z * th2
    else:
        raise ValueError(name)
    return y, g1 * z1, g2 * z1 * z1 + g1 * z2


def _mul3(a, b):
    return a[0] * b[0], a[1] * b[0] + a[0] * b[1], a[2] * b[0] + 2 * a[1] * b[1] + a[0] * b[2]


class _Margin:
    def __init__(self, n):
        self.v = np.full(n, np.inf)

    def see(self, z):
        self.v = np.minimum(self.v, np.abs(z.astype(np.float64)).min(-1))


def _mlp3(net, h, act, margin):
    for k, (W, b) in enumerate(net):
        h = (h[0] @ W + b, h[1] @ W, h[2] @ W)
        if k < 3:
            margin.see(h[0])
            h = act3(act, *h)
    return h


def time_derivs(flat, t, x, *, dim, masks, base_mean, base_cov, E=10, ignore_time=False, soft_init=1.0,
                act="celu", dtype=np.float64):
    """(log p_t(x), d/dt, d2/dt2, margin) for rows x [n, dim] and times t [n] (or one t)."""
    dt = np.dtype(dtype).type
    cast = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    masks = np.asarray(masks, dtype=np.float64)
    n_layers = masks.shape[0]
    temb, layers = nr.nvp_unflat(flat, dim, n_layers, E, ignore_time)
    if temb is not None:
        temb = [(cast(W), cast(b)) for W, b in temb]
    layers = [(cast(sf), [(cast(W), cast(b)) for W, b in sn], [(cast(W), cast(b)) for W, b in tn])
              for sf, sn, tn in layers]
    x0 = cast(x)
    n = x0.shape[0]
    tt = cast(np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
    zero = np.zeros_like(x0)
    xs = (x0.copy(), zero, zero)
    t3 = (tt[:, None], np.ones((n, 1), dtype), np.zeros((n, 1), dtype))
    margin = _Margin(n)
    if ignore_time:
        z0 = np.zeros((n, 0), dtype)
        tc = (z0, z0, z0)
    elif E > 0:
        half = E // 2
        w = cast(np.exp(np.arange(half) * -(np.log(10000) / (half - 1))))
        e = tt[:, None] * w
        s, c = np.sin(e), np.cos(e)
        se = (np.concatenate([s, c], -1), np.concatenate([w * c, -w * s], -1),
              np.concatenate([-w * w * s, -w * w * c], -1))
        (W1, b1), (W2, b2) = temb
        h = (se[0] @ W1 + b1, se[1] @ W1, se[2] @ W1)
        margin.see(h[0])
        h = act3(act, *h)
        tc = (h[0] @ W2 + b2, h[1] @ W2, h[2] @ W2)
    else:
        tc = t3
    ldj = (np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype))
    hard = (not ignore_time) and soft_init == 0.0
    for l in range(n_layers - 1, -1, -1):
        m = cast(masks[l])
        keep = dt(1) - m
        sf, snet, tnet = layers[l]
        xin = tuple(np.concatenate([xs[k] * m, tc[k]], -1) for k in range(3))
        s = _mlp3(snet, xin, act, margin)
        tr = _mlp3(tnet, xin, act, margin)
        if hard:
            s, tr = _mul3(t3, s), _mul3(t3, tr)
        f = np.exp(sf)
        u = tuple(s[k] / f for k in range(3))
        th = np.tanh(u[0])
        g1 = dt(1) - th * th
        sk = (th * f * keep, g1 * u[1] * f * keep, (g1 * u[2] - 2 * th * g1 * u[1] * u[1]) * f * keep)
        tr = tuple(tr[k] * keep for k in range(3))
        es0 = np.exp(sk[0])
        es = (es0, es0 * sk[1], es0 * (sk[2] + sk[1] * sk[1]))
        xs = _mul3(tuple(xs[k] + tr[k] for k in range(3)), es)
        ldj = tuple(ldj[k] + sk[k].sum(-1) for k in range(3))
    A = cast(np.linalg.inv(np.asarray(base_cov, dtype=np.float64)))
    log_det = dt(np.log(np.linalg.det(np.asarray(base_cov, dtype=np.float64) * 2 * np.pi)))
    off = xs[0] - cast(base_mean)
    q = lambda a, b: np.einsum("ni,ij,nj->n", a, A, b)
    quad = (q(off, off), q(xs[1], off) + q(off, xs[1]), q(xs[2], off) + 2 * q(xs[1], xs[1]) + q(off, xs[2]))
    half = dt(0.5)
    logp = -half * (log_det + quad[0]) + ldj[0]
    d1 = -half * quad[1] + ldj[1]
    d2 = -half * quad[2] + ldj[2]
    if ignore_time:
        d1, d2 = np.zeros(n, dtype), np.zeros(n, dtype)
    return logp, d1, d2, margin.v
