"""NumPy restatement of the RealNVP flow as a map, both directions (helper, not a test).

The algebra of oracle.numpy_ref.realnvp_apply plus logp, with a `dtype` argument: float64 is the reference,
float32 the same rule at the HIP kernels' precision (every array and product rounded to float32), which the GPU
tests of pdeinv_realnvp_map use to size their tolerance.
  reverse = True : layers L-1 .. 0, x <- (x + tr) e^s,  ldj += sum s, logp = log p0(y) + ldj
  reverse = False: layers 0 .. L-1, x <- x e^{-s} - tr, ldj -= sum s, logp = log p0(x_in) - ldj
"""
import numpy as np

from oracle import numpy_ref as nr


def _mlp(net, h, act):
    for k, (W, b) in enumerate(net):
        h = h @ W + b
        if k < 3:
            h = nr._nvp_act(act, h).astype(h.dtype)
    return h


def flow_map(flat, t, x, reverse, *, dim, masks, base_mean, base_cov, E=10, ignore_time=False, soft_init=1.0,
             act="celu", dtype=np.float64):
    """(y [n, dim], ldj [n], logp [n]) for rows x [n, dim] and times t [n] (or one t), in `dtype` arithmetic."""
    dt = np.dtype(dtype).type
    cast = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
    masks = np.asarray(masks, dtype=np.float64)
    n_layers = masks.shape[0]
    temb, layers = nr.nvp_unflat(flat, dim, n_layers, E, ignore_time)
    layers = [(cast(sf), [(cast(W), cast(b)) for W, b in sn], [(cast(W), cast(b)) for W, b in tn])
              for sf, sn, tn in layers]
    xs = cast(x).copy()
    n = xs.shape[0]
    tt = cast(np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)))
    if ignore_time:
        tc = np.zeros((n, 0), dtype)
    elif E > 0:
        half = E // 2
        w = cast(np.exp(np.arange(half) * -(np.log(10000) / (half - 1))))
        e = tt[:, None] * w
        se = np.concatenate([np.sin(e), np.cos(e)], -1)
        (W1, b1), (W2, b2) = [(cast(W), cast(b)) for W, b in temb]
        tc = nr._nvp_act(act, se @ W1 + b1).astype(dtype) @ W2 + b2
    else:
        tc = tt[:, None]
    A = cast(np.linalg.inv(np.asarray(base_cov, dtype=np.float64)))
    log_det = dt(np.log(np.linalg.det(np.asarray(base_cov, dtype=np.float64) * 2 * np.pi)))
    mean = cast(base_mean)

    def log_p0(z):
        off = z - mean
        return -dt(0.5) * (log_det + np.einsum("ni,ij,nj->n", off, A, off))

    lp0_in = log_p0(xs)
    ldj = np.zeros(n, dtype)
    hard = (not ignore_time) and soft_init == 0.0
    for l in (range(n_layers - 1, -1, -1) if reverse else range(n_layers)):
        m = cast(masks[l])
        keep = dt(1) - m
        sf, snet, tnet = layers[l]
        xt = np.concatenate([xs * m, tc], -1)
        s, tr = _mlp(snet, xt, act), _mlp(tnet, xt, act)
        if hard:
            s, tr = tt[:, None] * s, tt[:, None] * tr
        f = np.exp(sf)
        s = np.tanh(s / f) * f * keep
        tr = tr * keep
        if reverse:
            xs = (xs + tr) * np.exp(s)
            ldj = ldj + s.sum(-1)
        else:
            xs = xs * np.exp(-s) - tr
            ldj = ldj - s.sum(-1)
    logp = log_p0(xs) + ldj if reverse else lp0_in - ldj
    assert xs.dtype == ldj.dtype == logp.dtype == np.dtype(dtype)
    return xs, ldj, logp


# dim, mask, E, soft_init, ignore_time, act, n: the flows of tests/test_gpu_flow_time.py plus two that reach the
# identity layout at its edges (n: no multiple of a tile, wave or block size)
CASES = [
    (2, "loop", 10, 1.0, False, "celu", 2561),
    (4, "loop", 10, 1.0, False, "celu", 700),
    (8, "loop", 10, 1.0, False, "celu", 513),
    (1, "loop", 4, 0.0, False, "celu", 1),
    (1, "loop", 4, 0.0, False, "celu", 65),
    (3, "random", 0, 0.0, False, "tanh", 1000),
    (5, "random", 6, 0.0, False, "softplus", 900),
    (4, "loop", 16, 1.0, False, "silu", 130),
    (3, "random", 6, 1.0, True, "gelu", 64),
    (2, "loop", 10, 1.0, False, "relu", 300),
    (3, "random", 12, 0.0, False, "elu", 130),
    (6, "loop", 0, 1.0, False, "elu", 257),
    (7, "random", 14, 1.0, False, "celu", 129),
]


def case_id(c):
    return f"d{c[0]}-{c[1]}-E{c[2]}-s{c[3]:g}-{'ign-' if c[4] else ''}{c[5]}-n{c[6]}"


def case_inputs(dim, mask_type, E, soft_init, ignore_time, act, n):
    """The inputs of a case (NumPy only): parameters rounded to float32, the base Gaussian of
    test_gpu_flow_time._case, rows z = [x | v] (1.5 x standard normal, the likelihood direction's input, ld = 2 dim),
    x0 (a draw from the base, the generative direction's input), t ~ U(0.05, 2)."""
    couple = 3 if mask_type == "random" else (2 if dim >= 6 else 4)
    masks = nr.nvp_masks(dim, couple, mask_type)
    rng = np.random.default_rng(200 + dim)
    mean = rng.standard_normal(dim) * 0.3
    Lc = rng.standard_normal((dim, dim)) * 0.3
    cov = Lc @ Lc.T + np.eye(dim)
    flat = nr.nvp_init(dim, masks.shape[0], E, ignore_time, seed=dim + 1, scale=1.3, perturb=True)
    flat = flat.astype(np.float32).astype(np.float64)
    z = (rng.standard_normal((n, 2 * dim)) * 1.5).astype(np.float32)
    t = rng.uniform(0.05, 2.0, n).astype(np.float32)
    x0 = (mean + rng.standard_normal((n, dim)) @ np.linalg.cholesky(cov).T).astype(np.float32)
    kw = dict(dim=dim, masks=masks, base_mean=mean, base_cov=cov, E=E, ignore_time=ignore_time, soft_init=soft_init,
              act=act)
    return dict(flat=flat, z=z, t=t, x0=x0, kw=kw, couple=couple, mean=mean, cov=cov)
