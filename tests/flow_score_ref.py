"""NumPy restatement of the RealNVP score grad_x log p_t(x), reverse mode per sample (helper, not a test).

The likelihood pass is tests/flow_map_ref.flow_map(..., reverse=True), statement for statement: layers l = L-1 .. 0,
with m the mask, k = 1 - m, c = t under the hard parameterisation (else 1), f = e^alpha,
    s = tanh(c s^ / f) f k,   tau = c tau^ k,   x <- (x + tau) e^s,   ldj += sum s
then log p = log p0(x0) + ldj and the adjoint starts as g = -Sigma^-1 (x0 - mu). The backward sweep walks
l = 0 .. L-1, with x_out the layer's output and x_in its input:
    gs = (g x_out + 1) k,   s^bar = c gs (1 - tanh^2),   tau^bar = c g e^s k
    g <- g e^s + m (J_s^T s^bar + J_tau^T tau^bar)[:dim]
and after layer L-1 g is the score. Kinked activations take the derivative of the branch taken (flow_time_ref.act3).
`dtype` selects the arithmetic (float64: the reference; float32: the same rule at the HIP kernel's precision, which
the GPU tests use to size their tolerance). `margin` is the smallest |pre-activation| of the two nets over all layers.
keep_inputs=False rebuilds each layer's input by inverting the layer (x_in = x_out e^{-s} - tau) instead of keeping
it from the likelihood pass: that mode exists only to measure what it costs.
Two more knobs serve the tests of this yardstick only: `assoc` ("reverse": the adjoint goes through the transposed
layers one by one; "forward": the per-sample Jacobian of a net is multiplied up from its input side first, the
other association of the same matrix products) and `drop` (one term of the rule left out, a wrong score on purpose:
"plus1", "mask", "tanh2", "hard_t").
"""
import numpy as np

import flow_time_ref as ftr
from oracle import numpy_ref as nr

DROPS = ("plus1", "mask", "tanh2", "hard_t")


def _mlp_fwd(net, h, act, margin):
    """(output, [g' of the three hidden layers])"""
    d1s = []
    for k, (W, b) in enumerate(net):
        h = h @ W + b
        if k < 3:
            if margin is not None:
                margin.see(h)
            y, g1, _ = ftr.act3(act, h, np.ones_like(h), np.zeros_like(h))
            h = y.astype(h.dtype)
            d1s.append(g1.astype(h.dtype))
    return h, d1s


def _mlp_bwd(net, d1s, dout, dim, assoc):
    """(d out / d in[:dim])^T dout per sample"""
    if assoc == "reverse":
        d = dout
        for k in (3, 2, 1, 0):
            d = d @ net[k][0].T
            if k > 0:
                d = d * d1s[k - 1]
        return d[:, :dim]
    J = net[0][0][:dim][None] * d1s[0][:, None, :]          # [n, dim, 8]
    for k in (1, 2):
        J = (J @ net[k][0]) * d1s[k][:, None, :]
    J = J @ net[3][0]                                        # [n, dim, dim]
    return np.einsum("nio,no->ni", J, dout)


def score(flat, t, x, *, dim, masks, base_mean, base_cov, E=10, ignore_time=False, soft_init=1.0, act="celu",
          dtype=np.float64, keep_inputs=True, assoc="reverse", drop=None):
    """(score [n, dim], logp [n], margin [n]) for rows x [n, dim] and times t [n] (or one t), in `dtype` arithmetic."""
    assert assoc in ("reverse", "forward") and (drop is None or drop in DROPS)
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
    hard = (not ignore_time) and soft_init == 0.0
    c = tt[:, None] if hard else dt(1)
    margin = ftr._Margin(n)

    def couple(l, x_in, see):
        """The layer's terms at its input x_in: (tanh, s, e^s, tau, g' of the s net, g' of the tau net)"""
        m = cast(masks[l])
        keep = dt(1) - m
        sf, snet, tnet = layers[l]
        xt = np.concatenate([x_in * m, tc], -1)
        s, ds = _mlp_fwd(snet, xt, act, margin if see else None)
        tr, dtr = _mlp_fwd(tnet, xt, act, margin if see else None)
        if hard:
            s, tr = tt[:, None] * s, tt[:, None] * tr
        f = np.exp(sf)
        th = np.tanh(s / f)
        s = th * f * keep
        return th, s, np.exp(s), tr * keep, ds, dtr

    kept = [None] * n_layers
    ldj = np.zeros(n, dtype)
    for l in range(n_layers - 1, -1, -1):
        kept[l] = xs
        _, s, es, tr, _, _ = couple(l, xs, True)
        xs = (xs + tr) * es
        ldj = ldj + s.sum(-1)
    off = xs - mean
    logp = -dt(0.5) * (log_det + np.einsum("ni,ij,nj->n", off, A, off)) + ldj
    g = -(off @ A.T)
    for l in range(n_layers):
        m = cast(masks[l])
        keep = dt(1) - m
        sf, snet, tnet = layers[l]
        if keep_inputs:
            x_in = kept[l]
        else:   # the masked coordinates, which feed the nets, pass through a layer unchanged
            _, s, _, tr, _, _ = couple(l, xs, False)
            x_in = xs * np.exp(-s) - tr
        th, s, es, tr, ds, dtr = couple(l, x_in, False)
        gs = (g * xs + (dt(0) if drop == "plus1" else dt(1))) * keep
        cc = dt(1) if drop == "hard_t" else c
        sbar = cc * gs * (dt(1) if drop == "tanh2" else dt(1) - th * th)
        tbar = cc * g * es * keep
        gnet = _mlp_bwd(snet, ds, sbar, dim, assoc) + _mlp_bwd(tnet, dtr, tbar, dim, assoc)
        g = g * es + (gnet if drop == "mask" else m * gnet)
        xs = x_in
    assert g.dtype == logp.dtype == np.dtype(dtype)
    return g, logp, margin.v
