"""CPU checks of tests/mlp_resid_ref.py, the reference and tolerance of test_gpu_mlp_resid.py. Without them the GPU
tests could be vacuous: a tolerance no wrong kernel exceeds, or a restatement that is not the reference's algebra.

  * grad_rows restates oracle.numpy_ref.mlp_grad_rows: equal to fp64 rounding in fp64, bit for bit in fp32 with
    np.tanh; renumbering the units of every layer leaves the fp64 gradient where it was; the slots' reference equals
    oracle.numpy_ref.kfp_mlp_loss under the reference's weights;
  * at [8,256,256,40] (900 / 700 / 2500 rows), [2,128,128,40] (33 / 17 / 129 rows) and a 3-hidden-layer net, each
    mutation of the fp64 reference moves some entry of some block past RULE x E_block: the last row of each set
    dropped (one set at a time), s2 with the wrong sign, the s3 zd^2 term left out, the abar^T zeta pair left out, a
    bias gradient short of one row, c_init on the terminal set;
  * an evaluation of the fp32 restatement the yardstick has not seen (another row and unit order) stays below
    RULE / 2 in every block and slot.
"""
import numpy as np
import pytest

import mlp_resid_ref as R
from oracle import numpy_ref as nr

GAMMA, T = 0.5, 2.0
# dims, (n_init, n_term, n_0T)
SHAPES = [([8, 256, 256, 40], (900, 700, 2500)), ([2, 128, 128, 40], (33, 17, 129)),
          ([4, 64, 64, 64, 40], (65, 31, 257))]
_cases = {}


def _case(k):
    if k not in _cases:
        dims, (ni, nt, n0) = SHAPES[k]
        d = dims[0]
        params = R.make_params(dims, 10 + k)
        sets = [R.make_rows(d, n, 100 * k + j) for j, n in enumerate((n0, ni, nt))]
        F = nr.problem_constants(d).astype(np.float32).astype(np.float64)
        _cases[k] = R.Case(dims, params, sets, R.coefficients(n0, ni, nt, GAMMA, T), ("quad", F))
    return _cases[k]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_restatement_is_the_reference(k):
    c = _case(k)
    ref = c.ref_grad
    mine = nr.mlp_flat(R.grad_rows(c.params, c.Z, c.C)[0])
    assert np.max(np.abs(mine - ref)) <= 1e-13 * np.abs(ref).max()
    p32 = [(K.astype(np.float32), b.astype(np.float32)) for K, b in c.params]
    Z32, C32 = c.Z.astype(np.float32), c.C.astype(np.float32)
    a = nr.mlp_flat(nr.mlp_grad_rows(p32, Z32, C32))
    b = nr.mlp_flat(R.grad_rows(p32, Z32, C32)[0])
    assert a.dtype == np.float32 and np.array_equal(a, b)
    # the unit renumbering is undone exactly: the fp64 gradient moves by fp64 rounding only
    perms = R.unit_orders(c.dims, 3)
    g = R.unpermute_grads(nr.mlp_grad_rows(R.permute_units(c.params, perms), c.Z, c.C), perms)
    assert np.max(np.abs(nr.mlp_flat(g) - ref)) <= 1e-12 * np.abs(ref).max()
    # layout of the blocks = mlp_flat's
    o = 0
    for (name, s), arr in zip(c.blocks, [a for Kb in c.params for a in Kb]):
        assert s.start == o and s.stop == o + arr.size, name
        o = s.stop
    assert o == ref.size


def test_slots_reference_is_the_reference_loss():
    c = _case(1)
    z0, zi, zt = c.sets
    F = c.true[1]
    loss, loss_gt, parts = nr.kfp_mlp_loss(c.params, zi, zt, z0, nr.grad_quadratic(F), GAMMA, T)
    a = c.ref_acc
    want = [loss, loss_gt, parts["nabla"], parts["hessian"], parts["friction"] / GAMMA, parts["nabla_true"],
            parts["initial"], parts["terminal"]]
    assert np.allclose(a, want, rtol=1e-6, atol=0), (a, want)  # 1e-6: the coefficients are rounded to fp32
    z = np.linspace(-12, 12, 4001).astype(np.float32)
    assert np.max(np.abs(R.tanh_exp2(z).astype(np.float64) - np.tanh(z.astype(np.float64)))) < 3e-7
    assert R.tanh_exp2(np.float32([200.0, -200.0])).tolist() == [1.0, -1.0]


@pytest.mark.parametrize("mutate", ("drop0", "drop1", "drop2") + R.MUTATIONS + ("swap_boundary",))
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_mutations_exceed_the_rule(k, mutate):
    c = _case(k)
    r = c.block_ratios(c.mutated64(mutate))
    worst = max(r.values())
    print(f"{c.dims} {mutate}: max over blocks of |change| / E = {worst:.3g} ({max(r, key=r.get)})")
    assert worst > R.RULE, (mutate, r)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_fresh_order_within_half_the_rule(k):
    c = _case(k)
    for tanh in (np.tanh, R.tanh_exp2):
        g, a = c.eval32(R.N_ORDERS, tanh)
        rb, rs = c.block_ratios(g), c.slot_ratios(a)
        print(f"{c.dims} fresh order: grad {max(rb.values()):.3g} slots {rs.max():.3g}")
        assert max(rb.values()) <= R.RULE / 2 and rs.max() <= R.RULE / 2, (rb, rs)
    assert min(c.E_block.values()) > 0
