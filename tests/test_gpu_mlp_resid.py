"""GPU tests of the V_hypothesis residual (pdeinv_residual_kfp_mlp: csrc/mlp_fused.hip, mlp.hip, mlp_library.hip)
against fp64, per parameter block and entry and per accumulator slot.

Rule (tests/mlp_resid_ref.py): |gpu - fp64| <= 16 x E, E the fp32 restatement's own largest error against fp64 on the
same inputs, per block (K_l and b_l apart) and per slot; test_mlp_resid_ref.py shows on the CPU that one dropped row,
a wrong sign of s2 and four more wrong formulas exceed it. FUSED and AUTO are held to it everywhere; the LIBRARY
(rocBLAS) path runs through the same check where it takes the shape — an implementation under test, never a reference.

  (a) row tails: every set size of SIZES in every position, whole and in chunks of 64 and 100 rows;
  (b) the persistent grids' second pass: one chunk just past each launcher's grid cap (WRAPS says which);
  (c) strided rows out of NaN-filled buffers: bit-equal to the contiguous call;
  (d) one loss term at a time, and the V-weighted boundary of the overdamped problem;
  (e) the row engine behind pdeinv_mlp_potential at W = 128 .. 1024: V and grad V per row, and row prefixes.
The measured max |err| / E per kernel family is in DESIGN.md §3.1.
"""
import numpy as np
import pytest
import torch

import mlp_resid_ref as R
from oracle import numpy_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
AUTO, LIB, FUSED = 0, 1, 2  # native.MLP_IMPL_*
GAMMA, T = 0.5, 2.0
WHOLE = 1 << 18


def _ids(v):
    return "-".join(map(str, v)) if isinstance(v, list) else None


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _true(d, kind):
    if kind == "gmm":
        return "gmm", nr.gmm_centres(d, 3).astype(np.float32).astype(np.float64)
    return "quad", nr.problem_constants(d).astype(np.float32).astype(np.float64)


def _call(native, c, chunk, impl, sets=None):
    """(acc [8] fp64, grad [P] fp32) as NumPy arrays. sets: device tensors in place of the case's own rows."""
    z0, zi, zt = (_t(z) for z in c.sets) if sets is None else sets
    kind = native.POT_GMM if c.true[0] == "gmm" else native.POT_QUADRATIC
    acc, grad = native.residual_kfp_mlp(c.dims, _t(nr.mlp_flat(c.params)), zi, zt, z0, true_kind=kind,
                                        true_params=np.asarray(c.true[1], np.float32), gamma=GAMMA, total_time=T,
                                        chunk_rows=chunk, impl=impl, coefficients=c.coef, boundary_value=c.bval)
    return acc.cpu().numpy(), grad.cpu().numpy()


def _pool(dims, n_max=257):
    """Parameters and a pool of n_max rows per set for a shape; the sets of a case are prefixes of the pool."""
    key = tuple(dims)
    if key not in _pools:
        seed = 1000 + sum(dims) + len(dims)
        _pools[key] = (R.make_params(dims, seed), [R.make_rows(dims[0], n_max, seed + 1 + j) for j in range(3)])
    return _pools[key]


_pools = {}


def _case(dims, n0, ni, nt, true_kind="quad", coef=None, bval=False, n_orders=R.N_ORDERS):
    params, pool = _pool(dims)
    sets = [pool[0][:n0], pool[1][:ni], pool[2][:nt]]
    coef = R.coefficients(n0, ni, nt, GAMMA, T) if coef is None else coef
    return R.Case(dims, params, sets, coef, _true(dims[0], true_kind), bval, n_orders)


# ---- (a) row tails -------------------------------------------------------------------------------------------
SIZES = (0, 1, 15, 16, 17, 31, 33, 63, 65, 127, 129, 255, 257)


def _triple(k):
    """(n_init, n_term, n_0T): over k = 0 .. 12 every size stands once in every position (the 0T set cannot be
    empty: 257 takes the place of 0 there)."""
    n = len(SIZES)
    return SIZES[k], SIZES[(k + 5) % n], SIZES[(k + 9) % n] or 257


TAIL_SHAPES = [
    # rgemm / rgemm16 / wgrad2 / wgrad_o; run_chunk_fo2 on the boundary sets
    ([2, 128, 128, 40], FUSED), ([8, 256, 256, 40], FUSED),
    # a middle layer, a full third rgemm16 tile (48), the 64-column E_OUT_SEEDS1 (56)
    ([4, 128, 128, 128, 48], FUSED), ([4, 256, 256, 56], FUSED),
    # fgemm / fwgrad; first-order chunks on zeroed planes
    ([4, 64, 64, 40], FUSED), ([2, 32, 32, 32, 5], FUSED), ([16, 512, 512, 24], FUSED),
    # run_chunk_l1
    ([4, 64, 40], FUSED), ([8, 256, 40], FUSED),
    # out_features > 64: terms_sum_kernel, fgemm output tiles, no fo2
    ([8, 128, 128, 200], FUSED),
    # zero-padded d and W under AUTO
    ([3, 20, 20, 40], AUTO), ([5, 100, 100, 40], AUTO)]
LIB_SHAPES = ([2, 128, 128, 40], [4, 64, 64, 40], [4, 64, 40], [3, 20, 20, 40])


@pytest.mark.parametrize("k", range(len(SIZES)))
@pytest.mark.parametrize("dims,impl", TAIL_SHAPES, ids=_ids)
def test_row_tails(native, dims, impl, k):
    ni, nt, n0 = _triple(k)
    c = _case(dims, n0, ni, nt, "gmm" if k % 2 else "quad")
    name = {AUTO: "AUTO", FUSED: "FUSED"}[impl]
    for chunk in (WHOLE, 64, 100):
        acc, grad = _call(native, c, chunk, impl)
        c.check(f"tails {dims} {name} chunk {chunk}", grad, acc)
    if dims in LIB_SHAPES:
        acc, grad = _call(native, c, WHOLE, LIB)
        c.check(f"tails {dims} LIBRARY chunk {WHOLE}", grad, acc)


def test_triples_cover_every_size_in_every_position():
    t = [_triple(k) for k in range(len(SIZES))]
    assert {a for a, _, _ in t} == set(SIZES) and {b for _, b, _ in t} == set(SIZES)
    assert {c for _, _, c in t} == set(SIZES) - {0}


# ---- (b) the wrapped persistent grids ---------------------------------------------------------------------------
# Grid caps read from mlp_fused.hip's launchers (rows above which a workgroup takes a second row block):
#   rgemm, W = 128: S = 3 and S = 2 (BMR 128, 256 workgroups) 32768; S = 1 (BMR 256) 65536; W = 256 (2 column blocks,
#   128 workgroups each): S = 3 16384, S = 1 32768; rgemm_out / rgemm16 (BMR 256, 256 workgroups) 65536;
#   fgemm (kRowGridCap = 1024 workgroups over gy column blocks): 64 x 64 tiles 65536, 128 x 32 and the 128 x 64 output
#   tile 131072, 64 x 128 tiles at W = 512 (gy = 4) 16384; l1_grad_kernel rows per block > 64 past 65536; wgrad2 rows
#   per slice > 64 past 16384; l1_g_kernel (4 rows per block, 2048 blocks) past 8192.
# (dims, n_0T, n_init, n_term, what wraps). Tails: one more full row block and an odd remainder.
WRAPS = [
    ([2, 128, 128, 128, 40], 65536 + 256 + 37, 32768 + 128 + 29, 17,
     "0T: rgemm S = 3 / S = 1, rgemm_out / rgemm16, l1_grad_kernel, wgrad2; initial: rgemm S = 2 (fo2), wgrad2"),
    ([4, 256, 256, 40], 32768 + 256 + 41, 33, 17, "rgemm S = 3 and S = 1 at two column blocks, wgrad2"),
    ([4, 64, 64, 40], 65536 + 64 + 23, 33, 17, "fgemm 64 x 64 tiles"),
    ([2, 32, 32, 5], 131072 + 128 + 19, 33, 17, "fgemm 128 x 32 tiles and the 128 x 64 output tile"),
    # [2, 512, 512, 40] rather than [2, 1024, 1024, 40]: half the CPU reference's work (8 s on 8 cores)
    ([2, 512, 512, 40], 16384 + 64 + 13, 33, 17, "fgemm 64 x 128 tiles at gy = 4, l1_g_kernel past 2048 x 4 rows")]


@pytest.mark.parametrize("dims,n0,ni,nt,what", WRAPS, ids=[_ids(w[0]) for w in WRAPS])
def test_wrapped_grids(native, dims, n0, ni, nt, what):
    params = R.make_params(dims, 2000 + sum(dims))
    sets = [R.make_rows(dims[0], n, 2001 + sum(dims) + j) for j, n in enumerate((n0, ni, nt))]
    c = R.Case(dims, params, sets, R.coefficients(n0, ni, nt, GAMMA, T), _true(dims[0], "quad"), n_orders=2)
    assert WHOLE >= n0 and WHOLE * dims[1] <= 1 << 30  # one chunk per set, inside the 32-bit plane offsets
    acc, grad = _call(native, c, WHOLE, FUSED)
    c.check(f"wrap {dims} FUSED ({what})", grad, acc)


# ---- (c) strided rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,impl", [([8, 256, 256, 40], FUSED), ([4, 64, 64, 40], FUSED), ([4, 64, 40], FUSED),
                                       ([3, 20, 20, 40], AUTO)], ids=_ids)
def test_strided_rows_bit_equal(native, dims, impl):
    d = dims[0]
    c = _case(dims, 257, 129, 65, n_orders=1)
    views = []
    for z in c.sets:
        buf = torch.full((len(z), 2 * d + 3), float("nan"), device=DEV)
        buf[:, 1:1 + 2 * d] = _t(z)
        views.append(buf[:, 1:1 + 2 * d])
        assert views[-1].stride(0) == 2 * d + 3
    for chunk in (WHOLE, 100):
        acc, grad = _call(native, c, chunk, impl)
        acc_s, grad_s = _call(native, c, chunk, impl, sets=views)
        assert np.array_equal(grad, grad_s) and np.array_equal(acc, acc_s), chunk
        assert np.all(np.isfinite(grad)) and np.abs(grad).max() > 0


# ---- (d) one term at a time ---------------------------------------------------------------------------------------
TERM_SHAPES = [[8, 256, 256, 40], [4, 64, 64, 64, 40], [4, 64, 40]]


@pytest.mark.parametrize("term", R.COEF_KEYS)
@pytest.mark.parametrize("dims", TERM_SHAPES, ids=_ids)
def test_one_term(native, dims, term):
    """Exactly one weight non-zero. c_hess alone runs run_chunk_full on the 0T set; c_init / c_term alone (c_hess = 0)
    run run_chunk_fo2 at W = 256, the zeroed-plane first-order chain at W = 64 and run_chunk_l1 at L = 1; c_true
    alone leaves the gradient exactly zero and fills its slots."""
    n0, ni, nt = 257, 129, 65
    c = _case(dims, n0, ni, nt, "gmm", coef=R.only(term, n0, ni, nt, GAMMA, T))
    assert sum(v != 0 for v in c.coef.values()) == 1
    for chunk in (WHOLE, 100):
        acc, grad = _call(native, c, chunk, FUSED)
        c.check(f"term {term} {dims} FUSED chunk {chunk}", grad, acc)
    if term == "c_true":
        assert not grad.any() and acc[1] > 0 and acc[5] > 0
    else:
        assert np.abs(c.ref_grad).max() > 0


@pytest.mark.parametrize("which", ["mix", "c_init", "c_term"])
@pytest.mark.parametrize("dims", TERM_SHAPES, ids=_ids)
def test_boundary_value(native, dims, which):
    """boundary_value: the boundary sets weight V itself (c0, the overdamped problem) — in the reference's mix and
    with c_init / c_term alone."""
    n0, ni, nt = 257, 129, 65
    coef = R.coefficients(n0, ni, nt, GAMMA, T) if which == "mix" else R.only(which, n0, ni, nt, GAMMA, T)
    c = _case(dims, n0, ni, nt, "quad", coef=coef, bval=True)
    for chunk in (WHOLE, 100):
        acc, grad = _call(native, c, chunk, FUSED)
        c.check(f"bval {which} {dims} FUSED chunk {chunk}", grad, acc)
    assert np.abs(c.ref_grad).max() > 0


# ---- (e) the row engine behind pdeinv_mlp_potential ----------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8])
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("W", [128, 256, 512, 1024])
def test_potential_row_engine(native, W, L, d):
    """V and grad V per row through the fused kernels in gradient-only mode (path 1): rgemm / l1_g_mfma_kernel at
    W = 128, 256, fgemm / l1_g_kernel at W = 512, 1024. The rule with a row-wise scale (|V_r|, max_i |g_ri|); the
    prefixes return the full call's rows bit for bit (a row's numbers depend on the row only)."""
    dims = [d] + [W] * L + [40]
    assert native.mlp_potential_path(dims) == 1
    params = R.make_params(dims, 3000 + W + 10 * L + d)
    x = (1.5 * np.random.default_rng(3001 + W + L + d).standard_normal((300, d))).astype(np.float32)
    V64, g64, eV, eg = R.potential_rows(params, x)
    flat = _t(nr.mlp_flat(params))
    v, g = native.mlp_potential(dims, flat, _t(x))
    ev_gpu, eg_gpu = R.value_err(v.cpu().numpy(), V64).max(), R.grad_err(g.cpu().numpy(), g64).max()
    print(f"max|err|/E potential {dims}: value {ev_gpu / eV.max():.3g} grad {eg_gpu / eg.max():.3g}")
    assert ev_gpu <= R.RULE * eV.max(), (ev_gpu, eV.max())
    assert eg_gpu <= R.RULE * eg.max(), (eg_gpu, eg.max())
    for n in (1, 15, 16, 17, 63, 65, 129, 257):
        vn, gn = native.mlp_potential(dims, flat, _t(x[:n]))
        assert torch.equal(vn, v[:n]) and torch.equal(gn, g[:n]), n
