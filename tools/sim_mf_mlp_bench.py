#!/usr/bin/env python3
"""Time of the McKean–Vlasov simulator with a learned interaction Phi_theta (utils.mean_field.simulate_mean_field
with a MeanFieldMLPPotential: n + 1 pdeinv_mf_mlp_step updates) on the reference's KMV recipe: N = 5000 particles, d = 2,
the default hypothesis net (20 x 8 -> 40), n = 100 steps — 25 M pairs per update. Beside it, on the same GPU in the
same run:

* a torch autograd loop of the same system (V_hypothesis.apply on the pair differences + torch.autograd.grad + the
  element-wise update, torch.randn noise), the pairs taken in item blocks to bound its memory, over `--torch-steps`
  updates (it is about two orders slower), reported per update;
* the KMV residual (pdeinv_residual_kmv_mlp) on one time stamp of the same 5000 rows, whose pass 0 is the same
  pair-force kernel on the same pair count; the whole call is timed by events.

The variants are timed alternately (one round = each variant once, between two device events after a synchronise),
after a warm-up of each; reported: the median over the rounds and the spread. Also the issue model of DESIGN.md:
N^2 / 16 tile gradients of 157 MFMAs per update x 32 cycles over the SIMDs' clock, and the measured ratio to it.

    python tools/sim_mf_mlp_bench.py [--rounds 7] [--particles 5000] [--steps 100]  -> profiles/sim_mf_mlp_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pde-inverse-problem_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def mfma_per_tile(d: int, L: int) -> int:
    """16x16x4 MFMAs of one tile_grad call (mlp_tile.h), as tools/sim_mlp_bench.py counts them."""
    kd = 1 if d <= 4 else 2
    return 2 * kd + 10 * (L - 1) + 10 + 10 * (L - 1) + 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-rounds", type=int, default=2)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--torch-block", type=int, default=500, help="items per block of the torch loop's pair tensor")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--particles", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock of the issue model (MI355X peak)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_mf_mlp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_mf_mlp_bench: needs the GPU (a CPU run gives no time)")
    from core.model import V_hypothesis
    from core.potential import MeanFieldMLPPotential
    from example_problems.kinetic_fokker_planck_example_OU import initialize_configuration
    from example_problems.kinetic_mckean_vlasov_example_quadratic import dlogrho_coefficients
    from utils import native, prng
    from utils.mean_field import simulate_mean_field
    dev = "cuda"
    d, L, W, O = a.dim, 8, 20, 40
    N, n, dt, gamma = a.particles, a.steps, 0.02, 0.5
    model = V_hypothesis(1, [W] * L, out_features=O)
    tree = model.init(prng.PRNGKey(11), np.zeros(d), device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for p in tree["params"].values():  # off the zero-bias initialisation
        p["bias"].add_(0.1 * torch.randn(p["bias"].shape, device=dev, generator=g))
    pot = MeanFieldMLPPotential(model, tree)
    flat, dims = model.flat(tree), model.dims(d)
    z0 = torch.cat([1.5 * torch.randn((N, d), device=dev, generator=g),
                    0.3 * torch.randn((N, d), device=dev, generator=g)], 1)
    key = prng.PRNGKey(7)
    keep = {}

    def hip():
        keep["hip"] = simulate_mean_field(z0, n, dt, key, pot, gamma)

    def hip_force():
        keep["force"] = native.kmv_mlp_force(dims, flat, z0[:, :d])

    def torch_loop():
        q, p = z0[:, :d].clone(), z0[:, d:].clone()
        h = dt
        for _ in range(a.torch_steps):
            F = torch.empty_like(q)
            for lo in range(0, N, a.torch_block):
                y = (q[lo:lo + a.torch_block, None, :] - q[None, :, :]).reshape(-1, d).requires_grad_(True)
                gr, = torch.autograd.grad(model.apply(tree, y).sum(), y)
                F[lo:lo + a.torch_block] = gr.view(-1, N, d).mean(1)
            xi = torch.randn((N, d), device=dev, generator=g)
            p = p - h * F + h ** 0.5 * native.SQRT2 * xi - gamma * p * h
            q = q + h * p
        keep["torch"] = q

    ic = initialize_configuration(d)
    coef = torch.as_tensor(dlogrho_coefficients(np.array([0.9]), ic, d), dtype=torch.float32, device=dev)
    _, ds = native.kmv_weights(d, 1.0, coef, z0, 1, N, 2 * d, 2 * d, want_ds=True)

    def residual():
        keep["res"] = native.residual_kmv_mlp(dims, flat, z0, 1, N, 2 * d, 2 * d, ds, ic["tilde_F"], 1.0)

    variants = {"hip_simulate": hip, "hip_force_batch": hip_force, "residual_kmv_mlp": residual,
                "torch_loop": torch_loop}
    rounds = {k: a.rounds for k in variants}
    rounds["torch_loop"] = a.torch_rounds
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    assert torch.isfinite(keep["hip"]["last"]).all() and torch.isfinite(keep["torch"]).all()
    times = {k: [] for k in variants}
    for r in range(max(rounds.values())):
        for name, fn in variants.items():
            if r >= rounds[name]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    props = torch.cuda.get_device_properties(0)
    cus, clock_hz = props.multi_processor_count, a.clock_mhz * 1e6
    mf = mfma_per_tile(d, L)
    model_ms = (N * N / 16) * mf * 32 / (cus * 4 * clock_hz) * 1e3
    res = {"device": props.name, "cus": cus, "clock_mhz": a.clock_mhz, "d": d, "layers": L, "width": W,
           "out_features": O, "N": N, "n_steps": n, "pairs_per_update": N * N, "mfma_per_tile": mf,
           "issue_model_ms_per_update": model_ms, "torch_steps": a.torch_steps}
    for name, ts in times.items():
        res[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "rounds": len(ts)}
    per_update = res["hip_simulate"]["median_ms"] / (n + 1)
    torch_per_update = res["torch_loop"]["median_ms"] / a.torch_steps
    res["hip_ms_per_update"] = per_update
    res["hip_per_update_over_model"] = per_update / model_ms
    res["hip_force_batch_over_model"] = res["hip_force_batch"]["median_ms"] / model_ms
    res["torch_ms_per_update"] = torch_per_update
    res["torch_over_hip_per_update"] = torch_per_update / per_update
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
