#!/usr/bin/env python3
"""Cost of the RealNVP flow as a map (pdeinv_realnvp_map), per path and direction, against one
pdeinv_realnvp_logdensity pass (the cost of the likelihood direction before the map existed).

Batches: the reference's per-epoch batch (320 000 samples, d = 4, 16 loop-mask coupling layers, E = 10, celu), the
KMV recipe's stamp (5 000 samples, d = 2, 8 layers) and d = 8, 16 layers, 320 000 samples (the identity layout).
Per batch the variants are timed alternately (one round = each variant once, `--inner` back-to-back calls between
two device events), after a warm-up of every variant; reported: the median over the rounds of the per-call time and
its spread (min, max). Likelihood-direction rows are [x | v] (ld = 2d), as the trajectory dataset has them.

    (a) logdensity           pdeinv_realnvp_logdensity
    (b) general_rev / _gen   the map's per-thread path, likelihood direction / generation (y, ldj, logp)
    (c) matrix_rev / _gen    the map's matrix-core path, the same
        auto_rev_logp        the dispatched call, reverse = 1, logp only (the same arithmetic as (a))

    python tools/nvp_map_bench.py [--rounds 15] [--inner 5] [--out profiles/nvp_map_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="4:4:320000,2:4:5000,8:2:320000", help="dim:couple_mul:samples,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nvp_map_bench.jsonl"))
    a = ap.parse_args()
    from core.distribution import Gaussian
    from core.normalizing_flow import MNF, RealNVP
    from utils import native, prng
    if not torch.cuda.is_available():
        raise SystemExit("nvp_map_bench: needs the GPU (a CPU run gives no time)")
    dev = "cuda"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = []
    for spec in a.batches.split(","):
        dim, couple, n = (int(v) for v in spec.split(":"))
        gauss = Gaussian(np.zeros(dim), 4 * np.eye(dim))
        flow = RealNVP(MNF(dim, couple, "loop", 1.0, False, "celu", 10), gauss.logdensity)
        flat = flow.init(prng.PRNGKey(0), 0.0, np.zeros(dim))["params"]
        g = torch.Generator(device=dev).manual_seed(1)
        flat = flat + 0.05 * torch.randn(flat.shape, device=dev, generator=g)   # off the identity map
        z = torch.randn((n, 2 * dim), device=dev, generator=g) * 1.5
        x = z[:, :dim]
        x0 = gauss.sample(n, prng.PRNGKey(2))
        t = 0.05 + 1.95 * torch.rand(n, device=dev, generator=g)
        desc = flow._desc
        y = torch.empty((n, dim), device=dev)

        def mapped(impl, rev, want=("y", "ldj", "logp")):
            src = x if rev else x0
            out = y if "y" in want else None
            return lambda: native.realnvp_map(desc, flat, t, src, rev, impl=impl, out=out, want=want)

        variants = {"logdensity": lambda: native.realnvp_logdensity(desc, flat, t, x),
                    "general_rev": mapped("general", 1), "general_gen": mapped("general", 0),
                    "matrix_rev": mapped("matrix", 1), "matrix_gen": mapped("matrix", 0),
                    "auto_rev_logp": mapped("auto", 1, ("logp",))}
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.inner)
        rec = {"workload": f"RealNVP d={dim}, {flow.mnf.n_layers} coupling layers, E=10, celu", "samples": n,
               "rounds": a.rounds, "inner": a.inner, "auto_path": native.realnvp_map_path(desc, "auto"),
               "layout": "packed" if dim <= 4 else "identity"}
        for k, v in times.items():
            rec[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        gr, mr = mapped("general", 1, ("ldj", "logp"))(), mapped("matrix", 1, ("ldj", "logp"))()
        rec["paths_max_rel_diff_rev"] = {k: float((gr[k] - mr[k]).abs().max() / (1 + gr[k].abs().max())) for k in gr}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
