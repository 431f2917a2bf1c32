#!/usr/bin/env python3
"""Cost of the learned log-density's time derivatives (pdeinv_realnvp_time_derivs) against what a central
difference costs: three pdeinv_realnvp_logdensity calls.

Batches: the reference's per-epoch batch (320 000 samples, d = 4, 16 loop-mask coupling layers, E = 10, celu)
and the KMV recipe's stamp (5 000 samples, d = 2). Per batch the variants are timed alternately (one round =
each variant once, `--inner` back-to-back calls between two device events), after a warm-up of every variant;
reported: the median over the rounds of the per-call time and its spread (min, max). Rows [x | v] (ld = 2d), as
the trajectory dataset has them.

    (a) 3 x logdensity      three pdeinv_realnvp_logdensity calls (t - h, t, t + h)
    (b) time_derivs_general      one pdeinv_realnvp_time_derivs call (value, dt, dt2), the per-thread path forced
    (c) time_derivs_matrix_core  the same call, the MFMA tile path forced
        time_derivs              the same call as dispatched (AUTO)

PDEINV_LIBRARY=<path> times another build of the library (e.g. the parent commit's, for (a)).

    python tools/nvp_time_bench.py --tag r07 [--rounds 15] [--inner 5]   -> profiles/r07_nvp_time.jsonl
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
    ap.add_argument("--tag", required=True)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="4:320000,2:5000", help="dim:samples,...")
    a = ap.parse_args()
    from core.distribution import Gaussian
    from core.log_density_estimation import create_normalizing_flow_fn
    from utils import native, prng
    if not torch.cuda.is_available():
        raise SystemExit("nvp_time_bench: needs the GPU (a CPU run gives no time)")
    dev = "cuda"
    out_path = os.path.join(ROOT, "profiles", f"{a.tag}_nvp_time.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    lines = []
    for spec in a.batches.split(","):
        dim, n = (int(v) for v in spec.split(":"))
        flow = create_normalizing_flow_fn(Gaussian(np.zeros(dim), 4 * np.eye(dim)).logdensity, dim)
        flat = flow.init(prng.PRNGKey(0), 0.0, np.zeros(dim))["params"]
        g = torch.Generator(device=dev).manual_seed(1)
        flat = flat + 0.05 * torch.randn(flat.shape, device=dev, generator=g)   # off the identity map
        z = torch.randn((n, 2 * dim), device=dev, generator=g) * 1.5
        x = z[:, :dim]
        t = 0.05 + 1.95 * torch.rand(n, device=dev, generator=g)
        h = 1e-2
        tm, tp = t - h, t + h
        desc = flow._desc
        have_time = hasattr(native, "realnvp_time_derivs")

        def three():
            return (native.realnvp_logdensity(desc, flat, tm, x), native.realnvp_logdensity(desc, flat, t, x),
                    native.realnvp_logdensity(desc, flat, tp, x))

        def forced(impl):
            def run():
                native.realnvp_time_impl(desc, impl)
                try:
                    return native.realnvp_time_derivs(desc, flat, t, x)
                finally:
                    native.realnvp_time_impl(desc, native.NVP_TIME_AUTO)
            return run

        variants = {"3x_logdensity": three}
        if have_time:
            variants["time_derivs_general"] = forced(native.NVP_TIME_GENERAL)
            variants["time_derivs_matrix_core"] = forced(native.NVP_TIME_MATRIX)
            variants["time_derivs"] = lambda: native.realnvp_time_derivs(desc, flat, t, x)   # AUTO
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
               "rounds": a.rounds, "inner": a.inner, "library": os.environ.get("PDEINV_LIBRARY", "in-tree")}
        for k, v in times.items():
            rec[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        if have_time:
            # agreement of the two routes on the value and (loosely: the difference is fp32) on dt
            lm, l0, lp_ = three()
            logp, ds = native.realnvp_time_derivs(desc, flat, t, x)
            rec["value_max_abs_diff"] = float((logp - l0).abs().max())
            rec["dt_vs_central_diff_max_rel"] = float(((lp_ - lm) / (2 * h) - ds[:, 0]).abs().max() /
                                                      (1 + ds[:, 0].abs().max()))
            rec["auto_path"] = native.realnvp_time_impl(desc)
            lg, dg = forced(native.NVP_TIME_GENERAL)()
            lmx, dmx = forced(native.NVP_TIME_MATRIX)()
            rec["paths_max_rel_diff"] = [float((lg - lmx).abs().max() / (1 + lg.abs().max())),
                                         float((dg[:, 0] - dmx[:, 0]).abs().max() / (1 + dg[:, 0].abs().max())),
                                         float((dg[:, 1] - dmx[:, 1]).abs().max() / (1 + dg[:, 1].abs().max()))]
            rec["ratio_time_derivs_over_3x"] = rec["time_derivs"]["median_ms"] / rec["3x_logdensity"]["median_ms"]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
