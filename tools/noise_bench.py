"""Time the latent noise (gwen_amd.noise) on device events and print one JSON line.

    python tools/noise_bench.py [--nu 100] [--members 4] [--hidden 256] [--calls 100] [--rollout-calls 100]

* the fused injection gwen_noise_inject_f32 at rows = members x mesh nodes (c5: 4 x 100 002), H = hidden, for K in
  {16, 32, 64}, out of place: compulsory bytes 2 rows H 4 + H K 4 (x read, out written, Wz read), as a fraction of the
  8 TB/s HBM peak;
* the c5 rollout (hidden channels, members members, 4 steps, 4 processor blocks, graphed and batched: bench.py's call)
  without noise and with K = 32 noise, ms per rollout."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def timed(call, calls: int, warmup: int) -> float:
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=100)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rollout-calls", type=int, default=100)
    ap.add_argument("--rollout-steps", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--skip-rollout", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import noise
    from gwen_amd.forecaster import InteractionForecaster, ensemble_forecast
    dev = torch.device("cuda:0")
    mesh = gwen_amd.geodesic_mesh(a.nu)
    nodes, H = mesh.num_nodes, a.hidden
    rows = a.members * nodes
    g = torch.Generator(device=dev).manual_seed(23)
    x = torch.randn(rows, H, device=dev, generator=g)
    out = torch.empty_like(x)
    st = noise.NoiseStream(23, dev)
    inj = {}
    for K in (16, 32, 64):
        wz = torch.randn(H, K, device=dev, generator=g) * 0.1
        ms = timed(lambda: noise.inject(x, wz, st, nodes, out=out), max(a.calls, 100), 10)
        nbytes = 2 * rows * H * 4 + H * K * 4
        inj[str(K)] = {"us": round(ms * 1e3, 2), "compulsory_bytes": nbytes,
                       "fraction_of_8tbs_peak": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3)}
    copy_ms = timed(lambda: out.copy_(x), max(a.calls, 100), 10)
    line = {"tool": "noise_bench", "rows": rows, "nodes": nodes, "H": H, "inject": inj,
            "copy_us": round(copy_ms * 1e3, 2),
            "copy_fraction_of_8tbs_peak": round(2 * rows * H * 4 / (copy_ms * 1e-3) / PEAK_BYTES_PER_S, 3)}
    del x, out
    if not a.skip_rollout:
        n_grid = mesh.faces.shape[0]
        res = {}
        for K in (0, 32):
            torch.manual_seed(23)
            model = InteractionForecaster(H, H, a.blocks, noise_channels=K).to(dev).eval()
            if K:
                with torch.no_grad():
                    model.noise_embed.weight.normal_(0, 0.1)
            graphs = model.prepare(mesh, dev)
            xm = torch.stack([torch.randn(n_grid, H, generator=torch.Generator().manual_seed(23 + m))
                              for m in range(a.members)]).to(dev)
            cache = {}
            ns = noise.NoiseStream(5, dev) if K else None
            call = lambda: ensemble_forecast(model, graphs, xm, a.rollout_steps, a.members,   # noqa: E731
                                             graphed=True, batched=True, step_cache=cache, noise=ns)
            res["noise" if K else "deterministic"] = round(timed(call, max(a.rollout_calls, 1), 2), 3)
            del model, graphs, xm, cache
            torch.cuda.empty_cache()
        line["c5_rollout_ms"] = res
        line["c5_rollout_noise_overhead"] = round(res["noise"] / res["deterministic"] - 1.0, 4)
        line["c5_rollout"] = {"channels": H, "members": a.members, "steps": a.rollout_steps, "blocks": a.blocks,
                              "noise_channels": 32, "graphed": True, "batched": True}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
