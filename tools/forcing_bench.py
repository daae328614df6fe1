"""Time the static fields and forcings (gwen_amd.forcings) on device events; append one JSON line to
profiles/forcing_bench.jsonl (``--out``) and print it.

    python tools/forcing_bench.py [--nodes 200000] [--members 4] [--calls 200] [--rollout-calls 20] [--skip-rollout]

* the fused embedding gwen_forcing_embed_f32 at N = nodes x members, H = 64 and 256, solar + 3 given columns, with a
  base, out of place: compulsory bytes 2 rows H 4 + N H 4 + H F 4 (x read, out written, base and wf once), as a
  fraction of the 8 TB/s HBM peak -- beside a device copy of x (the same rows read and written) and the noise injection
  with K = 16 at the same shape;
* the c5 rollout (256 channels, 4 members, 4 steps, 4 processor blocks, graphed and batched: the call of
  tools/forecaster_bench.py 256 256 4 4) without and with static_channels=4, solar=True, alternating, ms per rollout
  (the median of the rounds)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    ap.add_argument("--nodes", type=int, default=200000)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rollout-calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forcing_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("forcing_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import forcings, noise
    from gwen_amd.forecaster import InteractionForecaster, ensemble_forecast
    dev = torch.device("cuda:0")
    N, M, Fg = a.nodes, a.members, 3
    F = forcings.SOLAR_CHANNELS + Fg
    rows = N * M
    g = torch.Generator(device=dev).manual_seed(23)
    lat = (torch.rand(N, device=dev, generator=g, dtype=torch.float64) - 0.5) * torch.pi
    lon = (torch.rand(N, device=dev, generator=g, dtype=torch.float64) - 0.5) * 2 * torch.pi
    latlon = torch.stack([lat, lon], dim=1).contiguous()
    given = torch.randn(N, Fg, device=dev, generator=g)
    clock = forcings.ForcingClock(772_416_000, 21600, dev)
    st = noise.NoiseStream(23, dev)
    emb = {}
    for H in (64, 256):
        x = torch.randn(rows, H, device=dev, generator=g)
        out = torch.empty_like(x)
        wf = torch.randn(H, F, device=dev, generator=g) * 0.1
        base = torch.randn(N, H, device=dev, generator=g)
        wz = torch.randn(H, 16, device=dev, generator=g) * 0.1
        ms = timed(lambda: forcings.embed(x, clock, latlon, given, wf, base, N, out=out), a.calls, 10)
        copy_ms = timed(lambda: out.copy_(x), a.calls, 10)
        noise_ms = timed(lambda: noise.inject(x, wz, st, N, out=out), a.calls, 10)
        nbytes = 2 * rows * H * 4 + N * H * 4 + H * F * 4
        frac = lambda b, t: round(b / (t * 1e-3) / PEAK_BYTES_PER_S, 3)                          # noqa: E731
        emb[str(H)] = {"us": round(ms * 1e3, 2), "compulsory_bytes": nbytes, "fraction_of_8tbs_peak": frac(nbytes, ms),
                       "copy_us": round(copy_ms * 1e3, 2), "copy_fraction_of_8tbs_peak": frac(2 * rows * H * 4, copy_ms),
                       "noise_inject_k16_us": round(noise_ms * 1e3, 2),
                       "noise_inject_k16_fraction_of_8tbs_peak": frac(2 * rows * H * 4 + H * 16 * 4, noise_ms)}
        del x, out, base
    solar_ms = timed(lambda: forcings.solar(clock, latlon), a.calls, 10)
    line = {"tool": "forcing_bench", "nodes": N, "members": M, "rows": rows, "forcing_columns": F, "embed": emb,
            "solar_alone_us": round(solar_ms * 1e3, 2)}
    if not a.skip_rollout:
        C = H = 256
        mesh = gwen_amd.geodesic_mesh(100, reorder="hilbert")
        n_grid = mesh.faces.shape[0]
        xm = torch.randn(M, n_grid, C, device=dev, generator=g)
        static = torch.randn(n_grid, 4, generator=torch.Generator().manual_seed(23))
        calls = {}
        for name, kw in (("plain", {}), ("forced", {"static_channels": 4, "solar": True})):
            torch.manual_seed(23)
            model = InteractionForecaster(C, H, 4, **kw).to(dev).eval()
            graphs = model.prepare(mesh, dev, grid_static=static if kw else None)
            ck = forcings.ForcingClock(772_416_000, 21600, dev) if kw else None
            cache = {}
            calls[name] = (lambda model=model, graphs=graphs, ck=ck, cache=cache:                # noqa: E731
                           ensemble_forecast(model, graphs, xm, 4, M, graphed=True, batched=True, step_cache=cache,
                                             clock=ck))
        ms = {name: [] for name in calls}
        for _ in range(a.rounds):                            # alternating: other work shares the host
            for name, call in calls.items():
                ms[name].append(timed(call, a.rollout_calls, 2))
        med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
        line["c5_rollout_ms"] = med
        line["c5_rollout_ms_rounds"] = {k: [round(t, 3) for t in v] for k, v in ms.items()}
        line["c5_rollout_forcing_overhead"] = round(med["forced"] / med["plain"] - 1.0, 4)
        line["c5_rollout"] = {"channels": H, "members": M, "steps": 4, "blocks": 4, "static_channels": 4, "solar": True,
                              "graphed": True, "batched": True}
    text = json.dumps(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
