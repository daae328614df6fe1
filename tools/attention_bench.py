"""Time the edge-attention kernel (csrc/attention.hip) on device events and print one JSON line per leg.
(BUILD-DEFINED, PARITY UNPINNED: the reference has no attention.)

    python tools/attention_bench.py [--nu 100] [--heads 8] [--calls 50] [--legs 64x16,256x4] [--skip-rollout]

Per leg "channels x members" (defaults: the HBM legs' sizes -- their arrays are beyond the 256 MiB Infinity Cache), on
the nu = 100 hilbert mesh as a block-diagonal graph of ``members`` copies, with the edge term:
* forward of the bare op, us and the fraction of the 8 TB/s HBM peak by compulsory bytes
  4 F (2 Nd + 2 Ns + E) + 4 E + 4 Nd + 4 Nd H  (q read, out written, k and v read once, ee streamed, src, rowptr, lse);
* forward + backward (autograd: pass T and pass S), us; compulsory bytes of the backward alone
  4 F (4 Nd + 4 Ns + 2 E) + 4 E (3 + 4 H) + 4 (Nd + Ns) + 4 Nd H  (pass T reads q, g, out, k, v, ee and writes gq, gee, P, DS; pass
  S reads q, g, P, DS, the edge-position CSR and dst and writes gk, gv);
* beside it, in the same session on the same edges, the by-target LayerNorm row kernel (ops.layer_norm_rows with
  rowptr, no row output: the same one-group-per-target shape), compulsory bytes 4 F (E + Nd) + 4 Nd.
Then one c5-shaped rollout (hidden channels, 4 members, 4 steps, 4 processor blocks, graphed and batched) with
processor="transformer", and with the default processor for scale, ms per rollout."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def timed(call, calls: int, warmup: int) -> float:
    """ms per call: warm, then one event pair around ``calls`` back-to-back calls"""
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


def frac(nbytes: int, ms: float) -> float:
    return round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=100)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--legs", default="64x16,256x4")
    ap.add_argument("--rollout-hidden", type=int, default=256)
    ap.add_argument("--rollout-calls", type=int, default=20)
    ap.add_argument("--skip-rollout", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import ops
    from gwen_amd.forecaster import InteractionForecaster, ensemble_forecast
    from gwen_amd.interaction import interaction_graph
    dev = torch.device("cuda:0")
    mesh = gwen_amd.geodesic_mesh(a.nu, reorder="hilbert")
    base = interaction_graph(torch.from_numpy(mesh.edge_index).to(dev), mesh.num_nodes, mesh.num_nodes)
    gen = torch.Generator(device=dev).manual_seed(23)
    H = a.heads
    for leg in a.legs.split(","):
        F, members = (int(t) for t in leg.split("x"))
        graph = base.batched(members)
        graph.segments("src")                                   # (index plumbing of the backward, built once per graph)
        n, e = graph.num_dst, graph.num_edges
        rn = lambda *s: torch.randn(*s, device=dev, generator=gen)                         # noqa: E731
        q, kv, ee, g = rn(n, F), rn(n, 2 * F), rn(e, F), rn(n, F)
        with torch.no_grad():
            fwd_ms = timed(lambda: gwen_amd.edge_attention_kv(q, kv, graph, H, ee), a.calls, 5)
        qg, kvg, eeg = (t.clone().requires_grad_(True) for t in (q, kv, ee))

        def train():
            qg.grad = kvg.grad = eeg.grad = None
            gwen_amd.edge_attention_kv(qg, kvg, graph, H, eeg).backward(g)

        both_ms = timed(train, a.calls, 5)
        del qg, kvg, eeg
        gamma, beta = torch.ones(F, device=dev), torch.zeros(F, device=dev)
        with torch.no_grad():
            ln_ms = timed(lambda: ops.layer_norm_rows(ee, gamma, beta, 1e-5, None, graph.rowptr, n, False,
                                                      want_out=False), a.calls, 5)
        fwd_b = 4 * F * (2 * n + 2 * n + e) + 4 * e + 4 * n + 4 * n * H
        bwd_b = 4 * F * (4 * n + 4 * n + 2 * e) + 4 * e * (3 + 4 * H) + 4 * (n + n) + 4 * n * H
        ln_b = 4 * F * (e + n) + 4 * n
        print(json.dumps({
            "tool": "attention_bench", "leg": leg, "nu": a.nu, "F": F, "H": H, "members": members, "Nd": n, "Ns": n, "E": e,
            "calls": a.calls, "forward_us": round(fwd_ms * 1e3, 1), "forward_compulsory_bytes": fwd_b,
            "forward_fraction_of_8tbs_peak": frac(fwd_b, fwd_ms),
            "forward_backward_us": round(both_ms * 1e3, 1), "backward_us": round((both_ms - fwd_ms) * 1e3, 1),
            "backward_compulsory_bytes": bwd_b, "backward_fraction_of_8tbs_peak": frac(bwd_b, both_ms - fwd_ms),
            "layer_norm_by_target_us": round(ln_ms * 1e3, 1), "layer_norm_compulsory_bytes": ln_b,
            "layer_norm_fraction_of_8tbs_peak": frac(ln_b, ln_ms),
            "forward_fraction_over_layer_norm_fraction": round(frac(fwd_b, fwd_ms) / max(frac(ln_b, ln_ms), 1e-9), 3),
        }), flush=True)
        del q, kv, ee, g
        torch.cuda.empty_cache()
    if a.skip_rollout:
        return
    hid, members, steps, blocks = a.rollout_hidden, 4, 4, 4
    n_grid = mesh.faces.shape[0]
    res = {}
    for kind in ("transformer", "interaction"):
        torch.manual_seed(23)
        model = InteractionForecaster(hid, hid, blocks, processor=kind, heads=H).to(dev).eval()
        graphs = model.prepare(mesh, dev)
        xm = torch.stack([torch.randn(n_grid, hid, generator=torch.Generator().manual_seed(23 + m))
                          for m in range(members)]).to(dev)
        cache = {}
        call = lambda: ensemble_forecast(model, graphs, xm, steps, members, graphed=True, batched=True,   # noqa: E731
                                         step_cache=cache)
        res[kind] = round(timed(call, max(a.rollout_calls, 1), 2), 3)
        del model, graphs, xm, cache
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "attention_bench", "leg": "c5_rollout", "nu": a.nu, "channels": hid, "heads": H,
                      "members": members, "steps": steps, "blocks": blocks, "graphed": True, "batched": True,
                      "rollout_ms": res}), flush=True)


if __name__ == "__main__":
    main()
