"""Time the device build of a Regridder (csrc/regrid.hip: k-nearest search + weights) and its apply (K2) against a host
yardstick on the same box; one JSON line per direction.

    python tools/regrid_bench.py [--nu 100] [--nlat 721] [--nlon 1440] [--k 4] [--rounds 5] [--channels 64] [--members 4]
                                 [--out profiles/regrid_bench.jsonl] [--no-host]

Shapes: the face centres of the nu = 100 mesh (200 000 points) -> the nlat x nlon lat-lon grid (721 x 1440 = 1 038 240
points) and back, "idw" with k = 4.

    device_build_ms      the search (every round of the doubling loop) + the weights, positions already on the device,
                         warm, median of --rounds brackets of device events.  The loop reads ONE number back per round and
                         those waits sit inside the bracket (it is what a caller waits for); search_rounds says how many
                         there were and readback_ms what one 4-byte read-back costs on the idle stream, so they can be
                         taken off
    regridder_ms         gwen_amd.Regridder(...) end to end on a host clock: normalisation, validation, uploads, the
                         device build, the edge list and the CSR (prepare_bipartite)
    apply_ms             regridder(x) at [members, Ns, C], warm, median of brackets over 10 calls each; apply_fraction_of_8TBs
                         = compulsory bytes (every source row the operator names read once, y written once, the CSR read once) / time / 8e12
    host_query_ms        scipy.spatial.cKDTree(src).query(dst, k, workers=16), tree build included -- when scipy imports"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

WORKERS = 16
PEAK_BYTES_PER_S = 8e12


def bracket(fn, calls: int = 1):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def warm(fn, seconds: float = 0.1):
    t0 = time.perf_counter()                          # the clocks ramp after idling
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=100)
    ap.add_argument("--nlat", type=int, default=721)
    ap.add_argument("--nlon", type=int, default=1440)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regrid_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import gridgraph as G, regrid as RG
    dev = torch.device("cuda:0")
    mesh = gwen_amd.geodesic_mesh(a.nu, reorder="hilbert")
    centres = G.unit_vectors(G.face_centres(mesh))
    latlon = G.unit_vectors(gwen_amd.latlon_grid(a.nlat, a.nlon)[0])
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    lines = []
    for name, src, dst in ((f"face centres -> latlon {a.nlat}x{a.nlon}", centres, latlon),
                           (f"latlon {a.nlat}x{a.nlon} -> face centres", latlon, centres)):
        sp, dp = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
        stats: dict = {}

        def build():
            idx, d2, count = RG.knn_device(sp, None, dp, a.k, stats=stats)
            return idx, RG.knn_weights(d2, count, "idw", 1.0)
        warm(build)
        ms = [bracket(build) for _ in range(a.rounds)]
        torch.cuda.synchronize()
        rb = []
        for _ in range(9):
            t0 = time.perf_counter()
            one.item()
            rb.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rg = gwen_amd.Regridder(src, dst, dev, k=a.k)
        torch.cuda.synchronize()
        e2e = (time.perf_counter() - t0) * 1e3
        ns, nd, e = rg.num_src, rg.num_dst, int(rg.edge_index.size(1))
        x = torch.randn(a.members, ns, a.channels, device=dev)
        rg(x)                                                        # the lazy layouts
        warm(lambda: rg(x))
        ap_ms = statistics.median(bracket(lambda: rg(x), 10) for _ in range(a.rounds))
        used = int(torch.unique(rg.edge_index[0]).numel())           # source rows the operator names at all
        nbytes = 4 * a.members * a.channels * (used + nd) + 4 * (nd + 1) + 8 * e
        line = {"tool": "regrid_bench", "shape": name, "method": "idw", "k": a.k, "num_src": ns, "num_dst": nd, "entries": e, "sources_used": used,
                "device_build_ms": round(statistics.median(ms), 3), "device_build_ms_min": round(min(ms), 3),
                "device_build_ms_max": round(max(ms), 3), "rounds": a.rounds, "search_rounds": stats.get("rounds"),
                "initial_radius": stats.get("initial_radius"), "readback_ms": round(statistics.median(rb), 4),
                "regridder_ms": round(e2e, 1), "channels": a.channels, "members": a.members,
                "apply_ms": round(ap_ms, 4), "apply_compulsory_bytes": nbytes,
                "apply_fraction_of_8TBs": round(nbytes / (ap_ms * 1e-3) / PEAK_BYTES_PER_S, 4)}
        if a.no_host:
            line["host"] = "skipped (--no-host)"
        else:
            try:
                from scipy.spatial import cKDTree
            except ImportError:
                line["host"] = "skipped: scipy does not import here"
            else:
                t0 = time.perf_counter()
                _, hidx = cKDTree(src).query(dst, k=a.k, workers=WORKERS)
                line["host_query_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                line["host_workers"] = WORKERS
                got = build()[0].cpu().numpy()
                # (cKDTree orders ties by its own traversal: rows may differ where distances tie, e.g. at the poles)
                line["host_rows_equal"] = int((np.sort(hidx, axis=1) == np.sort(got, axis=1)).all(axis=1).sum())
                line["device_over_host_query"] = round(statistics.median(ms) / line["host_query_ms"], 5)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rg, x, sp, dp
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
