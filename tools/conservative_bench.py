"""Time the device build of a conservative Regridder (csrc/conserve.hip: cell geometry, candidate search, one clip per
candidate pair, keep rule, weights) and its apply (K2); one JSON line per direction.

    python tools/conservative_bench.py [--nu 100] [--nlat 721] [--nlon 1440] [--rounds 5] [--channels 64] [--members 4]
                                       [--out profiles/conservative_bench.jsonl]

Shapes: the faces of the nu = 100 mesh (200 000 cells) -> the cells of the nlat x nlon lat-lon grid (721 x 1440 =
1 038 240 cells, the two polar rows wedges) and back, normalize="cell".

    device_build_ms      cell_overlaps_device + overlap_weights, validated cells already on the device, warm, median of
                         --rounds brackets of device events.  The build reads back the search radius, the candidate count
                         and (boolean masking) the kept count; those waits sit inside the bracket
    geometry_ms / search_ms / clip_ms / weights_ms
                         the parts, each bracketed alone: gwen_cell_areas on both sets; radius_edges_device over the
                         centres; gwen_cell_overlap_areas over the candidates; keep rule + compaction + row pointer +
                         gwen_cell_overlap_weights
    regridder_ms         Regridder.conservative(...) end to end on a host clock: validation of both cell sets on the
                         host, uploads, the device build, the CSR (prepare_bipartite)
    apply_ms             regridder(x) at [members, Ns, C], warm, median of brackets over 10 calls each
    candidates / kept / longest_row / longest_candidate_row
                         pair counts before and after the keep rule; the most entries / candidates of one target
    conservation_error   |sum_t A_t y_t - sum_s A_s x_s| / sum_s A_s |x_s| of the fp32 apply on randn x, worst channel of
                         member 0, sums formed in fp64 on the device; conservation_bound = (longest_row + 2) 2^-24
    idw_k4_build_ms      device_build_ms of the k = 4 inverse-distance build in profiles/regrid_bench.jsonl for the same
                         direction (face CENTRES <-> lat-lon POINTS): the only yardstick there is"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def median_ms(fn, rounds: int):
    warm(fn)
    ms = [bracket(fn) for _ in range(rounds)]
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def idw_yardstick():
    """device_build_ms of profiles/regrid_bench.jsonl by direction ("faces -> latlon" / "latlon -> faces")."""
    out = {}
    try:
        with open(os.path.join(ROOT, "profiles", "regrid_bench.jsonl")) as fh:
            for row in map(json.loads, fh):
                if row.get("method") == "idw" and row.get("k") == 4:
                    out["faces -> latlon" if row["shape"].startswith("face") else "latlon -> faces"] = row["device_build_ms"]
    except OSError:
        pass
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=100)
    ap.add_argument("--nlat", type=int, default=721)
    ap.add_argument("--nlon", type=int, default=1440)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conservative_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import gridgraph as G, regrid as RG
    dev = torch.device("cuda:0")
    mesh = gwen_amd.geodesic_mesh(a.nu, reorder="hilbert")
    faces, boxes = gwen_amd.mesh_cells(mesh), gwen_amd.latlon_cells(a.nlat, a.nlon)
    yard = idw_yardstick()
    lines = []
    for key, name, src, dst in (("faces -> latlon", f"nu={a.nu} faces -> latlon cells {a.nlat}x{a.nlon}", faces, boxes),
                                ("latlon -> faces", f"latlon cells {a.nlat}x{a.nlon} -> nu={a.nu} faces", boxes, faces)):
        sc, dc = (torch.from_numpy(RG.check_cells(c)).to(dev) for c in (src, dst))
        stats: dict = {}

        def build():
            ei, area, _, da = RG.cell_overlaps_device(sc, dc)
            return RG.overlap_weights(ei, area, da, "cell")
        build_ms = median_ms(build, a.rounds)
        RG.cell_overlaps_device(sc, dc, stats)
        s_geo, d_geo = RG.cell_geometry_device(sc), RG.cell_geometry_device(dc)
        pairs, rowptr = G.radius_edges_device(s_geo[0], d_geo[0], stats["search_radius"], with_rowptr=True)
        area = RG.overlap_areas_device(sc, dc, pairs, s_geo, d_geo)

        def finish():
            keep = area > RG.KEEP_FRACTION * torch.minimum(s_geo[2][pairs[0]], d_geo[2][pairs[1]])
            return RG.overlap_weights(pairs[:, keep].contiguous(), area[keep], d_geo[2], "cell")
        parts = {"geometry_ms": median_ms(lambda: (RG.cell_geometry_device(sc), RG.cell_geometry_device(dc)), a.rounds)[0],
                 "search_ms": median_ms(lambda: G.radius_edges_device(s_geo[0], d_geo[0], stats["search_radius"]), a.rounds)[0],
                 "clip_ms": median_ms(lambda: RG.overlap_areas_device(sc, dc, pairs, s_geo, d_geo), a.rounds)[0],
                 "weights_ms": median_ms(finish, a.rounds)[0]}
        longest_candidate_row = int((rowptr[1:] - rowptr[:-1]).max().item())
        del pairs, area, rowptr, s_geo, d_geo
        t0 = time.perf_counter()
        rg = gwen_amd.Regridder.conservative(src, dst, dev, normalize="cell")
        torch.cuda.synchronize()
        e2e = (time.perf_counter() - t0) * 1e3
        ns, nd, e = rg.num_src, rg.num_dst, int(rg.edge_index.size(1))
        longest = int(torch.bincount(rg.edge_index[1], minlength=nd).max().item())
        x = torch.randn(a.members, ns, a.channels, device=dev)
        y = rg(x)                                                    # the lazy layouts
        warm(lambda: rg(x))
        ap_ms = statistics.median(bracket(lambda: rg(x), 10) for _ in range(a.rounds))
        got = (rg.dst_area[:, None] * y[0].double()).sum(dim=0)
        want = (rg.src_area[:, None] * x[0].double()).sum(dim=0)
        scale = (rg.src_area[:, None] * x[0].double().abs()).sum(dim=0)
        line = {"tool": "conservative_bench", "shape": name, "normalize": "cell", "num_src": ns, "num_dst": nd,
                "candidates": stats["candidates"], "kept": stats["kept"], "entries": e, "longest_row": longest,
                "longest_candidate_row": longest_candidate_row, "search_radius": stats["search_radius"],
                "device_build_ms": build_ms[0], "device_build_ms_min": build_ms[1], "device_build_ms_max": build_ms[2],
                **parts, "rounds": a.rounds, "regridder_ms": round(e2e, 1), "channels": a.channels,
                "members": a.members, "apply_ms": round(ap_ms, 4),
                "coverage_min": float(rg.coverage.min().item()), "coverage_max": float(rg.coverage.max().item()),
                "conservation_error": float(((got - want).abs() / scale).max().item()),
                "conservation_bound": (longest + 2) * 2.0 ** -24, "idw_k4_build_ms": yard.get(key)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del rg, x, y, sc, dc
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
