"""Time the device build of the grid <-> mesh graphs (gwen_amd/gridgraph.py, csrc/gridgraph.hip) against a host yardstick on
the same box, and one c5-shaped rollout line; one JSON line per shape.

    python tools/gridgraph_bench.py [--nu 100] [--nlat 721] [--nlon 1440] [--rounds 5] [--out profiles/gridgraph_bench.jsonl]
                                    [--no-host] [--no-rollout] [--build-only K]

Shapes: an nlat x nlon lat-lon grid (721 x 1440 = 1 038 240 points) against the nu = 100 mesh at the default radius, and
the same mesh's own face centres.

    device_build_ms          g2m (radius edges: count, read-back of the total, fill) + m2g (containing faces), positions
                             already on the device, warm, median of --rounds brackets of device events -- the read-back
                             sits inside the bracket, so this is what a caller waits for
    grid_graphs_ms           gwen_amd.grid_graphs end to end on a host clock: normalisation, validation, uploads, the
                             device build, the m2g edge list and the degree statistics of ``info``
    host_*_ms                scipy.spatial.cKDTree(mesh nodes).query_ball_point(grid, r, workers=16) (tree build included;
                             flattening its Python lists into a sorted edge list is host_edge_list_ms, kept apart), plus a
                             point-in-triangle pass: the 6 nearest face centres of every point (cKDTree.query, workers=16)
                             tested with the library's three determinants in numpy
    rollout                  a 64-channel, 4-block forecaster, 4-step graphed rollout of one member on the lat-lon grid and
                             on the default grid of the same mesh: what the longer g2m rows cost in K6

--build-only K: K warm device builds of the lat-lon shape and nothing else (the target of a kernel trace)."""
from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

WORKERS = 16


def device_build(G, gp, mp, faces, centres, radius, max_edge):
    g2m = G.radius_edges_device(gp, mp, radius)
    face, w = G.containing_faces_device(gp, mp, faces, centres, max_edge)
    return g2m, face, w


def bracket(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def host_yardstick(grid, mesh, radius):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(mesh.pos)
    lists = tree.query_ball_point(grid, radius, workers=WORKERS)
    tq = time.perf_counter()
    lens = np.fromiter(map(len, lists), dtype=np.int64, count=len(lists))
    src = np.repeat(np.arange(grid.shape[0], dtype=np.int64), lens)
    dst = np.fromiter(itertools.chain.from_iterable(lists), dtype=np.int64, count=int(lens.sum()))
    order = np.lexsort((src, dst))
    g2m = np.stack([src[order], dst[order]])
    t1 = time.perf_counter()
    c = mesh.pos[mesh.faces].mean(axis=1)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    _, cand = cKDTree(c).query(grid, k=6, workers=WORKERS)                       # [N, 6] face ids, nearest first
    face = np.full(grid.shape[0], np.iinfo(np.int64).max)
    for k in range(cand.shape[1]):
        f = cand[:, k]
        a, b, cc = mesh.pos[mesh.faces[f, 0]], mesh.pos[mesh.faces[f, 1]], mesh.pos[mesh.faces[f, 2]]
        det = lambda u, v, w: np.einsum("ij,ij->i", u, np.cross(v, w))           # noqa: E731
        ok = (det(grid, b, cc) >= -1e-12) & (det(grid, cc, a) >= -1e-12) & (det(grid, a, b) >= -1e-12)
        face = np.where(ok & (f < face), f, face)
    t2 = time.perf_counter()
    return g2m, face, (tq - t0) * 1e3, (t1 - tq) * 1e3, (t2 - t1) * 1e3


def timed_rollout(model, graphs, x, steps=4, k=5):
    from gwen_amd.forecaster import GraphedStep
    with torch.no_grad():
        step = GraphedStep(model, graphs, x)

        def roll():
            cur = x
            for _ in range(steps):
                cur = step(cur)
        t0 = time.perf_counter()                      # >= 0.1 s of the same work first: the clocks ramp after idling
        while time.perf_counter() - t0 < 0.1:
            roll()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            roll()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=100)
    ap.add_argument("--nlat", type=int, default=721)
    ap.add_argument("--nlon", type=int, default=1440)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--build-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gridgraph_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import gridgraph as G
    from gwen_amd.forecaster import InteractionForecaster
    dev = torch.device("cuda:0")
    mesh = gwen_amd.geodesic_mesh(a.nu, reorder="hilbert")
    max_edge = mesh.max_edge_length()
    radius = G.RADIUS_FACTOR * max_edge
    mp, faces, centres = G.mesh_on_device(mesh, dev)
    shapes = [(f"latlon {a.nlat}x{a.nlon}", gwen_amd.latlon_grid(a.nlat, a.nlon)[0]), ("face centres", G.face_centres(mesh))]
    lines = []
    for name, grid in shapes:
        grid = G.unit_vectors(grid)
        gp = torch.from_numpy(grid).to(dev)
        build = lambda: device_build(G, gp, mp, faces, centres, radius, max_edge)  # noqa: E731
        for _ in range(3):
            build()
        torch.cuda.synchronize()
        if a.build_only:
            for _ in range(a.build_only):
                build()
            torch.cuda.synchronize()
            return
        ms = [bracket(build) for _ in range(a.rounds)]
        g2m, face, _ = build()
        t0 = time.perf_counter()
        _, _, info = gwen_amd.grid_graphs(mesh, grid, dev)
        torch.cuda.synchronize()
        e2e = (time.perf_counter() - t0) * 1e3
        line = {"tool": "gridgraph_bench", "shape": name, "nu": a.nu, "grid_points": int(grid.shape[0]),
                "mesh_nodes": mesh.num_nodes, "faces": int(mesh.faces.shape[0]), "radius": radius,
                "cells_per_axis": int(gwen_amd._lib.lib().gwen_gridgraph_cells(radius)),
                "device_build_ms": round(statistics.median(ms), 3), "device_build_ms_min": round(min(ms), 3),
                "device_build_ms_max": round(max(ms), 3), "rounds": a.rounds, "grid_graphs_ms": round(e2e, 1),
                **{k: v for k, v in info.items() if k != "radius"}}
        if not a.no_host:
            h_g2m, h_face, t_ball, t_list, t_tri = host_yardstick(grid, mesh, radius)
            line.update({"host_ball_query_ms": round(t_ball, 1), "host_edge_list_ms": round(t_list, 1),
                         "host_point_in_triangle_ms": round(t_tri, 1),
                         "host_total_ms": round(t_ball + t_list + t_tri, 1), "host_workers": WORKERS,
                         "host_g2m_equal": bool(np.array_equal(h_g2m, g2m.cpu().numpy())),
                         "host_face_mismatches": int((h_face != face.cpu().numpy()).sum()),
                         "device_over_host_query_and_triangles": round(statistics.median(ms) / (t_ball + t_tri), 4)})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if not a.no_rollout:
        torch.manual_seed(23)
        model = InteractionForecaster(64, 64, 4).to(dev).eval()
        line = {"tool": "gridgraph_bench", "shape": "rollout C=64 H=64 blocks=4 steps=4 members=1 graphed", "nu": a.nu}
        for key, grid in (("default_grid", None), ("latlon_grid", shapes[0][1])):
            graphs = model.prepare(mesh, dev, grid_pos=grid)
            x = torch.randn(graphs.grid_nodes, 64, device=dev)
            line[key] = {"grid_points": graphs.grid_nodes, "g2m_edges": graphs.g2m.num_edges,
                         "g2m_max_in_degree": graphs.g2m.max_degree, "m2g_edges": graphs.m2g.num_edges,
                         "rollout4_ms": round(timed_rollout(model, graphs, x), 3)}
            del graphs, x
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
