"""Time the InteractionNet block (K6) on the c2 mesh: per-launch times, HBM and MFMA figures.
Usage: python tools/inet_bench.py [--channels 64] [--nu 100] [--iters 50] [--members 1] [--precision 3xbf16|f16x3] [--layer-norm]
--layer-norm: K6 with a LayerNorm behind the second layer -- the edge and node launches without it, with it on the route the
library takes (fused where an instantiation exists) and forced through the unfused route, as JSON lines."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gwen_amd
from gwen_amd import ops
from gwen_amd.interaction import InteractionNet, interaction_graph, mlp2


def timed(fn, iters):
    import time
    t0 = time.perf_counter()             # 0.1 s of the same work first: the clocks ramp for tens of ms after idling
    while time.perf_counter() - t0 < 0.1:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--nu", type=int, default=100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--graph", default="mesh", choices=["mesh", "g2m", "m2g"])
    ap.add_argument("--reorder", default="morton", choices=["none", "morton", "hilbert"])
    ap.add_argument("--act", default="silu", choices=["none", "relu", "silu"])
    ap.add_argument("--precision", default="3xbf16", choices=["3xbf16", "f16x3"])
    ap.add_argument("--members", type=int, default=1, help="copies of the graph in one block-diagonal launch")
    ap.add_argument("--layer-norm", action="store_true", help="time K6 with LayerNorm: fused / unfused / without")
    args = ap.parse_args()
    P = args.precision
    lin = (lambda x, w, b: ops.linear(x, w, b, exact=False)) if P == "3xbf16" else \
        (lambda x, w, b: ops.linear(x, w, b, contract=P))                                    # noqa: E731
    dev = "cuda:0"
    F = args.channels
    mesh = gwen_amd.geodesic_mesh(args.nu, reorder=None if args.reorder == 'none' else args.reorder)
    if args.graph == "mesh":
        ei, ns, nd = torch.from_numpy(mesh.edge_index), mesh.num_nodes, mesh.num_nodes
    else:
        from gwen_amd import g2m
        a, b = g2m.grid_mesh_edges(mesh)
        ei, ns, nd = (torch.from_numpy(a), mesh.faces.shape[0], mesh.num_nodes) if args.graph == "g2m" \
            else (torch.from_numpy(b), mesh.num_nodes, mesh.faces.shape[0])
    g = interaction_graph(ei.to(dev), ns, nd).batched(args.members)
    ns, nd = ns * args.members, nd * args.members
    E = g.num_edges
    torch.manual_seed(23)
    net = InteractionNet(F, args.act, precision=P).to(dev)
    xs = torch.randn(ns, F, device=dev)
    xd = xs if args.graph == "mesh" else torch.randn(nd, F, device=dev)
    e = torch.randn(E, F, device=dev)
    with torch.no_grad():
        w1, b1 = net.edge_mlp[0].weight, net.edge_mlp[0].bias
        w1e, w1s, w1d = (w1[:, :F].contiguous(), w1[:, F:2 * F].contiguous(), w1[:, 2 * F:].contiguous())
        w2, b2 = net.edge_mlp[2].weight, net.edge_mlp[2].bias
        ps = lin(xs, w1s, None)
        pd = lin(xd, w1d, b1)
        t_proj = timed(lambda: lin(xs, w1s, None), args.iters)
        t_edge = timed(lambda: mlp2(e, w1e, w2, b2, g1=ps, idx1=g.src, g2=pd, idx2=g.dst, res=e, graph=g, act=args.act,
                                    contract=P), args.iters)
        t_edge_noagg = timed(lambda: mlp2(e, w1e, w2, b2, g1=ps, idx1=g.src, g2=pd, idx2=g.dst, res=e, act=args.act,
                                          contract=P), args.iters)
        t_edge_plain = timed(lambda: mlp2(e, w1e, w2, b2, res=e, act=args.act, contract=P), args.iters)
        _, agg = mlp2(e, w1e, w2, b2, g1=ps, idx1=g.src, g2=pd, idx2=g.dst, res=e, graph=g, act=args.act, contract=P)
        w3 = net.node_mlp[0].weight
        q = lin(xd, w3[:, :F].contiguous(), net.node_mlp[0].bias)
        w3b = w3[:, F:].contiguous()
        t_node = timed(lambda: mlp2(agg, w3b, net.node_mlp[2].weight, net.node_mlp[2].bias, g1=q, res=xd, act=args.act,
                                    contract=P), args.iters)
        t_block = timed(lambda: net(xs, xd, e, g), args.iters)
    if args.layer_norm:
        layer_norm_lines(args, net, g, e, w1e, ps, pd, agg, w3b, q, xs, xd)
    # algorithmic bytes of the edge launch: e read + e' write + two gathered rows + agg write + indices
    b_alg = 4 * F * (4 * E + nd) + 8 * E + 4 * nd
    flops = 4 * F * F * E                     # two F x F contractions per edge, fp32-equivalent
    print(f"graph {args.graph}: Ns={ns} Nd={nd} E={E} F={F} max_degree={g.max_degree} members={args.members} "
          f"precision={P}")
    print(f"node projection (K3)        {t_proj:8.1f} us")
    print(f"edge MLP + aggregate (K6)   {t_edge:8.1f} us   {b_alg / t_edge / 1e3:7.1f} GB/s algorithmic, "
          f"{flops / t_edge / 1e6:6.1f} TFLOP/s fp32-equivalent ({3 * flops / t_edge / 1e6:6.1f} bf16 issued), "
          f"{E / t_edge / 1e3:6.2f} G edges/s")
    print(f"  without aggregation       {t_edge_noagg:8.1f} us")
    print(f"  without gathers either    {t_edge_plain:8.1f} us")
    print(f"node MLP (K6)               {t_node:8.1f} us")
    print(f"whole block (1 K3 + 2 K6)    {t_block:8.1f} us   {E / t_block / 1e3:6.2f} G edges/s")


def layer_norm_lines(args, net, g, e, w1e, ps, pd, agg, w3b, q, xs, xd):
    """K6's edge and node launches without LayerNorm, with it (the library's route) and with it forced unfused; the row
    kernel alone with its compulsory bytes (x read, res read, out write, agg write) against 8 TB/s."""
    from gwen_amd import _lib, interaction
    F, P, E, nd = args.channels, args.precision, g.num_edges, g.num_dst
    lnet = InteractionNet(F, args.act, precision=P, layer_norm=True).to(e.device)
    lnet.load_state_dict(net.state_dict(), strict=False)
    w2, b2 = net.edge_mlp[2].weight, net.edge_mlp[2].bias
    edge = lambda **kw: mlp2(e, w1e, w2, b2, g1=ps, idx1=g.src, g2=pd, idx2=g.dst, res=e, graph=g, act=args.act,   # noqa: E731
                             contract=P, **kw)
    node = lambda **kw: mlp2(agg, w3b, net.node_mlp[2].weight, net.node_mlp[2].bias, g1=q, res=xd, act=args.act,    # noqa: E731
                             contract=P, **kw)
    code = interaction.MLP2_CONTRACTS[P]
    fused = {s: bool(_lib.lib().gwen_mlp2_ln_supported(F, code, c))
             for s, c in (("edge", _lib.MLP2_LN_EDGE), ("node", _lib.MLP2_LN_NODE))}
    with torch.no_grad():
        out = {"tool": "inet_bench --layer-norm", "channels": F, "precision": P, "members": args.members, "edges": E,
               "targets": nd, "fused_instantiation": fused,
               "edge_us_no_ln": round(timed(edge, args.iters), 1), "node_us_no_ln": round(timed(node, args.iters), 1),
               "edge_us_ln": round(timed(lambda: edge(**lnet._ln("edge")), args.iters), 1),
               "node_us_ln": round(timed(lambda: node(**lnet._ln("node")), args.iters), 1),
               "block_us_no_ln": round(timed(lambda: net(xs, xd, e, g), args.iters), 1),
               "block_us_ln": round(timed(lambda: lnet(xs, xd, e, g), args.iters), 1)}
        interaction._LN_FORCE_UNFUSED = True
        out["edge_us_ln_unfused"] = round(timed(lambda: edge(**lnet._ln("edge")), args.iters), 1)
        out["node_us_ln_unfused"] = round(timed(lambda: node(**lnet._ln("node")), args.iters), 1)
        interaction._LN_FORCE_UNFUSED = False
        kw = lnet._ln("edge")
        gy = torch.randn_like(e)                  # (the pre-norm rows of the unfused route: an array of their own)
        t_row = timed(lambda: ops.layer_norm_rows(gy, kw["ln_weight"], kw["ln_bias"], kw["ln_eps"], e, g.rowptr, nd), args.iters)
        t_bwd = timed(lambda: ops.layer_norm_backward(e, gy, kw["ln_weight"], kw["ln_eps"]), args.iters)
    out["row_kernel_us"], out["row_kernel_bwd_us"] = round(t_row, 1), round(t_bwd, 1)
    out["row_kernel_fraction_of_8TBps"] = round(4 * F * (3 * E + nd) / (t_row * 1e-6) / 8e12, 3)
    out["row_kernel_bwd_fraction_of_8TBps"] = round(4 * F * 3 * E / (t_bwd * 1e-6) / 8e12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
