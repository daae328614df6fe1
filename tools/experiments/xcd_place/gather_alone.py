"""k_gather<16> of the c2 step outside the step, to be run under rocprofv3 (kernel trace, or --pmc alone):
    python tools/experiments/xcd_place/gather_alone.py static|pair|copy|alias|ring [launches] [graph]
static  the kernel relaunched on one input that nothing rewrites (the per-kernel A/B campaigns' way)
pair    every launch reads what a K5 32->16 launch (the step's producer, the same row range -> blockIdx & 7 map) has just
        written into the same buffer
copy    every launch reads what an elementwise copy kernel (no such map) has just written into the same buffer
alias   pair, with the buffers laid out as the step's scratch: the K5 launch reads [N, 32] at offset 0 and writes at offset
        64 N floats, the gather reads that and writes [N, 16] at offset 0 -- over the rows its producer has just read
ring    alias, but the gather writes at offset 128 N floats: a third buffer, as the stack launcher's ring of three
graph   the launches are captured into one hipGraph and replayed, so that they queue back to back as the step's six do
        (issued one by one from Python the GPU is idle between two launches of this size); the replay is timed with
        events and the time per captured iteration printed
Same mesh, ordering, entries, contraction and entry point as the step (gwen_gcn_chain_tuned3_f32, library choices)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
import numpy as np
import torch
import gwen_amd
from gwen_amd import _lib


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "static"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 220
    graphed = len(sys.argv) > 3 and sys.argv[3] == "graph"
    assert mode in ("static", "pair", "copy", "alias", "ring")
    dev = torch.device("cuda:0")
    mesh = gwen_amd.geodesic_mesh(100, reorder="hilbert")
    n = mesh.num_nodes
    g = gwen_amd.prepare_graph(torch.from_numpy(np.ascontiguousarray(mesh.edge_index.astype(np.int64))).to(dev), n)
    gr, gc, gv = g.grouped()
    assert gr is None and g.entries() == 7
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    torch.manual_seed(23)
    x32 = torch.randn(n, 32, device=dev)
    w = torch.randn(16, 32, device=dev) / 32 ** 0.5
    b32, b16 = 0.1 * torch.randn(32, device=dev), 0.1 * torch.randn(16, device=dev)
    src = torch.randn(n, 16, device=dev)
    t = src.clone()                                    # k_gather's input
    out = torch.empty(n, 16, device=dev)
    if mode in ("alias", "ring"):
        scratch = torch.zeros(3 * n * 64, device=dev)
        scratch[:n * 32] = x32.view(-1)
        x32, t, out = scratch[:n * 32].view(n, 32), scratch[n * 64:n * 80].view(n, 16), scratch[:n * 16].view(n, 16)
        if mode == "ring":
            out = scratch[n * 128:n * 144].view(n, 16)
    x6 = _lib.CONTRACT_BF16X6

    def gather():
        rc = L.gwen_gcn_chain_tuned3_f32(p(gr), p(gc), p(gv), p(t), None, None, p(b16), p(out), n, 16, 0, 0, 1, 1, 1,
                                         n * 16, n * 16, x6, 7, 0, 0, 0, None, None, 0, stream())
        assert rc == 0, rc

    def producer():
        rc = L.gwen_gcn_chain_tuned3_f32(p(gr), p(gc), p(gv), p(x32), p(w), None, p(b32), p(t), n, 32, 16, 0, 1, 1, 1,
                                         n * 32, n * 16, x6, 7, 0, 0, 0, None, None, 0, stream())
        assert rc == 0, rc

    def iterations():
        for _ in range(reps):
            if mode in ("pair", "alias", "ring"):
                producer()
            elif mode == "copy":
                t.copy_(src)
            gather()

    if not graphed:
        iterations()
        torch.cuda.synchronize()
        print(mode, reps, float(out.abs().sum()))
        return
    producer(); gather()                               # the launchers' one-time occupancy queries, outside the capture
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        iterations()
    for _ in range(3):
        cg.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    walls = []
    for _ in range(5):
        a.record(); cg.replay(); b.record()
        torch.cuda.synchronize()
        walls.append(a.elapsed_time(b) * 1e3 / reps)
    print(mode, "graph", reps, "us per iteration:", " ".join(f"{w:.2f}" for w in walls), float(out.abs().sum()))


if __name__ == "__main__":
    main()
