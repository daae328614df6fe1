"""Training through rollouts: time and memory of one training iteration (forward sweep, loss, backward -- timed
together) of ``InteractionForecaster.rollout(grad=True)``, the plain chain (``checkpoint=False``) next to the
checkpointed one (``checkpoint=True``), on the BASELINE config c5 shape: geodesic mesh nu = 100 (100 002 vertices,
200 000 grid cells), 4 processor blocks.  One JSON line per configuration (hidden x members x n_steps), appended to
profiles/rollout_train_bench.jsonl.
python tools/rollout_train_bench.py [--nu 100] [--channels 64] [--hidden 64 256] [--members 1 4] [--steps 1 4 8]
                                    [--iters 5] [--warmup 2] [--out FILE]
The loss is the mean squared error of every state against a fixed target.  Per configuration both chains are warmed up
(every shape once, then at least 0.1 s of the same work), then timed alternately, one synchronised iteration at a time;
the figures are medians.  Memory: ``torch.cuda.max_memory_allocated`` over one iteration above ``memory_allocated`` just
before it (weights, graphs, inputs and the caches the warm-up filled are the resident baseline; the parameter gradients
are inside the figure, for both chains alike).  A configuration whose plain chain runs out of memory is recorded as
skipped, with the checkpointed chain's figures alone."""
import argparse, gc, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, gwen_amd
from gwen_amd.forecaster import InteractionForecaster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--nu", type=int, default=100)
ap.add_argument("--channels", type=int, default=64)
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
ap.add_argument("--members", type=int, nargs="+", default=[1, 4])
ap.add_argument("--steps", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_train_bench.jsonl"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_train_bench: needs the GPU (a CPU run measures nothing)")
dev = "cuda:0"
mesh = gwen_amd.geodesic_mesh(args.nu, reorder="hilbert")
n = mesh.faces.shape[0]


def iteration(model, graphs, x, y, steps, checkpoint):
    model.zero_grad(set_to_none=True)
    states = model.rollout(x, graphs, steps, grad=True, checkpoint=checkpoint)
    loss = sum((s - y).square().mean() for s in states)
    loss.backward()
    return loss


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def peak_above_baseline(fn, model):
    model.zero_grad(set_to_none=True)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = float(fn().detach())
    return torch.cuda.max_memory_allocated() - base, base, loss


def release(model=None):
    if model is not None:
        model.zero_grad(set_to_none=True)
    gc.collect()
    torch.cuda.empty_cache()


os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for hidden in args.hidden:
    torch.manual_seed(23)
    model = InteractionForecaster(args.channels, hidden, args.blocks).to(dev)
    graphs = model.prepare(mesh, dev)
    for members in args.members:
        shape = (n, args.channels) if members == 1 else (members, n, args.channels)
        x, y = torch.randn(*shape, device=dev), torch.randn(*shape, device=dev)
        for steps in args.steps:
            run = {c: (lambda c=c: iteration(model, graphs, x, y, steps, c)) for c in (False, True)}
            modes, skipped = [False, True], None
            try:                                           # every shape once: code objects, tilings, the graphs' caches
                for _ in range(args.warmup):
                    run[False]()
                torch.cuda.synchronize()
            except torch.OutOfMemoryError as exc:
                modes, skipped = [True], f"the plain chain does not fit: {str(exc).splitlines()[0]}"
                release(model)
            for _ in range(args.warmup):
                run[True]()
            t0 = time.perf_counter()                       # >= 0.1 s of the same work: the clocks ramp after idling
            while time.perf_counter() - t0 < 0.1:
                for c in modes:
                    run[c]()
                torch.cuda.synchronize()
            times = {c: [] for c in modes}
            for _ in range(args.iters):                    # alternating: both chains see the same machine
                for c in modes:
                    times[c].append(timed_once(run[c]))
            mem, loss, base = {}, {}, None
            for c in modes:
                mem[c], base, loss[c] = peak_above_baseline(run[c], model)
            rec = {"tool": "rollout_train_bench", "device": torch.cuda.get_device_name(0), "nu": args.nu, "grid": n,
                   "mesh_nodes": mesh.num_nodes, "mesh_edges": graphs.mesh.num_edges, "channels": args.channels,
                   "hidden": hidden, "processor_blocks": args.blocks, "members": members, "n_steps": steps,
                   "iters": args.iters, "warmup": args.warmup, "resident_baseline_bytes": base,
                   "ckpt_ms": round(statistics.median(times[True]) * 1e3, 3),
                   "ckpt_ms_min_max": [round(min(times[True]) * 1e3, 3), round(max(times[True]) * 1e3, 3)],
                   "ckpt_peak_bytes": mem[True]}
            if skipped is None:
                rec.update({"plain_ms": round(statistics.median(times[False]) * 1e3, 3),
                            "plain_ms_min_max": [round(min(times[False]) * 1e3, 3), round(max(times[False]) * 1e3, 3)],
                            "plain_peak_bytes": mem[False],
                            "time_ratio_ckpt_over_plain": round(statistics.median(times[True]) /
                                                                statistics.median(times[False]), 3),
                            "peak_ratio_plain_over_ckpt": round(mem[False] / max(mem[True], 1), 2),
                            "same_loss_bits": loss[True] == loss[False]})
            else:
                rec["plain_skipped"] = skipped
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            release(model)
        del x, y
    del model, graphs
    release()
