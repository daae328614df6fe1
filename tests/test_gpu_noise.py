"""Latent noise on the MI355X (csrc/noise.hip through gwen_amd.noise and the forecaster) against numpy's Philox and
fp64 compositions: the generator, its statistics, the fused injection, shard invariance, the forecaster's paths and
training, and two ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import noise_ref as NR
from ensemble_ref import reference
from helpers import SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


@pytest.mark.parametrize("seed", [0, 23, (1 << 64) - 1])
@pytest.mark.parametrize("tag", [0, 1])
def test_normal_matches_numpy_philox(ga, seed, tag):
    from gwen_amd import noise
    nodes, K = 1000, 64
    for draw in (0, 1, 1 << 40):
        st = noise.NoiseStream(seed, DEV, draw=draw)
        assert st.draw == draw
        got = noise.normal(st, 4, nodes, K, tag=tag).double().cpu().numpy()
        for m in range(4):
            assert np.abs(got[m] - NR.normal(seed, tag, draw, m, nodes, K)).max() <= 4e-6, (draw, m)
        hi = noise.normal(st, 2, nodes, K, member0=1 << 33, tag=tag).double().cpu().numpy()
        for m in range(2):
            assert np.abs(hi[m] - NR.normal(seed, tag, draw, (1 << 33) + m, nodes, K)).max() <= 4e-6, (draw, m)
    st = noise.NoiseStream(seed, DEV, draw=3)                    # any K: the last block is cut
    got = noise.normal(st, 2, 50, 13, member0=5, tag=tag).double().cpu().numpy()
    for m in range(2):
        assert np.abs(got[m] - NR.normal(seed, tag, 3, 5 + m, 50, 13)).max() <= 4e-6


def test_normal_statistics(ga):
    from gwen_amd import noise
    st = noise.NoiseStream(SEED, DEV, draw=11)
    a = noise.normal(st, 4, 16384, 64).double()                  # 4.2e6 samples
    st.advance(1)
    b = noise.normal(st, 4, 16384, 64).double()
    z = a.flatten()
    assert abs(float(z.mean())) <= 3e-3
    assert abs(float(z.var()) - 1.0) <= 3e-3
    assert abs(float((z ** 4).mean()) - 3.0) <= 2e-2

    def corr(u, v):
        u, v = u.flatten() - u.mean(), v.flatten() - v.mean()
        return float((u * v).mean() / (u.std() * v.std()))

    assert abs(corr(a[1:], a[:-1])) <= 3e-3                     # member
    assert abs(corr(a[:, 1:], a[:, :-1])) <= 3e-3               # node
    assert abs(corr(a[..., 1:], a[..., :-1])) <= 3e-3           # k
    assert abs(corr(a, b)) <= 3e-3                              # draw
    assert st.draw == 12


@pytest.mark.parametrize("H", [32, 64, 128, 256, 320, 512])      # (320, 512: two column blocks, the last partial)
@pytest.mark.parametrize("K", [8, 32, 64])
def test_inject_vs_fp64(ga, H, K):
    from gwen_amd import noise
    g = torch.Generator().manual_seed(SEED + H + K)
    nodes, member0 = 37, 2
    rows = nodes * 3 + 11                                       # a partial member at the end
    x = torch.randn(rows, H, generator=g).to(DEV)
    wz = (torch.randn(H, K, generator=g) * 0.3).to(DEV)
    st = noise.NoiseStream(SEED, DEV, draw=4)
    z = noise.normal(st, 4, nodes, K, member0=member0).view(-1, K)[:rows]
    want = x.double() + z.double() @ wz.double().t()
    got = noise.inject(x, wz, st, nodes, member0)
    assert rel_err(got, want) <= 1e-6
    assert torch.equal(got, noise.inject(x, wz, st, nodes, member0))
    xi = x.clone()
    assert noise.inject(xi, wz, st, nodes, member0, out=xi).data_ptr() == xi.data_ptr()
    assert torch.equal(xi, got)
    assert st.draw == 4


def test_inject_many_rows(ga):
    """More row groups than the grid has waves: the grid-stride loop."""
    from gwen_amd import noise
    g = torch.Generator().manual_seed(SEED)
    nodes, rows, H, K = 100002, 300007, 32, 64
    x = torch.randn(rows, H, generator=g).to(DEV)
    wz = (torch.randn(H, K, generator=g) * 0.3).to(DEV)
    st = noise.NoiseStream(7, DEV, draw=2)
    z = noise.normal(st, 4, nodes, K).view(-1, K)[:rows]
    want = x.double() + z.double() @ wz.double().t()
    assert rel_err(noise.inject(x, wz, st, nodes), want) <= 1e-6


def test_inject_is_shard_invariant(ga):
    from gwen_amd import noise
    g = torch.Generator().manual_seed(SEED)
    nodes, H, K = 641, 64, 16
    x = torch.randn(5 * nodes, H, generator=g).to(DEV)
    wz = torch.randn(H, K, generator=g).to(DEV)
    st = noise.NoiseStream(99, DEV, draw=6)
    full = noise.inject(x, wz, st, nodes)
    for m in range(5):
        one = noise.inject(x[m * nodes:(m + 1) * nodes].contiguous(), wz, st, nodes, member0=m)
        assert torch.equal(one, full[m * nodes:(m + 1) * nodes])
    tail = noise.inject(x[3 * nodes:].contiguous(), wz, st, nodes, member0=3)
    assert torch.equal(tail, full[3 * nodes:])


def _models(ga, K=16, H=64, C=6, steps=2, precision="3xbf16", scale=0.0):
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(SEED)
    det = InteractionForecaster(C, H, steps, precision=precision)
    torch.manual_seed(SEED)
    noisy = InteractionForecaster(C, H, steps, precision=precision, noise_channels=K)
    with torch.no_grad():
        for p in det.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
        noisy.load_state_dict({**det.state_dict(), "noise_embed.weight": noisy.noise_embed.weight}, strict=True)
        noisy.noise_embed.weight.normal_(0, scale) if scale else noisy.noise_embed.weight.zero_()
    return det.to(DEV), noisy.to(DEV)


def test_zero_noise_weight_is_deterministic(ga):
    from gwen_amd import noise
    m = ga.geodesic_mesh(5)
    det, noisy = _models(ga)
    graphs = det.prepare(m, DEV)
    x = torch.randn(m.faces.shape[0], 6, device=DEV)
    st = noise.NoiseStream(SEED, DEV)
    with torch.no_grad():
        assert torch.equal(noisy(x, graphs, noise=st), det(x, graphs))
        assert torch.equal(noisy(x, graphs), det(x, graphs))
    a = noisy.rollout(x, graphs, 3, noise=st)
    b = det.rollout(x, graphs, 3)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert st.draw == 4


def test_model_pickled_before_noise_runs_deterministically(ga):
    """A model pickled before noise_channels existed has no such attribute: it loads as K = 0, and a step given a
    stream runs the deterministic path (and still advances the draw)."""
    import pickle
    from gwen_amd import noise
    m = ga.geodesic_mesh(4)
    det, _ = _models(ga)
    graphs = det.prepare(m, DEV)
    x = torch.randn(m.faces.shape[0], 6, device=DEV)
    old = pickle.loads(pickle.dumps(det))
    del old.__dict__["noise_channels"]
    old = pickle.loads(pickle.dumps(old))
    assert "noise_channels" not in old.__dict__
    st = noise.NoiseStream(SEED, DEV)
    with torch.no_grad():
        assert torch.equal(old(x, graphs, noise=st), det(x, graphs))
    assert st.draw == 1


@pytest.mark.parametrize("precision,tol", [("f16x3", 1e-6), ("3xbf16", 1e-4)])
def test_noisy_step_vs_fp64(ga, precision, tol):
    from gwen_amd import noise
    m = ga.geodesic_mesh(5)
    _, model = _models(ga, K=32, H=64, precision=precision, scale=0.3)
    graphs = model.prepare(m, DEV)
    x0 = torch.randn(2, m.faces.shape[0], 6, generator=torch.Generator().manual_seed(SEED))
    st = noise.NoiseStream(5, DEV, draw=9)
    z = noise.normal(st, 2, m.num_nodes, 32, member0=4).double().cpu()
    with torch.no_grad():
        got = model(x0.to(DEV), graphs, noise=st, member0=4)
    assert st.draw == 10
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    inp = NR.graph_inputs(m)
    for i in range(2):
        want = NR.forecaster_step_noisy(sd, x0[i].double(), *inp, 2, z=z[i])
        assert rel_err(got[i], want) <= tol, i
    assert float((z[0] @ sd["noise_embed.weight"].t()).abs().max()) > 0.1           # the noise term is not negligible


def test_crps_gradients_with_noise(ga):
    from gwen_amd import noise
    m = ga.geodesic_mesh(4, reorder="hilbert")
    _, model = _models(ga, K=16, H=64, precision="f16x3", scale=0.5)
    graphs = model.prepare(m, DEV)
    nf = m.faces.shape[0]
    x0 = torch.randn(nf, 6, generator=torch.Generator().manual_seed(SEED))
    y = torch.randn(nf, 6, generator=torch.Generator().manual_seed(SEED + 1))
    xm = x0.unsqueeze(0).repeat(4, 1, 1).to(DEV)
    areas = torch.from_numpy(m.face_areas()).float()
    crit = ga.EnsembleCRPSLoss(node_weights=areas).to(DEV)

    def run():
        model.zero_grad(set_to_none=True)
        st = noise.NoiseStream(17, DEV, draw=3)
        out = model(xm, graphs, noise=st)
        crit(out, y.to(DEV)).backward()
        return out.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}

    out, grads = run()
    assert float((out[0] - out[1]).abs().max()) > 1e-3 and float(out.std(0).mean()) > 0
    st = noise.NoiseStream(17, DEV, draw=3)
    z = noise.normal(st, 4, m.num_nodes, 16).double().cpu()
    sd = {k: v.detach().double().cpu().requires_grad_() for k, v in model.state_dict().items()}
    inp = NR.graph_inputs(m)
    pred = torch.stack([NR.forecaster_step_noisy(sd, x0.double(), *inp, 2, z=z[i]) for i in range(4)])
    reference(pred, y.double(), areas.double())[0].backward()
    for k, g in grads.items():
        assert rel_err(g, sd[k].grad) <= 1e-5, k
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_every_path_one_answer(ga):
    from gwen_amd import noise
    from gwen_amd.forecaster import GraphedStep, ensemble_forecast
    m = ga.geodesic_mesh(4)
    _, model = _models(ga, K=8, H=64, scale=0.5)
    model.eval()
    graphs = model.prepare(m, DEV)
    xm = torch.randn(3, m.faces.shape[0], 6, device=DEV)
    d, n = 21, 3
    want = []
    for i in range(3):
        st = noise.NoiseStream(SEED, DEV, draw=d)
        want.append(model.rollout(xm[i], graphs, n, noise=st, member0=i)[-1])
        assert st.draw == d + n
    want = torch.stack(want)
    assert float((want[0] - want[1]).abs().max()) > 0
    st = noise.NoiseStream(SEED, DEV, draw=d)
    got = model.rollout(xm[1], graphs, n, graphed=True, noise=st, member0=1)
    assert torch.equal(got[-1], want[1]) and st.draw == d + n
    st = noise.NoiseStream(SEED, DEV, draw=d)
    step = GraphedStep(model, graphs, xm[2], noise=st, member0=2)
    assert st.draw == d
    cur = xm[2]
    for _ in range(n):
        cur = step(cur)
    assert torch.equal(cur, want[2]) and st.draw == d + n
    for graphed in (False, True):
        for batched in (True, False):
            st = noise.NoiseStream(SEED, DEV, draw=d)
            got = ensemble_forecast(model, graphs, xm, n, 3, graphed=graphed, batched=batched, noise=st)
            assert torch.equal(got, want), (graphed, batched)
            assert st.draw == d + n, (graphed, batched)
    cache = {}                                                   # ONE stream: the second call replays the cached
    st = noise.NoiseStream(SEED, DEV, draw=d)                    # step, which reads the live draw
    assert torch.equal(ensemble_forecast(model, graphs, xm, n, 3, step_cache=cache, noise=st), want)
    assert st.draw == d + n and len(cache) == 1
    step = next(iter(cache.values()))
    later = ensemble_forecast(model, graphs, xm, n, 3, step_cache=cache, noise=st)
    assert st.draw == d + 2 * n and len(cache) == 1 and next(iter(cache.values())) is step
    assert not torch.equal(later, want)
    st2 = noise.NoiseStream(SEED, DEV, draw=d + n)
    assert torch.equal(later, ensemble_forecast(model, graphs, xm, n, 3, graphed=False, noise=st2))
    st.advance(-2 * n)                                           # rewound: the cached step gives the first answer again
    assert torch.equal(ensemble_forecast(model, graphs, xm, n, 3, step_cache=cache, noise=st), want)


def test_captured_training_step_draws_fresh_noise(ga):
    from gwen_amd import noise
    m = ga.geodesic_mesh(4, reorder="hilbert")
    _, model = _models(ga, K=16, H=32, scale=0.5)
    graphs = model.prepare(m, DEV)
    nf = m.faces.shape[0]
    xm = torch.randn(nf, 6, device=DEV).unsqueeze(0).repeat(4, 1, 1)
    y = torch.randn(nf, 6, device=DEV)
    crit = ga.EnsembleCRPSLoss(node_weights=m.face_areas()).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.0, fused=True, capturable=True)
    st = noise.NoiseStream(3, DEV)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(model(xm, graphs, noise=st), y)
        loss.backward()
        opt.step()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert st.draw == 3
    gph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(gph):
        loss = crit(model(xm, graphs, noise=st), y)
        loss.backward()
        opt.step()
    assert st.draw == 3                                          # capture runs nothing
    losses, draws = [], []
    for _ in range(4):
        draws.append(st.draw)
        gph.replay()
        torch.cuda.synchronize()
        losses.append(loss.detach().clone())
    assert st.draw == 7 and draws == [3, 4, 5, 6]
    assert len({float(v) for v in losses}) == 4
    for k, d in enumerate(draws):                                # (the forward of a training step, eagerly)
        eager = crit(model(xm, graphs, noise=noise.NoiseStream(3, DEV, draw=d)), y)
        assert torch.equal(eager.detach(), losses[k]), k


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import gwen_amd
        from gwen_amd import ensemble, noise
        from gwen_amd.forecaster import ensemble_forecast
        members = 5
        m = gwen_amd.geodesic_mesh(4)
        _, model = _models(gwen_amd, K=8, H=64, scale=0.5)
        model.eval()
        graphs = model.prepare(m, DEV)
        x0 = torch.randn(m.faces.shape[0], 6, generator=torch.Generator().manual_seed(SEED)).to(DEV)
        mine = ensemble.perturbed_members(x0, members, 0.1, 41)
        lo, hi = ensemble.member_range(members, rank, world)
        z = noise.normal(noise.NoiseStream(41, DEV), members, m.faces.shape[0], 6, tag=noise.TAG_INITIAL)
        all_x = x0.unsqueeze(0) + 0.1 * z
        ok_ic = torch.equal(ensemble.gather_members(mine, members), all_x) and torch.equal(mine, all_x[lo:hi])
        st = noise.NoiseStream(SEED, DEV, draw=2)
        got = ensemble_forecast(model, graphs, mine, 3, members, noise=st)
        st1 = noise.NoiseStream(SEED, DEV, draw=2)
        one = ensemble_forecast(model, graphs, all_x, 3, members, gather=False, member0=0, noise=st1)
        q.put((rank, bool(ok_ic), bool(torch.equal(got, one)), st.draw))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_forecast_and_perturbation_equal_one_process(ga):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    assert all(r[1] and r[2] and r[3] == 5 for r in res), res
