"""Static fields and forcings on the MI355X (csrc/forcing.hip through gwen_amd.forcings and the forecaster) against the
fp64 restatement of tests/forcing_ref.py: the solar vector, the clock, the fused embedding, shard invariance, the
forecaster's step, gradients and paths, and the combinations with noise and the transformer processor."""
import numpy as np
import pytest
import torch

import forcing_ref as FR
import noise_ref as NR
from ensemble_ref import reference
from helpers import SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0, DT = 772_416_000 + 5 * 3600, 21600            # 2024-06-23 05:00 UTC, 6 h steps


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def _points(n, seed=SEED):
    """n random (lat, lon) and the exact poles / date-line values"""
    g = np.random.default_rng(seed)
    ll = np.stack([g.uniform(-np.pi / 2, np.pi / 2, n), g.uniform(-np.pi, np.pi, n)], axis=1)
    edge = np.array([[p, l] for p in (np.pi / 2, -np.pi / 2, 0.0) for l in (-np.pi, 0.0, np.pi)])
    return np.concatenate([ll, edge])


# ---- 1. the solar vector ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 86399, -1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 12345, 10 ** 11 + 7])
def test_solar_vs_fp64(ga, t):
    """|got - want| <= 2^-23: values are <= 1.036, so a correctly rounded fp32 result is within 2^-24; one more ulp for a
    device / numpy libm difference that straddles a rounding boundary.  t >= 2^31 and t < 0 fail on a modulus taken
    after a conversion to float or as a truncating %."""
    from gwen_amd import forcings
    ll = _points(1000)
    ck = forcings.ForcingClock(t, 3600, DEV)
    got = forcings.solar(ck, torch.from_numpy(ll).to(DEV)).double().cpu().numpy()
    want = FR.solar(t, ll)
    err = np.abs(got - want).max(axis=0)
    print(f"solar t={t}: max abs err per channel {err} (bound {2.0 ** -23:.3e})")
    assert got.shape == (1009, 5) and err.max() <= 2.0 ** -23
    assert ck.time == t


# ---- 2. the clock -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [21600, 3600])
def test_clock_advances(ga, dt):
    import datetime
    from gwen_amd import forcings
    ck = forcings.ForcingClock(T0, dt, DEV)
    assert ck.time == T0 and ck.advance(3).time == T0 + 3 * dt and ck.advance(-3).time == T0
    assert ck.advance(-2).time == T0 - 2 * dt
    assert int(ck.snapshot()[1]) == dt and ga.ForcingClock is forcings.ForcingClock
    assert forcings.ForcingClock(datetime.datetime(2024, 6, 23, 5), dt, DEV).time == T0
    assert forcings.ForcingClock(np.datetime64("2024-06-23T05:00"), dt, DEV).time == T0
    assert forcings.ForcingClock(-5, dt, DEV).advance(1).time == dt - 5


def test_captured_solar_and_advance_see_the_time_of_every_replay(ga):
    from gwen_amd import forcings
    ll = _points(300)
    lld = torch.from_numpy(ll).to(DEV)
    ck = forcings.ForcingClock(T0, DT, DEV)
    forcings.solar(ck, lld)                                        # warm-up
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        s = forcings.solar(ck, lld)
        ck.advance(1)
    assert ck.time == T0                                           # capture runs nothing
    got = []
    for _ in range(3):
        gph.replay()
        torch.cuda.synchronize()
        got.append(s.double().cpu().numpy().copy())
    assert ck.time == T0 + 3 * DT
    for k in range(3):
        assert np.abs(got[k] - FR.solar(T0 + k * DT, ll)).max() <= 2.0 ** -23, k
    assert np.abs(got[0] - got[1]).max() > 0.1 and np.abs(got[1] - got[2]).max() > 0.1


# ---- 3. the fused embedding ---------------------------------------------------------------------------------------------
def _embed_case(H, width, nodes, members, seed, base=True, device_x=False):
    """(x, clock time or None, latlon, given, wf, base) of a case: solar first when the width has room for it"""
    g = torch.Generator().manual_seed(seed)
    sol = width in (5, 8)
    Fg = width - 5 * sol
    if device_x:
        x = torch.randn(members * nodes, H, generator=torch.Generator(DEV).manual_seed(seed), device=DEV)
    else:
        x = torch.randn(members * nodes, H, generator=g).to(DEV)
    ll = _points(nodes - 9, seed)
    given = torch.randn(nodes, Fg, generator=g).to(DEV) if Fg else None
    wf = (torch.randn(H, width, generator=g) * 0.3).to(DEV)
    b = torch.randn(nodes, H, generator=g).to(DEV) if base else None
    return x, sol, torch.from_numpy(ll).to(DEV), given, wf, b


def _embed_want(x, t, ll, given, wf, base, nodes):
    """fp64 on the device, from the restatement's solar vector"""
    parts = ([] if t is None else [torch.from_numpy(FR.solar(t, ll.cpu().numpy())).to(DEV)]) + \
        ([] if given is None else [given.double()])
    return FR.embed(x.double(), torch.cat(parts, dim=1), wf.double(), None if base is None else base.double(), nodes)


def _rel_dev(got, want) -> float:
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("H", [32, 64, 128, 256, 320, 512])      # (320, 512: two column blocks, the last partial)
@pytest.mark.parametrize("width", [5, 8, 1, 64])                 # solar only, solar + 3, given only (1 and 64)
def test_embed_vs_fp64(ga, H, width):
    from gwen_amd import forcings
    nodes, members = 37, 3
    for with_base in (True, False):
        x, sol, ll, given, wf, base = _embed_case(H, width, nodes, members, SEED + H + width, with_base)
        ck = forcings.ForcingClock(T0, DT, DEV) if sol else None
        want = _embed_want(x, T0 if sol else None, ll, given, wf, base, nodes)
        got = forcings.embed(x, ck, ll if sol else None, given, wf, base, nodes)
        err = _rel_dev(got, want)
        print(f"embed H={H} width={width} base={with_base}: rel err {err:.3e} (bound 1e-6)")
        assert err <= 1e-6
        assert torch.equal(got, forcings.embed(x, ck, ll if sol else None, given, wf, base, nodes))
        xi = x.clone()
        assert forcings.embed(xi, ck, ll if sol else None, given, wf, base, nodes, out=xi).data_ptr() == xi.data_ptr()
        assert torch.equal(xi, got)
        assert ck is None or ck.time == T0


@pytest.mark.parametrize("H", [32, 256])
def test_embed_many_rows(ga, H):
    """N = 100 002 x 3 members.  H = 32: 1 563 groups of 64 points; H = 256: 12 501 groups of 8 points on a grid capped
    at 8 192 waves, so that every wave takes a second group (the grid-stride loop) and the last group is partial."""
    from gwen_amd import forcings
    nodes, members = 100002, 3
    x, sol, ll, given, wf, base = _embed_case(H, 8, nodes, members, SEED + H, device_x=True)
    ck = forcings.ForcingClock(T0, DT, DEV)
    want = _embed_want(x, T0, ll, given, wf, base, nodes)
    got = forcings.embed(x, ck, ll, given, wf, base, nodes)
    assert _rel_dev(got, want) <= 1e-6
    assert _rel_dev(got[-nodes:], want[-nodes:]) <= 1e-6           # the last member, the last rows


def test_embed_rejects_what_the_kernel_cannot_take(ga):
    from gwen_amd import forcings
    x, sol, ll, given, wf, base = _embed_case(32, 8, 37, 3, SEED)
    ck = forcings.ForcingClock(T0, DT, DEV)
    with pytest.raises(ValueError):
        forcings.embed(x, ck, None, given, wf, base, 37)           # a clock without latlon
    with pytest.raises(ValueError):
        forcings.embed(x, ck, ll, given, wf, base, 36)             # rows % nodes
    with pytest.raises(ValueError):
        forcings.embed(x, None, None, given, wf, base, 37)         # wf has 8 columns for 3
    with pytest.raises(ValueError):
        forcings.embed(x, None, None, None, wf, base, 37)          # no forcing at all
    with pytest.raises(ValueError):
        forcings.embed(x, ck, ll.float(), given, wf, base, 37)     # latlon is float64
    with pytest.raises(RuntimeError):
        forcings.embed(x.cpu(), ck, ll, given, wf, base, 37)


# ---- 4. shard invariance ------------------------------------------------------------------------------------------------
def test_embed_is_shard_invariant(ga):
    """Members share forcings: there is no member0 here."""
    from gwen_amd import forcings
    nodes = 641
    x, sol, ll, given, wf, base = _embed_case(64, 8, nodes, 5, SEED)
    ck = forcings.ForcingClock(T0, DT, DEV)
    full = forcings.embed(x, ck, ll, given, wf, base, nodes)
    for m in range(5):
        one = forcings.embed(x[m * nodes:(m + 1) * nodes].contiguous(), ck, ll, given, wf, base, nodes)
        assert torch.equal(one, full[m * nodes:(m + 1) * nodes])
    tail = forcings.embed(x[3 * nodes:].contiguous(), ck, ll, given, wf, base, nodes)
    assert torch.equal(tail, full[3 * nodes:])


def test_embed_gradients_vs_fp64(ga):
    from gwen_amd import forcings
    nodes, members, H = 203, 3, 64
    x, sol, ll, given, wf, base = _embed_case(H, 8, nodes, members, SEED + 1)
    w = torch.randn(members * nodes, H, generator=torch.Generator().manual_seed(SEED)).to(DEV)
    xs, ws, bs = (t.clone().requires_grad_() for t in (x, wf, base))
    ck = forcings.ForcingClock(T0, DT, DEV)
    out = forcings.embed(xs, ck, ll, given, ws, bs, nodes)
    ck.advance(5)                                                  # the backward regenerates f from the saved time
    (out * w).sum().backward()
    xd, wd, bd = (t.double().clone().requires_grad_() for t in (x, wf, base))
    f = torch.cat([torch.from_numpy(FR.solar(T0, ll.cpu().numpy())).to(DEV), given.double()], dim=1)
    (FR.embed(xd, f, wd, bd, nodes) * w.double()).sum().backward()
    assert torch.equal(xs.grad, w)
    assert rel_err(ws.grad, wd.grad) <= 1e-5 and rel_err(bs.grad, bd.grad) <= 1e-6
    with pytest.raises(ValueError):
        forcings.embed(xs, ck, ll, given, ws, bs, nodes, out=torch.empty_like(x))


# ---- 5 - 9. the forecaster ----------------------------------------------------------------------------------------------
def _models(ga, S=3, solar=True, Fg=2, H=64, C=6, steps=2, precision="3xbf16", zero=False, **kw):
    """(the plain model, the same weights with static fields and forcings)"""
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(SEED)
    det = InteractionForecaster(C, H, steps, precision=precision, **kw)
    torch.manual_seed(SEED)
    forced = InteractionForecaster(C, H, steps, precision=precision, static_channels=S, solar=solar,
                                   forcing_channels=Fg, **kw)
    with torch.no_grad():
        for k, p in det.named_parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
                if k.endswith(("norm1.weight", "norm2.weight")):
                    p.add_(1.0)
        if kw.get("noise_channels"):
            det.noise_embed.weight.normal_(0, 0.3)
        extra = {k: v for k, v in forced.state_dict().items() if k.startswith(("static_embed", "forcing_embed"))}
        forced.load_state_dict({**det.state_dict(), **extra}, strict=True)
        if zero:
            for k in extra:
                getattr(forced, k.split(".")[0]).weight.zero_()
    return det.to(DEV), forced.to(DEV)


def _fields(n, S=3, Fg=2, steps=3, seed=SEED):
    g = torch.Generator().manual_seed(seed + 7)
    return torch.randn(n, S, generator=g), torch.randn(steps, n, Fg, generator=g)


def _f64(graphs, t, given):
    """[N, 5 + Fg] fp64 on the CPU: the restatement's solar vector at the graphs' own lat/lon, then the given columns"""
    ll = graphs.grid_latlon.cpu().numpy()
    return torch.cat([torch.from_numpy(FR.solar(t, ll)), given.double()], dim=1)


def _grid_inputs(ga, mesh, grid):
    """noise_ref.graph_inputs for given grid points: edge lists from the library, features over the unit vectors"""
    from gwen_amd.forecaster import edge_features
    g2m, m2g, _ = ga.grid_graphs(mesh, grid, DEV)
    a, b = g2m.cpu().numpy(), m2g.cpu().numpy()
    upos = ga.gridgraph.unit_vectors(grid)
    f = [torch.from_numpy(x).double() for x in (edge_features(upos, mesh.pos, a),
                                                 edge_features(mesh.pos, mesh.pos, mesh.edge_index),
                                                 edge_features(mesh.pos, upos, b))]
    return (torch.from_numpy(mesh.pos.astype(np.float32)).double(), torch.from_numpy(a),
            torch.from_numpy(mesh.edge_index), torch.from_numpy(b), *f)


@pytest.mark.parametrize("grid", ["faces", "latlon"])
@pytest.mark.parametrize("precision,tol", [("f16x3", 1e-6), ("3xbf16", 1e-4)])
def test_forced_step_vs_fp64(ga, precision, tol, grid):
    from gwen_amd import forcings
    m = ga.geodesic_mesh(5)
    _, model = _models(ga, precision=precision)
    if grid == "faces":
        n = m.faces.shape[0]
        static, given = _fields(n)
        graphs = model.prepare(m, DEV, grid_static=static)
        inp = NR.graph_inputs(m)
        cell = m.pos[m.faces].mean(axis=1)
        want_ll = FR.latlon_of(cell / np.linalg.norm(cell, axis=1, keepdims=True))
    else:
        pos = ga.latlon_grid(19, 36)[0]
        n = pos.shape[0]
        static, given = _fields(n)
        graphs = model.prepare(m, DEV, grid_pos=pos, grid_static=static)
        inp = _grid_inputs(ga, m, pos)
        want_ll = FR.latlon_of(ga.gridgraph.unit_vectors(pos))
        assert abs(want_ll[0, 0] + np.pi / 2) < 1e-12 and abs(want_ll[-1, 0] - np.pi / 2) < 1e-12       # the pole rows
    ll = graphs.grid_latlon
    assert ll.dtype == torch.float64 and tuple(ll.shape) == (n, 2) and tuple(graphs.grid_static.shape) == (n, 3)
    assert np.abs(ll.cpu().numpy() - want_ll).max() <= 1e-14
    gb = graphs.batched(2)
    assert gb.grid_latlon is graphs.grid_latlon and gb.grid_static is graphs.grid_static and gb.grid_nodes == n
    x0 = torch.randn(2, n, 6, generator=torch.Generator().manual_seed(SEED))
    ck = forcings.ForcingClock(T0, DT, DEV)
    with torch.no_grad():
        got = model(x0.to(DEV), graphs, clock=ck, forcing=given[0].to(DEV))
    assert ck.time == T0 + DT
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    f = _f64(graphs, T0, given[0])
    for i in range(2):
        want = FR.forecaster_step_forced(sd, x0[i].double(), *inp, 2, grid_static=static.double(), f=f)
        err = rel_err(got[i], want)
        print(f"forced step {grid} {precision} member {i}: rel err {err:.3e} (bound {tol:.0e})")
        assert err <= tol, i
    assert float(FR.forcing_term(sd, grid_static=static.double()).abs().max()) > 0.1      # neither term is negligible
    assert float(FR.forcing_term(sd, f=f).abs().max()) > 0.1
    plain = FR.forecaster_step_forced(sd, x0[0].double(), *inp, 2)
    assert rel_err(got[0], plain) > 10 * tol


def test_static_fields_alone(ga):
    """static_channels without forcings: the static fields are the kernel's given columns."""
    m = ga.geodesic_mesh(5)
    _, model = _models(ga, solar=False, Fg=0, precision="f16x3")
    n = m.faces.shape[0]
    static, _ = _fields(n)
    graphs = model.prepare(m, DEV, grid_static=static)
    x0 = torch.randn(n, 6, generator=torch.Generator().manual_seed(SEED))
    with torch.no_grad():
        got = model(x0.to(DEV), graphs)
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    assert "forcing_embed.weight" not in sd
    want = FR.forecaster_step_forced(sd, x0.double(), *NR.graph_inputs(m), 2, grid_static=static.double())
    assert rel_err(got, want) <= 1e-6


def test_missing_inputs_raise(ga):
    from gwen_amd import forcings
    m = ga.geodesic_mesh(4)
    _, model = _models(ga)
    n = m.faces.shape[0]
    static, given = _fields(n)
    x = torch.randn(n, 6, device=DEV)
    graphs, bare = model.prepare(m, DEV, grid_static=static), model.prepare(m, DEV)
    ck = forcings.ForcingClock(T0, DT, DEV)
    f = given[0].to(DEV)
    with torch.no_grad():
        with pytest.raises(ValueError, match="clock"):
            model(x, graphs, forcing=f)
        with pytest.raises(ValueError, match="forcing"):
            model(x, graphs, clock=ck)
        with pytest.raises(ValueError, match="forcing"):
            model(x, graphs, clock=ck, forcing=f[:, :1].contiguous())
        with pytest.raises(ValueError, match="grid_static"):
            model(x, bare, clock=ck, forcing=f)
        with pytest.raises(ValueError, match="n_steps"):
            model.rollout(x, graphs, 3, clock=ck, forcing=given[:2].to(DEV))
    with pytest.raises(ValueError):
        model.prepare(m, DEV, grid_static=static[:-1])
    assert ck.time == T0


def test_off_means_off(ga):
    from gwen_amd import forcings
    m = ga.geodesic_mesh(5)
    det, forced = _models(ga, zero=True)
    n = m.faces.shape[0]
    static, given = _fields(n)
    graphs = forced.prepare(m, DEV, grid_static=static)
    x = torch.randn(n, 6, device=DEV)
    ck = forcings.ForcingClock(T0, DT, DEV)
    gd = given.to(DEV)
    with torch.no_grad():
        assert torch.equal(forced(x, graphs, clock=ck, forcing=gd[0]), det(x, graphs))
    assert ck.time == T0 + DT
    ck = forcings.ForcingClock(T0, DT, DEV)
    a = forced.rollout(x, graphs, 3, clock=ck, forcing=gd)
    b = det.rollout(x, graphs, 3)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert ck.time == T0 + 3 * DT
    with torch.no_grad():                                          # a plain model given a clock: the step advances it
        assert torch.equal(det(x, graphs, clock=ck), det(x, graphs))
    assert ck.time == T0 + 4 * DT


def test_crps_gradients_with_forcings(ga):
    from gwen_amd import forcings
    m = ga.geodesic_mesh(4, reorder="hilbert")
    _, model = _models(ga, precision="f16x3")
    nf = m.faces.shape[0]
    static, given = _fields(nf)
    graphs = model.prepare(m, DEV, grid_static=static)
    g = torch.Generator().manual_seed(SEED)
    xm = torch.randn(4, nf, 6, generator=g)
    y = torch.randn(nf, 6, generator=g)
    areas = torch.from_numpy(m.face_areas()).float()
    crit = ga.EnsembleCRPSLoss(node_weights=areas).to(DEV)

    def run():
        model.zero_grad(set_to_none=True)
        ck = forcings.ForcingClock(T0, DT, DEV)
        out = model(xm.to(DEV), graphs, clock=ck, forcing=given[0].to(DEV))
        crit(out, y.to(DEV)).backward()
        assert ck.time == T0 + DT
        return out.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}

    out, grads = run()
    assert "static_embed.weight" in grads and "forcing_embed.weight" in grads
    sd = {k: v.detach().double().cpu().requires_grad_() for k, v in model.state_dict().items()}
    inp = NR.graph_inputs(m)
    f = _f64(graphs, T0, given[0])
    pred = torch.stack([FR.forecaster_step_forced(sd, xm[i].double(), *inp, 2, grid_static=static.double(), f=f)
                        for i in range(4)])
    reference(pred, y.double(), areas.double())[0].backward()
    for k, gr in grads.items():
        err = rel_err(gr, sd[k].grad)
        print(f"crps gradient {k}: rel err {err:.3e} (bound 1e-5)")
        assert err <= 1e-5, k
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_every_path_one_answer(ga):
    from gwen_amd import forcings
    from gwen_amd.forecaster import GraphedStep, ensemble_forecast
    m = ga.geodesic_mesh(4)
    _, model = _models(ga)
    model.eval()
    nf = m.faces.shape[0]
    static, given = _fields(nf, steps=6)
    graphs = model.prepare(m, DEV, grid_static=static)
    xm = torch.randn(3, nf, 6, device=DEV)
    n = 3
    F0, F1 = given[:3].to(DEV), given[3:].to(DEV)
    clock = lambda k=0: forcings.ForcingClock(T0 + k * DT, DT, DEV)                              # noqa: E731
    want = []
    for i in range(3):
        ck = clock()
        want.append(model.rollout(xm[i], graphs, n, clock=ck, forcing=F0)[-1])
        assert ck.time == T0 + n * DT
    want = torch.stack(want)
    still = model.rollout(xm[0], graphs, n, clock=clock(), forcing=F0[:1].repeat(3, 1, 1))[-1]
    assert not torch.equal(still, want[0])                         # (the given forcings of steps 1, 2 are there)
    late = model.rollout(xm[0], graphs, n, clock=clock(1), forcing=F0)[-1]
    assert not torch.equal(late, want[0])                          # (and the clock)
    ck = clock()
    got = model.rollout(xm[1], graphs, n, graphed=True, clock=ck, forcing=F0)
    assert torch.equal(got[-1], want[1]) and ck.time == T0 + n * DT
    ck = clock()
    step = GraphedStep(model, graphs, xm[2], clock=ck, forcing=F0[0])
    assert ck.time == T0
    cur = xm[2]
    for t in range(n):
        cur = step(cur, forcing=F0[t])
    assert torch.equal(cur, want[2]) and ck.time == T0 + n * DT
    for graphed in (False, True):
        for batched in (True, False):
            ck = clock()
            got = ensemble_forecast(model, graphs, xm, n, 3, graphed=graphed, batched=batched, clock=ck, forcing=F0)
            assert torch.equal(got, want), (graphed, batched)
            assert ck.time == T0 + n * DT, (graphed, batched)
    cache = {}                                                     # ONE clock: the second call replays the cached
    ck = clock()                                                   # step, which reads the live time
    assert torch.equal(ensemble_forecast(model, graphs, xm, n, 3, step_cache=cache, clock=ck, forcing=F0), want)
    assert ck.time == T0 + n * DT and len(cache) == 1
    step = next(iter(cache.values()))
    later = ensemble_forecast(model, graphs, xm, n, 3, step_cache=cache, clock=ck, forcing=F1)
    assert ck.time == T0 + 2 * n * DT and len(cache) == 1 and next(iter(cache.values())) is step
    assert not torch.equal(later, want)
    assert torch.equal(later, ensemble_forecast(model, graphs, xm, n, 3, graphed=False, clock=clock(n), forcing=F1))
    ck.advance(-2 * n)                                             # rewound: the cached step gives the first answer again
    assert torch.equal(ensemble_forecast(model, graphs, xm, n, 3, step_cache=cache, clock=ck, forcing=F0), want)


@pytest.mark.parametrize("precision,tol", [("f16x3", 1e-6), ("3xbf16", 1e-4)])
def test_forcings_with_noise(ga, precision, tol):
    from gwen_amd import forcings, noise
    m = ga.geodesic_mesh(5)
    _, model = _models(ga, precision=precision, noise_channels=16)
    n = m.faces.shape[0]
    static, given = _fields(n)
    graphs = model.prepare(m, DEV, grid_static=static)
    x0 = torch.randn(2, n, 6, generator=torch.Generator().manual_seed(SEED))
    st = noise.NoiseStream(5, DEV, draw=9)
    z = noise.normal(st, 2, m.num_nodes, 16, member0=4).double().cpu()
    ck = forcings.ForcingClock(T0, DT, DEV)
    with torch.no_grad():
        got = model(x0.to(DEV), graphs, noise=st, member0=4, clock=ck, forcing=given[0].to(DEV))
    assert st.draw == 10 and ck.time == T0 + DT
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    f = _f64(graphs, T0, given[0])
    inp = NR.graph_inputs(m)
    for i in range(2):
        want = FR.forecaster_step_forced(sd, x0[i].double(), *inp, 2, grid_static=static.double(), f=f, z=z[i])
        assert rel_err(got[i], want) <= tol, i


@pytest.mark.parametrize("precision,tol", [("f16x3", 1e-6), ("3xbf16", 1e-4)])
def test_forcings_with_the_transformer_processor(ga, precision, tol):
    from gwen_amd import forcings
    m = ga.geodesic_mesh(5)
    _, model = _models(ga, precision=precision, processor="transformer", heads=4)
    n = m.faces.shape[0]
    static, given = _fields(n)
    graphs = model.prepare(m, DEV, grid_static=static)
    x0 = torch.randn(2, n, 6, generator=torch.Generator().manual_seed(SEED))
    ck = forcings.ForcingClock(T0, DT, DEV)
    with torch.no_grad():
        got = model(x0.to(DEV), graphs, clock=ck, forcing=given[0].to(DEV))
    assert ck.time == T0 + DT
    sd = {k: v.double().cpu() for k, v in model.state_dict().items()}
    f = _f64(graphs, T0, given[0])
    inp = NR.graph_inputs(m)
    for i in range(2):
        want = FR.forecaster_step_forced(sd, x0[i].double(), *inp, 2, grid_static=static.double(), f=f, heads=4)
        assert rel_err(got[i], want) <= tol, i
    ck = forcings.ForcingClock(T0, DT, DEV)                        # the captured step, transformer blocks inside
    a = model.rollout(x0[0].to(DEV), graphs, 2, clock=ck, forcing=given[:2].to(DEV))
    ck = forcings.ForcingClock(T0, DT, DEV)
    b = model.rollout(x0[0].to(DEV), graphs, 2, graphed=True, clock=ck, forcing=given[:2].to(DEV))
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and ck.time == T0 + 2 * DT
