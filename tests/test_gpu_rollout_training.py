"""Training through rollouts on the MI355X: ``InteractionForecaster.rollout(grad=True)`` -- the checkpointed chain
(gwen_amd/checkpoint.py) against the plain chain of ``_step`` calls under autograd, against the fp64 oracle, its memory,
a short training run and its misuse.  Geodesic mesh nu = 4 (162 nodes, 320 faces), 6 channels, 2 processor blocks and
3 steps unless a test says otherwise."""
import gc
import json

import numpy as np
import pytest
import torch

import noise_ref as NR
from helpers import REL_TOL, SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, BLOCKS, T = 6, 2, 3
T0, DT = 772_416_000 + 5 * 3600, 21600            # 2024-06-23 05:00 UTC, 6 h steps


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


@pytest.fixture(scope="module")
def mesh4(ga):
    return ga.geodesic_mesh(4)


def _model(ga, hidden, **kw):
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(SEED)
    model = InteractionForecaster(C, hidden, BLOCKS, **kw)
    with torch.no_grad():
        if kw.get("noise_channels"):
            model.noise_embed.weight.normal_(0, 0.3)
    return model.to(DEV)


def _inputs(n, members, steps=T):
    g = torch.Generator().manual_seed(SEED + 3)
    shape = (n, C) if members == 1 else (members, n, C)
    x0 = torch.randn(*shape, generator=g).to(DEV)
    w = [torch.randn(*shape, generator=g).to(DEV) * (t + 1) for t in range(steps)]      # weighted by lead time
    return x0, w


def _plain_chain(model, x0, graphs, steps, **kw):
    """the hand-written chain: the static embeddings once, then ``_step`` under grad"""
    batched = x0.dim() == 3
    gb = graphs.batched(x0.size(0)) if batched else graphs
    static = model._static(gb)
    states, cur = [], x0.reshape(-1, x0.size(-1)) if batched else x0
    forcing = kw.pop("forcing", None)
    for t in range(steps):
        cur = model._step(cur, gb, static, **kw, **({} if forcing is None else {"forcing": forcing[t]}))
        states.append(cur.view_as(x0) if batched else cur)
    return states


def _grads(model, x0, states, w):
    model.zero_grad(set_to_none=True)
    x0.grad = None
    sum((s * wt).sum() for s, wt in zip(states, w)).backward()
    out = {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
    out["x0"] = x0.grad.clone()
    return out


def _worst(got, want, label):
    errs = {}
    for k, g in want.items():
        assert (g is None) == (got[k] is None), k
        if g is not None:
            errs[k] = rel_err(got[k], g)
    k = max(errs, key=errs.get)
    print(f"{label}: max rel err over {len(errs)} gradients {errs[k]:.3e} at {k}")
    return errs


# ---- 1. states and gradients against the plain chain ----------------------------------------------------------------
CASES = [(64, "interaction", False, 1), (32, "interaction", True, 3), (64, "transformer", False, 2)]


def _case(ga, mesh4, hidden, processor, layer_norm, members):
    extra = {"heads": 4} if processor == "transformer" else {}
    model = _model(ga, hidden, processor=processor, layer_norm=layer_norm, **extra)
    graphs = model.prepare(mesh4, DEV)
    x0, w = _inputs(mesh4.faces.shape[0], members)
    return model, graphs, x0.requires_grad_(), w


@pytest.mark.parametrize("hidden,processor,layer_norm,members", CASES)
def test_checkpointed_rollout_vs_plain_chain(ga, mesh4, hidden, processor, layer_norm, members):
    """(64, interaction, no LayerNorm) takes the fused edge backward, (32, LayerNorm) the general walk, the third the
    attention blocks with their per-block static edge terms.  States: bitwise the plain chain's.  Gradients: within
    REL_TOL of the plain chain's (for T >= 2 the state gradient at a step boundary is summed in another association, so
    not bitwise in general), bitwise reproducible, and bitwise the plain chain's at T = 1."""
    model, graphs, x0, w = _case(ga, mesh4, hidden, processor, layer_norm, members)
    plain = _plain_chain(model, x0, graphs, T)
    gp = _grads(model, x0, plain, w)
    ckpt = model.rollout(x0, graphs, T, grad=True)
    assert len(ckpt) == T and all(s.shape == x0.shape and s.requires_grad for s in ckpt)
    gc_ = _grads(model, x0, ckpt, w)
    unchk = model.rollout(x0, graphs, T, grad=True, checkpoint=False)
    for t in range(T):
        assert torch.equal(ckpt[t], plain[t]) and torch.equal(unchk[t], plain[t]), t
    errs = _worst(gc_, gp, f"T={T} H={hidden} {processor} ln={layer_norm} members={members}")
    for k, e in errs.items():
        assert e <= REL_TOL, (k, e)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in gc_.values())
    gu = _grads(model, x0, unchk, w)                                 # checkpoint=False IS the hand-written chain
    assert all(torch.equal(gu[k], gp[k]) for k in gp)
    again = _grads(model, x0, model.rollout(x0, graphs, T, grad=True), w)
    assert all(torch.equal(again[k], gc_[k]) for k in gc_)
    one_p = _grads(model, x0, _plain_chain(model, x0, graphs, 1), w[:1])
    one_c = _grads(model, x0, model.rollout(x0, graphs, 1, grad=True), w[:1])
    assert all(torch.equal(one_c[k], one_p[k]) for k in one_p)


@pytest.mark.parametrize("hidden,processor,layer_norm,members", CASES)
def test_checkpointed_states_are_the_no_grad_rollouts(ga, mesh4, hidden, processor, layer_norm, members):
    """The states of ``rollout(grad=True)`` are bitwise those of the no-grad ``rollout`` (run over the batched graphs:
    it takes [N, C] only), and so are the plain chain's: ``_step`` calls the same launchers with and without gradients
    (the transformer's feed-forward half included: ``attention._FeedForwardFunction``)."""
    model, graphs, x0, _ = _case(ga, mesh4, hidden, processor, layer_norm, members)
    ckpt = model.rollout(x0, graphs, T, grad=True)
    plain = _plain_chain(model, x0, graphs, T)
    nograd = model.rollout(x0.detach().reshape(-1, C), graphs.batched(members), T)
    assert len(nograd) == T and not any(s.requires_grad for s in nograd)
    diff = max(rel_err(a.detach().reshape(-1, C), b) for a, b in zip(ckpt, nograd))
    diff_plain = max(rel_err(a.detach().reshape(-1, C), b) for a, b in zip(plain, nograd))
    print(json.dumps({"test": "rollout_training_vs_no_grad_rollout", "hidden": hidden, "processor": processor,
                      "layer_norm": layer_norm, "members": members, "max_rel_diff_ckpt": diff,
                      "max_rel_diff_plain_chain": diff_plain}))
    for t in range(T):
        assert torch.equal(ckpt[t].detach().reshape(-1, C), nograd[t]), t
        assert torch.equal(plain[t].detach().reshape(-1, C), nograd[t]), t


# ---- 2. everything on -----------------------------------------------------------------------------------------------
def test_noise_static_fields_and_forcings(ga, mesh4):
    from gwen_amd import forcings, noise
    members, draw0 = 3, 7
    model = _model(ga, 64, noise_channels=16, static_channels=3, solar=True, forcing_channels=2)
    n = mesh4.faces.shape[0]
    g = torch.Generator().manual_seed(SEED + 7)
    static, given = torch.randn(n, 3, generator=g), torch.randn(T, n, 2, generator=g).to(DEV)
    graphs = model.prepare(mesh4, DEV, grid_static=static)
    x0, w = _inputs(n, members)
    x0.requires_grad_()
    st, ck = noise.NoiseStream(17, DEV, draw=draw0), forcings.ForcingClock(T0, DT, DEV)
    plain = _plain_chain(model, x0, graphs, T, noise=st, member0=2, clock=ck, forcing=given)
    gp = _grads(model, x0, plain, w)
    st, ck = noise.NoiseStream(17, DEV, draw=draw0), forcings.ForcingClock(T0, DT, DEV)
    ckpt = model.rollout(x0, graphs, T, noise=st, member0=2, clock=ck, forcing=given, grad=True)
    assert st.draw == draw0 + T and ck.time == T0 + T * DT
    gc_ = _grads(model, x0, ckpt, w)
    assert st.draw == draw0 + T and ck.time == T0 + T * DT           # the backward leaves them there
    assert all(torch.equal(a, b) for a, b in zip(ckpt, plain))
    assert float((ckpt[0][0] - ckpt[0][1]).detach().abs().max()) > 1e-3       # (the members got different noise)
    errs = _worst(gc_, gp, "T=3 noise + static + solar + forcing, 3 members")
    for k in ("noise_embed.weight", "static_embed.weight", "forcing_embed.weight"):
        assert float(gp[k].abs().max()) > 0 and float(gc_[k].abs().max()) > 0, k
    for k, e in errs.items():
        assert e <= REL_TOL, (k, e)
    st2, ck2 = noise.NoiseStream(17, DEV, draw=draw0 + 1), forcings.ForcingClock(T0 + DT, DT, DEV)
    other = model.rollout(x0, graphs, 1, noise=st2, member0=2, clock=ck2, forcing=given[:1], grad=True)
    assert not torch.equal(other[0], ckpt[0])                        # (the draw and the time do enter the step)


# ---- 3. against the fp64 oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["3xbf16", "f16x3"])
def test_two_step_gradients_vs_fp64_oracle(ga, mesh4, precision):
    """err = the largest rel_err of any parameter gradient against fp64 autograd of the oracle's step chained twice.
    The plain chain is the yardstick: err_ckpt <= 1.5 err_plain + 1e-7 (the factor: the other summation order; the
    floor: about one fp32 ulp at the tensor's scale)."""
    from oracle import interaction_oracle as IO
    model = _model(ga, 64, precision=precision)
    graphs = model.prepare(mesh4, DEV)
    x0, w = _inputs(mesh4.faces.shape[0], 1, steps=2)
    sd = {k: v.detach().double().cpu().requires_grad_() for k, v in model.state_dict().items()}
    inp = NR.graph_inputs(mesh4)
    x1 = IO.forecaster_step(sd, x0.double().cpu(), *inp, BLOCKS)
    x2 = IO.forecaster_step(sd, x1, *inp, BLOCKS)
    ((x1 * w[0].double().cpu()).sum() + (x2 * w[1].double().cpu()).sum()).backward()
    x0.requires_grad_()
    plain = _plain_chain(model, x0, graphs, 2)
    assert rel_err(plain[1], x2.detach()) <= REL_TOL
    gp = _grads(model, x0, plain, w)
    gc_ = _grads(model, x0, model.rollout(x0, graphs, 2, grad=True), w)
    err_plain = max(rel_err(gp[k], v.grad) for k, v in sd.items())
    err_ckpt = max(rel_err(gc_[k], v.grad) for k, v in sd.items())
    print(json.dumps({"test": "rollout_training_vs_fp64", "precision": precision, "T": 2, "err_plain": err_plain,
                      "err_ckpt": err_ckpt}))
    assert err_ckpt <= 1.5 * err_plain + 1e-7


# ---- 4. memory ------------------------------------------------------------------------------------------------------
def test_memory_grows_by_states_only(ga):
    """nu = 8 (642 nodes, 1 280 faces, 3 840 mesh edges), hidden 64, one member, MSE on every state.  Delta(T) = the peak
    of max_memory_allocated over forward and backward above memory_allocated just before.  The checkpointed chain may
    grow by 8 state-sized allocations per extra step (the output, the loss residual, gradients, rounding); the plain
    chain must grow by more than that, or the yardstick measures nothing (predicted from the sizes: 2 processor blocks
    x 0.98 MB of saved edge state per step alone)."""
    m = ga.geodesic_mesh(8)
    model = _model(ga, 64)
    graphs = model.prepare(m, DEV)
    n = m.faces.shape[0]
    g = torch.Generator().manual_seed(SEED)
    x0, y = torch.randn(n, C, generator=g).to(DEV), torch.randn(n, C, generator=g).to(DEV)
    s = x0.numel() * x0.element_size()
    assert s == 30720 and graphs.mesh.num_edges == 3840

    def delta(steps, checkpoint):
        model.zero_grad(set_to_none=True)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        states = model.rollout(x0, graphs, steps, grad=True, checkpoint=checkpoint)
        sum((st - y).square().mean() for st in states).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    for checkpoint in (True, False):                                 # (the caches a first call fills stay out of it)
        delta(2, checkpoint)
    d = {(steps, c): delta(steps, c) for c in (True, False) for steps in (2, 8)}
    allowance = 6 * 8 * s
    grow_ckpt, grow_plain = d[8, True] - d[2, True], d[8, False] - d[2, False]
    print(json.dumps({"test": "rollout_training_memory", "state_bytes": s, "allowance": allowance,
                      "delta_ckpt_2": d[2, True], "delta_ckpt_8": d[8, True], "delta_plain_2": d[2, False],
                      "delta_plain_8": d[8, False], "growth_ckpt": grow_ckpt, "growth_plain": grow_plain}))
    assert grow_ckpt <= allowance
    assert grow_plain > allowance


# ---- 5. it trains ---------------------------------------------------------------------------------------------------
def test_crps_fine_tune_over_lead_times(ga, mesh4):
    from gwen_amd import noise
    members = 3
    model = _model(ga, 32, noise_channels=16)
    graphs = model.prepare(mesh4, DEV)
    n = mesh4.faces.shape[0]
    g = torch.Generator().manual_seed(SEED + 11)
    x0 = torch.randn(n, C, generator=g).unsqueeze(0).repeat(members, 1, 1).to(DEV)
    ys = torch.randn(T, n, C, generator=g).to(DEV)
    crit = ga.EnsembleCRPSLoss(node_weights=torch.from_numpy(mesh4.face_areas()).float()).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        st = noise.NoiseStream(17, DEV, draw=3)                      # the same draw: a deterministic objective
        states = model.rollout(x0, graphs, T, noise=st, grad=True)
        loss = sum(crit(s, ys[t]) for t, s in enumerate(states))
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    print("3-step CRPS fine-tune, loss per iteration:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0]


# ---- 6. misuse ------------------------------------------------------------------------------------------------------
def test_misuse(ga, mesh4):
    model = _model(ga, 32)
    graphs = model.prepare(mesh4, DEV)
    x0, _ = _inputs(mesh4.faces.shape[0], 1)
    with pytest.raises(ValueError, match="graphed"):
        model.rollout(x0, graphs, 2, graphed=True, grad=True)
    states = model.rollout(x0, graphs, 2, grad=True)
    states[0].add_(1.0)                                              # the next step saved it as its input
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        sum(s.sum() for s in states).backward()
