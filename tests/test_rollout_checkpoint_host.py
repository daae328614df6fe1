"""gwen_amd.checkpoint on the CPU: ``checkpointed_step`` against the plain chain of ``_step`` calls, over a small
pure-torch fp64 model with the forecaster's protocol (``_static`` / ``_step``) and duck-typed stream and clock objects
(``state``, ``snapshot()``, ``advance()``; the real NoiseStream and ForcingClock live on the device only)."""
import pytest
import torch
from torch import nn

from gwen_amd.checkpoint import checkpointed_step, flatten_static, restore_static
from helpers import SEED, rel_err

N, C, H, FG, BLOCKS = 11, 3, 8, 2, 2
DRAW0, T0, DT = 5, 1000, 60


class Stream:
    """{seed, draw} as the NoiseStream keeps them; ``advance`` moves the draw in place."""

    def __init__(self, seed, draw):
        self.state = torch.tensor([seed, draw], dtype=torch.int64)

    def snapshot(self):
        return self.state.clone()

    def advance(self, n=1):
        self.state[1] += n
        return self


class Clock:
    """{t, dt} as the ForcingClock keeps them."""

    def __init__(self, t, dt):
        self.state = torch.tensor([t, dt], dtype=torch.int64)

    def snapshot(self):
        return self.state.clone()

    def advance(self, n=1):
        self.state[0] += n * self.state[1]
        return self


class Graphs:
    def __init__(self, gen):
        self.pos = torch.randn(N, 3, dtype=torch.float64, generator=gen)


class Toy(nn.Module):
    """x' = x + readout(blocks(tanh(embed(x) + vm + noise + solar + forcing))): every ingredient of the real step --
    static embeddings with a nested list, a draw-dependent and a time-dependent term, a per-step forcing -- and a log of
    what every ``_step`` call saw."""

    def __init__(self):
        super().__init__()
        self.embed = nn.Linear(C, H)
        self.mesh_embed = nn.Linear(3, H)
        self.edge_terms = nn.ModuleList([nn.Linear(3, H) for _ in range(BLOCKS)])
        self.blocks = nn.ModuleList([nn.Linear(H, H) for _ in range(BLOCKS)])
        self.noise_embed = nn.Linear(4, H, bias=False)
        self.time_embed = nn.Linear(2, H, bias=False)
        self.forcing_embed = nn.Linear(FG, H, bias=False)
        self.readout = nn.Linear(H, C)
        self.unused = nn.Parameter(torch.ones(2))                   # takes part in nothing
        self.calls = []                                             # (grad enabled, draw, time, forcing[0, 0]) per _step

    def _static(self, graphs):
        return (self.mesh_embed(graphs.pos), [lin(graphs.pos) for lin in self.edge_terms])

    def _step(self, x, graphs, static, noise=None, member0=0, clock=None, forcing=None):
        vm, ees = static
        self.calls.append((torch.is_grad_enabled(), None if noise is None else int(noise.state[1]),
                           None if clock is None else int(clock.state[0]),
                           None if forcing is None else float(forcing[0, 0])))
        h = self.embed(x) + vm
        if clock is not None:
            t = clock.state[0].double() / 977.0
            h = h + self.time_embed(torch.stack([torch.sin(t), torch.cos(t)]))
            clock.advance(1)
        if noise is not None:
            k = torch.arange(N * 4, dtype=torch.float64).view(N, 4)
            z = torch.sin(k * 1.7 + noise.state[1].double() * 0.37 + member0 + noise.state[0].double())
            h = h + self.noise_embed(z)
            noise.advance(1)
        if forcing is not None:
            h = h + self.forcing_embed(forcing)
        h = torch.tanh(h)
        for lin, ee in zip(self.blocks, ees):
            h = h + torch.tanh(lin(h) * ee)
        return x + self.readout(h)


def _setup(frozen=()):
    torch.manual_seed(SEED)
    model = Toy().double()
    for name in frozen:
        model.get_parameter(name).requires_grad_(False)
    gen = torch.Generator().manual_seed(SEED + 1)
    graphs = Graphs(gen)
    x0 = torch.randn(N, C, dtype=torch.float64, generator=gen)
    forcing = torch.randn(8, N, FG, dtype=torch.float64, generator=gen)
    targets = torch.randn(8, N, C, dtype=torch.float64, generator=gen)
    return model, graphs, x0, forcing, targets


def _chain(model, graphs, x0, forcing, T, ckpt, noise, clock):
    static = model._static(graphs)
    states, cur = [], x0
    for t in range(T):
        kw = dict(noise=noise, member0=2, clock=clock, forcing=forcing[t])
        cur = checkpointed_step(model, cur, graphs, static, **kw) if ckpt else model._step(cur, graphs, static, **kw)
        states.append(cur)
    return states


def _loss(states, targets):
    """a term on every state, weighted by lead time"""
    return sum((t + 1.0) * (s - targets[t]).square().mean() for t, s in enumerate(states))


def _run(T, ckpt, frozen=(), x_grad=True):
    model, graphs, x0, forcing, targets = _setup(frozen)
    x0.requires_grad_(x_grad)
    noise, clock = Stream(9, DRAW0), Clock(T0, DT)
    states = _chain(model, graphs, x0, forcing, T, ckpt, noise, clock)
    _loss(states, targets).backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    grads["x0"] = x0.grad
    return [s.detach() for s in states], grads, model, noise, clock, forcing


def test_gradients_match_the_plain_chain():
    """T = 4: the states are the plain chain's bits; every gradient within 1e-12 relative (fp64 rounding with four
    orders of headroom: the state gradient at a step boundary is summed in another association)."""
    sp, gp, *_ = _run(4, False)
    sc, gc, *_ = _run(4, True)
    assert all(torch.equal(a, b) for a, b in zip(sp, sc))
    assert gp["unused"] is None and gc["unused"] is None
    worst = 0.0
    for k, want in gp.items():
        if want is None:
            continue
        assert gc[k] is not None and float(want.abs().max()) > 0, k
        err = rel_err(gc[k], want)
        worst = max(worst, err)
        assert err <= 1e-12, (k, err)
    print(f"T=4 fp64: max rel err of any gradient against the plain chain {worst:.3e} (bound 1e-12)")


def test_one_step_is_bitwise_the_plain_chain():
    sp, gp, *_ = _run(1, False)
    sc, gc, *_ = _run(1, True)
    assert torch.equal(sp[0], sc[0])
    for k, want in gp.items():
        assert (want is None and gc[k] is None) or torch.equal(gc[k], want), k


def test_call_pattern():
    """T calls without grad (the forward sweep), then T with grad (the recomputes); the plain chain: T with grad."""
    T = 3
    *_, model, _, _, _ = _run(T, True)
    assert [c[0] for c in model.calls] == [False] * T + [True] * T
    *_, model, _, _, _ = _run(T, False)
    assert [c[0] for c in model.calls] == [True] * T


def test_recompute_sees_its_own_step_and_leaves_the_live_state():
    T = 4
    model, graphs, x0, forcing, targets = _setup()
    x0.requires_grad_()
    noise, clock = Stream(9, DRAW0), Clock(T0, DT)
    states = _chain(model, graphs, x0, forcing, T, True, noise, clock)
    assert int(noise.state[1]) == DRAW0 + T and int(clock.state[0]) == T0 + T * DT and int(noise.state[0]) == 9
    _loss(states, targets).backward()
    assert int(noise.state[1]) == DRAW0 + T and int(clock.state[0]) == T0 + T * DT and int(clock.state[1]) == DT
    sweep, again = model.calls[:T], model.calls[T:]
    assert [c[1:] for c in sweep] == [(DRAW0 + t, T0 + t * DT, float(forcing[t, 0, 0])) for t in range(T)]
    assert [c[1:] for c in again] == [c[1:] for c in reversed(sweep)]          # the backward walks the steps in reverse


def test_two_backwards_over_a_retained_graph():
    """the snapshots are not consumed: the second recompute draws what the first drew"""
    model, graphs, x0, forcing, targets = _setup()
    x0.requires_grad_()
    noise, clock = Stream(9, DRAW0), Clock(T0, DT)
    loss = _loss(_chain(model, graphs, x0, forcing, 3, True, noise, clock), targets)
    leaves = [x0] + [p for p in model.parameters()]
    first = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    second = torch.autograd.grad(loss, leaves, allow_unused=True)
    assert len(model.calls) == 9
    assert [c[1:] for c in model.calls[3:6]] == [c[1:] for c in model.calls[6:]]
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b)
    assert int(noise.state[1]) == DRAW0 + 3 and int(clock.state[0]) == T0 + 3 * DT


def test_nested_static_round_trips():
    a, b, c, d = (torch.full((2,), float(i)) for i in range(4))
    static = (a, [b, c], d, [])
    flat, layout = flatten_static(static)
    assert [t.data_ptr() for t in flat] == [t.data_ptr() for t in (a, b, c, d)] and layout == (-1, 2, -1, 0)
    back = restore_static(flat, layout)
    assert isinstance(back, tuple) and len(back) == 4 and back[0] is a and back[2] is d
    assert isinstance(back[1], list) and back[1][0] is b and back[1][1] is c and back[3] == []
    with pytest.raises(ValueError):
        restore_static(flat[:-1], layout)
    with pytest.raises(TypeError):
        flatten_static((a, "b"))
    # and through the step: the gradient reaches the parameters behind the list
    _, gc, *_ = _run(2, True)
    assert all(float(gc[f"edge_terms.{k}.weight"].abs().max()) > 0 for k in range(BLOCKS))


def test_frozen_inputs_get_no_gradient():
    frozen = ("blocks.0.weight", "mesh_embed.weight", "mesh_embed.bias", "readout.bias")
    _, gp, *_ = _run(3, False, frozen, x_grad=False)
    _, gc, *_ = _run(3, True, frozen, x_grad=False)
    assert gc["x0"] is None and all(gc[k] is None for k in frozen)
    for k, want in gp.items():
        if want is None:
            assert gc[k] is None, k
        else:
            assert rel_err(gc[k], want) <= 1e-12, k
    # nothing requires grad at all: the step runs as it is and returns a plain tensor
    model, graphs, x0, forcing, _ = _setup([k for k, _ in Toy().named_parameters()])
    y = checkpointed_step(model, x0, graphs, model._static(graphs), forcing=forcing[0])
    assert not y.requires_grad and len(model.calls) == 1
