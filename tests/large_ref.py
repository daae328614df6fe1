"""Helpers of tests/test_gpu_address_range.py: tensors past 4 GiB that never leave the device.

A big input is a block of ``P`` random rows repeated (``P`` odd, ``P * F * 4`` no divisor of 2^32) plus a ragged tail, so
that a row-independent kernel must write a P-periodic output: the first block is checked against an fp64 reference on
the CPU, every later block bitwise against the first, on the device and in chunks.  An address that wraps at 2^32 bytes
or 2^31 elements lands on another phase of the period (or on memory that is still NaN) and shows."""
from __future__ import annotations

import gc

import torch

P = 1007                       # rows per repeated block: odd, and 1007 = 19 * 53 shares no factor with 2^32
BYTES32 = 1 << 32              # the 32-bit byte-offset boundary
ELEMS31 = 1 << 31              # the int32 element-index boundary
MEM_CAP = 48 << 30             # no test may hold more device memory than this at its peak
HOST_CAP = 64 << 20            # ... nor copy a tensor larger than this to the host


_held = 0                      # bytes other tests' fixtures (or a failed test's traceback) hold when a test starts


def start(dev) -> None:
    global _held
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    _held = torch.cuda.memory_allocated(dev)


def finish(dev, what: str) -> None:
    """End of a test (its tensors deleted by the caller): give the memory back, print and bound the test's own peak."""
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    peak = torch.cuda.max_memory_allocated(dev)
    print(f"{what}: peak device memory {peak / 2 ** 30:.2f} GiB ({_held / 2 ** 30:.2f} GiB held before the test)")
    assert peak - _held <= MEM_CAP, (what, peak, _held)


def host(t: torch.Tensor) -> torch.Tensor:
    """A device tensor on the CPU in fp64 -- small ones only."""
    assert t.numel() * t.element_size() <= HOST_CAP, tuple(t.shape)
    return t.detach().double().cpu()


def periodic(base: torch.Tensor, rows: int) -> torch.Tensor:
    """[rows, ...] on base's device: ``base`` ([p, ...]) repeated along dim 0, the last repeat cut short."""
    p = base.size(0)
    out = torch.empty(rows, *base.shape[1:], dtype=base.dtype, device=base.device)
    full = rows // p
    if full:
        out[:full * p].view(full, p, *base.shape[1:]).copy_(base.unsqueeze(0).expand(full, *base.shape))
    if rows - full * p:
        out[full * p:].copy_(base[:rows - full * p])
    return out


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_periodic(t: torch.Tensor, p: int, what: str, chunk_blocks: int = 256) -> None:
    """Rows k p .. k p + p - 1 of ``t`` are bitwise rows 0 .. p - 1 for every k (NaN included: bits, not values), the
    ragged tail likewise; compared on the device, ``chunk_blocks`` blocks at a time."""
    t = _bits(t.detach())
    rows = t.size(0)
    first = t[:p].unsqueeze(0)
    full = rows // p
    for k0 in range(1, full, chunk_blocks):
        k1 = min(full, k0 + chunk_blocks)
        same = (t[k0 * p:k1 * p].view(k1 - k0, p, *t.shape[1:]) == first).flatten(1).all(1)
        if not bool(same.all()):
            bad = k0 + int((~same).nonzero()[0])
            row = bad * p + int((t[bad * p:(bad + 1) * p] != t[:p]).flatten(1).any(1).nonzero()[0])
            raise AssertionError(f"{what}: row {row} (block {bad} of period {p}) differs from row {row % p}")
    tail = rows - full * p
    if full and tail:
        assert torch.equal(t[full * p:], t[:tail]), f"{what}: the ragged tail (rows {full * p} ..) differs"


def assert_members_cycle(t: torch.Tensor, bases, what: str) -> None:
    """t [members, ...]: member k is bitwise ``bases[k % len(bases)]``."""
    for k in range(t.size(0)):
        assert torch.equal(_bits(t[k]), _bits(bases[k % len(bases)])), f"{what}: member {k} differs from its base"


def nan_blocks(dev, *shapes) -> set:
    """Method 4: allocate one fp32 block per shape, fill it with NaN and free it again -- the caching allocator hands
    the same blocks to the launch that follows, so a row the kernel leaves unwritten reads NaN instead of an earlier
    (correct) result.  Returns the blocks' addresses for ``assert_fresh``."""
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    blocks = [torch.full(tuple(s), float("nan"), dtype=torch.float32, device=dev) for s in shapes]
    ptrs = {b.data_ptr() for b in blocks}
    del blocks
    return ptrs


def assert_fresh(ptrs: set, *outs) -> None:
    for o in outs:
        assert o.data_ptr() in ptrs, "the output did not land in a NaN-filled block: the test cannot see unwritten rows"


def nan_tensor(dev, *shape) -> torch.Tensor:
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def all_nan(t: torch.Tensor) -> bool:
    return bool(torch.isnan(t).all())


def rel(got: torch.Tensor, want: torch.Tensor) -> float:
    """helpers.rel_err's measure (max |got - want| / max |want|) for SMALL tensors: moved to the CPU in fp64."""
    got, want = host(got), host(want)
    scale = float(want.abs().max()) if want.numel() else 0.0
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0) if want.numel() else 0.0


def per_row(got: torch.Tensor, want: torch.Tensor) -> float:
    """test_gpu_f16x3's per-row measure: the largest row error relative to the row's own largest |value|."""
    got, want = host(got), host(want)
    diff = (got - want).abs().flatten(1).amax(1)
    scale = want.abs().flatten(1).amax(1)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return float((diff / scale).max())


def act64(name: str, v: torch.Tensor) -> torch.Tensor:
    return {"none": lambda t: t, "relu": torch.relu, "silu": torch.nn.functional.silu}[name](v)


def mlp2_want(a, w1, w2, b2, tab=None, idx=None, b1=None, res=None, act="silu") -> torch.Tensor:
    """K6 on the CPU in fp64: (res +) act(a W1^T + tab[idx] + b1) W2^T + b2."""
    d = lambda t: host(t)                                                               # noqa: E731
    pre = d(a) @ d(w1).t()
    if tab is not None:
        pre = pre + d(tab)[idx.cpu().long()]
    if b1 is not None:
        pre = pre + d(b1)
    y = act64(act, pre) @ d(w2).t()
    if b2 is not None:
        y = y + d(b2)
    return y if res is None else d(res) + y


def layer_norm_want(x, gamma, beta, eps, res=None) -> torch.Tensor:
    x = host(x)
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps) * host(gamma) + host(beta)
    return y if res is None else host(res) + y


def ring_edges(n: int, dev) -> torch.Tensor:
    """int64 [2, 4 n] on the device: node i receives from i - 2, i - 1, i + 1, i + 2 (mod n) -- bounded degree and, in
    its own order, at most 68 distinct sources per 64 consecutive rows, so the graph tiles for K8."""
    i = torch.arange(n, dtype=torch.int64, device=dev)
    src = torch.cat([(i + d) % n for d in (-2, -1, 1, 2)])
    return torch.stack([src, i.repeat(4)])


def ring_conv_want(x_rows, deg_inv, w, b, relu: bool) -> torch.Tensor:
    """GCNConv on the ring for a few target rows: ``x_rows`` [k, 5, Fin] holds, per target, rows i - 2 .. i + 2 of x
    (the self-loop in the middle); every node has degree 5, so every normalised weight is ``deg_inv`` = 1 / 5."""
    y = (host(x_rows).sum(1) * deg_inv) @ host(w).t() + host(b)
    return torch.relu(y) if relu else y


# ---- fp64 references evaluated ON THE DEVICE (mesh-sized bases: too large for the host cap above) -----------------------

def rel_dev(got: torch.Tensor, want: torch.Tensor) -> float:
    """``rel`` without leaving the device."""
    want = want.detach().double()
    scale = float(want.abs().max())
    return float((got.detach().double() - want).abs().max()) / (scale if scale > 0 else 1.0)


def per_row_dev(got: torch.Tensor, want: torch.Tensor) -> float:
    """``per_row`` without leaving the device."""
    want = want.detach().double()
    diff = (got.detach().double() - want).abs().flatten(1).amax(1)
    scale = want.abs().flatten(1).amax(1)
    return float((diff / torch.where(scale > 0, scale, torch.ones_like(scale))).max())


def _ln64(m, gamma, beta, eps):
    mu = m.mean(1, keepdim=True)
    return (m - mu) / torch.sqrt(((m - mu) ** 2).mean(1, keepdim=True) + eps) * gamma + beta


def interaction_want(sd: dict, x: torch.Tensor, e: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, act: str,
                     mean: bool, eps: float = 1e-5):
    """The InteractionNet block of oracle/interaction_oracle.py restated for fp64 tensors on any device, edges in the
    graph's stored order (``src`` / ``dst`` int64), square graph: (x', e', agg).  ``sd``: the block's state_dict in fp64
    (with ``edge_norm.*`` / ``node_norm.*`` when it has LayerNorm).  Differentiable."""
    n = x.size(0)
    h = torch.cat([e, x[src], x[dst]], dim=1) @ sd["edge_mlp.0.weight"].t() + sd["edge_mlp.0.bias"]
    m = act64(act, h) @ sd["edge_mlp.2.weight"].t() + sd["edge_mlp.2.bias"]
    if "edge_norm.weight" in sd:
        m = _ln64(m, sd["edge_norm.weight"], sd["edge_norm.bias"], eps)
    agg = torch.zeros(n, m.size(1), dtype=m.dtype, device=m.device).index_add(0, dst, m)
    if mean:
        deg = torch.zeros(n, dtype=m.dtype, device=m.device).index_add(0, dst, torch.ones_like(dst, dtype=m.dtype))
        agg = agg / deg.clamp(min=1).view(-1, 1)
    h = torch.cat([x, agg], dim=1) @ sd["node_mlp.0.weight"].t() + sd["node_mlp.0.bias"]
    y = act64(act, h) @ sd["node_mlp.2.weight"].t() + sd["node_mlp.2.bias"]
    if "node_norm.weight" in sd:
        y = _ln64(y, sd["node_norm.weight"], sd["node_norm.bias"], eps)
    return x + y, e + m, agg


def gcn_want(g, x: torch.Tensor, w: torch.Tensor, b, relu: bool) -> torch.Tensor:
    """act((A~ x) W^T + b) in fp64 on the device over the prepared graph's own CSR (rowptr, col, val), x [N_src, Fin]."""
    nnz = int(g.rowptr[-1])
    rows = torch.repeat_interleave(torch.arange(g.num_nodes, device=x.device),
                                   (g.rowptr[1:] - g.rowptr[:-1]).long())
    col, val = g.col[:nnz].long(), g.val[:nnz].double()
    agg = torch.zeros(g.num_nodes, x.size(1), dtype=torch.float64, device=x.device)
    agg.index_add_(0, rows, x.double()[col] * val.view(-1, 1))
    y = agg @ w.double().t()
    if b is not None:
        y = y + b.double()
    return torch.relu(y) if relu else y
