"""Every kernel past 4 GiB and at its 32-bit offset limits.

The kernels mix address widths by hand (int64 row offsets, uint32 byte offsets inside a pass or into a gathered table)
and hand-placed guards decide which path runs; the rest of the suite stops at 0.6 GB per tensor.  Here every launch gets
a tensor that really crosses 2^32 bytes (and, where named, 2^31 elements) -- asserted before the launch -- and the big
tensors never leave the device (tests/large_ref.py):
  * row-independent launches: a block of P = 1007 rows repeated; the first block against an fp64 reference on the CPU,
    every later block bitwise against the first;
  * graph launches: three random base members cycled over the members axis / the block-diagonal graph; member k bitwise
    the single-member launch of base k mod 3, each base against an fp64 reference;
  * reductions over the whole tensor: against the fp64 combination of per-block results;
  * the memory an output will occupy is NaN before the first big launch (an unwritten row cannot pass), the big launch
    is checked on its FIRST run, the determinism re-run comes after, and the inputs are compared with their copies.
Tolerances are the project's own: 1e-4 ("3xbf16"), 2e-6 forward / 1e-5 gradients (the fp32-class tiers).

What a dropped cast trips (each mutant was compiled for gfx950 in a scratch copy; a wrapped WRITE offset leaves its buffer,
so those two were traced by reading and never run):
  * csrc/interact.hip, ``pass_off = (int64_t)cur.w0 * F`` as a 32-bit product: negative from element 2^31 on, i.e. from
    row 16 777 216 at 128 channels and 67 108 864 at 32 -- those rows of ``out`` are written elsewhere and stay NaN, and
    ``assert_periodic(out, ..)`` of test_k6_row_mlp_past_4gib[128-..] / [32-..] fails at exactly that row (hence row
    counts past 2^31 elements at every width but 64; interact_rows.hip has the same product, caught at 256 channels);
  * csrc/wide.hip, ``out + (int64_t)m * mstride_o`` as a 32-bit product: 44 members of [100 002, 256] are 1.13e9
    elements and still fit, so test_k8_wide_layer_over_members also runs 88 -- members 84 .. 87 then stay NaN and
    ``assert_members_cycle(out, singles, ..)`` fails with "member 84 differs from its base";
  * csrc/wide.hip, the member offset of the READS (``x + (int64_t)m * mstride_x``, both sites) cut to 32 bits of bytes stays
    inside x and was run: test_k8_wide_layer_over_members[256-44-f16x3] fails in ``assert_members_cycle`` at member 42,
    the first whose offset passes 2^32 bytes."""
import numpy as np
import pytest
import torch

import large_ref as L
from helpers import REL_TOL, SEED, make_params
from large_ref import BYTES32, ELEMS31, P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL32 = 2e-6                   # the fp32-class tiers, forward
GRAD_TOL32 = 1e-5              # ... and their gradients
FWD_TOL = {"3xbf16": REL_TOL, "f16x3": TOL32, "bf16x6": TOL32}
GRAD_TOL = {"3xbf16": REL_TOL, "f16x3": GRAD_TOL32, "bf16x6": GRAD_TOL32, None: GRAD_TOL32, "fp32": GRAD_TOL32}


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


@pytest.fixture(scope="module")
def mesh100(ga):
    """nu = 100 in hilbert order (100 002 nodes, 600 000 edges): the mesh, its edge_index on the device, the K6 edge
    graph and the prepared GCN graph."""
    from gwen_amd.interaction import interaction_graph
    m = ga.geodesic_mesh(100, reorder="hilbert")
    ei = torch.from_numpy(m.edge_index).to(DEV)
    eg = interaction_graph(ei, m.num_nodes, m.num_nodes)
    g = ga.prepare_graph(ei, m.num_nodes)
    assert (m.num_nodes, eg.num_edges) == (100002, 600000)
    return m, ei, eg, g


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(SEED + seed)).to(DEV)


def _err(contract, got, want):
    """the tier's own measure: per row for the fp32-class tiers (rows differ in scale), the tensor's scale for 3xbf16"""
    return L.rel(got, want) if contract == "3xbf16" else L.per_row(got, want)


# ---- cases 1-3: K6 as a row MLP ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("contract", ["3xbf16", "f16x3"])
@pytest.mark.parametrize("F,R,elems31", [(256, 8_500_003, True), (64, 17_000_003, False), (128, 17_000_003, True),
                                         (32, 68_000_003, True)])
def test_k6_row_mlp_past_4gib(ga, F, R, elems31, contract):
    """Cases 1-3.  out = a + act(a W1^T + tab[idx] + b1) W2^T + b2 with res = a, b1 and one indexed table, on the
    row-stationary kernel (256 and 64 channels) and the ``launch_tiles`` kernel (128 and 32): A and out cross 2^32 bytes
    (at 256, 128 and 32 channels also 2^31 elements: the pass offset ``(int64_t)w0 * F`` of either kernel is the product
    that would wrap there), the row count ends ragged against the 64- and 128-row passes."""
    from gwen_amd.interaction import mlp2
    L.start(DEV)
    assert R * F * 4 > BYTES32 and (not elems31 or R * F > ELEMS31) and BYTES32 % (P * F * 4) != 0
    base = _randn(P, F, seed=F)
    w1, w2 = _randn(F, F, seed=1) / F ** 0.5, _randn(F, F, seed=2) / F ** 0.5
    b1, b2, tab = _randn(F, seed=3), _randn(F, seed=4), _randn(777, F, seed=5)
    a = L.periodic(base, R)
    idx = ((torch.arange(R, device=DEV) % P) * 13 % 777).to(torch.int32)
    ptrs = L.nan_blocks(DEV, (R, F))
    out, agg = mlp2(a, w1, w2, b2, g1=tab, idx1=idx, b1=b1, res=a, contract=contract)
    L.assert_fresh(ptrs, out)
    assert agg is None
    want = L.mlp2_want(base, w1, w2, b2, tab, idx[:P], b1, base)
    err = _err(contract, out[:P], want)
    print(f"K6 rows F={F} {contract}: first block err {err:.2e}")
    assert err <= FWD_TOL[contract]
    L.assert_periodic(out, P, f"K6 rows F={F} {contract}")
    assert torch.equal(a[:P], base)
    L.assert_periodic(a, P, "K6's input A")
    again, _ = mlp2(a, w1, w2, b2, g1=tab, idx1=idx, b1=b1, res=a, contract=contract)
    assert torch.equal(out, again)
    del a, idx, out, again
    L.finish(DEV, f"K6 rows F={F} {contract}")


# ---- cases 7-8: K3 on both sides of its 4 GiB switch ------------------------------------------------------------------

@pytest.mark.parametrize("contract", ["3xbf16", "bf16x6"])
@pytest.mark.parametrize("fin,fout,rows,big_in", [(256, 256, 4_400_007, True), (64, 256, 16_700_000, False)])
def test_k3_linear_either_side_of_4gib_input(ga, fin, fout, rows, big_in, contract):
    """Case 7: 256 -> 256 on 4 400 007 rows -- the input is past 4 GiB, so the tall-input route is left for
    k_linear_split.  Case 8: 64 -> 256 on 16 700 000 rows -- the input stays just under 4 GiB, K8's pipeline runs and
    writes a 17 GB output, past 2^32 bytes and 2^31 elements."""
    from gwen_amd import ops
    L.start(DEV)
    if big_in:
        assert rows * fin * 4 > BYTES32
    else:
        assert rows * fin * 4 < BYTES32 and rows * fout * 4 > 3 * BYTES32 and rows * fout > ELEMS31
    base = _randn(P, fin, seed=fin + fout)
    w, b = (t.to(DEV) for t in make_params(fin, fout))
    x = L.periodic(base, rows)
    ptrs = L.nan_blocks(DEV, (rows, fout))
    out = ops.linear(x, w, b, relu=True, contract=contract)
    L.assert_fresh(ptrs, out)
    want = torch.relu(L.host(base) @ L.host(w).t() + L.host(b))
    err = _err(contract, out[:P], want)
    print(f"K3 {fin}->{fout} {contract}: first block err {err:.2e}")
    assert err <= FWD_TOL[contract]
    L.assert_periodic(out, P, f"K3 {fin}->{fout} {contract}")
    assert torch.equal(x[:P], base)
    L.assert_periodic(x, P, "K3's input")
    again = ops.linear(x, w, b, relu=True, contract=contract)
    assert torch.equal(out, again)
    del x, out, again
    L.finish(DEV, f"K3 {fin}->{fout} {contract}")


# ---- case 6 (row half): LayerNorm forward and backward ----------------------------------------------------------------

def test_layer_norm_rows_past_4gib(ga):
    """Case 6, ``ops.layer_norm`` on [17 000 003, 64] (4.35 GB): the forward (with a residual) per block against the fp64
    reference, the backward's g_x likewise, gamma / beta gradients against the fp64 sum of per-block gradients."""
    from gwen_amd import ops
    L.start(DEV)
    rows, F, eps = 17_000_003, 64, 1e-5
    assert rows * F * 4 > BYTES32
    bx, br, bg = _randn(P, F, seed=61) * 3 + 1, _randn(P, F, seed=62), _randn(P, F, seed=63)
    gamma, beta = _randn(F, seed=64), _randn(F, seed=65)
    x, res = L.periodic(bx, rows), L.periodic(br, rows)
    ptrs = L.nan_blocks(DEV, (rows, F))
    out = ops.layer_norm(x, gamma, beta, eps, res)
    L.assert_fresh(ptrs, out)
    assert L.per_row(out[:P], L.layer_norm_want(bx, gamma, beta, eps, br)) <= TOL32
    L.assert_periodic(out, P, "layer_norm forward")
    assert torch.equal(out, ops.layer_norm(x, gamma, beta, eps, res))
    del out, res
    # backward: fp64 autograd of the reference on one block; the parameter gradients add up over blocks
    g = L.periodic(bg, rows)
    x64, gam64, bet64 = (L.host(t).requires_grad_() for t in (bx, gamma, beta))
    mu = x64.mean(1, keepdim=True)
    y = (x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + eps) * gam64 + bet64
    full, tail = divmod(rows, P)
    gw_b, gb_b, gx_b = torch.autograd.grad((y * L.host(bg)).sum(), (gam64, bet64, x64), retain_graph=True)
    gw_t, gb_t = torch.autograd.grad((y * L.host(bg))[:tail].sum(), (gam64, bet64))
    ptrs = L.nan_blocks(DEV, (rows, F))
    gx, gp = ops.layer_norm_backward(x, g, gamma, eps)
    L.assert_fresh(ptrs, gx)
    assert L.per_row(gx[:P], gx_b) <= GRAD_TOL32
    L.assert_periodic(gx, P, "layer_norm backward g_x")
    want = torch.cat([full * gw_b + gw_t, full * gb_b + gb_t])
    err = L.rel(gp[:F], want[:F]), L.rel(gp[F:], want[F:])
    print(f"layer_norm gamma / beta gradients over {rows} rows: err {err[0]:.2e} / {err[1]:.2e}")
    assert max(err) <= GRAD_TOL32
    gx2, gp2 = ops.layer_norm_backward(x, g, gamma, eps)
    assert torch.equal(gx, gx2) and torch.equal(gp, gp2)
    assert torch.equal(x[:P], bx) and torch.equal(g[:P], bg)
    del x, g, gx, gx2
    L.finish(DEV, "layer_norm rows")


# ---- case 16: noise ---------------------------------------------------------------------------------------------------

def _z_rows(seed, tag, draw, member, node0, count, K):
    """[count, K] fp64: z(seed, tag, draw, member, node0 + i, k) from the numpy Philox oracle"""
    import noise_ref as NR
    nb = (K + 7) // 8
    z = np.stack([NR.box_muller(NR.philox_blocks(seed, tag, node0, count, member, draw, b)) for b in range(nb)], axis=1)
    return torch.from_numpy(z.reshape(count, nb * 8)[:, :K])


def test_noise_past_4gib(ga):
    """Case 16.  ``gwen_noise_normal_f32`` on [44, 100 002, 256] and ``NoiseStream`` injection into [44 * 100 002, 256]
    (4.5 GB each): the counter-based generator makes every row checkable alone -- the rows either side of byte 2^32, the
    first and the last row against tests/noise_ref.py (4e-6 absolute for z, 1e-6 of the scale for the injected rows: the
    bounds of test_gpu_noise.py), and the whole tensor bitwise against two launches of half the members each."""
    from gwen_amd import noise
    L.start(DEV)
    seed, draw, members, nodes, K = 20240607, 3, 44, 100002, 256
    assert members * nodes * K * 4 > BYTES32
    st = noise.NoiseStream(seed, DEV, draw)
    ptrs = L.nan_blocks(DEV, (members, nodes, K))
    z = noise.normal(st, members, nodes, K, member0=5)
    L.assert_fresh(ptrs, z)
    flat = z.view(-1, K)
    r32 = BYTES32 // (K * 4)
    for r in (0, r32 - 1, r32, r32 + 1, members * nodes - 1):
        m, n = divmod(r, nodes)
        want = _z_rows(seed, noise.TAG_LATENT, draw, 5 + m, n, 1, K)
        assert float((L.host(flat[r:r + 1]) - want).abs().max()) <= 4e-6, r
    half = members // 2
    assert torch.equal(z[:half], noise.normal(st, half, nodes, K, member0=5))
    assert torch.equal(z[half:], noise.normal(st, members - half, nodes, K, member0=5 + half))
    assert not bool(torch.isnan(z).any())
    del z, flat
    # injection: out = x + z Wz^T, row r = node r % nodes of member member0 + r // nodes
    H, Kz = 256, 32
    rows = members * nodes
    assert rows * H * 4 > BYTES32
    wz = _randn(H, Kz, seed=71)
    bx = _randn(P, H, seed=72)
    x = L.periodic(bx, rows)
    ptrs = L.nan_blocks(DEV, (rows, H))
    out = noise.inject(x, wz, st, nodes, member0=2)
    L.assert_fresh(ptrs, out)
    r32 = BYTES32 // (H * 4)
    for r in (0, r32 - 1, r32, r32 + 1, rows - 1):
        m, n = divmod(r, nodes)
        want = L.host(x[r:r + 1]) + _z_rows(seed, noise.TAG_LATENT, draw, 2 + m, n, 1, Kz) @ L.host(wz).t()
        assert L.rel(out[r:r + 1], want) <= 1e-6, r
    cut = half * nodes
    assert torch.equal(out[:cut], noise.inject(x[:cut], wz, st, nodes, member0=2))
    assert torch.equal(out[cut:], noise.inject(x[cut:], wz, st, nodes, member0=2 + half))
    assert not bool(torch.isnan(out).any())
    assert torch.equal(x[:P], bx)
    L.assert_periodic(x, P, "the injection's input")
    del x, out
    L.finish(DEV, "noise")


# ---- case 14: CRPS ----------------------------------------------------------------------------------------------------

def test_crps_and_scores_at_the_bench_shape(ga):
    """Case 14: M = 32, N = 200 000, C = 256 (tools/ensemble_bench.py's shape, 6.5 GB per tensor).  Every member is a block
    of P nodes repeated, node weights likewise: the loss and the scores against the fp64 combination of the launches on
    one block and on the tail (themselves against tests/ensemble_ref.py in fp64), the gradient's first block against the
    fp64 reference and every later block bitwise against the first -- which covers the nodes either side of byte 2^32
    (member 20), compared once more by value below."""
    import ensemble_ref as ER
    from gwen_amd import losses
    L.start(DEV)
    M, N, C, alpha = 32, 200_000, 256, 1.0
    assert M * N * C * 4 > BYTES32
    full, tail = divmod(N, P)
    base = _randn(M, P, C, seed=81)
    tb = _randn(P, C, seed=82)
    wb = torch.rand(P, generator=torch.Generator().manual_seed(SEED)).to(DEV) + 0.5
    v = torch.rand(C, generator=torch.Generator().manual_seed(SEED + 1)).to(DEV) + 0.5
    pred = torch.empty(M, N, C, dtype=torch.float32, device=DEV)
    for m in range(M):
        pred[m] = L.periodic(base[m], N)
    target, w = L.periodic(tb, N), L.periodic(wb, N)
    # the small launches, checked against the fp64 reference (evaluated on the device: 32 x 32 pairs per point)
    parts = []
    for n in (P, tail):
        x64 = base[:, :n].double().requires_grad_()
        want_loss, want_sc = ER.reference(x64, tb[:n].double(), wb[:n], v, alpha)
        (want_g,) = torch.autograd.grad(want_loss, x64)
        xs = base[:, :n].clone().requires_grad_()
        got = losses.ensemble_crps(xs, tb[:n].contiguous(), wb[:n].contiguous(), v, alpha)
        got.backward()
        sc = losses.ensemble_scores(base[:, :n].contiguous(), tb[:n].contiguous(), wb[:n].contiguous(), alpha)
        assert L.rel(got.detach().view(1), want_loss.detach().view(1)) <= 1e-5
        assert L.rel(xs.grad, want_g) <= 2e-6
        assert L.rel(sc["crps"], want_sc[0].detach()) <= 1e-5
        sw = float(wb[:n].double().sum())
        parts.append((sw, float(got.detach().double()) * sw, sc["crps"].double() * sw, sc["rmse"].double() ** 2 * sw,
                      sc["spread"].double() ** 2 * sw, want_g * sw))
    (sw_b, l_b, c_b, r_b, s_b, g_b), (sw_t, l_t, c_t, r_t, s_t, _) = parts
    sw = full * sw_b + sw_t
    pred.requires_grad_()
    ptrs = L.nan_blocks(DEV, (M, N, C), (M, N, C))          # the kernel's gradient and its product with the upstream factor
    loss = losses.ensemble_crps(pred, target, w, v, alpha)
    loss.backward()
    grad = pred.grad
    L.assert_fresh(ptrs, grad)
    err = abs(float(loss.detach().double()) - (full * l_b + l_t) / sw) / ((full * l_b + l_t) / sw)
    print(f"CRPS loss at [{M}, {N}, {C}]: err {err:.2e}")
    assert err <= 1e-5
    assert L.rel(grad[:, :P], g_b / sw) <= 2e-6
    for m in range(M):
        L.assert_periodic(grad[m], P, f"CRPS gradient, member {m}")
    m32, n32 = divmod(BYTES32 // 4, N * C)
    n32 //= C
    for n in (n32 - 1, n32, n32 + 1):
        assert L.rel(grad[m32, n:n + 1], (g_b / sw)[m32, n % P:n % P + 1]) <= 2e-6, n
    with torch.no_grad():
        sc = losses.ensemble_scores(pred.detach(), target, w, alpha)
    assert L.rel(sc["crps"], (full * c_b + c_t) / sw) <= 1e-5
    assert L.rel(sc["rmse"], ((full * r_b + r_t) / sw).sqrt()) <= 1e-5
    assert L.rel(sc["spread"], ((full * s_b + s_t) / sw).sqrt()) <= 1e-5
    first = grad.clone()
    pred.grad = None
    loss2 = losses.ensemble_crps(pred, target, w, v, alpha)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(first, pred.grad)
    assert torch.equal(pred.detach()[:, :P], base) and torch.equal(target[:P], tb)
    del pred, grad, first, target, w, loss, loss2
    L.finish(DEV, "CRPS")


# ---- case 15: masked_l1 -----------------------------------------------------------------------------------------------

def test_masked_l1_past_2_31_elements(ga):
    """Case 15: [43, 200 000, 256] = 2.2e9 elements per tensor.  Three base members cycled, each a block of P nodes
    repeated, the mask likewise: the value against the fp64 combination of the launches on one member's block and tail
    (themselves against the plain formula in fp64), the gradient sign(o - t) mask / count exactly."""
    from gwen_amd.models_gnn import loss_func
    L.start(DEV)
    members, N, C = 43, 200_000, 256
    assert members * N * C > ELEMS31
    full, tail = divmod(N, P)
    bo, bt = _randn(3, P, C, seed=91), _randn(3, P, C, seed=92)
    mb = (torch.rand(P, generator=torch.Generator().manual_seed(SEED)) < 0.6).to(DEV)
    out = torch.empty(members, N, C, dtype=torch.float32, device=DEV)
    tgt = torch.empty(members, N, C, dtype=torch.float32, device=DEV)
    for k in range(members):
        out[k], tgt[k] = L.periodic(bo[k % 3], N), L.periodic(bt[k % 3], N)
    mask = L.periodic(mb, N)
    sums = []
    for b in range(3):
        per = []
        for n in (P, tail):
            got = loss_func(bo[b:b + 1, :n].contiguous(), bt[b:b + 1, :n].contiguous(), mb[:n].contiguous())
            cnt = int(mb[:n].sum()) * C
            want = float(((bo[b, :n] - bt[b, :n]).double().abs() * mb[:n].double().view(-1, 1)).sum()) / cnt
            assert abs(float(got) - want) <= 1e-6 * want
            per.append(float(got.detach().double()) * cnt)
        sums.append(full * per[0] + per[1])
    count = members * (full * int(mb.sum()) + int(mb[:tail].sum())) * C
    want = sum(sums[k % 3] for k in range(members)) / count
    out.requires_grad_()
    ptrs = L.nan_blocks(DEV, (members, N, C), (members, N, C))      # the kernel's gradient and its upstream product
    loss = loss_func(out, tgt, mask)
    loss.backward()
    L.assert_fresh(ptrs, out.grad)
    err = abs(float(loss.detach().double()) - want) / want
    print(f"masked_l1 over {members * N * C} elements: err {err:.2e}")
    assert err <= 1e-6                                  # (test_gpu_parity.py's bound for the value)
    for b in range(3):
        wg = torch.sign(bo[b] - bt[b]).double() * mb.double().view(-1, 1) / count
        assert torch.allclose(L.host(out.grad[b, :P]), L.host(wg), rtol=1e-6, atol=0)
        L.assert_periodic(out.grad[b], P, f"masked_l1 gradient, member {b}")
    L.assert_members_cycle(out.grad, [out.grad[0], out.grad[1], out.grad[2]], "masked_l1 gradient")
    assert torch.equal(out.detach()[:3, :P], bo) and torch.equal(tgt[:3, :P], bt)
    del out, tgt, mask, loss
    L.finish(DEV, "masked_l1")


# ---- case 17: weight and bias gradients -------------------------------------------------------------------------------

def test_grad_batch_past_4gib(ga):
    """Case 17: ``GradBatch`` on [8 500 003, 256] rows (g and x 8.7 GB each, past 2^31 elements) on every contraction,
    the weight + bias launch and the bias reduction alone: against the fp64 sum of per-block gradients, full *
    (g_b^T x_b) + the tail's, evaluated on the CPU from one block."""
    from gwen_amd import ops
    L.start(DEV)
    rows, F = 8_500_003, 256
    assert rows * F * 4 > BYTES32 and rows * F > ELEMS31
    full, tail = divmod(rows, P)
    bg, bx = _randn(P, F, seed=101), _randn(P, F, seed=102) + 0.25
    g, x = L.periodic(bg, rows), L.periodic(bx, rows)
    g64, x64 = L.host(bg), L.host(bx)
    want_w = full * (g64.t() @ x64) + g64[:tail].t() @ x64[:tail]
    want_b = full * g64.sum(0) + g64[:tail].sum(0)
    for contract in (None, "3xbf16", "bf16x6", "f16x3"):
        small = ops.grad_weight(bg, bx, contract)
        assert L.rel(small, g64.t() @ x64) <= GRAD_TOL[contract], contract
        gb = ops.GradBatch()
        gw = gb.grad_weight(g, x, contract)
        gw2, gbias = gb.grad_weight_bias(g, x, contract)
        gb1 = gb.grad_bias(g)
        gb.finish()
        err = [L.rel(gw, want_w), L.rel(gw2, want_w), L.rel(gbias, want_b), L.rel(gb1, want_b)]
        print(f"GradBatch {contract}: err weight {err[0]:.2e} / {err[1]:.2e}, bias {err[2]:.2e} / {err[3]:.2e}")
        assert max(err) <= GRAD_TOL[contract], contract
        gb = ops.GradBatch()
        again = gb.grad_weight(g, x, contract), *gb.grad_weight_bias(g, x, contract), gb.grad_bias(g)
        gb.finish()
        assert all(torch.equal(a, b) for a, b in zip(again, (gw, gw2, gbias, gb1)))
        for t in (small, gw, gw2, gbias, gb1, *again):      # a recycled block must not hand the next contraction a result
            t.fill_(float("nan"))
        del small, gw, gw2, gbias, gb1, again
    assert torch.equal(g[:P], bg) and torch.equal(x[:P], bx)
    L.assert_periodic(g, P, "GradBatch's g")
    L.assert_periodic(x, P, "GradBatch's x")
    del g, x
    L.finish(DEV, "GradBatch")


# ---- graph launches: three base members cycled over the block-diagonal graph / the members axis ------------------------

def _net(F, aggr, prec, seed, layer_norm=False):
    from gwen_amd.interaction import InteractionNet
    torch.manual_seed(SEED + seed)
    net = InteractionNet(F, "silu", aggr, precision=prec, layer_norm=layer_norm)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "norm.weight" in name:
                p.normal_(1.0, 0.1)
            elif p.dim() == 1:
                p.normal_(0, 0.1)
    return net.to(DEV)


def _cycled(bases, members):
    return torch.cat([bases[k % len(bases)] for k in range(members)], 0)


def _block_forward_case(net, eg, members, prec, what):
    """One InteractionNet block on ``members`` block-diagonal copies of the mesh: x', e' and the aggregate of member k
    bitwise the single-member launch of base k mod 3, every base against the fp64 reference at the tier's tolerance, the
    outputs in NaN-filled memory on the first run, a second run bitwise equal, the inputs unchanged."""
    F, N, E = net.channels, eg.num_dst, eg.num_edges
    assert members * E * F * 4 > BYTES32
    gb = eg.batched(members)
    xb = [_randn(N, F, seed=40 + k) for k in range(3)]
    eb = [_randn(E, F, seed=50 + k) for k in range(3)]
    x, e = _cycled(xb, members), _cycled(eb, members)
    from gwen_amd import interaction as I
    shapes = [(members * E, F), (members * N, F), (members * N, F), (members * N, 3 * F)]
    if net.layer_norm and I._LN_FORCE_UNFUSED:              # K6 writes the messages, the row kernel e' / x'
        shapes += [(members * E, F), (members * N, F)]
    ptrs = L.nan_blocks(DEV, *shapes)
    with torch.no_grad():
        x1, e1, agg, _, _ = net._forward_k6(x, x, e, gb, return_agg=True)
    L.assert_fresh(ptrs, x1, e1, agg)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    singles = []
    for k in range(3):
        with torch.no_grad():
            xs, es, ags, _, _ = net._forward_k6(xb[k], xb[k], eb[k], eg, return_agg=True)
        wx, we, wa = L.interaction_want(sd, xb[k].double(), eb[k].double(), eg.src.long(), eg.dst.long(), "silu",
                                        net.aggr == "mean")
        err = (L.rel_dev(xs, wx), L.rel_dev(es, we), L.rel_dev(ags, wa))
        print(f"{what}: base {k} err x' {err[0]:.2e}, e' {err[1]:.2e}, agg {err[2]:.2e}")
        assert max(err) <= FWD_TOL[prec]
        del wx, we, wa
        singles.append((xs, es, ags))
    for name, big, j, n in (("x'", x1, 0, N), ("e'", e1, 1, E), ("agg", agg, 2, N)):
        L.assert_members_cycle(big.view(members, n, F), [s[j] for s in singles], f"{what}: {name}")
    L.assert_members_cycle(x.view(members, N, F), xb, "the input x")
    L.assert_members_cycle(e.view(members, E, F), eb, "the input e")
    del singles
    with torch.no_grad():
        x2, e2 = net(x, x, e, gb)
    assert torch.equal(x1, x2) and torch.equal(e1, e2)


@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("prec", ["3xbf16", "f16x3"])
def test_k6_edge_shape_8_members_at_256(ga, mesh100, prec, aggr):
    """Case 4: nu = 100 mesh, 256 channels, 8 batched members -- e and e' are 4.9 GB (4.8 M edges)."""
    L.start(DEV)
    _block_forward_case(_net(256, aggr, prec, 4), mesh100[2], 8, prec, f"K6 edges 256 {prec} {aggr}")
    L.finish(DEV, f"K6 edge shape 256 {prec} {aggr}")


@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("prec", ["3xbf16", "f16x3"])
def test_k6_layer_norm_28_members_at_64(ga, mesh100, prec, unfused, monkeypatch):
    """Cases 5 and 6: nu = 100 mesh, 64 channels, 28 batched members (4.3 GB edge state) with LayerNorm behind both MLPs
    -- fused into K6, and (``_LN_FORCE_UNFUSED``) K6 followed by the row kernel."""
    from gwen_amd import interaction as I
    monkeypatch.setattr(I, "_LN_FORCE_UNFUSED", unfused)
    L.start(DEV)
    _block_forward_case(_net(64, "mean" if unfused else "sum", prec, 5, layer_norm=True), mesh100[2], 28, prec,
                        f"K6 + LayerNorm 64 {prec} unfused={unfused}")
    L.finish(DEV, f"K6 + LayerNorm 64 {prec} unfused={unfused}")


def test_backward_pieces_on_the_8_member_graph(ga, mesh100):
    """Case 13: ``act_pair``, ``act_pair_seg``, the segment sums, ``gather_add`` and ``ew`` on the case 4 graph at 256
    channels (4.9 GB edge arrays): member k bitwise the single-member launch of base k mod 3, each base against fp64 on
    the device (elementwise and sums of at most six rows: 2e-6, sums 1e-6 as test_gpu_interaction.py)."""
    from gwen_amd import _lib
    from gwen_amd import interaction as I
    L.start(DEV)
    eg = mesh100[2]
    F, members, N, E = 256, 8, eg.num_dst, eg.num_edges
    assert members * E * F * 4 > BYTES32
    gb = eg.batched(members)
    ab = [_randn(E, F, seed=130 + k) for k in range(3)]
    psb = [_randn(N, F, seed=133 + k) for k in range(3)]
    pab = [_randn(N, 3 * F, seed=136 + k) for k in range(3)]
    a, ps, pall = _cycled(ab, members), _cycled(psb, members), _cycled(pab, members)
    pd = pall[:, F:2 * F]                                                    # a strided view, as in the backward
    h = a.clone()                                           # (act(pre) overwrites its input)
    ptrs = L.nan_blocks(DEV, (members * E, F))
    h, d = I._act_pair(h, "silu", ps, gb.src, pd, gb.dst)
    L.assert_fresh(ptrs, d)
    h2 = a.clone()
    ptrs = L.nan_blocks(DEV, (members * E, F), (members * N, F))
    h2, d2, hs = I._act_pair_seg(h2, "silu", ps, gb.src, pd, gb.rowptr, members * N)
    L.assert_fresh(ptrs, d2, hs)
    assert torch.equal(h, h2) and torch.equal(d, d2)
    del h2, d2
    inv = eg.inv_degree()
    sums = {key: I._segsum(gb.segments(*key), h, members * N) for key in (("dst",), ("src",), ("dst", True))}
    assert torch.equal(sums[("dst",)], hs)
    ga_ = I._gather_add(a, ps, gb.dst, gb.inv_degree())
    singles = []
    for k in range(3):
        pdk = pab[k][:, F:2 * F]
        hk, dk = I._act_pair(ab[k].clone(), "silu", psb[k], eg.src, pdk, eg.dst)
        pre = ab[k].double() + psb[k].double()[eg.src.long()] + pdk.double()[eg.dst.long()]
        sig = torch.sigmoid(pre)
        assert L.rel_dev(hk, pre * sig) <= TOL32 and L.rel_dev(dk, sig * (1 + pre * (1 - sig))) <= TOL32
        del pre, sig
        sk = {key: I._segsum(eg.segments(*key), hk, N) for key in sums}
        zero = torch.zeros(N, F, dtype=torch.float64, device=DEV)
        want_d = zero.index_add(0, eg.dst.long(), hk.double())
        assert L.rel_dev(sk[("dst",)], want_d) <= 1e-6
        assert L.rel_dev(sk[("dst", True)], want_d * inv.double().view(-1, 1)) <= 1e-6
        assert L.rel_dev(sk[("src",)], zero.index_add(0, eg.src.long(), hk.double())) <= 1e-6
        gk = I._gather_add(ab[k], psb[k], eg.dst, inv)
        assert L.rel_dev(gk, ab[k].double() + (psb[k].double() * inv.double().view(-1, 1))[eg.dst.long()]) <= TOL32
        singles.append((hk, dk, gk, sk))
        del want_d, zero
    L.assert_members_cycle(h.view(members, E, F), [s[0] for s in singles], "act_pair: h")
    L.assert_members_cycle(d.view(members, E, F), [s[1] for s in singles], "act_pair: act'")
    L.assert_members_cycle(ga_.view(members, E, F), [s[2] for s in singles], "gather_add")
    for key in sums:
        L.assert_members_cycle(sums[key].view(members, N, F), [s[3][key] for s in singles], f"segment sums {key}")
    del ga_, sums, hs, singles
    # ew: one rounded product / sum per element -- torch's own, bit for bit, over the whole array
    assert torch.equal(I._ew(_lib.EW_MUL, h.clone(), d), h * d)
    assert torch.equal(I._ew(_lib.EW_ADD, h.clone(), d), h + d)
    L.assert_members_cycle(a.view(members, E, F), ab, "the input a")
    L.assert_members_cycle(ps.view(members, N, F), psb, "the table ps")
    del a, ps, pall, pd, h, d
    L.finish(DEV, "backward pieces")


@pytest.mark.parametrize("prec", ["3xbf16", "f16x3"])
def test_training_8_members_at_256_takes_the_general_edge_route(ga, mesh100, prec, monkeypatch):
    """The fused edge backward (gwen_mlp2_bwd_contract_f32) refuses from 2^32 bytes of edge rows: 4.19 M edges at 256
    channels, 7 batched members of this mesh.  The backward now takes it only in range; the case 4 block (8 members)
    trains on the general walk: input gradients of member k bitwise the single-member backward of base k mod 3 ON THE
    SAME ROUTE, parameter gradients against the fp64 sum of the per-member gradients (each member's checked against
    fp64 autograd of the reference) at the tier's gradient tolerance, two runs bitwise equal.  In range (one member)
    the fused launch is still made -- counted, not timed."""
    from gwen_amd import interaction as I
    L.start(DEV)
    eg = mesh100[2]
    F, members, N, E = 256, 8, eg.num_dst, eg.num_edges
    assert members * E * F * 4 > BYTES32 and not I._fused_edge_backward(F, members * E, members * N)
    assert I._fused_edge_backward(F, E, N)
    fused_calls = []
    real = I._edge_backward
    monkeypatch.setattr(I, "_edge_backward", lambda *a, **k: (fused_calls.append(1), real(*a, **k))[1])
    net = _net(F, "sum", prec, 7)
    params = list(net.parameters())
    xb, eb = [_randn(N, F, seed=140 + k) for k in range(3)], [_randn(E, F, seed=143 + k) for k in range(3)]
    gxb, geb = xb, eb          # the upstream gradients of x' and e': the (random) inputs themselves, to save their memory

    def run(x, e, graph, gxo, geo):
        x, e = x.detach().requires_grad_(), e.detach().requires_grad_()
        for p in params:
            p.grad = None
        x1, e1 = net(x, x, e, graph)
        torch.autograd.backward((x1, e1), (gxo, geo))
        return x.grad, e.grad, [p.grad.clone() for p in params]

    per = []
    for k in range(3):
        del fused_calls[:]
        run(xb[k], eb[k], eg, gxb[k], geb[k])
        assert len(fused_calls) == 1                        # in range: the one-launch route
        with monkeypatch.context() as mp:
            mp.setattr(I, "_fused_edge_backward", lambda f, e, n: False)
            del fused_calls[:]
            gx, ge, gp = run(xb[k], eb[k], eg, gxb[k], geb[k])
            assert not fused_calls
        sd = {n_: v.detach().double().requires_grad_() for n_, v in net.named_parameters()}
        x64, e64 = xb[k].double().requires_grad_(), eb[k].double().requires_grad_()
        wx, we, _ = L.interaction_want(sd, x64, e64, eg.src.long(), eg.dst.long(), "silu", False)
        torch.autograd.backward((wx, we), (gxb[k].double(), geb[k].double()))
        err = [L.rel_dev(gx, x64.grad), L.rel_dev(ge, e64.grad)] + \
              [L.rel_dev(g, sd[n_].grad) for g, (n_, _) in zip(gp, net.named_parameters())]
        print(f"training 256 {prec}: base {k} largest gradient err {max(err):.2e}")
        assert max(err) <= GRAD_TOL[prec]
        per.append((gx, ge, [g.double() for g in gp]))
        del sd, x64, e64, wx, we
    gb = eg.batched(members)
    x, e = _cycled(xb, members), _cycled(eb, members)
    gxo, geo = x, e
    L.nan_blocks(DEV, (members * E, F), (members * E, F), (members * E, F), (members * N, F), (members * N, F))
    del fused_calls[:]
    gx, ge, gp = run(x, e, gb, gxo, geo)
    assert not fused_calls                                  # out of range: the general walk
    L.assert_members_cycle(gx.view(members, N, F), [p_[0] for p_ in per], "x gradient")
    L.assert_members_cycle(ge.view(members, E, F), [p_[1] for p_ in per], "e gradient")
    for j, (name, _) in enumerate(net.named_parameters()):
        want = sum(per[k % 3][2][j] for k in range(members))
        err = L.rel_dev(gp[j], want)
        print(f"training 256 {prec}: {name} gradient over {members} members err {err:.2e}")
        assert err <= GRAD_TOL[prec], name
    del gx, ge                                              # (bitwise the bases': the second run is compared with them)
    gx2, ge2, gp2 = run(x, e, gb, gxo, geo)
    L.assert_members_cycle(gx2.view(members, N, F), [p_[0] for p_ in per], "x gradient, second run")
    L.assert_members_cycle(ge2.view(members, E, F), [p_[1] for p_ in per], "e gradient, second run")
    assert all(torch.equal(a, b) for a, b in zip(gp, gp2))
    L.assert_members_cycle(x.view(members, N, F), xb, "the input x")
    L.assert_members_cycle(e.view(members, E, F), eb, "the input e")
    for p in params:
        p.grad = None
    del x, e, gxo, geo, gx2, ge2, per
    L.finish(DEV, f"training 256 {prec}")


# ---- cases 9-12: K8, K4, K2 and the GCN stack through the members axis ------------------------------------------------

@pytest.mark.parametrize("contract", ["f16x3", "3xbf16", "bf16x6"])
@pytest.mark.parametrize("fin,members", [(256, 44), (64, 44), (256, 88), (64, 88)])
def test_k8_wide_layer_over_members(ga, mesh100, fin, members, contract):
    """Cases 9 and 10: nu = 100 hilbert, 256 -> 256 (input and output 4.5 GB, each member below 4 GiB) and 64 -> 256
    (the output only) over 44 members; over 88 members the member offsets ``m * mstride`` also pass 2^31 ELEMENTS."""
    from gwen_amd import ops
    L.start(DEV)
    g = mesh100[3]
    N, fout = g.num_nodes, 256
    assert members * N * fout * 4 > BYTES32 and N * fin * 4 < BYTES32
    assert (members * N * fin * 4 > BYTES32) == (fin == 256)
    assert (members * N * fout > ELEMS31) == (members == 88)
    assert g.tiles() is not None and g.tiles()[3] <= 128
    xb = [_randn(N, fin, seed=90 + k) for k in range(3)]
    x = torch.stack([xb[k % 3] for k in range(members)])
    w, b = (t.to(DEV) for t in make_params(fin, fout))
    ptrs = L.nan_blocks(DEV, (members, N, fout))
    out = ops.wide_layer(g, x, w, b, relu=True, contract=contract)
    L.assert_fresh(ptrs, out)
    singles = []
    for k in range(3):
        singles.append(ops.wide_layer(g, xb[k], w, b, relu=True, contract=contract))
        err = L.rel_dev(singles[k], L.gcn_want(g, xb[k], w, b, True))
        print(f"K8 {fin}->{fout} {contract}: base {k} err {err:.2e}")
        assert err <= FWD_TOL[contract]
    L.assert_members_cycle(out, singles, f"K8 {fin}->{fout} {contract}")
    L.assert_members_cycle(x, xb, "K8's input")
    assert torch.equal(out, ops.wide_layer(g, x, w, b, relu=True, contract=contract))
    del x, out
    L.finish(DEV, f"K8 {fin}->{fout} {contract}")


def test_k4_k2_and_the_stack_over_340_members_at_64(ga, mesh100):
    """Cases 11 and 12: [340, 100 002, 64] (8.7 GB, past 2^31 elements) through K4 (``layer_fused``), K2 (``propagate``), ``StackForward``
    and ``GNNModel``: member k bitwise the single-member launch of base k mod 3 (the stack: bitwise member k mod 3 of the
    same launch), each base against fp64."""
    from gwen_amd import ops
    from oracle import gcn_oracle as O
    L.start(DEV)
    m, ei, _, g = mesh100
    N, F, members = g.num_nodes, 64, 340
    assert members * N * F * 4 > BYTES32 and members * N * F > ELEMS31
    xb = [_randn(N, F, seed=110 + k) for k in range(3)]
    x = torch.stack([xb[k % 3] for k in range(members)])
    w, b = (t.to(DEV) for t in make_params(F, F))
    w2, b2 = (t.to(DEV) for t in make_params(F, F, seed=SEED + 1))
    eye = torch.eye(F, device=DEV)
    want1 = [L.gcn_want(g, xb[k], w, b, True) for k in range(3)]
    cases = [(f"K4 {c}", (lambda t, c=c: ops.layer_fused(g, t, w, b, relu=True, contract=c)), want1, FWD_TOL[c])
             for c in ("3xbf16", "bf16x6")]
    cases.append(("K2", lambda t: ops.propagate(g, t, b, relu=True),
                  [L.gcn_want(g, xb[k], eye, b, True) for k in range(3)], TOL32))
    for what, fn, wants, tol in cases:
        ptrs = L.nan_blocks(DEV, (members, N, F))
        out = fn(x)
        L.assert_fresh(ptrs, out)
        singles = [fn(xb[k]) for k in range(3)]
        err = max(L.rel_dev(singles[k], wants[k]) for k in range(3))
        print(f"{what} over {members} members: largest base err {err:.2e}")
        assert err <= tol, what
        L.assert_members_cycle(out, singles, what)
        assert torch.equal(out, fn(x)), what
        del out, singles
    # the stack launcher: two AUTO layers (fp32-class), into a NaN-filled buffer of the test's own
    plan = ga.StackForward([(w, b, True, "auto"), (w2, b2, False, "auto")], g)
    out = L.nan_tensor(DEV, members, N, F)
    plan.run(x, out=out)
    # (the launcher picks its kernels by N x members, so a one-member launch is no bitwise yardstick here: the first
    #  three members against fp64, every later member bitwise against its base among them)
    for k in range(3):
        assert L.rel_dev(out[k], L.gcn_want(g, want1[k], w2, b2, False)) <= TOL32
    L.assert_members_cycle(out, [out[0], out[1], out[2]], "StackForward")
    assert torch.equal(out, plan.run(x))
    del out, want1, plan
    # the model (the reference's layer stack), against the CPU oracle per base
    torch.manual_seed(SEED)
    refm = O.OracleGNNModel(O.OracleGNNConfig(N, N, F, F, F))
    model = ga.GNNModel(ga.GNNConfig(N, N, F, F, F))
    model.load_state_dict(refm.state_dict())
    model = model.to(DEV).eval()
    ptrs = L.nan_blocks(DEV, (members, N, F))
    with torch.no_grad():
        out = model(x, ei)
        L.assert_fresh(ptrs, out)
        for k in range(3):
            assert L.rel(out[k], refm(xb[k].cpu(), ei.cpu())) <= REL_TOL
        L.assert_members_cycle(out, [out[0], out[1], out[2]], "GNNModel")
        assert torch.equal(out, model(x, ei))
    L.assert_members_cycle(x, xb, "the stack's input")
    del x, out
    L.finish(DEV, "K4 / K2 / stack over 340 members")


# ---- the limits themselves: both sides of every guard, on really allocated buffers ------------------------------------

def _mlp2_abi(a, w1, w2, b2, g1, idx1, out, contract):
    """gwen_mlp2_ln_f32 through the C ABI with the test's own output buffer; returns the code."""
    from gwen_amd import _lib
    from gwen_amd.graph import _ptr, _stream
    from gwen_amd.interaction import MLP2_CONTRACTS
    lib, f, code = _lib.lib(), a.size(1), MLP2_CONTRACTS[contract]
    nws = int(lib.gwen_mlp2_contract_workspace_bytes(f, code))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV) if nws > 0 else None
    with torch.cuda.device(a.device):
        return lib.gwen_mlp2_ln_f32(_ptr(a), _ptr(w1), _ptr(g1), _ptr(idx1), g1.size(0), g1.stride(0), None, None, 0, 0,
                                    None, _ptr(w2), _ptr(b2), _ptr(a), _ptr(out), a.size(0), f, _lib.ACT_SILU, None, None,
                                    0, None, 0, 0, code, None, None, 1e-5, _ptr(ws), nws, _stream(a.device))


@pytest.mark.parametrize("F", [256, 64])
def test_k6_table_either_side_of_its_limit(ga, F):
    """K6 gathers table rows through 32-bit byte offsets: a column block of a [rows, 3F] node table (the forecaster's
    [Ps | Pd | Q]) works up to floor((2^32 - 1) / (12 F)) rows -- the last row, and the rows either side of byte 2^31,
    against fp64 -- and one row more is refused: ``ValueError`` from ``mlp2`` naming the size and the limit, GWEN_ERANGE
    from the C ABI, the output still NaN.  The table is allocated at the size it claims on both sides."""
    from gwen_amd import _lib
    from gwen_amd.interaction import mlp2
    L.start(DEV)
    ld = 3 * F
    rows_max = (BYTES32 - 1) // (ld * 4)
    assert rows_max * ld * 4 < BYTES32 <= (rows_max + 1) * ld * 4
    table = torch.randn(rows_max + 1, ld, device=DEV, generator=torch.Generator(DEV).manual_seed(SEED))
    r31, R = (1 << 31) // (ld * 4), 333
    special = torch.tensor([0, r31 - 1, r31, r31 + 1, rows_max - 2, rows_max - 1])
    idx = torch.cat([special, torch.randint(0, rows_max, (R - 6,), generator=torch.Generator().manual_seed(SEED))])
    idx = idx.to(torch.int32).to(DEV)
    a, w1, w2, b2 = _randn(R, F, seed=1), _randn(F, F, seed=2) / F ** 0.5, _randn(F, F, seed=3) / F ** 0.5, _randn(F, seed=4)
    ok, bad = table[:rows_max, F:2 * F], table[:, F:2 * F]
    rows_copy = table[special.to(DEV)].clone()
    for contract in ("3xbf16", "f16x3"):
        out = L.nan_tensor(DEV, R, F)
        _lib.check(_mlp2_abi(a, w1, w2, b2, ok, idx, out, contract), "gwen_mlp2_ln_f32")
        want = L.mlp2_want(a, w1, w2, b2, ok[idx.long()], torch.arange(R), None, a)
        err = _err(contract, out, want)
        print(f"K6 table of {rows_max} rows x {ld * 4} bytes, {contract}: err {err:.2e}")
        assert err <= FWD_TOL[contract]
        got, _ = mlp2(a, w1, w2, b2, g1=ok, idx1=idx, res=a, contract=contract)
        assert torch.equal(got, out)
        # one row more
        out = L.nan_tensor(DEV, R, F)
        rc = _mlp2_abi(a, w1, w2, b2, bad, idx, out, contract)
        assert rc == -2                                     # GWEN_ERANGE
        with pytest.raises(_lib.GwenHipError, match="code -2"):
            _lib.check(rc, "gwen_mlp2_ln_f32")
        assert L.all_nan(out)
        with pytest.raises(ValueError, match=f"{(rows_max + 1) * ld * 4} bytes.*limit is {BYTES32 - 1} bytes"):
            mlp2(a, w1, w2, b2, g1=bad, idx1=idx, res=a, contract=contract)
    assert torch.equal(table[special.to(DEV)], rows_copy)
    del table, ok, bad
    L.finish(DEV, f"K6 table limit F={F}")


def test_forecaster_node_table_limit_is_a_value_error_before_any_launch(ga, mesh100, monkeypatch):
    """14 batched members of the 100 002-node mesh at 256 channels make a [1 400 028, 768] node table, 4.3 GB: past
    K6's 32-bit table offsets (1 398 101 rows at this stride).  The block raises ``ValueError`` naming the table's size
    and the limit before it launches anything (the projections included); nothing above the C layer said so before."""
    from gwen_amd import interaction as I, ops
    L.start(DEV)
    eg = mesh100[2]
    F, members = 256, 14
    gb = eg.batched(members)
    rows = members * eg.num_dst
    assert rows * 3 * F * 4 >= BYTES32 > (rows - eg.num_dst) * 3 * F * 4
    launches = []
    monkeypatch.setattr(ops, "linear", lambda *a, **k: launches.append("K3"))
    monkeypatch.setattr(I, "mlp2", lambda *a, **k: launches.append("K6"))
    net = _net(F, "sum", "3xbf16", 9)
    x = torch.zeros(rows, F, device=DEV)
    e = torch.zeros(gb.num_edges, F, device=DEV)
    with pytest.raises(ValueError, match=f"{rows} rows.*{rows * 3 * F * 4} bytes.*limit is {BYTES32 - 1} bytes"):
        with torch.no_grad():
            net(x, x, e, gb)
    with pytest.raises(ValueError, match="limit is"):
        net(x.requires_grad_(), x, e, gb)
    assert not launches
    del x, e
    L.finish(DEV, "forecaster node table limit")


def test_batched_graph_refuses_past_int32(ga, mesh100):
    eg = mesh100[2]
    assert 3580 * eg.num_edges >= 2 ** 31 - 1 > 3579 * eg.num_edges
    with pytest.raises(ValueError, match="int32"):
        eg.batched(3580)


@pytest.mark.parametrize("contract", ["3xbf16", "f16x3"])
def test_fused_edge_backward_either_side_of_its_limit(ga, contract):
    """gwen_mlp2_bwd_contract_f32 reads d1 as a table, row for row: R * F * 4 < 2^32.  At 256 channels R = 4 194 303
    works -- every block of P rows bitwise the first, the first against fp64 -- and R = 4 194 304 answers GWEN_ERANGE with
    both outputs still NaN.  All buffers are allocated at the refused size."""
    from gwen_amd import _lib
    from gwen_amd.graph import _ptr, _stream
    from gwen_amd.interaction import MLP2_CONTRACTS
    L.start(DEV)
    lib, F, code = _lib.lib(), 256, MLP2_CONTRACTS[contract]
    R = BYTES32 // (F * 4)
    assert R * F * 4 == BYTES32
    bge, bd1 = _randn(P, F, seed=161), _randn(P, F, seed=162)
    ge, d1 = L.periodic(bge, R), L.periodic(bd1, R)
    tab = _randn(1000, F, seed=163)
    dst = ((torch.arange(R, device=DEV) % P) * 7 % 1000).to(torch.int32)
    w2t, wet = _randn(F, F, seed=164) / F ** 0.5, _randn(F, F, seed=165) / F ** 0.5
    nws = int(lib.gwen_mlp2_contract_workspace_bytes(F, code))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)

    def call(rows):
        g_pre1 = L.nan_tensor(DEV, int(lib.gwen_mlp2_bwd_rows(R)), F)
        g_e = L.nan_tensor(DEV, R, F)
        with torch.cuda.device(DEV):
            rc = lib.gwen_mlp2_bwd_contract_f32(_ptr(ge), _ptr(w2t), _ptr(d1), _ptr(tab), _ptr(dst), tab.size(0),
                                                tab.stride(0), _ptr(wet), _ptr(g_pre1), _ptr(g_e), rows, F, code, _ptr(ws),
                                                nws, _stream(torch.device(DEV)))
        return rc, g_pre1, g_e

    rc, g_pre1, g_e = call(R)
    assert rc == -2
    with pytest.raises(_lib.GwenHipError, match="code -2"):
        _lib.check(rc, "gwen_mlp2_bwd_contract_f32")
    assert L.all_nan(g_pre1) and L.all_nan(g_e)
    del g_pre1, g_e
    rc, g_pre1, g_e = call(R - 1)
    _lib.check(rc, "gwen_mlp2_bwd_contract_f32")
    want_pre = (L.host(bge) @ L.host(w2t).t() + L.host(tab)[dst[:P].cpu().long()]) * L.host(bd1)
    want_e = L.host(bge) + want_pre @ L.host(wet).t()
    err = _err(contract, g_pre1[:P], want_pre), _err(contract, g_e[:P], want_e)
    print(f"fused edge backward at R = {R - 1}, {contract}: err g_pre1 {err[0]:.2e}, g_e {err[1]:.2e}")
    assert max(err) <= GRAD_TOL[contract]
    L.assert_periodic(g_pre1[:R - 1], P, "g_pre1")
    L.assert_periodic(g_e[:R - 1], P, "g_e")
    assert L.all_nan(g_e[R - 1:])                           # the row past the launch stays unwritten
    assert torch.equal(ge[:P], bge) and torch.equal(d1[:P], bd1)
    del ge, d1, g_pre1, g_e
    L.finish(DEV, f"fused edge backward limit {contract}")


def test_k8_k4_chain_source_either_side_of_its_limit(ga):
    """K8, K4 and K5 gather source rows through 32-bit byte offsets: N_src * Fin * 4 < 2^32.  On a ring lattice built on
    the device (every node receives from i - 2 .. i + 2: it tiles in its own order) with 64 channels, N = 16 777 215
    works in all three -- rows 0, 1, the rows either side of byte 2^31, the last rows and a random sample against fp64
    evaluated for those rows only, and (the input being a block of P nodes repeated) every interior block bitwise block
    1 -- and N = 16 777 216 is refused: ``ValueError`` from ``ops.layer_fused``, GWEN_ERANGE from ``wide_layer`` and
    ``chain``, and the stack launcher falls back or raises the same way; no output byte is written."""
    from gwen_amd import _lib, ops
    L.start(DEV)
    F = 64
    n_ok = (BYTES32 - 1) // (F * 4)
    assert n_ok * F * 4 < BYTES32 == (n_ok + 1) * F * 4
    base = _randn(P, F, seed=170)
    x_all = L.periodic(base, n_ok + 1)                      # allocated at the refused size; the accepted one is a prefix
    w, b = (t.to(DEV) for t in make_params(F, F))
    r31 = (1 << 31) // (F * 4)
    gen = torch.Generator().manual_seed(SEED)

    def spots(n):
        rows = torch.cat([torch.tensor([0, 1, 2, r31 - 1, r31, r31 + 1, n - 3, n - 2, n - 1]),
                          torch.randint(0, n, (55,), generator=gen)]).to(DEV)
        nb = (rows.view(-1, 1) + torch.arange(-2, 3, device=DEV).view(1, -1)) % n
        return rows, nb

    g = ga.prepare_graph(L.ring_edges(n_ok, DEV), n_ok)
    assert g.tiles() is not None
    x = x_all[:n_ok]
    rows, nb = spots(n_ok)
    agg = L.host(x[nb.reshape(-1)].view(-1, 5, F)).sum(1) * 0.2         # degree 5 with the self-loop: every weight 1 / 5
    conv = torch.relu(agg @ L.host(w).t() + L.host(b))
    full = n_ok // P
    launches = [("K8 f16x3", lambda: ops.wide_layer(g, x, w, b, relu=True, contract="f16x3"), conv, TOL32),
                ("K8 3xbf16", lambda: ops.wide_layer(g, x, w, b, relu=True, contract="3xbf16"), conv, REL_TOL),
                ("K4 bf16x6", lambda: ops.layer_fused(g, x, w, b, relu=True, contract="bf16x6"), conv, TOL32),
                ("K4 3xbf16", lambda: ops.layer_fused(g, x, w, b, relu=True, contract="3xbf16"), conv, REL_TOL),
                ("K5 bf16x6", lambda: ops.chain(g, x, w, None, b, True, True, contract="bf16x6"),
                 torch.relu(agg + L.host(b)) @ L.host(w).t(), TOL32)]
    for what, fn, want, tol in launches:
        ptrs = L.nan_blocks(DEV, (n_ok, F))
        out = fn()
        L.assert_fresh(ptrs, out)
        err = L.rel(out[rows], want)
        print(f"{what} at N_src = {n_ok}: err on {rows.numel()} rows {err:.2e}")
        assert err <= tol, what
        L.assert_periodic(out[P:full * P], P, what)         # (block 0 and the tail see the ring close: checked by rows)
        assert not bool(torch.isnan(out).any()), what
        del out
    del g, x
    # one node more
    n_bad = n_ok + 1
    g = ga.prepare_graph(L.ring_edges(n_bad, DEV), n_bad)
    assert g.tiles() is not None
    for what, fn, exc in (("K8", lambda: ops.wide_layer(g, x_all, w, b, relu=True, contract="f16x3"), _lib.GwenHipError),
                          ("K4", lambda: ops.layer_fused(g, x_all, w, b, relu=True), ValueError),
                          ("K5", lambda: ops.chain(g, x_all, w, None, b, True, True, contract="bf16x6"),
                           _lib.GwenHipError)):
        ptrs = L.nan_blocks(DEV, (n_bad, F))
        with pytest.raises(exc, match="32-bit" if exc is ValueError else "code -2"):
            fn()
        probe = torch.empty(n_bad, F, dtype=torch.float32, device=DEV)   # the block the wrapper's output had (or would have)
        assert probe.data_ptr() in ptrs and L.all_nan(probe), what
        del probe
    out = L.nan_tensor(DEV, n_bad, F)
    plan = ga.StackForward([(w, b, True, "auto")], g)
    try:
        plan.run(x_all, out=out)
    except _lib.GwenHipError as err:
        assert "code -2" in str(err) and L.all_nan(out)
    else:                                                   # a fall-back (K3 + K2) must be right
        rows, nb = spots(n_bad)
        agg = L.host(x_all[nb.reshape(-1)].view(-1, 5, F)).sum(1) * 0.2
        assert L.rel(out[rows], torch.relu(agg @ L.host(w).t() + L.host(b))) <= TOL32
        assert not bool(torch.isnan(out).any())
    assert torch.equal(x_all[:P], base)
    L.assert_periodic(x_all, P, "the limit test's input")
    del g, x_all, out, plan
    L.finish(DEV, "K8 / K4 / K5 source limit")
