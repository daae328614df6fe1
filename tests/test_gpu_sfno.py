"""gwen_amd.sfno on the device against the fp64 restatements of tests/sfno_ref.py.

Tolerances.  The spectral convolution is the split arithmetic of K3 at K <= 512, so it is held to K3's own figures in
tests/test_gpu_parity.py: helpers.rel_err <= 2e-6 on the default tier (bf16x6) and 2e-5 on "3xbf16".  Inputs are standard
normal and W is scaled by Cin^-1/2, so the output's magnitude does not depend on l and no degree can hide in the tensor's
scale; every degree is checked against its own maximum as well (1e-3: a wrong group or tail is O(1)).  The weight
gradient grows with 2l + 1 and is therefore normalised per degree."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_ref as L  # noqa: E402
import sfno_ref as F  # noqa: E402
import sht_ref as R  # noqa: E402
from helpers import REL_TOL, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f16x3": 2e-6, "3xbf16": 2e-5}
PRECISIONS = ["f16x3", "3xbf16"]
CHANNELS = [(16, 16), (16, 48), (48, 16), (64, 64), (256, 64), (64, 256)]
LEADS = [(), (3,), (2, 2)]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


_inputs = {}


def inputs(lmax, cin, cout, lead):
    """(coef, W, r) in fp32 numpy and the restatement's (out, g_coef, g_W) of them, made once a shape."""
    key = (lmax, cin, cout, lead)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * lmax + 7 * cin + cout + len(lead))
        t = (lmax + 1) ** 2
        coef = rng.standard_normal(lead + (t, cin)).astype(np.float32)
        w = (rng.standard_normal((lmax + 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
        r = rng.standard_normal(lead + (t, cout)).astype(np.float32)
        flat, rflat = coef.reshape(-1, t, cin), r.reshape(-1, t, cout)
        g_coef, g_w = F.spectral_conv_grads(flat, w, rflat)
        _inputs[key] = (coef, w, r, F.spectral_conv(flat, w).reshape(lead + (t, cout)), g_coef.reshape(coef.shape), g_w)
    return _inputs[key]


def per_degree(got, want, lmax):
    """max over l of max |err| / max |ref| on the rows of degree l; got, want [..., T, C]."""
    worst = 0.0
    for l in range(lmax + 1):
        a, b = got[..., l * l:(l + 1) ** 2, :], want[..., l * l:(l + 1) ** 2, :]
        worst = max(worst, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)))
    return worst


# ---- 1. forward against the restatement ---------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("lead", LEADS, ids=["one", "b3", "b2x2"])
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("lmax", [0, 1, 7, 8, 40])
def test_forward_matches_the_restatement(ga, lmax, cin, cout, lead, precision):
    from gwen_amd import _lib, sfno
    coef, w, _, want, _, _ = inputs(lmax, cin, cout, lead)
    c, wd = dev(coef), dev(w)
    t = (lmax + 1) ** 2
    out = L.nan_tensor(DEV, *lead, t, cout)                       # an unwritten row stays NaN and fails
    batch = int(np.prod(lead, dtype=np.int64))
    sfno._launch(c, wd, batch, lmax, cin, cout, False, _lib.CONTRACT_NAMES[precision], out=out)
    got = host(out)
    assert np.isfinite(got).all()
    err, deg = rel_err(got, want), per_degree(got, want, lmax)
    print(f"lmax {lmax} {cin}->{cout} {lead} {precision}: rel_err {err:.2e}, worst degree {deg:.2e}")
    assert err <= TOL[precision]
    assert deg <= 1e-3
    assert same_bits(ga.spectral_conv(c, wd, precision=precision), out)     # the public call is this launch
    assert same_bits(ga.spectral_conv(c, wd, lmax=lmax, precision=precision), out)


# ---- 2. group isolation, bitwise ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("lmax,cin,cout", [(8, 16, 48), (40, 64, 64), (7, 256, 64)])
def test_groups_and_items_are_isolated_bitwise(ga, lmax, cin, cout, precision):
    coef, w, _, _, _, _ = inputs(lmax, cin, cout, (3,))
    c, wd = dev(coef), dev(w)
    base = ga.spectral_conv(c, wd, precision=precision)
    assert same_bits(base, ga.spectral_conv(c, wd, precision=precision))          # two runs
    for l0 in sorted({0, min(3, lmax), lmax}):
        w2 = wd.clone()
        w2[l0] += 1.0
        got = ga.spectral_conv(c, w2, precision=precision)
        changed = (got.view(torch.int32) != base.view(torch.int32)).any(-1).any(0)        # [T]
        want = torch.zeros_like(changed)
        want[l0 * l0:(l0 + 1) ** 2] = True
        assert torch.equal(changed, want), f"W[{l0}] reached rows {changed.nonzero().flatten().tolist()}"
    c2 = c.clone()
    c2[1] = c2[1] * 3.0 + 1.0
    got = ga.spectral_conv(c2, wd, precision=precision)
    assert same_bits(got[0], base[0]) and same_bits(got[2], base[2]) and not same_bits(got[1], base[1])
    for b in range(3):                                                              # a batch of 3 = three launches
        assert same_bits(ga.spectral_conv(c[b], wd, precision=precision), base[b])
        assert same_bits(ga.spectral_conv(c[b:b + 1], wd, precision=precision)[0], base[b])


# ---- 3. gradients -----------------------------------------------------------------------------------------------------------

GRAD_SHAPES = [(lmax, ci, co, lead) for lmax in (0, 1, 7, 8) for ci, co in CHANNELS for lead in LEADS] + \
              [(40, 64, 64, lead) for lead in LEADS]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("lmax,cin,cout,lead", GRAD_SHAPES,
                         ids=[f"l{a}-{b}to{c}-{'x'.join(map(str, d)) or 'one'}" for a, b, c, d in GRAD_SHAPES])
def test_gradients_match_fp64_autograd(ga, lmax, cin, cout, lead, precision):
    coef, w, r, _, want_c, want_w = inputs(lmax, cin, cout, lead)
    if (lmax, cin, cout, lead) == (1, 16, 48, (3,)):                   # the restated gradients ARE torch's fp64 autograd
        ct, wt = torch.from_numpy(coef).double().requires_grad_(), torch.from_numpy(w).double().requires_grad_()
        deg = torch.from_numpy(R.degrees(lmax))
        (torch.einsum("...tc,tcd->...td", ct, wt[deg]) * torch.from_numpy(r).double()).sum().backward()
        assert np.abs(ct.grad.numpy() - want_c).max() <= 1e-12 and np.abs(wt.grad.numpy() - want_w).max() <= 1e-12
    rd = dev(r)

    def grads():
        c, wd = dev(coef).requires_grad_(), dev(w).requires_grad_()
        (ga.spectral_conv(c, wd, precision=precision) * rd).sum().backward()
        return c.grad, wd.grad

    g_c, g_w = grads()
    err_c = rel_err(g_c, want_c)
    gw = host(g_w)
    err_w = max(float(np.abs(gw[l] - want_w[l]).max() / np.abs(want_w[l]).max()) for l in range(lmax + 1))
    print(f"lmax {lmax} {cin}->{cout} {lead} {precision}: g_coef {err_c:.2e}, g_weight worst degree {err_w:.2e}")
    assert np.isfinite(gw).all()
    assert err_c <= TOL[precision]
    assert err_w <= TOL[precision]
    again_c, again_w = grads()
    assert same_bits(again_c, g_c) and same_bits(again_w, g_w)
    # either gradient alone is the same bits
    c, wd = dev(coef).requires_grad_(), dev(w)
    (ga.spectral_conv(c, wd, precision=precision) * rd).sum().backward()
    assert same_bits(c.grad, g_c)


# ---- 4. module equals composition -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,nlat,nlon", [("gauss", 9, 18), ("equiangular", 17, 32)])
def test_module_is_the_composition_of_public_pieces(ga, grid, nlat, nlon):
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=8, grid=grid)
    other = ga.SphericalHarmonics(12, 24, DEV, lmax=8, grid="gauss")
    torch.manual_seed(11)
    x = torch.randn(2, nlat * nlon, 16, device=DEV)
    for sh_out in (None, other):
        for precision in PRECISIONS:
            m = ga.SpectralConv(sh, 16, 48, precision=precision, sh_out=sh_out).to(DEV)
            assert m.weight.shape == (9, 16, 48)
            y = m(x)
            out = sh if sh_out is None else sh_out
            want = out.synthesis(ga.spectral_conv(sh.analysis(x), m.weight, precision=precision))
            assert y.shape == (2, out.rows, 48) and same_bits(y.detach(), want.detach())
    with pytest.raises(ValueError):
        ga.SpectralConv(sh, 16, 48, sh_out=ga.SphericalHarmonics(12, 24, DEV, lmax=7, grid="gauss"))


# ---- 5. rotation equivariance on the device ---------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_rotation_equivariance_on_the_device(ga, precision):
    """Gauss 12 x 24, lmax 8, 16 -> 48: the layer of the field turned by 5 longitudes against the turned output of the
    layer.  In exact arithmetic they are equal.  The bound, a side, with a the coefficients of x and c = a . W[deg]:
      * the analysis stores a in fp32: |da| <= 2^-24 |a| (its fp64 sums are 1e-10 X sqrt(2l + 1) at most,
        tests/test_gpu_sht.py), which the convolution carries to at most 2^-24 (|a| . |W[deg]|) a coefficient;
      * the convolution itself: test 1's tolerance, tol max |c|, on every coefficient;
      * the synthesis: a point's terms sum to at most sum_lm |dc_lm| sqrt(2l + 1) (tests/test_gpu_sht.py), plus its own
        1e-10 S and one fp32 rounding of the result, 2^-24 |y|.
    Both sides carry it, hence twice.  With sum_l (2l + 1)^(3/2) = 274 at lmax 8, max |c| ~ 0.2 and max |y| ~ 2 this is
    ~2e-4 (default tier) and ~2e-3 ("3xbf16"): the test requires the bound to stay below 1e-2 max |y|, for the per-m
    mix-up measured at 2.45 max |y| in tests/test_sfno_host.py must not fit under it."""
    grid, nlat, nlon, lmax, cin, cout = "gauss", 12, 24, 8, 16, 48
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid=grid)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, nlat * nlon, cin)).astype(np.float32)
    w = (rng.standard_normal((lmax + 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    m = ga.SpectralConv(sh, cin, cout, precision=precision).to(DEV)
    with torch.no_grad():
        m.weight.copy_(dev(w))
        y = host(m(dev(x)))
        y_turned = host(m(dev(F.roll(x, nlat, nlon, 5))))
    # the bound, from the restatement's fp64 values of the same inputs
    a = R.analysis(x, grid, nlat, nlon, lmax)
    c = F.spectral_conv(a, w)
    amp = np.sqrt(2.0 * R.degrees(lmax) + 1.0)[None, :, None]
    d_in = 2.0 ** -24 * F.spectral_conv(np.abs(a), np.abs(w))
    d_c = d_in + TOL[precision] * np.abs(c).max()
    ymax = float(np.abs(y).max())
    bound = 2.0 * float(((d_c + 1e-10 * np.abs(c)) * amp).sum(1).max() + 2.0 ** -24 * ymax)
    got = float(np.abs(y_turned - F.roll(y, nlat, nlon, 5)).max())
    print(f"equivariance defect on the device ({precision}): {got:.2e}, bound {bound:.2e}, max |y| {ymax:.2f}")
    assert bound < 1e-2 * ymax
    assert got <= bound
    assert rel_err(y, F.layer(x, w, grid, nlat, nlon, lmax)) <= REL_TOL


# ---- 6. the whole model ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("layer_norm,residual", [(True, False), (False, False), (True, True)],
                         ids=["ln", "no-ln", "ln-residual"])
def test_whole_model_against_the_fp64_restatement(ga, layer_norm, residual, precision):
    grid, nlat, nlon = "gauss", 9, 18
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, grid=grid)
    assert sh.lmax == 8
    torch.manual_seed(23)
    model = ga.SFNO(sh, 3, 2, channels=16, blocks=2, layer_norm=layer_norm, precision=precision, residual=residual)
    with torch.no_grad():                                          # biases and norms away from their trivial start
        for name, p in model.named_parameters():
            if name.endswith("bias"):
                p.normal_(0.0, 0.1)
            elif "norm" in name:
                p.normal_(1.0, 0.1)
    ref = F.RefSFNO(grid, nlat, nlon, sh.lmax, 3, 2, 16, 2, layer_norm=layer_norm, residual=residual)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    model = model.to(DEV)
    x = torch.randn(2, nlat * nlon, 3)
    r = torch.randn(2, nlat * nlon, 2)
    xd = x.to(DEV).requires_grad_()
    xr = x.double().requires_grad_()
    out = model(xd)
    want = ref(xr)
    assert out.shape == (2, nlat * nlon, 2)
    (out * r.to(DEV)).sum().backward()
    (want * r.double()).sum().backward()
    errs = {"forward": rel_err(out.detach(), want.detach()), "x": rel_err(xd.grad, xr.grad)}
    refs = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        errs[name] = rel_err(p.grad, refs[name].grad)
    worst = max(errs, key=errs.get)
    print(f"SFNO ln={layer_norm} residual={residual} {precision}: forward {errs['forward']:.2e}, input gradient "
          f"{errs['x']:.2e}, worst {worst} {errs[worst]:.2e}")
    bad = {k: v for k, v in errs.items() if not v <= REL_TOL}
    assert not bad, bad


# ---- 7. capture -------------------------------------------------------------------------------------------------------------

def test_block_captures_into_a_graph(ga):
    sh = ga.SphericalHarmonics(9, 18, DEV, grid="gauss")
    torch.manual_seed(3)
    block = ga.SFNOBlock(sh, 16).to(DEV)
    first, second, third = (torch.randn(2, sh.rows, 16, device=DEV) for _ in range(3))
    with torch.no_grad():
        eager = [block(t) for t in (first, second, third)]
        buf = first.clone()
        block(buf)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = block(buf)
        for src, want in ((second, eager[1]), (third, eager[2])):
            buf.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(out, want)
    assert not same_bits(eager[1], eager[2])


# ---- 8. past 4 GiB ------------------------------------------------------------------------------------------------------------

def test_coefficients_past_4_gib(ga):
    """lmax 255, 64 -> 64, 260 items of one 3-item pattern repeated: coef, out and g_coef each cross 2^32 bytes (and 2^30
    elements times 4: the offsets batch * T * C are 64-bit or wrong).  The first 3 items against the restatement, every
    later item bitwise against its base, on the device; outputs land in memory that was NaN.  g_weight on a 6-item batch
    (the pattern twice) against twice the restatement's sums, per degree, at test 3's tolerance."""
    lmax, cin, cout, items = 255, 64, 64, 260
    t = (lmax + 1) ** 2
    L.start(DEV)
    assert items * t * cin * 4 > L.BYTES32 and items * t * cout * 4 > L.BYTES32
    rng = np.random.default_rng(255)
    base = rng.standard_normal((3, t, cin)).astype(np.float32)
    w = (rng.standard_normal((lmax + 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    rbase = rng.standard_normal((3, t, cout)).astype(np.float32)
    want, (want_c, want_w) = F.spectral_conv(base, w), F.spectral_conv_grads(base, w, rbase)
    wd = dev(w)
    for precision in PRECISIONS:
        coef = L.periodic(dev(base), items).requires_grad_()
        r = L.periodic(dev(rbase), items)
        ptrs = L.nan_blocks(DEV, (items, t, cout))
        out = ga.spectral_conv(coef, wd, precision=precision)
        L.assert_fresh(ptrs, out)
        err = rel_err(out[:3].detach(), want)
        print(f"past 4 GiB {precision}: forward {err:.2e}")
        assert err <= TOL[precision]
        L.assert_periodic(out, 3, f"spectral_conv {precision}", chunk_blocks=8)
        ptrs = L.nan_blocks(DEV, (items, t, cin))
        (g_c,) = torch.autograd.grad(out, coef, r)
        L.assert_fresh(ptrs, g_c)
        err = rel_err(g_c[:3], want_c)
        print(f"past 4 GiB {precision}: g_coef {err:.2e}")
        assert err <= TOL[precision]
        L.assert_periodic(g_c, 3, f"g_coef {precision}", chunk_blocks=8)
        assert torch.equal(coef.detach()[:3], dev(base))
        del coef, r, out, g_c
        six = dev(np.concatenate([base, base])).contiguous()
        wg = wd.clone().requires_grad_()
        (ga.spectral_conv(six, wg, precision=precision) * dev(np.concatenate([rbase, rbase]))).sum().backward()
        gw = host(wg.grad)
        err = max(float(np.abs(gw[l] - 2.0 * want_w[l]).max() / np.abs(want_w[l] * 2.0).max()) for l in range(lmax + 1))
        print(f"past 4 GiB {precision}: g_weight worst degree {err:.2e}")
        assert err <= TOL[precision]
        del six, wg
    L.finish(DEV, "spectral_conv past 4 GiB")
