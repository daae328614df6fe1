"""Every GCN entry point of the C ABI (include/gwen_hip.h) at non-packed row pitches and member strides.

The wrappers in gwen_amd/ops.py and every other GPU test pass packed operands (ld == F, mstride == rows * F), so a
kernel that used Fout for ldo, N * Fin for mstride_x or a 32-bit product for a pitch kept the suite green.  Here each
entry point runs once packed -- the form the parity tests tie to the oracle -- and then on the same logical values in
the layouts of tests/strided.py.  Per case:

  * the logical output is BITWISE the packed call's wherever the launcher's own alignment / % 4 rules select the same
    kernel; where the layout changes the kernel (the ``odd`` layouts: scalar fallbacks of K3, linear_nn and the weight
    gradient) it is held against an fp64 torch restatement at the bound the entry point's parity test uses
    (helpers.LINEAR_TOL, LINEAR_NN_TOL, GRAD_W_TOL); K2 stays bitwise at every vector width;
  * no cell outside the logical output changed, bit for bit: output padding, guards, the inputs and their padding
    (``Arena.verify``), and every logical output cell was written;
  * a second identical call gives the same bits.

Each test counts the cases it launched and asserts the count its lists give; the last test prints the totals.
"""
import collections
import ctypes as C
import itertools

import pytest
import torch

from helpers import GRAD_B_TOL, GRAD_W_TOL, LINEAR_NN_TOL, LINEAR_TOL, SEED, graph_cases, make_params, rel_err
from strided import Arena, layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = collections.Counter()
ERANGE = -2
CONTRACT_NAME = {0: "3xbf16", 1: "fp32", 2: "bf16x6", 3: "f16x3"}


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


@pytest.fixture(scope="module")
def L(hip_lib):
    return hip_lib


@pytest.fixture(scope="module")
def graphs(ga):
    """Prepared graphs by name, built on first use and shared by every test of the module."""
    cache = {}

    def get(name):
        if name not in cache:
            if name.startswith("mesh"):                       # mesh8, mesh13, mesh13-hilbert, mesh13-morton
                nu, _, order = name[4:].partition("-")
                m = ga.geodesic_mesh(int(nu), reorder=order or None)
                cache[name] = ga.prepare_graph(torch.from_numpy(m.edge_index).to(DEV), m.num_nodes)
            elif name == "multi":                             # the random multigraph: long rows, a row pointer
                _, n, ei = next(c for c in graph_cases() if c[0] == "multi")
                cache[name] = ga.prepare_graph(ei.to(DEV), n)
            elif name.startswith("K"):
                n = int(name[1:])
                cache[name] = ga.prepare_graph(torch.from_numpy(ga.complete_graph(n)).to(DEV), n)
        return cache[name]
    return get


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(SEED + seed + 131 * shape[-1] + len(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case(kernel, what, launch, ins, in_lays, out_shape, out_lay):
    """One launch at the given layouts, with every check that needs no reference; the logical output, packed."""
    ar = Arena(DEV)
    ops = [ar.input(v, lay) for v, lay in zip(ins, in_lays)]
    out = ar.output(*out_shape, out_lay)
    ar.commit()
    rc = launch(*ops, out)
    assert rc == 0, (what, rc)
    ar.verify(what)
    first = out.values()
    assert bool(torch.isfinite(first).all()), what
    ar.reset()
    assert launch(*ops, out) == 0
    ar.verify(what + ", second call")
    assert same_bits(first, out.values()), what + ": the second identical call differs"
    COUNTS[kernel] += 1
    return first


def _members(*widths):
    return 2 if max(widths) >= 256 else 3


# ---------------------------------------------------------------------------------------------------------------------
# K2  gwen_gcn_propagate_f32: ldh, ldo, mstride_h, mstride_o.  Bitwise at every vector width (4: 16-byte aligned and
# everything % 4; 2: the ``even`` layout's 8-byte base; 1: ``odd``).
# ---------------------------------------------------------------------------------------------------------------------
K2_PAIRS = [(n, n) for n in ("row_pad", "member_gap", "window", "interleaved", "odd", "even")] + \
           [("interleaved", "packed"), ("packed", "interleaved"), ("even", "row_pad")]


@pytest.mark.parametrize("F", [1, 3, 4, 6, 64, 100, 256, 260])
def test_k2_propagate(L, graphs, F):
    members, ran = _members(F), 0
    for gname in ("mesh8", "mesh13", "multi"):
        g = graphs(gname)
        n = g.num_nodes
        h, b = _randn(members, n, F), _randn(F, scale=0.1)
        for bias, relu in ((None, 0), (b, 1)):
            def launch(hh, oo):
                return L.gwen_gcn_propagate_f32(_p(g.rowptr), _p(g.col), _p(g.val), hh.ptr, _p(bias), oo.ptr, n, F, hh.ld,
                                                oo.ld, members, hh.mstride, oo.mstride, relu, _st())
            packed = _case("K2", f"K2 {gname} F={F} packed", launch, [h], [layout("packed", members, n, F)],
                           (members, n, F), layout("packed", members, n, F))
            for lh, lo in K2_PAIRS:
                what = f"K2 {gname} F={F} relu={relu} h:{lh} out:{lo}"
                got = _case("K2", what, launch, [h], [layout(lh, members, n, F, k=1, j=1)], (members, n, F),
                            layout(lo, members, n, F, k=2, j=3))
                assert same_bits(got, packed), what
                ran += 1
    assert ran >= 3 * 2 * len(K2_PAIRS)


# ---------------------------------------------------------------------------------------------------------------------
# K3  gwen_gcn_linear_f32 and gwen_gcn_linear_nn_f32: ldx, ldh
# ---------------------------------------------------------------------------------------------------------------------
K3_PAIRS = [("row_pad", "row_pad"), ("window", "window"), ("row_pad", "packed"), ("packed", "window"),
            ("odd", "odd"), ("odd", "packed"), ("packed", "odd")]


def _k3_path(rows, fin, fout, exact, lx, lh):
    """The kernel gwen_gcn_linear_f32 selects (csrc/linear.hip): vector loads of x, and the tall pipeline."""
    vec = fin % 4 == 0 and lx.ld % 4 == 0 and lx.base % 4 == 0
    tall = exact != 1 and rows >= 16384 and vec and (fin in (64, 128) or (fin == 256 and exact != 2)) and \
        fout % 64 == 0 and fout <= 2048 and lh.ld % 4 == 0 and lh.base % 4 == 0 and rows * lx.ld * 4 < 2 ** 32
    return vec, tall


# (rows, Fin, Fout, contractions, what the shape is there for)
K3_SHAPES = [
    (642, 64, 64, (1, 0, 2), "vec, 64-column blocks"),
    (642, 64, 96, (1, 0, 2), "vec, 128-column blocks"),
    (129, 100, 260, (1, 0, 2), "Fin % 4 == 0 but no multiple of a tile"),
    (33, 7, 5, (1, 0, 2), "non-vec whatever the layout"),
    (125, 2048, 48, (0, 2), "split-K: ldh matters in the reduce only"),
    (16400, 64, 320, (0, 2), "tall: 256 + 64 column groups at h + c0"),
    (16400, 128, 320, (0, 2), "tall"),
    (16400, 256, 320, (0, 2), "tall on bf16x3; bf16x6 falls back to the split kernel"),
]


@pytest.mark.parametrize("rows,fin,fout,exacts,why", K3_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in K3_SHAPES])
def test_k3_linear(L, rows, fin, fout, exacts, why):
    x = _randn(1, rows, fin)
    w, b = (t.to(DEV) for t in make_params(fin, fout))
    nws = int(L.gwen_gcn_linear_workspace_floats(rows, fin, fout))
    assert (nws > 0) == (fin == 2048)
    ws = torch.empty(max(nws, 4), device=DEV)
    want = torch.relu(x[0].double() @ w.double().t() + b.double())
    ran = 0
    for exact in exacts:
        def launch(xx, hh):
            return L.gwen_gcn_linear_f32(xx.ptr, _p(w), _p(b), hh.ptr, rows, fin, fout, xx.ld, hh.ld, 1, exact,
                                         _p(ws) if nws else None, nws, _st())
        pk = layout("packed", 1, rows, fin), layout("packed", 1, rows, fout)
        packed = _case("K3", f"K3 {rows}x{fin}x{fout} exact={exact} packed", launch, [x], [pk[0]], (1, rows, fout), pk[1])
        p0 = _k3_path(rows, fin, fout, exact, *pk)
        if rows >= 16384:
            assert p0[1] == (not (fin == 256 and exact == 2)), "the tall path is not reached as the issue lists it"
        for lx, lh in K3_PAIRS:
            a, o = layout(lx, 1, rows, fin, k=2, j=1), layout(lh, 1, rows, fout, k=3, j=2)
            what = f"K3 {rows}x{fin}x{fout} exact={exact} x:{lx} h:{lh}"
            got = _case("K3", what, launch, [x], [a], (1, rows, fout), o)
            if _k3_path(rows, fin, fout, exact, a, o) == p0:
                assert same_bits(got, packed), what
            else:
                err = rel_err(got[0], want)
                print(what, "other kernel than packed, rel_err", err)
                assert err <= LINEAR_TOL[CONTRACT_NAME[exact]], (what, err)
            ran += 1
    assert ran >= len(exacts) * len(K3_PAIRS)


NN_SHAPES = [(300, 20, 48, 0), (300, 20, 50, 0), (300, 20, 48, 1), (513, 96, 130, 0), (125, 2048, 48, 0)]


@pytest.mark.parametrize("rows,k,n,woff", NN_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}+{s[3]}" for s in NN_SHAPES])
def test_k3_linear_nn(L, rows, k, n, woff):
    """wvec (16-byte loads of Wt) on: n % 4 == 0 and Wt aligned; off: n = 50, or Wt one float past alignment."""
    x = _randn(1, rows, k)
    wbuf = torch.zeros(k * n + 4, device=DEV)
    wt = wbuf[woff:woff + k * n].view(k, n)
    wt.copy_(_randn(k, n, scale=k ** -0.5))
    assert wt.data_ptr() % 16 == 4 * woff
    b = _randn(n, scale=0.1)
    nws = int(L.gwen_gcn_linear_workspace_floats(rows, k, n))
    assert (nws > 0) == (k == 2048)
    ws = torch.empty(max(nws, 4), device=DEV)
    want = torch.relu(x[0].double() @ wt.double() + b.double())
    ran = 0
    for contract in (0, 2):
        def launch(xx, hh):
            return L.gwen_gcn_linear_nn_f32(xx.ptr, _p(wt), _p(b), hh.ptr, rows, k, n, xx.ld, n, hh.ld, 1, contract,
                                            _p(ws) if nws else None, nws, _st())
        packed = _case("K3nn", f"nn {rows}x{k}x{n} packed", launch, [x], [layout("packed", 1, rows, k)], (1, rows, n),
                       layout("packed", 1, rows, n))
        assert rel_err(packed[0], want) <= LINEAR_NN_TOL[CONTRACT_NAME[contract]]
        for lx, lh in K3_PAIRS:
            a, o = layout(lx, 1, rows, k, k=1, j=2), layout(lh, 1, rows, n, k=2, j=1)
            what = f"nn {rows}x{k}x{n} contract={contract} x:{lx} h:{lh}"
            got = _case("K3nn", what, launch, [x], [a], (1, rows, n), o)
            if (k % 4 == 0 and a.ld % 4 == 0 and a.base % 4 == 0) == (k % 4 == 0):       # `vec` of the launcher
                assert same_bits(got, packed), what
            else:
                err = rel_err(got[0], want)
                print(what, "other kernel than packed, rel_err", err)
                assert err <= LINEAR_NN_TOL[CONTRACT_NAME[contract]], (what, err)
            ran += 1
    assert ran >= 2 * len(K3_PAIRS)


# ---------------------------------------------------------------------------------------------------------------------
# K4 / K5: the grouped gathers.  Configurations: uniform layout (mesh) with 7 / 8 gathered entries x gather depth x index
# mode where the launcher has them (depth 2 and records act on narrow kernels), and the row-pointer layout (multigraph).
# ---------------------------------------------------------------------------------------------------------------------
OUT_LAYS = ("row_pad", "member_gap", "window", "interleaved")


def _gather_configs(graphs, is_narrow):
    mesh = graphs("mesh8" if is_narrow else "mesh13")
    assert mesh.grouped()[0] is None and mesh.entries() == 7
    multi = graphs("multi")
    assert multi.grouped()[0] is not None
    cfg = [(mesh, e, d, im) for e in (7, 8) for d in (1, 2) for im in ((1, 2) if is_narrow else (1,))]
    return cfg + [(multi, 8, d, 1) for d in (1, 2)]


@pytest.mark.parametrize("fin,fout", [(16, 32), (32, 16), (64, 64), (128, 128), (256, 256), (64, 256), (256, 64)])
def test_k4_layer(L, graphs, fin, fout):
    members, ran = _members(fin, fout), 0
    w, b = (t.to(DEV) for t in make_params(fin, fout))
    configs = _gather_configs(graphs, fin <= 64 and fout <= 64)
    for (g, entries, depth, im), exact in itertools.product(configs, (0, 1, 2)):
        n = g.num_nodes
        gr, gc, gv = g.grouped()
        x = _randn(members, n, fin)

        def launch(xx, oo):
            assert xx.ld == fin
            return L.gwen_gcn_layer_tuned2_f32(_p(gr), _p(gc), _p(gv), xx.ptr, _p(w), _p(b), oo.ptr, n, fin, fout, fin,
                                               oo.ld, members, xx.mstride, oo.mstride, 1, exact, entries, depth, 0, im,
                                               _st())
        tag = f"K4 {fin}->{fout} exact={exact} rowptr={gr is not None} e={entries} d={depth} im={im}"
        pk = lambda f: layout("packed", members, n, f)
        packed = _case("K4", tag + " packed", launch, [x], [pk(fin)], (members, n, fout), pk(fout))
        for lx, lo in [("member_gap", lo) for lo in OUT_LAYS] + [("member_gap", "packed"), ("packed", "row_pad")]:
            what = f"{tag} x:{lx} out:{lo}"
            got = _case("K4", what, launch, [x], [layout(lx, members, n, fin, k=3)], (members, n, fout),
                        layout(lo, members, n, fout, k=1, j=2))
            assert same_bits(got, packed), what
            ran += 1
    assert ran >= len(configs) * 3 * (len(OUT_LAYS) + 1)


# (Fin, F1, F2, pre): layer + chained projection; activation-first + projection; activation-first alone
K5_FORMS = [(64, 64, 32, 0), (32, 32, 16, 0), (16, 64, 16, 0), (64, 128, 64, 0), (64, 128, 32, 0),
            (64, 32, 0, 1), (32, 64, 0, 1), (128, 64, 0, 1), (128, 128, 0, 1),
            (16, 0, 0, 1), (64, 0, 0, 1), (128, 0, 0, 1)]


@pytest.mark.parametrize("fin,f1,f2,pre", K5_FORMS, ids=["-".join(map(str, f)) for f in K5_FORMS])
def test_k5_chain(L, graphs, fin, f1, f2, pre):
    fw = f2 or f1 or fin
    members, ran, contracts = 3, 0, [c for c in (0, 2) if L.gwen_gcn_chain_supported(fin, f1, f2, pre, c)]
    assert 0 in contracts                                          # every listed form exists on bf16x3
    w1 = make_params(fin, f1)[0].to(DEV) if f1 else None
    w2 = make_params(f1, f2, seed=SEED + 1)[0].to(DEV) if f2 else None
    bias = _randn(fin if pre else f1, scale=0.1)
    configs = _gather_configs(graphs, fin <= 64 and f1 <= 64)
    for (g, entries, depth, im), contract in itertools.product(configs, contracts):
        n = g.num_nodes
        gr, gc, gv = g.grouped()
        x = _randn(members, n, fin)

        def launch(xx, oo):
            assert xx.ld == fin and oo.ld == fw
            return L.gwen_gcn_chain_tuned2_f32(_p(gr), _p(gc), _p(gv), xx.ptr, _p(w1), _p(w2), _p(bias), oo.ptr, n, fin, f1,
                                               f2, pre, 1, members, xx.mstride, oo.mstride, contract, entries, depth, 0,
                                               im, _st())
        tag = f"K5 {fin},{f1},{f2} pre={pre} contract={contract} rowptr={gr is not None} e={entries} d={depth} im={im}"
        packed = _case("K5", tag + " packed", launch, [x], [layout("packed", members, n, fin)], (members, n, fw),
                       layout("packed", members, n, fw))
        for kx, ko in ((1, 2), (5, 0), (0, 3)):                    # different gaps on the two sides; one side packed
            what = f"{tag} member_gap x:{4 * kx} out:{4 * ko}"
            got = _case("K5", what, launch, [x], [layout("member_gap", members, n, fin, k=kx)], (members, n, fw),
                        layout("member_gap", members, n, fw, k=ko))
            assert same_bits(got, packed), what
            ran += 1
    assert ran >= len(configs) * len(contracts) * 3


# ---------------------------------------------------------------------------------------------------------------------
# K8  gwen_gcn_wide_layer_f32: ldo, mstride_x, mstride_o
# ---------------------------------------------------------------------------------------------------------------------
def _k8_launch(L, tiles, w, b, n, n_src, fin, fout, members, contract):
    t_rows, t_lid, t_val, umax = tiles

    def launch(xx, oo):
        assert xx.ld == fin
        return L.gwen_gcn_wide_layer_f32(_p(t_rows), _p(t_lid), _p(t_val), xx.ptr, _p(w), _p(b), oo.ptr, n, n_src, fin,
                                         fout, oo.ld, members, xx.mstride, oo.mstride, 1, umax, contract, _st())
    return launch


@pytest.mark.parametrize("order", ["hilbert", "morton"])
@pytest.mark.parametrize("fin,fout", list(itertools.product((64, 128, 256), repeat=2)))
def test_k8_wide_layer(L, graphs, fin, fout, order):
    """hilbert: unions within 128 rows (two chunks of DMA in flight, SKEW at 256 -> 128 / 256, bf16x6 with its two-launch
    256 -> 256); morton: the 192-slot kernels of unions above 128 rows, where bf16x6 answers GWEN_ERANGE.  On this small
    mesh the morton order's largest union may itself stay within 128 rows: union_max is an upper bound the caller gives
    ("any upper bound <= GWEN_TILE_UNION is correct"), so the class is then entered with GWEN_TILE_UNION."""
    g = graphs(f"mesh13-{order}")
    n, tiles = g.num_nodes, g.tiles()
    assert n == 1692 and tiles is not None and tiles[3] <= 192
    if order == "hilbert":
        assert tiles[3] <= 128
    elif tiles[3] <= 128:
        tiles = (*tiles[:3], 192)
    members, ran, refused = _members(fin, fout), 0, 0
    w, b = (t.to(DEV) for t in make_params(fin, fout))
    x = _randn(members, n, fin)
    for contract in (0, 2, 3):
        assert L.gwen_gcn_wide_contract_supported(fin, fout, contract)
        launch = _k8_launch(L, tiles, w, b, n, n, fin, fout, members, contract)
        if contract == 2 and order == "morton":                    # refused before any launch (csrc/wide.hip)
            out = torch.zeros(members, n, fout, device=DEV)
            assert L.gwen_gcn_wide_layer_f32(_p(tiles[0]), _p(tiles[1]), _p(tiles[2]), _p(x), _p(w), _p(b), _p(out), n, n, fin,
                                             fout, fout, members, n * fin, n * fout, 1, tiles[3], 2, _st()) == ERANGE
            torch.cuda.synchronize()
            assert not bool(out.any())
            refused += 1
            continue
        tag = f"K8 {fin}->{fout} {order} contract={contract}"
        pk = lambda f: layout("packed", members, n, f)
        packed = _case("K8", tag + " packed", launch, [x], [pk(fin)], (members, n, fout), pk(fout))
        for lx, lo in [("packed", lo) for lo in OUT_LAYS] + [("member_gap", "window")]:
            what = f"{tag} x:{lx} out:{lo}"
            got = _case("K8", what, launch, [x], [layout(lx, members, n, fin, k=2)], (members, n, fout),
                        layout(lo, members, n, fout, k=1, j=1))
            assert same_bits(got, packed), what
            ran += 1
    assert refused == (order == "morton") and ran >= (3 - refused) * len(OUT_LAYS)


def test_k8_bipartite_member_gap_on_x(ga, L):
    """N_src != N (built as in test_gpu_wide.py::test_wide_bipartite): the member stride of x belongs to N_src rows."""
    from gwen_amd.g2m import grid_mesh_edges
    from gwen_amd.graph import prepare_bipartite
    m = ga.geodesic_mesh(12, reorder="morton")
    g2m_e, m2g_e = grid_mesh_edges(m)
    n_mesh, n_grid = m.num_nodes, m.faces.shape[0]
    ran = 0
    for e, n_src, n in ((g2m_e, n_grid, n_mesh), (m2g_e, n_mesh, n_grid)):
        g = prepare_bipartite(torch.from_numpy(e).to(DEV), n_src, n)
        if g.tiles() is None:
            continue
        assert n_src != n
        fin, fout, members = 64, 128, 3
        w, b = (t.to(DEV) for t in make_params(fin, fout))
        x = _randn(members, n_src, fin)
        for contract in (0, 3):
            launch = _k8_launch(L, g.tiles(), w, b, n, n_src, fin, fout, members, contract)
            packed = _case("K8", "K8 bipartite packed", launch, [x], [layout("packed", members, n_src, fin)],
                           (members, n, fout), layout("packed", members, n, fout))
            for lo in ("packed", "member_gap", "interleaved"):
                what = f"K8 bipartite {n_src}->{n} contract={contract} x:member_gap out:{lo}"
                got = _case("K8", what, launch, [x], [layout("member_gap", members, n_src, fin, k=3)], (members, n, fout),
                            layout(lo, members, n, fout, k=1))
                assert same_bits(got, packed), what
                ran += 1
    assert ran >= 2 * 3


# ---------------------------------------------------------------------------------------------------------------------
# K7  gwen_gcn_small_layer_f32: mstride_x, mstride_o
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [125, 200])
def test_k7_small_layer(L, graphs, n):
    g = graphs(f"K{n}")
    dense, members, ran = g.dense(), 3, 0
    assert int(L.gwen_gcn_small_pad(n)) == (128 if n == 125 else 256)
    for (fin, fout), contract in itertools.product(((64, 64), (2048, 64)), (0, 2)):
        assert L.gwen_gcn_small_supported(n, fin, fout, contract)
        w, b = (t.to(DEV) for t in make_params(fin, fout))
        x = _randn(members, n, fin)
        nws = int(L.gwen_gcn_small_workspace_floats(n, members, fin, fout))
        ws = torch.empty(max(nws, 4), device=DEV)

        def launch(xx, oo):
            return L.gwen_gcn_small_layer_f32(_p(dense), xx.ptr, _p(w), None, _p(b), oo.ptr, n, fin, fout, members,
                                              xx.mstride, oo.mstride, 1, _p(ws) if nws else None, nws, contract, _st())
        tag = f"K7 N={n} {fin}->{fout} contract={contract} split-K={nws > 0}"
        packed = _case("K7", tag + " packed", launch, [x], [layout("packed", members, n, fin)], (members, n, fout),
                       layout("packed", members, n, fout))
        for kx, ko in ((1, 2), (4, 0), (0, 1)):
            what = f"{tag} member_gap x:{4 * kx} out:{4 * ko}"
            got = _case("K7", what, launch, [x], [layout("member_gap", members, n, fin, k=kx)], (members, n, fout),
                        layout("member_gap", members, n, fout, k=ko))
            assert same_bits(got, packed), what
            ran += 1
    assert ran >= 2 * 2 * 3


# ---------------------------------------------------------------------------------------------------------------------
# Gradient kernels: ldg, ldx (the results are packed)
# ---------------------------------------------------------------------------------------------------------------------
GRAD_PAIRS = [(a, b) for a in ("packed", "row_pad", "window") for b in ("packed", "row_pad", "window")][1:] + [("odd", "odd")]

# (rows, Fout, Fin, contract) from test_gpu_parity.py's test_grad_weight_* lists, and the stage-1 kernel each reaches
GRAD_SHAPES = [
    (300, 64, 64, 2, "k_grad_w_lds 64 x 64 (DMA-staged); odd: k_grad_w_split"),
    (5000, 128, 128, 0, "k_grad_w_lds 128 x 128, several chunks"),
    (3000, 256, 64, 2, "k_grad_w_lds 128 x 64"),
    (2049, 128, 256, 0, "k_grad_w_lds 128 x 128, one row past a chunk"),
    (5000, 16, 32, 1, "k_grad_w_few<4>: one 32 x 32 tile"),
    (513, 64, 32, 2, "k_grad_w_few<2>: two tiles"),
    (777, 20, 48, 0, "k_grad_w_few<2>, widths that are no multiple of 4"),
    (300, 64, 64, 1, "k_grad_w: four tiles on the fp32 MFMA"),
    (40000, 48, 64, 2, "k_grad_w, many chunks"),
]


@pytest.mark.parametrize("rows,fout,fin,contract,why", GRAD_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{s[3]}" for s in GRAD_SHAPES])
def test_grad_weight(L, rows, fout, fin, contract, why):
    g = _randn(1, rows, fout, seed=1)
    x = _randn(1, rows, fin, seed=2)
    want = g[0].double().t() @ x[0].double()
    split = contract != 1 and fin % 64 == 0 and fout % 64 == 0          # `wide_grad`: the LDS-staged split kernels
    assert bool(L.gwen_gcn_grad_weight_bias_supported(fin, fout, contract)) == split
    nch = int(L.gwen_gcn_grad_weight_chunks(rows, fin, fout, contract))
    ws = torch.empty(int(L.gwen_gcn_grad_workspace_floats(rows, fin, fout)), device=DEV)
    partial_b = torch.empty(nch * fout + 4, device=DEV)

    def full(gg, xx, oo):
        return L.gwen_gcn_grad_weight_f32(gg.ptr, xx.ptr, oo.ptr, rows, fin, fout, gg.ld, xx.ld, _p(ws), contract, _st())

    def part(gg, xx, oo):
        return L.gwen_gcn_grad_weight_partial_f32(gg.ptr, xx.ptr, oo.ptr, rows, fin, fout, gg.ld, xx.ld, contract, _st())

    def part_wb(gg, xx, oo):
        return L.gwen_gcn_grad_weight_bias_partial_f32(gg.ptr, xx.ptr, oo.ptr, _p(partial_b), rows, fin, fout, gg.ld,
                                                       xx.ld, contract, _st())
    entries = [("grad_w", full, (1, fout, fin)), ("grad_w_partial", part, (1, nch, fout * fin))]
    if split:
        entries.append(("grad_wb_partial", part_wb, (1, nch, fout * fin)))
    ran = 0
    for name, launch, oshape in entries:
        pk = lambda r, f: layout("packed", 1, r, f)
        packed = _case(name, f"{name} {rows}x{fout}x{fin} packed", launch, [g, x], [pk(rows, fout), pk(rows, fin)], oshape,
                       pk(*oshape[1:]))
        packed_b = partial_b[:nch * fout].clone()
        for lg, lx in GRAD_PAIRS:
            if lg == "odd" and name == "grad_wb_partial":
                continue                       # documented refusal (GWEN_EINVAL): asserted in test_strides_host.py
            a, c = layout(lg, 1, rows, fout, k=1, j=2), layout(lx, 1, rows, fin, k=2, j=1)
            what = f"{name} {rows}x{fout}x{fin} contract={contract} g:{lg} x:{lx}"
            got = _case(name, what, launch, [g, x], [a, c], oshape, pk(*oshape[1:]))
            if lg != "odd" or not split:       # launch_grad_w's alignment test only exists on the split kernels
                assert same_bits(got, packed), what
                if name == "grad_wb_partial":
                    assert same_bits(partial_b[:nch * fout], packed_b), what
            else:
                total = got[0].double().sum(0).view(fout, fin) if name != "grad_w" else got[0]
                err = rel_err(total, want)
                print(what, "fallback kernel, rel_err", err)
                assert err <= GRAD_W_TOL[CONTRACT_NAME[contract]], (what, err)
            ran += 1
    assert ran >= 2 * len(GRAD_PAIRS)


@pytest.mark.parametrize("rows,F", [(300, 64), (5000, 100), (777, 20), (40000, 48)])
def test_grad_bias(L, rows, F):
    g = _randn(1, rows, F, seed=3)
    nch = int(L.gwen_gcn_grad_chunks(rows))
    ws = torch.empty(int(L.gwen_gcn_grad_workspace_floats(rows, F, 1)), device=DEV)

    def full(gg, oo):
        return L.gwen_gcn_grad_bias_f32(gg.ptr, oo.ptr, rows, F, gg.ld, _p(ws), _st())

    def part(gg, oo):
        return L.gwen_gcn_grad_bias_partial_f32(gg.ptr, oo.ptr, rows, F, gg.ld, _st())
    ran = 0
    for name, launch, oshape in (("grad_b", full, (1, 1, F)), ("grad_b_partial", part, (1, nch, F))):
        packed = _case(name, f"{name} {rows}x{F} packed", launch, [g], [layout("packed", 1, rows, F)], oshape,
                       layout("packed", *oshape))
        assert rel_err(packed[0].double().sum(0), g[0].double().sum(0)) <= GRAD_B_TOL
        for lg in ("row_pad", "window", "odd"):                   # one kernel whatever the alignment: bitwise
            what = f"{name} {rows}x{F} g:{lg}"
            got = _case(name, what, launch, [g], [layout(lg, 1, rows, F, k=2, j=3)], oshape, layout("packed", *oshape))
            assert same_bits(got, packed), what
            ran += 1
    assert ran >= 2 * 3


def test_zz_launched_case_counts(capsys):
    """Runs last in the file and prints the cases every kernel was launched on (a case = two launches and all checks;
    the floor of every kernel is asserted by its own test above)."""
    with capsys.disabled():
        print("\nstride cases launched per kernel:", dict(sorted(COUNTS.items())))
