"""Packed W of the narrow K4 / K5 forward (csrc/packw.hip; k_layer's and k_chain's PK): the kernels read the weight's bf16
images, cut once per weight version, instead of reading fp32 rows of W and splitting them in every wave.  The images are
cut by the arithmetic the kernels use on W, so the packed path must equal the unpacked path of the same build BIT FOR BIT
(compared as int32 patterns; x holds rows of -0.0): at every width pair, on both splits, both gather depths, both index
modes, every block size, with 7 and 8 gathered entries, for 1 and 3 members, on meshes below one gather pass up to
several blocks with a partial last one, and on a row-pointer layout with rows longer than one group.  Outputs are
pre-filled with NaN and followed by a NaN guard.  The whole stack, the staleness rule of StackForward's image cache and
the pack kernel itself (against a numpy restatement of the split) are checked below."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import SEED, random_multigraph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (16, 32, 64)
GUARD = 4096                                   # floats behind the last row
EINVAL = -1
# block_rows a width accepts through the entry points with images (0 = the library's choice): whole gather passes of
# 1024 / Fin rows; 80 rows exist at Fin = 64 only
LAYER_ROWS = {64: (0, 64, 80, 96, 112, 128), 32: (0, 64, 96, 128), 16: (0, 64, 128)}
CHAIN_ROWS = {64: (0, 64, 80, 96, 112), 32: (0, 64, 96), 16: (0, 64)}
GRAPHS = ["mesh1", "mesh3", "mesh6", "multi"]
# (fin, f1, f2, pre): every form of the widths 16 / 32 / 64 that contracts -- chained, and activation-first
CHAIN_FORMS = ([(fi, f1, f2, False) for fi in WIDTHS for f1 in WIDTHS for f2 in WIDTHS if f2 < f1] +
               [(fi, f1, 0, True) for fi in WIDTHS for f1 in WIDTHS])


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


_graphs = {}


def _graph(ga, name):
    """mesh1: N = 12 (less than one gather pass); mesh3: N = 92; mesh6: N = 362 (several blocks, a partial last one);
    multi: a random multigraph of 300 nodes with duplicate edges, self loops and an isolated node -- the row-pointer
    layout, rows of more than 8 entries (the long-row loop)."""
    if name in _graphs:
        return _graphs[name]
    if name.startswith("mesh"):
        nu = int(name[4:])
        m = ga.geodesic_mesh(nu)
        g = ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(m.edge_index.astype(np.int64))).to(DEV), m.num_nodes)
        assert g.num_nodes == 10 * nu * nu + 2
        assert g.grouped()[0] is None and g.entries() == 7
    else:
        ei = random_multigraph(300, 3000, seed=SEED, self_loops=20, dup=100, isolate=1)
        g = ga.prepare_graph(ei.to(DEV), 300)
        assert g.grouped()[0] is not None and g.entries() == 8
        assert int(np.diff(g.rowptr.cpu().numpy()).max()) > 8
    _graphs[name] = g
    return g


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _out(shape):
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), float("nan"), device=DEV)
    return buf[:numel].view(shape), buf[numel:]


def _whole(out, guard, what):
    assert torch.isfinite(out).all(), ("a row < N was not written", what)
    assert torch.isnan(guard).all(), ("written behind the last row", what)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_images = {}


def _pack(w, contract):
    """The packed images of w, cut once per (weight, contraction) of the module; NaN-guarded."""
    from gwen_amd import _lib
    key = (w.data_ptr(), contract)
    if key not in _images:
        fout, fin = w.shape
        nbytes = _lib.lib().gwen_gcn_packw_bytes(fin, fout, contract)
        assert nbytes == fin * fout * 2 * (3 if contract == _lib.CONTRACT_BF16X6 else 2)
        buf = torch.full((nbytes // 4 + 256,), float("nan"), device=DEV)
        rc = _lib.lib().gwen_gcn_packw_f32(_p(w), fin, fout, contract, _p(buf), _st())
        assert rc == 0
        assert torch.isnan(buf[nbytes // 4:]).all(), "the pack kernel wrote behind its images"
        _images[key] = (w, buf)                # w kept: its address stays taken
    return _images[key][1]


def _layer(g, x, w, b, relu, contract, depth, rows, mode, entries, wp, packed, expect=0, with_w=True):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin, fout = g.num_nodes, w.size(1), w.size(0)
    out, guard = _out((*x.shape[:-1], fout))
    rc = _lib.lib().gwen_gcn_layer_tuned3_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w) if with_w else None, _p(b), _p(out), n,
                                              fin, fout, fin, fout, m, n * fin, n * fout, int(relu), contract, entries,
                                              depth, rows, mode, _p(wp), packed, _st())
    assert rc == expect, (rc, fin, fout, contract, depth, rows, mode, entries, packed)
    return out, guard


def _chain(g, x, w1, w2, b, relu, pre, contract, depth, rows, mode, entries, w1p, w2p, packed, expect=0, with_w=True):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin = g.num_nodes, x.size(-1)
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    fw = f2 or f1 or fin
    out, guard = _out((*x.shape[:-1], fw))
    rc = _lib.lib().gwen_gcn_chain_tuned3_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w1) if with_w else None,
                                              _p(w2) if with_w else None, _p(b), _p(out), n, fin, f1, f2, int(pre),
                                              int(relu), m, n * fin, n * fw, contract, entries, depth, rows, mode,
                                              _p(w1p), _p(w2p), packed, _st())
    assert rc == expect, (rc, fin, f1, f2, pre, contract, depth, rows, mode, entries, packed)
    return out, guard


def _inputs(n, members, fin, seed=SEED):
    """Random rows; from three rows on, row 1 and the last row of every member are all -0.0."""
    g = torch.Generator().manual_seed(seed + 131 * fin + members)
    x = torch.randn(members, n, fin, generator=g)
    if n > 2:
        x[:, 1] = -0.0
        x[:, n - 1] = -0.0
        assert torch.signbit(x[:, 1]).all() and (x[:, 1] == 0).all()
    return (x[0] if members == 1 else x).contiguous().to(DEV)


_weights = {}


def _params(fin, fout, seed=0):
    key = (fin, fout, seed)
    if key not in _weights:
        g = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
        _weights[key] = ((torch.randn(fout, fin, generator=g) / fin ** 0.5).to(DEV),
                         (torch.randn(fout, generator=g) * 0.1).to(DEV))
    return _weights[key]


def _variants(g):
    """(depth, index mode, entries) a graph admits: records and 7 entries on the uniform layout only."""
    uniform = g.grouped()[0] is None
    return [(d, im, e) for d in (1, 2) for im in ((1, 2) if uniform else (1,)) for e in ((7, 8) if uniform else (8,))]


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_k4_packed_equals_split_in_kernel(ga, name, members):
    from gwen_amd import _lib
    g = _graph(ga, name)
    n = g.num_nodes
    for fin in WIDTHS:
        x = _inputs(n, members, fin)
        for fout in WIDTHS:
            w, b = _params(fin, fout)
            for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
                wp = _pack(w, contract)
                for rows in LAYER_ROWS[fin]:
                    for depth, mode, entries in _variants(g):
                        bias, relu = (rows + depth + mode + entries) % 2 == 0, (rows // 16 + depth) % 2 == 0
                        what = (name, members, fin, fout, contract, rows, depth, mode, entries, bias, relu)
                        # the kernels that split W themselves have no 80-row form: block rows change no value, so 64 serves
                        one, g1 = _layer(g, x, w, b if bias else None, relu, contract, depth, 64 if rows == 80 else rows, mode,
                                         entries, None, 1)
                        two, g2 = _layer(g, x, w, b if bias else None, relu, contract, depth, rows, mode, entries, wp, 2)
                        _whole(one, g1, what)
                        _whole(two, g2, what)
                        assert _same_bits(one, two), what


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_k5_packed_equals_split_in_kernel(ga, name, members):
    from gwen_amd import _lib
    g = _graph(ga, name)
    n = g.num_nodes
    ran = 0
    for fin, f1, f2, pre in CHAIN_FORMS:
        x = _inputs(n, members, fin)
        w1 = _params(fin, f1)[0]
        w2 = _params(f1, f2, seed=1)[0] if f2 else None
        bvec = (torch.randn(fin if pre else f1, generator=torch.Generator().manual_seed(SEED + fin + f1)) * 0.1).to(DEV)
        for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
            if not _lib.lib().gwen_gcn_chain_supported(fin, f1, f2, int(pre), contract):
                continue
            ran += 1
            w1p = _pack(w1, contract)
            w2p = _pack(w2, contract) if f2 else None
            for rows in CHAIN_ROWS[fin]:
                for depth, mode, entries in _variants(g):
                    bias, relu = (rows + depth + mode + entries) % 2 == 0, (rows // 16 + depth) % 2 == 0
                    what = (name, members, fin, f1, f2, pre, contract, rows, depth, mode, entries, bias, relu)
                    one, g1 = _chain(g, x, w1, w2, bvec if bias else None, relu, pre, contract, depth,
                                     64 if rows == 80 else rows, mode, entries, None, None, 1)
                    two, g2 = _chain(g, x, w1, w2, bvec if bias else None, relu, pre, contract, depth, rows, mode, entries,
                                     w1p, w2p, 2)
                    _whole(one, g1, what)
                    _whole(two, g2, what)
                    assert _same_bits(one, two), what
    assert ran >= 2 * (9 + 9) - 6                  # all forms on bf16x3; bf16x6 may lack a few for their LDS


def test_images_alone_suffice_and_arguments_are_checked(ga):
    """packed = 2 reads no W (NULL is accepted); packed = 0 is the mode the library names; refused calls write nothing."""
    from gwen_amd import _lib
    L = _lib.lib()
    g = _graph(ga, "mesh6")
    n = g.num_nodes
    x = _inputs(n, 1, 64)
    w, b = _params(64, 64)
    w2 = _params(64, 32, seed=1)[0]
    for c in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
        wp, w2p = _pack(w, c), _pack(w2, c)
        want, _ = _layer(g, x, w, b, True, c, 0, 0, 0, 7, None, 1)
        got, gg = _layer(g, x, w, b, True, c, 0, 0, 0, 7, wp, 2, with_w=False)
        _whole(got, gg, c)
        assert _same_bits(want, got)
        auto, _ = _layer(g, x, w, b, True, c, 0, 0, 0, 7, wp, 0)
        assert L.gwen_gcn_layer_packed_mode(64, 64, c) in (1, 2) and _same_bits(want, auto)
        want, _ = _chain(g, x, w, w2, b, True, False, c, 0, 0, 0, 7, None, None, 1)
        got, gg = _chain(g, x, w, w2, b, True, False, c, 0, 0, 0, 7, wp, w2p, 2, with_w=False)
        _whole(got, gg, c)
        assert _same_bits(want, got)
        auto, _ = _chain(g, x, w, w2, b, True, False, c, 0, 0, 0, 7, wp, w2p, 0)
        assert _same_bits(want, auto)
        for out, guard in (_layer(g, x, w, b, True, c, 0, 0, 0, 7, None, 2, expect=EINVAL),
                           _layer(g, x, w, b, True, c, 0, 0, 0, 7, wp, 3, expect=EINVAL),
                           _layer(g, x, w, b, True, _lib.CONTRACT_F32, 0, 0, 0, 7, wp, 2, expect=EINVAL),
                           _chain(g, x, w, w2, b, True, False, c, 0, 0, 0, 7, wp, None, 2, expect=EINVAL),
                           _chain(g, x, w, w2, b, True, False, c, 0, 0, 0, 7, None, w2p, 2, expect=EINVAL),
                           _chain(g, x, None, None, None, True, True, c, 0, 0, 0, 7, wp, None, 2, expect=EINVAL)):
            assert torch.isnan(out).all() and torch.isnan(guard).all()


def _c2(ga, seed=SEED):
    torch.manual_seed(seed)
    model = ga.GNNModel(ga.GNNConfig(1, 1, 64, 64, 64)).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return model


def _plan(ga, layers, g, mode):
    plan = ga.StackForward(layers, g)
    plan.packed_mode = mode
    return plan


def test_stack_packed_equals_tables_off(ga):
    """The c2 model's six layers on the nu = 6 mesh through StackForward: images read wherever they exist (2), the
    library's own tables (0) and no images at all (1) give the same bits."""
    g = _graph(ga, "mesh6")
    model = _c2(ga)
    x = _inputs(g.num_nodes, 1, 64)
    off = _plan(ga, model.stack(), g, 1)
    want = off.run(x)
    assert torch.isfinite(want).all() and off.pack_launches == 0
    on = _plan(ga, model.stack(), g, 2)
    assert [(d.fin, d.fout) for d in on.desc] == [(64, 64), (64, 32), (32, 16), (16, 32), (32, 64), (64, 64)]
    assert _same_bits(want, on.run(x)) and on.pack_launches == 6
    assert _same_bits(want, ga.StackForward(model.stack(), g).run(x))
    x3 = _inputs(g.num_nodes, 3, 64)
    assert _same_bits(off.run(x3), on.run(x3)) and on.pack_launches == 6


def test_stale_images_are_never_read(ga):
    """The images are keyed on (data_ptr, version, shape, contraction) per layer and the key is checked on every run:
    an in-place update and a replaced weight tensor are both packed again; unchanged weights launch no pack kernel."""
    g = _graph(ga, "mesh6")
    model = _c2(ga)
    x = _inputs(g.num_nodes, 1, 64)
    plan = _plan(ga, model.stack(), g, 2)
    first = plan.run(x)
    assert plan.pack_launches == 6
    assert _same_bits(first, plan.run(x)) and plan.pack_launches == 6            # nothing changed: nothing packed
    w3 = model.stack()[3][0]
    with torch.no_grad():
        w3.add_(1)
    got = plan.run(x)
    assert plan.pack_launches == 7
    assert not _same_bits(first, got)
    assert _same_bits(got, _plan(ga, model.stack(), g, 2).run(x))
    assert _same_bits(got, _plan(ga, model.stack(), g, 1).run(x))
    # a replaced weight tensor: a new plan on the same image cache (what GNNModel.forward builds per call) sees another
    # data_ptr under the layer's index and packs that layer again, and only that layer
    cache = plan._packw
    layers = model.stack()
    new_w = (torch.randn(layers[5][0].shape, generator=torch.Generator().manual_seed(SEED + 5)) * 0.1).to(DEV)
    layers[5] = (new_w, layers[5][1], layers[5][2], layers[5][3])
    shared = ga.StackForward(layers, g, packw_cache=cache)
    shared.packed_mode = 2
    got = shared.run(x)
    assert shared.pack_launches == 1
    assert _same_bits(got, _plan(ga, layers, g, 2).run(x))
    assert _same_bits(got, _plan(ga, layers, g, 1).run(x))
    assert _same_bits(got, shared.run(x)) and shared.pack_launches == 1
    again = ga.StackForward(layers, g, packw_cache=cache)
    again.packed_mode = 2
    assert _same_bits(got, again.run(x)) and again.pack_launches == 0          # the cache outlives the plan


@pytest.mark.parametrize("mode", [0, 2])
def test_graph_replay_reads_fresh_images(ga, mode):
    """A captured forward launches kernels that read the image buffers; a replay does not pass through StackForward.run.
    GraphedForward checks the keys before every replay and packs changed weights again into the same buffers: after an
    in-place update of a weight of a packed layer (layer 0: K5 64 -> 64 -> 32 in the library's own tables) the replay
    equals a fresh plan bit for bit -- with the library's tables (0) and with images everywhere (2)."""
    g = _graph(ga, "mesh6")
    model = _c2(ga)
    x = _inputs(g.num_nodes, 1, 64)
    plan = _plan(ga, model.stack(), g, mode)
    graphed = ga.GraphedForward(plan, x)
    first = graphed().clone()
    assert _same_bits(first, _plan(ga, model.stack(), g, 1).run(x))
    packs = plan.pack_launches
    assert packs == (6 if mode == 2 else 4)
    assert _same_bits(first, graphed()) and plan.pack_launches == packs         # nothing changed: nothing packed
    with torch.no_grad():
        for i in (0, 3, 5):
            model.stack()[i][0].add_(0.25)
    got = graphed().clone()
    assert plan.pack_launches == packs + (3 if mode == 2 else 2)                 # layer 3 (16 -> 32) is not in the tables
    assert not _same_bits(first, got)
    assert _same_bits(got, _plan(ga, model.stack(), g, mode).run(x))
    assert _same_bits(got, _plan(ga, model.stack(), g, 1).run(x))
    assert _same_bits(got, graphed())


def test_inference_mode_weights_are_packed_on_every_run(ga):
    """A tensor created under torch.inference_mode() has no version counter: its image is never trusted."""
    g = _graph(ga, "mesh3")
    model = _c2(ga)
    x = _inputs(g.num_nodes, 1, 64)
    want = _plan(ga, model.stack(), g, 2).run(x)
    with torch.inference_mode():
        layers = [(w.detach().clone(), b.detach().clone(), r, o) for w, b, r, o in model.stack()]
        plan = _plan(ga, layers, g, 2)
        got = plan.run(x.clone())
        assert plan.pack_launches == 6
        again = plan.run(x.clone())
        assert plan.pack_launches == 12
        assert _same_bits(want, got.clone()) and _same_bits(want, again.clone())


def _bf16_rne(x):
    """(bits uint16, value float32) of x rounded to bfloat16, round to nearest even; x float32, finite."""
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return r, (r.astype(np.uint32) << 16).view(np.float32)


def _host_images(w, ns):
    """split_images restated: im[s] = bf16(x - im[0] - .. - im[s-1]), in the kernels' fragment order
    [j][ks][s][lane][KF] with lane (mi, mh) holding W[16 j + mi][KF (4 ks + mh) .. + KF)."""
    fout, fin = w.shape
    kf = 8 if fin >= 32 else 4
    ks_n = fin // (4 * kf)
    imgs, r = [], w.copy()
    for _ in range(ns):
        bits, val = _bf16_rne(r)
        imgs.append(bits)
        r = (r - val).astype(np.float32)                     # exact in fp32
    out = np.empty((fout // 16, ks_n, ns, 64, kf), dtype=np.uint16)
    lane = np.arange(64)
    mi, mh = lane & 15, lane >> 4
    for j in range(fout // 16):
        for ks in range(ks_n):
            for s in range(ns):
                for e in range(kf):
                    out[j, ks, s, :, e] = imgs[s][16 * j + mi, kf * (4 * ks + mh) + e]
    return out.reshape(-1)


@pytest.mark.parametrize("fout,fin", [(64, 64), (32, 16)])
def test_pack_kernel_equals_host_split(ga, fout, fin):
    """Bytes of gwen_gcn_packw_f32 against the numpy restatement, on weights that hold 0, -0, subnormals, 2^+-60 and values
    exactly half-way between two bf16 numbers (ties go to the even one)."""
    from gwen_amd import _lib
    rng = np.random.default_rng(SEED + fin)
    w = rng.standard_normal((fout, fin)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-45, 2.0 ** -140, 2.0 ** 60, -2.0 ** 60, 2.0 ** -60, -2.0 ** -60,
                        1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -16,
                        1.0 + 2.0 ** -8 + 2.0 ** -17, 3.0 * 2.0 ** -134], dtype=np.float32)
    assert np.signbit(special[1]) and special[2] != 0 and special[3] != 0
    w.reshape(-1)[:special.size] = special
    w[-1, -special.size:] = special[::-1]
    wt = torch.from_numpy(w).to(DEV)
    for contract, ns in ((_lib.CONTRACT_BF16X3, 2), (_lib.CONTRACT_BF16X6, 3)):
        nbytes = _lib.lib().gwen_gcn_packw_bytes(fin, fout, contract)
        assert nbytes == fin * fout * ns * 2
        buf = torch.full((nbytes // 4 + 64,), float("nan"), device=DEV)
        assert _lib.lib().gwen_gcn_packw_f32(_p(wt), fin, fout, contract, _p(buf), _st()) == 0
        assert torch.isnan(buf[nbytes // 4:]).all()
        got = buf[:nbytes // 4].cpu().numpy().view(np.uint16)
        want = _host_images(w, ns)
        assert got.shape == want.shape and np.array_equal(got, want), (fin, fout, contract,
                                                                      np.flatnonzero(got != want)[:8])
