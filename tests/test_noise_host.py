"""Latent noise without a GPU: the numpy oracle's known answer, the forecaster's noise_channels setting (state_dict,
pickling), argument checks of the C entry points, and member0 of ensemble_forecast on two gloo ranks."""
import ctypes
import os
import pickle
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from noise_ref import KAT_ZERO, box_muller, philox_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_oracle_reproduces_the_philox4x64_known_answer():
    bg = np.random.Philox(key=0, counter=(1 << 256) - 1)
    assert tuple(int(w) for w in bg.random_raw(4)) == KAT_ZERO
    assert tuple(int(w) for w in philox_blocks(0, 0, 0, 1, 0, 0, 0)[0]) == KAT_ZERO
    # consecutive nodes are consecutive counters: block 1 of a run starting at node 0 is node 1's own block
    assert np.array_equal(philox_blocks(23, 1, 0, 3, 5, 7, 2)[1:], philox_blocks(23, 1, 1, 2, 5, 7, 2))


def test_oracle_box_muller_pairs():
    w = np.array([[0, (1 << 64) - 1, 0x0123456789abcdef, 1 << 40]], dtype=np.uint64)
    z = box_muller(w)
    assert z.shape == (1, 8) and np.isfinite(z).all()
    u1 = 0.5 * 2.0 ** -24                                           # word 0: both halves 0
    assert z[0, 0] == pytest.approx(np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u1), rel=1e-15)
    assert abs(z[0, 2]) < 1e-3                                      # word 1: u = 1 - 2^-25 in both halves


def _model(**kw):
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(23)
    return InteractionForecaster(6, 32, 2, **kw)


def test_noise_channels_state_dict():
    base = _model()
    assert base.noise_channels == 0 and not hasattr(base, "noise_embed")
    for k in (8, 16, 32, 64):
        m = _model(noise_channels=k)
        keys = list(m.state_dict().keys())
        assert keys == list(base.state_dict().keys()) + ["noise_embed.weight"]
        w = m.state_dict()["noise_embed.weight"]
        assert w.shape == (32, k) and torch.count_nonzero(w) == 0
        for name, t in base.state_dict().items():          # the noise weights are drawn last: the rest is unchanged
            assert torch.equal(t, m.state_dict()[name]), name
    with pytest.raises(ValueError):
        _model(noise_channels=12)


def test_noise_channels_pickles():
    m = _model(noise_channels=16)
    back = pickle.loads(pickle.dumps(m))
    assert back.noise_channels == 16 and torch.equal(back.noise_embed.weight, m.noise_embed.weight)
    assert list(back.state_dict().keys()) == list(m.state_dict().keys())
    # a model pickled before the setting (no noise_channels attribute) runs a noisy step as K = 0:
    # tests/test_gpu_noise.py::test_model_pickled_before_noise_runs_deterministically


def test_noise_entry_points_reject_bad_arguments(hip_lib):
    L = hip_lib
    st, x, w, o = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000))
    null = None
    inj = L.gwen_noise_inject_f32
    assert inj(null, 0, 8, 4, x, w, 32, 16, o, null) == EINVAL                           # NULL state
    assert inj(ctypes.c_void_p(0x10004), 0, 8, 4, x, w, 32, 16, o, null) == EINVAL       # misaligned state
    for k in (0, 4, 12, 24, 128):
        assert inj(st, 0, 8, 4, x, w, 32, k, o, null) == EINVAL, k                       # K
    for h in (0, 2, 30, -4):
        assert inj(st, 0, 8, 4, x, w, h, 16, o, null) == EINVAL, h                       # H
    assert inj(st, 0, -1, 4, x, w, 32, 16, o, null) == EINVAL                            # rows
    assert inj(st, 0, 8, 0, x, w, 32, 16, o, null) == EINVAL                             # nodes
    assert inj(st, -1, 8, 4, x, w, 32, 16, o, null) == EINVAL                            # member0
    assert inj(st, 0, 8, 4, ctypes.c_void_p(0x20008), w, 32, 16, o, null) == EINVAL      # x not 16-byte aligned
    assert inj(st, 0, 8, 4, x, w, 32, 16, ctypes.c_void_p(0x40004), null) == EINVAL      # out not 16-byte aligned
    assert inj(st, 0, 8, 4, x, ctypes.c_void_p(0x30002), 32, 16, o, null) == EINVAL      # wz not 4-byte aligned
    assert inj(st, 0, 8, 4, null, w, 32, 16, o, null) == EINVAL
    nrm = L.gwen_noise_normal_f32
    assert nrm(null, 0, 0, 2, 3, 8, o, null) == EINVAL
    assert nrm(ctypes.c_void_p(0x10004), 0, 0, 2, 3, 8, o, null) == EINVAL
    assert nrm(st, 0, 0, 2, 3, 0, o, null) == EINVAL                                     # K >= 1
    assert nrm(st, 0, -1, 2, 3, 8, o, null) == EINVAL
    assert nrm(st, 0, 0, -1, 3, 8, o, null) == EINVAL
    assert nrm(st, 0, 0, 2, 3, 8, null, null) == EINVAL
    assert nrm(st, 0, 0, 2, 3, 8, ctypes.c_void_p(0x40002), null) == EINVAL
    assert L.gwen_noise_advance(null, 1, null) == EINVAL
    assert L.gwen_noise_advance(ctypes.c_void_p(0x10004), 1, null) == EINVAL


def test_noise_needs_a_device():
    from gwen_amd import noise
    with pytest.raises(RuntimeError):
        noise.NoiseStream(1, "cpu")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _member0_worker(rank, world, port, members, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gwen_amd.forecaster import ensemble_forecast

        class Stream:                                    # stands in for a NoiseStream: counts the draws
            draw = 0

            def advance(self, n=1):
                self.draw += n

        class Graphs:
            def batched(self, m):
                return ("batched", m)

        seen = []

        class RecordingModel:                             # records what the driver hands the step
            def _static(self, graphs):
                return graphs

            def _step(self, x, graphs, static, noise=None, member0=0):
                seen.append((graphs[1] if isinstance(graphs, tuple) else 1, member0))
                noise.advance(1)
                return x + 1.0

        n = 7
        xm = torch.zeros(3 if rank == 0 else 2, n, 2)
        stream = Stream()
        got = ensemble_forecast(RecordingModel(), Graphs(), xm, 2, members, graphed=False, noise=stream)
        batched = (list(seen), stream.draw)
        seen.clear()
        stream = Stream()
        ensemble_forecast(RecordingModel(), Graphs(), xm, 2, members, graphed=False, batched=False, noise=stream)
        seen_mbm, draw_mbm = list(seen), stream.draw
        # one member on two ranks: rank 1 holds none, and its stream still ends n_steps on
        seen.clear()
        stream = Stream()
        one = ensemble_forecast(RecordingModel(), Graphs(), xm[: 1 - rank], 2, 1, graphed=False, noise=stream)
        empty = (list(seen), stream.draw, tuple(one.shape))
        q.put((rank, batched, (list(seen_mbm), draw_mbm), tuple(got.shape), float(got.sum()), empty))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_hand_the_model_its_first_global_member():
    """5 members over 2 ranks (3 + 2): rank 0 starts at member 0, rank 1 at member 3; the member-by-member path hands
    every member its own index and leaves the stream n_steps draws on.  With 1 member, the rank without one still
    advances its stream, so both ranks keep the same draw."""
    world, members = 2, 5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_member0_worker, args=(r, world, port, members, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=180) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    (r0, b0, s0, shape0, tot0, e0), (r1, b1, s1, shape1, tot1, e1) = res
    assert e0 == ([(1, 0), (1, 0)], 2, (1, 7, 2)) and e1 == ([], 2, (1, 7, 2))
    assert b0 == ([(3, 0), (3, 0)], 2) and b1 == ([(2, 3), (2, 3)], 2)
    assert s0 == ([(1, 0), (1, 0), (1, 1), (1, 1), (1, 2), (1, 2)], 2)
    assert s1 == ([(1, 3), (1, 3), (1, 4), (1, 4)], 2)
    assert shape0 == shape1 == (5, 7, 2) and tot0 == tot1 == 5 * 7 * 2 * 2.0
