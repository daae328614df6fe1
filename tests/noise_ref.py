"""Independent oracle of gwen_amd.noise: numpy.random.Philox (Philox4x64-10) blocks and fp64 Box-Muller, and the noisy
forecaster step composed from oracle.interaction_oracle (test infrastructure)."""
from __future__ import annotations

import numpy as np
import torch

M64, M256 = (1 << 64) - 1, (1 << 256) - 1
KAT_ZERO = (0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b)   # counter 0, key 0


def philox_blocks(seed: int, tag: int, node0: int, count: int, member: int, draw: int, blk: int) -> np.ndarray:
    """[count, 4] uint64: the blocks of counters (node0 + i, member, draw, blk).  numpy increments its counter BEFORE
    each block, so it is seeded with the first counter minus one; word 0 runs fastest, so consecutive nodes are
    consecutive blocks (node0 + count must not carry into the member word)."""
    ctr = (node0 | (member << 64) | (draw << 128) | (blk << 192)) & M256
    bg = np.random.Philox(key=(seed & M64) | ((tag & M64) << 64), counter=(ctr - 1) & M256)
    return bg.random_raw(4 * count).reshape(count, 4)


def box_muller(words: np.ndarray) -> np.ndarray:
    """[..., 4] uint64 -> [..., 8] float64 normals (include/gwen_hip.h, "Latent noise")."""
    lo = (words & np.uint64(0xffffffff)) >> np.uint64(8)
    hi = (words >> np.uint64(32)) >> np.uint64(8)
    u1 = (lo.astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = (hi.astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], axis=-1)
    return z.reshape(words.shape[:-1] + (8,))


def normal(seed: int, tag: int, draw: int, member: int, nodes: int, K: int) -> np.ndarray:
    """[nodes, K] float64: z(seed, tag, draw, member, n, k)."""
    nb = (K + 7) // 8
    z = np.stack([box_muller(philox_blocks(seed, tag, 0, nodes, member, draw, b)) for b in range(nb)], axis=1)
    return z.reshape(nodes, nb * 8)[:, :K]


def forecaster_step_noisy(sd: dict, grid_x, mesh_pos, g2m, mesh_ei, m2g, f_g2m, f_mesh, f_m2g, steps: int, z=None,
                          act: str = "silu", aggr: str = "sum"):
    """oracle.interaction_oracle.forecaster_step with the latent noise: vm += z Wz^T after the encoder (z [Nm, K])."""
    from oracle.interaction_oracle import _sub, interaction
    lin = lambda x, name: x @ sd[name + ".weight"].t() + sd[name + ".bias"]      # noqa: E731
    vg, vm = lin(grid_x, "grid_embed"), lin(mesh_pos, "mesh_embed")
    e_g2m, e_m, e_m2g = lin(f_g2m, "g2m_edge_embed"), lin(f_mesh, "mesh_edge_embed"), lin(f_m2g, "m2g_edge_embed")
    vm, _ = interaction(vg, vm, e_g2m, g2m, _sub(sd, "encoder."), act, aggr)
    if z is not None:
        vm = vm + z @ sd["noise_embed.weight"].t()
    for k in range(steps):
        vm, e_m = interaction(vm, vm, e_m, mesh_ei, _sub(sd, f"processor.{k}."), act, aggr)
    vg, _ = interaction(vm, vg, e_m2g, m2g, _sub(sd, "decoder."), act, aggr)
    return grid_x + lin(vg, "readout")


def graph_inputs(mesh):
    """Edge lists and edge features of the forecaster's three graphs in the caller's order, fp64."""
    from gwen_amd import g2m
    from gwen_amd.forecaster import edge_features
    a, b = g2m.grid_mesh_edges(mesh)
    cell = mesh.pos[mesh.faces].mean(axis=1)
    cell /= np.linalg.norm(cell, axis=1, keepdims=True)
    f = [torch.from_numpy(x).double() for x in (edge_features(cell, mesh.pos, a),
                                                 edge_features(mesh.pos, mesh.pos, mesh.edge_index),
                                                 edge_features(mesh.pos, cell, b))]
    return (torch.from_numpy(mesh.pos.astype(np.float32)).double(), torch.from_numpy(a),
            torch.from_numpy(mesh.edge_index), torch.from_numpy(b), *f)
