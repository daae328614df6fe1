"""Independent fp64 restatement of gwen_amd.forcings (include/gwen_hip.h, "Forcings"): the solar vector in numpy with
Python's integer floor modulus, and the forecaster step with static fields and forcings composed from
oracle.interaction_oracle / the restatements of tests/test_attention.py (test infrastructure)."""
from __future__ import annotations

import numpy as np
import torch

YEAR, DAY = 31556926, 86400


def phases(t: int):
    """(gamma, tau): Python's ``%`` on ints is the floor modulus."""
    t = int(t)
    return 2.0 * np.pi * (t % YEAR) / YEAR, 2.0 * np.pi * (t % DAY) / DAY


def spencer(gamma):
    """(declination, equation of time [rad], eccentricity factor) of Spencer's series."""
    c1, s1, c2, s2, c3, s3 = (np.cos(gamma), np.sin(gamma), np.cos(2 * gamma), np.sin(2 * gamma), np.cos(3 * gamma),
                              np.sin(3 * gamma))
    d = 0.006918 - 0.399912 * c1 + 0.070257 * s1 - 0.006758 * c2 + 0.000907 * s2 - 0.002697 * c3 + 0.00148 * s3
    E = 0.000075 + 0.001868 * c1 - 0.032077 * s1 - 0.014615 * c2 - 0.040849 * s2
    e0 = 1.000110 + 0.034221 * c1 + 0.001280 * s1 + 0.000719 * c2 + 0.000077 * s2
    return d, E, e0


def solar(t: int, latlon: np.ndarray) -> np.ndarray:
    """[N, 5] float64: [e0 max(mu, 0), sin(tau + lon), cos(tau + lon), sin gamma, cos gamma] at time t."""
    ll = np.asarray(latlon, dtype=np.float64)
    lat, lon = ll[:, 0], ll[:, 1]
    gamma, tau = phases(t)
    d, E, e0 = spencer(gamma)
    h = tau + lon + E - np.pi
    mu = np.sin(lat) * np.sin(d) + np.cos(lat) * np.cos(d) * np.cos(h)
    one = np.ones_like(lat)
    return np.stack([e0 * np.maximum(mu, 0.0), np.sin(tau + lon), np.cos(tau + lon), np.sin(gamma) * one,
                     np.cos(gamma) * one], axis=1)


def latlon_of(unit: np.ndarray) -> np.ndarray:
    """[N, 2] (lat, lon) of unit vectors, as ``InteractionForecaster.prepare`` fills ``grid_latlon``."""
    u = np.asarray(unit, dtype=np.float64)
    return np.stack([np.arctan2(u[:, 2], np.hypot(u[:, 0], u[:, 1])), np.arctan2(u[:, 1], u[:, 0])], axis=1)


def embed(x, f, wf, base=None, nodes=None):
    """x + base + f wf^T in the dtype of the inputs; rows of x are members x nodes, f and base have ``nodes`` rows."""
    term = f @ wf.t()
    if base is not None:
        term = term + base
    nodes = term.size(0) if nodes is None else nodes
    return (x.view(-1, nodes, x.size(1)) + term).view_as(x)


def forcing_term(sd: dict, grid_static=None, f=None):
    """base + f Wf^T of a forecaster's state_dict: what the step adds to the grid embedding ([N, hidden])."""
    term = 0.0
    if grid_static is not None:
        term = term + grid_static @ sd["static_embed.weight"].t()
    if f is not None:
        term = term + f @ sd["forcing_embed.weight"].t()
    return term


def forecaster_step_forced(sd: dict, grid_x, mesh_pos, g2m, mesh_ei, m2g, f_g2m, f_mesh, f_m2g, steps: int,
                           grid_static=None, f=None, z=None, heads=None, act: str = "silu", aggr: str = "sum"):
    """tests/noise_ref.forecaster_step_noisy with ``vg += base + f Wf^T`` right after the grid embedding
    (grid_static [N, S], f [N, 5 solar + Fg] = [solar, given]).  ``heads``: processor="transformer"."""
    from oracle.interaction_oracle import _sub, interaction
    lin = lambda x, name: x @ sd[name + ".weight"].t() + sd[name + ".bias"]      # noqa: E731
    vg, vm = lin(grid_x, "grid_embed"), lin(mesh_pos, "mesh_embed")
    vg = vg + forcing_term(sd, grid_static, f)
    e_g2m, e_m, e_m2g = lin(f_g2m, "g2m_edge_embed"), lin(f_mesh, "mesh_edge_embed"), lin(f_m2g, "m2g_edge_embed")
    vm, _ = interaction(vg, vm, e_g2m, g2m, _sub(sd, "encoder."), act, aggr)
    if z is not None:
        vm = vm + z @ sd["noise_embed.weight"].t()
    for k in range(steps):
        if heads is None:
            vm, e_m = interaction(vm, vm, e_m, mesh_ei, _sub(sd, f"processor.{k}."), act, aggr)
        else:
            from test_attention import block_ref
            vm = block_ref(vm, vm, e_m, mesh_ei[0], mesh_ei[1], _sub(sd, f"processor.{k}."), heads, act, same=True)
    vg, _ = interaction(vm, vg, e_m2g, m2g, _sub(sd, "decoder."), act, aggr)
    return grid_x + lin(vg, "readout")
