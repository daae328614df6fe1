"""fp64 restatements of gwen_amd.sfno: the spectral convolution in numpy (a loop over degrees), its gradients, and a torch
fp64 CPU model on a dense basis ``Y [N, T]`` (tests/sht_ref.py's synthesis of the identity), so that autograd gives the
gradients of the whole SFNO.  Analysis is ``(Y * q)^T x``, synthesis ``Y c``."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402


def spectral_conv(coef, w):
    """coef [B, T, Cin], w [lmax + 1, Cin, Cout] -> [B, T, Cout]: rows l^2 .. l^2 + 2l times w[l]."""
    coef, w = np.asarray(coef, dtype=np.float64), np.asarray(w, dtype=np.float64)
    out = np.empty(coef.shape[:-1] + (w.shape[2],))
    for l in range(w.shape[0]):
        out[:, l * l:(l + 1) ** 2] = coef[:, l * l:(l + 1) ** 2] @ w[l]
    return out


def spectral_conv_per_m(coef, w):
    """The map the layer must NOT be: a weight of its own for every (l, m), w [T, Cin, Cout]."""
    return np.einsum("btc,tcd->btd", np.asarray(coef, dtype=np.float64), np.asarray(w, dtype=np.float64))


def spectral_conv_grads(coef, w, r):
    """Gradients of ``(spectral_conv(coef, w) * r).sum()``: (g_coef [B, T, Cin], g_w [lmax + 1, Cin, Cout])."""
    coef, w, r = (np.asarray(a, dtype=np.float64) for a in (coef, w, r))
    g_coef, g_w = np.empty_like(coef), np.empty_like(w)
    for l in range(w.shape[0]):
        rows = slice(l * l, (l + 1) ** 2)
        g_coef[:, rows] = r[:, rows] @ w[l].T
        g_w[l] = np.einsum("bjc,bjd->cd", coef[:, rows], r[:, rows])
    return g_coef, g_w


def basis(grid, nlat, nlon, lmax):
    """(Y [N, T], q [N]): every harmonic on the grid, and the points' quadrature weights."""
    t = (lmax + 1) ** 2
    y = R.synthesis(np.eye(t)[None], grid, nlat, nlon, lmax)[0]
    return y, R.point_weights(grid, nlat, nlon)


def layer(x, w, grid, nlat, nlon, lmax, per_m=False):
    """synthesis(conv(analysis(x))) in numpy: x [B, N, Cin] -> [B, N, Cout]."""
    c = R.analysis(x, grid, nlat, nlon, lmax)
    c = spectral_conv_per_m(c, w) if per_m else spectral_conv(c, w)
    return R.synthesis(c, grid, nlat, nlon, lmax)


def roll(x, nlat, nlon, shift):
    """The field turned by ``shift`` longitudes: x [B, nlat * nlon, C]."""
    b, _, c = x.shape
    return np.roll(x.reshape(b, nlat, nlon, c), shift, axis=2).reshape(b, nlat * nlon, c)


class RefBlock(nn.Module):
    def __init__(self, lmax, channels, mlp_ratio, activation, layer_norm):
        super().__init__()
        self.conv = nn.Module()
        self.conv.weight = nn.Parameter(torch.zeros(lmax + 1, channels, channels, dtype=torch.float64))
        self.norm1 = nn.LayerNorm(channels, dtype=torch.float64) if layer_norm else None
        self.norm2 = nn.LayerNorm(channels, dtype=torch.float64) if layer_norm else None
        self.skip = nn.Linear(channels, channels, bias=False, dtype=torch.float64)
        act = {"none": nn.Identity, "relu": nn.ReLU, "silu": nn.SiLU}[activation]()
        self.mlp = nn.Sequential(nn.Linear(channels, mlp_ratio * channels, dtype=torch.float64), act,
                                 nn.Linear(mlp_ratio * channels, channels, dtype=torch.float64))

    def forward(self, x, y, yq, deg):
        n = x if self.norm1 is None else self.norm1(x)
        c = torch.einsum("nt,...nc->...tc", yq, n)
        c = torch.einsum("...tc,tcd->...td", c, self.conv.weight[deg])
        h = x + torch.einsum("nt,...tc->...nc", y, c) + self.skip(n)
        return h + self.mlp(h if self.norm2 is None else self.norm2(h))


class RefSFNO(nn.Module):
    """gwen_amd.SFNO in torch fp64 on the CPU with the same ``state_dict`` names."""

    def __init__(self, grid, nlat, nlon, lmax, in_channels, out_channels, channels, blocks, mlp_ratio=2,
                 activation="silu", layer_norm=True, residual=False):
        super().__init__()
        y, q = basis(grid, nlat, nlon, lmax)
        self.y = torch.from_numpy(y)
        self.yq = torch.from_numpy(y * q[:, None])
        self.deg = torch.from_numpy(R.degrees(lmax))
        self.out_channels, self.residual = out_channels, residual
        self.encoder = nn.Linear(in_channels, channels, dtype=torch.float64)
        self.blocks = nn.ModuleList(RefBlock(lmax, channels, mlp_ratio, activation, layer_norm) for _ in range(blocks))
        self.decoder = nn.Linear(channels, out_channels, dtype=torch.float64)

    def forward(self, x):
        h = self.encoder(x)
        for b in self.blocks:
            h = b(h, self.y, self.yq, self.deg)
        out = self.decoder(h)
        return out + x[..., :self.out_channels] if self.residual else out
