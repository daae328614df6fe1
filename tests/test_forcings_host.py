"""Static fields and forcings without a GPU: the fp64 restatement's astronomy, the forecaster's settings (state_dict,
pickling, defaults unchanged), the host-side time conversion, and argument checks of the C entry points."""
import ctypes
import datetime
import pickle

import numpy as np
import pytest
import torch

import forcing_ref as FR

EINVAL = -1
DEG = 180.0 / np.pi


def _days_of_2000():
    """(day number 1 .. 366, gamma) at 12:00 UTC of every day of 2000 (t = 0 is 2000-01-01 00:00)."""
    days = np.arange(366)
    return days + 1, np.array([FR.phases(int(d) * 86400 + 43200)[0] for d in days])


def test_reference_declination_equation_of_time_and_eccentricity():
    day, gamma = _days_of_2000()
    d, E, e0 = FR.spencer(gamma)
    assert 23.4 <= d.max() * DEG <= 23.5 and 171 <= day[d.argmax()] <= 173
    assert -23.5 <= d.min() * DEG <= -23.4 and 353 <= day[d.argmin()] <= 357
    minutes = E * 229.18
    assert 16.0 <= minutes.max() <= 17.0 and 300 <= day[minutes.argmax()] <= 310
    assert -15.0 <= minutes.min() <= -14.0 and 40 <= day[minutes.argmin()] <= 48
    assert day[e0.argmax()] <= 10 and 1.03 <= e0.max() <= 1.04
    assert 180 <= day[e0.argmin()] <= 192 and 0.96 <= e0.min() <= 0.97


def test_reference_phases_use_the_floor_modulus():
    g, tau = FR.phases(-1)
    assert g == pytest.approx(2 * np.pi * (FR.YEAR - 1) / FR.YEAR, rel=1e-15)
    assert tau == pytest.approx(2 * np.pi * 86399 / 86400, rel=1e-15)
    big = 10 ** 11 + 7
    assert FR.phases(big) == FR.phases(big % (FR.YEAR * 86400))       # (Y and 86400: a common period)
    assert FR.phases(0) == (0.0, 0.0)


def test_reference_sun_is_overhead_at_the_subsolar_point():
    """At 12:00 UTC minus the equation of time the sun stands over (declination, 0): mu = 1 there and 0 at the antipode."""
    t = 172 * 86400 + 43200
    gamma, tau = FR.phases(t)
    d, E, e0 = FR.spencer(gamma)
    lon = np.pi - tau - E                                            # h = 0
    f = FR.solar(t, np.array([[d, lon], [-d, lon + np.pi], [d, lon + 0.5 * np.pi]]))
    assert f[0, 0] == pytest.approx(e0, rel=1e-12) and f[1, 0] == 0.0
    assert f[2, 0] == pytest.approx(e0 * np.sin(d) ** 2, rel=1e-9)
    assert np.allclose(f[:, 1] ** 2 + f[:, 2] ** 2, 1.0) and np.allclose(f[:, 3] ** 2 + f[:, 4] ** 2, 1.0)


def _model(**kw):
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(23)
    return InteractionForecaster(6, 32, 2, **kw)


def test_forcing_settings_state_dict():
    m = _model(static_channels=3, solar=True, forcing_channels=2)
    sd = m.state_dict()
    assert tuple(sd["static_embed.weight"].shape) == (32, 3) and tuple(sd["forcing_embed.weight"].shape) == (32, 7)
    assert "static_embed.bias" not in sd and "forcing_embed.bias" not in sd
    assert float(sd["static_embed.weight"].abs().max()) > 0 and float(sd["forcing_embed.weight"].abs().max()) > 0
    base = _model()
    assert list(sd.keys()) == list(base.state_dict().keys()) + ["static_embed.weight", "forcing_embed.weight"]
    for name, t in base.state_dict().items():              # the new weights are drawn last: the rest is unchanged
        assert torch.equal(t, sd[name]), name
    assert "forcing_embed.weight" not in _model(static_channels=4).state_dict()
    assert tuple(_model(solar=True).state_dict()["forcing_embed.weight"].shape) == (32, 5)
    assert "static_embed.weight" not in _model(forcing_channels=1).state_dict()
    for bad in ({"forcing_channels": 65}, {"solar": True, "forcing_channels": 60}, {"static_channels": -1},
                {"forcing_channels": -2}):
        with pytest.raises(ValueError):
            _model(**bad)
    from gwen_amd.forecaster import InteractionForecaster
    with pytest.raises(ValueError):
        InteractionForecaster(6, 30, 2, solar=True)                 # hidden % 4


def test_default_model_is_what_it_was():
    m = _model()
    assert (m.static_channels, m.solar, m.forcing_channels) == (0, False, 0)
    assert not hasattr(m, "static_embed") and not hasattr(m, "forcing_embed")
    names = ["grid_embed", "mesh_embed", "g2m_edge_embed", "mesh_edge_embed", "m2g_edge_embed"]
    keys = list(m.state_dict().keys())
    assert keys[:10] == [f"{n}.{p}" for n in names for p in ("weight", "bias")]
    assert keys[-2:] == ["readout.weight", "readout.bias"]
    assert all(k.split(".")[0] in names + ["encoder", "processor", "decoder", "readout"] for k in keys)


def test_forcing_settings_pickle_and_older_pickles_load_as_off():
    m = _model(static_channels=3, solar=True, forcing_channels=2)
    back = pickle.loads(pickle.dumps(m))
    assert (back.static_channels, back.solar, back.forcing_channels) == (3, True, 2)
    assert torch.equal(back.forcing_embed.weight, m.forcing_embed.weight)
    old = pickle.loads(pickle.dumps(_model()))
    for k in ("static_channels", "solar", "forcing_channels"):
        del old.__dict__[k]
    old = pickle.loads(pickle.dumps(old))
    assert old._forcing_widths() == (0, 0)


def test_forecast_graphs_fields_are_optional_and_trailing():
    import dataclasses
    from gwen_amd.forecaster import ForecastGraphs
    names = [f.name for f in dataclasses.fields(ForecastGraphs)]
    assert names[-2:] == ["grid_latlon", "grid_static"]
    g = ForecastGraphs(*[None] * 7)
    assert g.grid_latlon is None and g.grid_static is None


def test_seconds_since_2000():
    from gwen_amd import forcings
    assert forcings.seconds(12345) == 12345 and forcings.seconds(-7) == -7
    assert forcings.seconds(datetime.datetime(2000, 1, 1)) == 0
    assert forcings.seconds(datetime.datetime(2000, 1, 2, 0, 0, 1)) == 86401
    assert forcings.seconds(datetime.datetime(1999, 12, 31, 23, 59, 59, tzinfo=datetime.timezone.utc)) == -1
    plus2 = datetime.timezone(datetime.timedelta(hours=2))
    assert forcings.seconds(datetime.datetime(2000, 1, 1, 2, 0, 0, tzinfo=plus2)) == 0
    assert forcings.seconds(np.datetime64("2000-01-01T00:00:00")) == 0
    assert forcings.seconds(np.datetime64("2024-02-29T06:00")) == (8825 * 86400 + 6 * 3600)
    assert forcings.seconds(np.datetime64("1999-12-31T23:59:59")) == -1
    assert forcings.seconds(datetime.datetime(3000, 1, 1)) > 2 ** 32


def test_clock_needs_a_device():
    from gwen_amd import forcings
    with pytest.raises(RuntimeError):
        forcings.ForcingClock(0, 3600, "cpu")


def test_forcing_entry_points_reject_bad_arguments(hip_lib):
    L = hip_lib
    ck, ll, gv, wf, bs, x, o = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000,
                                                            0x70000))
    null = None
    emb = L.gwen_forcing_embed_f32

    def call(clock=ck, latlon=ll, given=gv, Fg=3, w=wf, base=bs, rows=12, N=4, xx=x, H=32, out=o):
        return emb(clock, latlon, given, Fg, w, base, rows, N, xx, H, out, null)

    assert call(rows=13) == EINVAL and call(rows=2) == EINVAL                        # rows % N
    assert call(rows=-4) == EINVAL and call(N=0) == EINVAL
    for h in (0, 2, 30, 33, -4):
        assert call(H=h) == EINVAL, h                                                # H % 4
    assert call(clock=null, latlon=null, given=null, Fg=0) == EINVAL                 # width 0
    assert call(clock=null, latlon=null, Fg=65) == EINVAL                            # width 65
    assert call(Fg=60) == EINVAL                                                     # 5 + 60 = 65
    assert call(Fg=-1) == EINVAL
    assert call(latlon=null) == EINVAL                                               # a clock without latlon
    assert call(given=null) == EINVAL                                                # Fg columns of nothing
    assert call(clock=ctypes.c_void_p(0x10004)) == EINVAL
    assert call(xx=null) == EINVAL and call(out=null) == EINVAL and call(w=null) == EINVAL
    assert call(xx=ctypes.c_void_p(0x60008)) == EINVAL and call(out=ctypes.c_void_p(0x70004)) == EINVAL
    assert call(w=ctypes.c_void_p(0x40008)) == EINVAL and call(base=ctypes.c_void_p(0x50008)) == EINVAL
    sol = L.gwen_forcing_solar_f32
    assert sol(null, ll, 4, o, null) == EINVAL
    assert sol(ck, null, 4, o, null) == EINVAL                                       # a clock without latlon
    assert sol(ctypes.c_void_p(0x10004), ll, 4, o, null) == EINVAL
    assert sol(ck, ll, -1, o, null) == EINVAL and sol(ck, ll, 4, null, null) == EINVAL
    assert sol(ck, ctypes.c_void_p(0x20004), 4, o, null) == EINVAL
    adv = L.gwen_forcing_advance
    assert adv(null, 1, null) == EINVAL and adv(ctypes.c_void_p(0x10004), 1, null) == EINVAL
