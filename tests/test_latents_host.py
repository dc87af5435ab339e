"""Host checks (no GPU) of the full-latent encode: the C entry point `glowhip_plan_bind_latents`, the oracle-side eps against the
vectors the real reference recorded (tests/golden/g11_glow_latents.npz, made by tests/golden/make_golden_latents.py), the
`Latents` container, and the per-level temperature list."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import Latents
from pytorch_glow_amd.network.model import level_eps_stds
from oracle import glow_oracle as O

import latents_oracle as LO
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "glowhip.h")


def _squeeze_plan(lib):
    d = (_lib.LayerDesc * 2)()
    d[0].kind, d[0].C, d[0].H, d[0].W = _lib.LAYER_SQUEEZE, 3, 8, 8
    d[1].kind, d[1].C, d[1].H, d[1].W = _lib.LAYER_SQUEEZE, 12, 4, 4
    h = lib.glowhip_plan_create(d, 2)
    assert h
    return ctypes.c_void_p(h)


def test_bind_latents_is_exported_and_in_the_signature_table():
    assert "glowhip_plan_bind_latents" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "glowhip_plan_bind_latents")
    assert "int glowhip_plan_bind_latents(glowhip_plan* plan, float* const* eps_out, int n_eps);" in open(HEADER).read()


def test_bind_latents_counts_on_a_squeeze_only_plan():
    lib = G.lib()
    h = _squeeze_plan(lib)
    try:
        assert lib.glowhip_plan_bind_latents(h, None, 0) == 0                       # nothing to unbind: fine
        buf = (ctypes.c_void_p * 3)(0x1000, 0x2000, 0x3000)                        # never dereferenced: the count is checked first
        assert lib.glowhip_plan_bind_latents(h, buf, 3) == -1                       # GLOWHIP_EINVAL
        msg = lib.glowhip_last_error().decode()
        assert "3 latent buffers" in msg and "0 Split2d" in msg, msg
        assert lib.glowhip_plan_bind_latents(h, None, 2) == -1
        assert "2 latent buffers" in lib.glowhip_last_error().decode()
        assert lib.glowhip_plan_bind_latents(None, None, 0) == -1
        assert lib.glowhip_plan_bind_latents(h, None, 0) == 0
    finally:
        lib.glowhip_plan_destroy(h)


def test_oracle_eps_reproduce_the_reference_recording(golden):
    """The oracle's walk gives the reference's z2 / prior / eps at every Split2d, and `flow_decode(z, eps)` its reconstruction, at
    the per-layer bar 1e-5."""
    g = golden("g11_glow_latents")
    sd, cfg = LO.g11_state(g), LO.G11
    z, _, splits = LO.flow_encode_latents(g["x"] + g["noise"], torch.zeros(4), sd, cfg)
    assert (z - g["z"]).abs().max().item() <= 1e-5
    assert len(splits) == cfg["L"] - 1
    for k, s in enumerate(splits):
        for name in ("z2", "mean", "logs", "eps"):
            assert s[name].shape == g[f"{name}_{k}"].shape
            err = (s[name] - g[f"{name}_{k}"]).abs().max().item()
            assert err <= 1e-5, f"split {k} {name}: {err:.2e}"
    assert splits[0]["eps"].shape[2] < splits[1]["eps"].shape[2], "decode order: the deepest split first"
    assert min(float(s["logs"].abs().max()) for s in splits) > 0.05, "the fixture's priors are meant to be non-trivial"
    recon = O.flow_decode(g["z"], sd, cfg, [g[f"eps_{k}"] for k in range(2)])
    assert (recon - g["recon_x"]).abs().max().item() <= 1e-5
    # and the recording is a round trip of the reference itself, inside the project's decode tolerance
    assert (g["recon_x"] - (g["x"] + g["noise"])).abs().max().item() <= 1e-4
    _, nll, _ = O.glow_forward(g["x"], g["noise"], dict(sd), cfg)
    assert (nll - g["nll"]).abs().max().item() <= 1e-5


def _latents(n=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return Latents(torch.randn(n, 48, 4, 4, generator=g), [torch.randn(n, 12, 8, 8, generator=g), torch.randn(n, 6, 16, 16, generator=g)],
                   torch.randn(n, generator=g))


def test_latents_indexing():
    lat = _latents()
    assert len(lat) == 5 and len(lat.tensors()) == 3
    one = lat[2]
    assert len(one) == 1 and torch.equal(one.z[0], lat.z[2]) and torch.equal(one.eps[1][0], lat.eps[1][2]) and torch.equal(one.nll, lat.nll[2:3])
    assert torch.equal(lat[-1].z, lat.z[4:5])
    part = lat[1:4]
    assert len(part) == 3 and all(torch.equal(a, b[1:4]) for a, b in zip(part.tensors(), lat.tensors()))
    picked = lat[[0, 3]]
    assert len(picked) == 2 and torch.equal(picked.eps[0], lat.eps[0][[0, 3]])
    with pytest.raises(IndexError):
        lat[5]
    with pytest.raises(AssertionError):
        Latents(torch.zeros(2, 4, 2, 2), [torch.zeros(3, 4, 2, 2)])


def test_latents_lerp():
    a, b = _latents(seed=1), _latents(seed=2)
    mid = a.lerp(b, 0.25)
    assert mid.nll is None
    for m, x, y in zip(mid.tensors(), a.tensors(), b.tensors()):
        assert torch.allclose(m, 0.75 * x + 0.25 * y, atol=1e-6)
    for end, t in ((a, 0.0), (b, 1.0)):      # the endpoints are the operands themselves
        assert all(torch.equal(m, x) for m, x in zip(a.lerp(b, t).tensors(), end.tensors()))
    path = a[0].lerp(b[0], torch.linspace(0, 1, 7))
    assert len(path) == 7
    assert all(torch.equal(p[0], x[0]) for p, x in zip(path.tensors(), a.tensors()))
    assert all(torch.equal(p[6], y[0]) for p, y in zip(path.tensors(), b.tensors()))
    assert torch.allclose(path.eps[1][3], 0.5 * (a.eps[1][0] + b.eps[1][0]), atol=1e-6)
    with pytest.raises(AssertionError):
        a.lerp(b, [0.0, 1.0])                # a sequence of weights blends ONE pair


def test_latents_state_dict_round_trip():
    lat = _latents()
    sd = lat.state_dict()
    assert sorted(sd) == ["eps.0", "eps.1", "nll", "z"]
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = Latents.from_state_dict(torch.load(buf))
    assert all(torch.equal(x, y) for x, y in zip(back.tensors(), lat.tensors())) and torch.equal(back.nll, lat.nll)
    no_nll = Latents.from_state_dict(Latents(lat.z, lat.eps).state_dict())
    assert no_nll.nll is None and len(no_nll.eps) == 2
    with pytest.raises(KeyError):
        Latents.from_state_dict({"eps.0": lat.eps[0]})
    with pytest.raises(KeyError):
        Latents.from_state_dict({"z": lat.z, "eps.1": lat.eps[1]})


def test_eps_std_list_validation():
    """A sequence of temperatures has one entry per level, in decode order: the top prior, then every Split2d from the deepest;
    each entry follows the reference's ``eps_std or 1.`` (network/module.py:419).  A number passes through as it is."""
    assert level_eps_stds(None, 3) == (None, [None, None])
    assert level_eps_stds(0.7, 3) == (0.7, [0.7, 0.7])
    assert level_eps_stds(np.float32(0.5), 2) == (0.5, [0.5]) and level_eps_stds(torch.tensor(0.5), 2)[1] == [torch.tensor(0.5)]
    assert level_eps_stds([0.5, 0.0, 0.25], 3) == (0.5, [1.0, 0.25])
    assert level_eps_stds((0, 1, 2), 3) == (1.0, [1.0, 2.0])
    assert level_eps_stds(torch.tensor([0.5, 0.6]), 2) == (0.5, [pytest.approx(0.6)])
    for bad in ([0.5, 0.5], [0.5] * 4, []):
        with pytest.raises(ValueError, match="L = 3"):
            level_eps_stds(bad, 3)
    # through FlowModel.draw_eps (CPU draws; the plan is only asked for its input shape)
    fm = G.FlowModel(in_shape=(16, 16, 3), hidden_channels=8, K=1, L=3)

    class Shape:
        in_chw = (3, 16, 16)

    torch.manual_seed(3)
    a = fm.draw_eps(2, Shape, [9.0, 0.5, 2.0], "cpu")
    torch.manual_seed(3)
    b = fm.draw_eps(2, Shape, None, "cpu")
    assert [tuple(e.shape) for e in a] == [(2, 12, 4, 4), (2, 6, 8, 8)]
    assert torch.equal(a[0], b[0] * 0.5) and torch.equal(a[1], b[1] * 2.0)
    torch.manual_seed(3)
    c = fm.draw_eps(2, Shape, 0.5, "cpu")
    torch.manual_seed(3)
    d = fm.draw_eps(2, Shape, [0.5] * 3, "cpu")
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    with pytest.raises(ValueError):
        fm.draw_eps(2, Shape, [0.5, 0.5], "cpu")
