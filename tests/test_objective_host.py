"""Host-only: the expectations of tests/test_gpu_objective.py come from the oracle, not from the code under test.  Every input of
that file keeps the fp32 CPU reference finite, and every case falls in the class of the accumulator's documented range
(tests/objective_oracle.py: fine / coarse / beyond) that the GPU test asserts."""
import pytest
import torch

from oracle import glow_oracle as O

import objective_oracle as OO


def _ref32(mean, logs, x):
    z = torch.zeros_like(x)
    return O.gaussian_logp(z if mean is None else mean, z if logs is None else logs, x)


@pytest.mark.parametrize("shape", OO.SHAPES, ids=str)
def test_shape_cases_are_ordinary(shape):
    x, mean, logs, inp = OO.logp_case(shape)
    for args in OO.ARGS:
        m, l = OO.pick(args, mean, logs)
        ref = _ref32(m, l, x)
        assert ref.shape == (shape[0],) and bool(torch.isfinite(ref).all())
        assert set(OO.classify(OO.partials64(m, l, x))) == {"fine"}
        assert float(OO.bar(m, l, x, inp).max()) < 2e-2, "the bar must stay far below one element (~1.4 nats): a dropped one shows"


@pytest.mark.parametrize("name", list(OO.RANGE_CASES))
def test_range_cases_are_what_the_gpu_test_says(name):
    n, i, what, cls, beyond = OO.RANGE_CASES[name]
    x, mean, logs, x0, ii = OO.range_case(name)
    assert ii == i and x.shape == (n, 4, 16, 16) and float(mean[i].abs().max()) == 0.0 and float(logs[i].abs().max()) == 0.0
    ref32, ref64 = _ref32(mean, logs, x), OO.logp64(mean, logs, x)
    assert bool(torch.isfinite(ref32).all()), "the fp32 reference itself must stay finite"
    rel32 = float(((ref32.double() - ref64) / ref64).abs().max())
    print(f"{name} ({what}): fp64 {float(ref64[i]):.6e}, fp32 reference {rel32:.1e} relative from it")
    assert rel32 <= OO.REL / 5, "the bar must leave room over the reference's own error"
    classes = OO.classify(OO.partials64(mean, logs, x))
    assert classes[i] == cls and all(c == "fine" for k, c in enumerate(classes) if k != i), classes
    assert (abs(float(ref64[i])) > 1.01 * OO.FINE_RANGE) == beyond and (beyond or abs(float(ref64[i])) < 0.99 * OO.FINE_RANGE)
    others = [k for k in range(n) if k != i]
    assert torch.equal(x[others], x0[others]) and set(OO.classify(OO.partials64(mean, logs, x0))) == {"fine"}
    if name == "b":      # the figures of the issue: -4 608 000 941 in fp64, partials of -1.152e9
        assert abs(float(ref64[i]) + 4608000941.0) < 1.0
        assert bool((OO.partials64(mean, logs, x)[i] + 1.152e9).abs().max() < 1e6)
    if name == "c":
        assert abs(float(ref64[i]) + 1.999e9) < 1e6


@pytest.mark.parametrize("route,c,h,w", OO.SPLIT_ROUTES)
def test_split_route_cases_stay_in_the_coarse_range(route, c, h, w):
    sd, x, x0 = OO.split_case(c, h, w)
    with torch.no_grad():
        _, ld32 = O.split2d(x, torch.zeros(OO.SPLIT_N), sd, "", reverse=False)
        mean, logs, z2 = OO.split_prior64(sd, x)
        m0, l0, _ = OO.split_prior64(sd, x0)
    assert bool(torch.isfinite(ld32).all())
    assert torch.equal(mean, m0) and torch.equal(logs, l0), "z2 must not feed the prior"
    want, mag = OO.logp64(mean, logs, z2), OO.abs_terms64(mean, logs, z2)
    rel32 = float(((ld32.double() - want) / want).abs().max())
    print(f"{route} ({c}, {h}, {w}): fp64 {want.tolist()}, fp32 reference {rel32:.1e} relative")
    assert rel32 <= OO.REL / 2
    i = OO.SPLIT_I
    # whatever elements a workgroup owns: the one holding the 1e6 element exceeds 2^31 on its own, none can reach 2^43
    assert float(OO.terms64(mean, logs, z2)[i].abs().max()) > 2 * OO.FINE_RANGE and float(mag[i]) < OO.COARSE_MAX / 2
    assert all(float(mag[k]) < 1e6 for k in range(OO.SPLIT_N) if k != i)      # ordinary: three decades inside the Q31.32 word


def test_head_case_has_a_finite_reference_in_the_coarse_range():
    cfg, sd, x, yo = OO.head_case()
    assert bool(torch.isfinite(x).all())
    z32, nll32 = OO.forward64(x, torch.zeros_like(x), sd, cfg, yo, dtype=torch.float32)
    z64, nll64 = OO.forward64(x, torch.zeros_like(x), sd, cfg, yo)
    assert bool(torch.isfinite(nll32).all()) and bool(torch.isfinite(nll64).all())
    rel32 = float(((nll32.double() - nll64) / nll64).abs().max())
    print(f"head case: nll fp64 {nll64.tolist()}, fp32 reference {rel32:.1e} relative, top latent max {float(z64[1].abs().max()):.6e}")
    assert rel32 <= OO.REL / 2
    assert float(z64[1].abs().max()) > 0.99e6 and float(z64[[0, 2, 3]].abs().max()) < 10.0
    n = OO.nats(nll64, x)
    assert OO.FINE_RANGE * 2 < float(n[1]) < OO.COARSE_MAX / 2 and float(n[[0, 2, 3]].max()) < 1e5


def test_scaled_pixels_have_a_finite_reference_in_the_coarse_range():
    cfg, sd, x, noise = OO.scaled_case()
    _, nll32 = OO.forward64(x, noise, sd, cfg, dtype=torch.float32)
    _, nll64 = OO.forward64(x, noise, sd, cfg)
    assert bool(torch.isfinite(nll32).all()) and bool(torch.isfinite(nll64).all())
    rel32 = float(((nll32.double() - nll64) / nll64).abs().max())
    print(f"pixels x 1e4: nll fp64 {nll64.tolist()}, fp32 reference {rel32:.1e} relative")
    assert rel32 <= OO.REL / 2
    n = OO.nats(nll64, x)
    assert bool((n > 2 * OO.FINE_RANGE).all()) and bool((n < OO.COARSE_MAX / 2).all())
