"""Host checks of the optimiser oracle (no GPU).  (1) tests/optim_oracle.py with ``exact_constants`` against torch.optim.Adam /
Adamax (foreach=False) + clip_grad_value_ + clip_grad_norm_ on float64 CPU parameters: the oracle has the reference's semantics,
independently of the kernel.  (2) A float32 restatement of the update -- `step_f32` below, one numpy operation per rounding of
csrc/optim.hip, written here and not in the oracle -- stays within `bound()` of the oracle on EVERY input set the GPU tests run
(optim_oracle.CASES, the generators are shared): no GPU case has to leave an element out.  (3) The bound is not slack: the
restatement with the weight-decay line dropped, with Adamax's `+ eps` dropped, or with the bias-corrected step size of the wrong
step leaves it."""
import math

import numpy as np
import pytest
import torch

import optim_oracle as OO

F = np.float32


def step_f32(kind, p, g, m, v, hyper, coef, mutate=None):
    """k_optim_clip_sumsq's clamp and k_optim_update's `elem` in float32 numpy, operation for operation (numpy rounds every
    operation once and contracts nothing).  Returns (stored gradient, exp_avg, exp_avg_sq / exp_inf, parameter).  ``mutate``:
    a deliberately wrong variant, for the tightness test only."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    b1, b2 = (float(b) for b in hyper["betas"])
    step = int(hyper["step"]) + (1 if mutate == "step+1" else 0)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    lr, beta2, omb1, omb2 = F(hyper["lr"]), F(b2), F(1.0 - b1), F(1.0 - b2)
    eps, wd = F(hyper["eps"]), F(hyper["weight_decay"])
    step_size, bc2_sqrt = F(float(lr) / bc1), F(math.sqrt(bc2))
    clip, max_norm = F(hyper["clip_value"]), F(hyper["max_norm"])
    with np.errstate(all="ignore"):
        if clip > 0:
            g = np.where(g < -clip, -clip, np.where(g > clip, clip, g))
        if max_norm > 0:
            g = g * F(coef)
        ge = g
        if wd != 0 and mutate != "no-wd":
            ge = ge + wd * p
        m = m + (ge - m) * omb1
        if kind == "adam":
            v = v * beta2 + omb2 * ge * ge
            denom = np.sqrt(v) / bc2_sqrt + eps
            p = p - step_size * (m / denom)
        else:
            a = v * beta2
            b = np.abs(ge) if mutate == "no-eps" else np.abs(ge) + eps
            v = np.where(a > b, a, b)
            p = p - step_size * (m / v)
    assert all(x.dtype == F for x in (g, m, v, p))
    return g, m, v, p


def test_hand_values():
    assert OO.U == 2.0 ** -24 and OO.FLOOR == 2.0 ** -126
    g = np.array([7.5, -7.5, 5.0, -5.0, -0.0, 0.0, np.nan, np.inf, -np.inf, 1.25], F)
    c = OO.clamp(g, 5.0)
    assert np.array_equal(c[[0, 1, 2, 3, 7, 8, 9]], np.array([5, -5, 5, -5, 5, -5, 1.25], F)) and np.isnan(c[6])
    assert np.signbit(c[4]) and not np.signbit(c[5]) and c.dtype == F
    assert OO.clamp(g, 0.0) is not None and np.array_equal(OO.clamp(g, 0.0)[:6], g[:6])
    assert OO.total_norm([np.array([3.0], F), np.array([0.0, -4.0], F)], 0.0) == 5.0
    assert OO.total_norm([np.array([3e19, 3e19], F)], 0.0) == math.sqrt(2.0) * float(F(3e19))          # squares overflow fp32 only
    assert OO.total_norm([np.array([30.0, -40.0], F)], 4.0) == math.sqrt(32.0)
    assert math.isnan(OO.total_norm([np.array([1.0, np.nan], F)], 5.0)) and OO.total_norm([np.array([np.inf], F)], 5.0) == 5.0
    # the coefficient: off, clamped at exactly 1, the two float32 roundings, NaN kept, inf -> 0
    assert OO.coef_from_norm(F(3.0), 0.0) == 1.0 and OO.coef_from_norm(F(50.0), 100.0) == 1.0 and OO.coef_from_norm(F(0.0), 100.0) == 1.0
    assert OO.coef_from_norm(F(100.0), 100.0) == F(100.0) / (F(100.0) + F(1e-6)) == 1.0      # 1e-6 is below half an ulp of 100
    assert OO.coef_from_norm(F(300.0), 100.0) == F(100.0) / F(300.0) and OO.coef_from_norm(F(300.0), 100.0).dtype == F
    assert np.isnan(OO.coef_from_norm(F(np.nan), 100.0)) and OO.coef_from_norm(F(np.inf), 100.0) == 0.0
    # one Adam step from zero state, by hand: m = 0.1 g, v = 1e-4 g^2 (beta2 = 0.9999), p' = p - lr * sign(g) up to eps
    h = OO.hyper("adam", 1, lr=0.5, betas=(0.9, 0.9999), eps=0.0)
    gq, m1, v1, p1 = OO.step("adam", [1.0], [2.0], [0.0], [0.0], h, 1.0, exact_constants=True)
    assert gq[0] == 2.0 and abs(m1[0] - 0.2) < 1e-15 and abs(v1[0] - 4e-4) < 1e-15 and abs(p1[0] - 0.5) < 1e-12
    h = OO.hyper("adamax", 1, lr=0.5, betas=(0.9, 0.9999), eps=0.0)
    _, m1, v1, p1 = OO.step("adamax", [1.0], [-2.0], [0.0], [0.0], h, 1.0, exact_constants=True)
    assert v1[0] == 2.0 and abs(p1[0] - 1.5) < 1e-12
    # the cases: every tensor size and every clip combination the GPU file names
    assert OO.GEOMETRY[:11] == (1, 3, 4, 5, 1020, 1024, 1028, 65535, 65536, 65537, 131076) and max(OO.GEOMETRY) == 2 * 2 ** 16 + 4
    assert len(OO.CASES) == 40 and sum(n.startswith("arith-") for n in OO.CASES) == 20


SMALL = (5, 1028, 300, 1)


@pytest.mark.parametrize("kind", OO.KINDS)
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("clip,max_norm", OO.CLIPS)
def test_oracle_is_torchs_optimiser_on_float64(kind, weight_decay, clip, max_norm):
    """Three steps of torch's single-tensor Adam / Adamax on float64 after torch's two clippings against step(exact_constants=True)
    fed torch's own previous state: every element of the gradient, both state tensors and the parameter within 1e-12 relative.
    Measured (torch CPU, the 20 combinations): worst 2.2e-13 (adam, weight_decay 0.01, (0, 100)), 2.9e-16 .. 7e-14 elsewhere --
    the operations are the same ones in the same order, so what is left is a few fp64 roundings, largest (relative to the
    result) presumably where g * coef + wd * p cancels."""
    rs = np.random.RandomState(7)
    ps = [torch.nn.Parameter(torch.from_numpy(0.1 * rs.randn(n))) for n in SMALL]
    cls = torch.optim.Adam if kind == "adam" else torch.optim.Adamax
    args = dict(lr=1e-3 if kind == "adam" else 2e-3, betas=OO.BETAS, eps=1e-8, weight_decay=weight_decay, foreach=False)
    opt = cls(ps, **args)
    second = "exp_avg_sq" if kind == "adam" else "exp_inf"
    worst = 0.0
    for step in (1, 2, 3):
        g32 = OO.grads(SMALL, step, seed=3)
        for p, g in zip(ps, g32):
            p.grad = torch.from_numpy(g.astype(np.float64))
        before = [(p.detach().numpy().copy(),
                   opt.state[p]["exp_avg"].numpy().copy() if step > 1 else np.zeros(p.numel()),
                   opt.state[p][second].numpy().copy() if step > 1 else np.zeros(p.numel())) for p in ps]
        if clip > 0:
            torch.nn.utils.clip_grad_value_(ps, clip, foreach=False)
        coef = 1.0
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
            ref_norm = OO.total_norm(g32, clip)
            assert abs(norm - ref_norm) <= 1e-14 * ref_norm
            coef = min(max_norm / (norm + 1e-6), 1.0)
            assert (coef == 1.0) == (max_norm == 1e6)
        opt.step()
        h = dict(args, step=step, clip_value=clip, max_norm=max_norm)
        for p, g, (p0, m0, v0) in zip(ps, g32, before):
            ref = OO.step(kind, p0, g, m0, v0, h, coef, exact_constants=True)
            got = (p.grad.numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p][second].numpy(), p.detach().numpy())
            for name, a, b in zip("gmvp", got, ref):
                err = np.abs(a - b)
                assert np.all(err <= 1e-12 * np.abs(a)), (step, name, float(err.max()))
                nz = a != 0
                if nz.any():
                    worst = max(worst, float((err[nz] / np.abs(a[nz])).max()))
    print(f"oracle vs torch float64 {kind} wd={weight_decay} clip=({clip}, {max_norm}): worst relative difference {worst:.2e}")


def _run_case(case, mutate=None):
    """The case's steps with the float32 restatement carrying the state; per step the restatement against the oracle in units of
    the bound.  Returns the worst multiple per output (g, m, v, p)."""
    p = OO.cat(case.params())
    m, v = np.zeros_like(p), np.zeros_like(p)
    worst = np.zeros(4)
    for step in case.steps:
        grads = case.grads(step)
        g, h = OO.cat(grads), case.hyper(step)
        norm = F(OO.total_norm(grads, case.clip_value))
        assert np.isfinite(norm)
        coef = OO.coef_from_norm(norm, case.max_norm)
        ref, E = OO.step(case.kind, p, g, m, v, h, coef), OO.bound(case.kind, p, g, m, v, h, coef)
        assert all(np.isfinite(r).all() for r in ref) and all(np.isfinite(e).all() for e in E), (case.name, step)
        got = step_f32(case.kind, p, g, m, v, h, coef, mutate=mutate)
        worst = np.maximum(worst, [OO.worst_multiple(a, b, e) for a, b, e in zip(got, ref, E)])
        if case.max_norm == 0:
            assert np.array_equal(got[0].view(np.uint32), OO.clamp(g, case.clip_value).view(np.uint32))
        _, m, v, p = step_f32(case.kind, p, g, m, v, h, coef)
    return worst


@pytest.mark.parametrize("name", list(OO.CASES))
def test_float32_restatement_stays_within_the_bound(name):
    """Every input set of tests/test_gpu_optim.py (state carried by the restatement itself, the coefficient from the float of the
    fp64 norm): the oracle is finite on every element and the float32 arithmetic lies within bound() of it, so a device result
    outside the bound is a device that does not do this arithmetic."""
    worst = _run_case(OO.CASES[name])
    print(f"{name}: float32 restatement, worst multiple of the bound  g {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}  p {worst[3]:.3f}")
    assert (worst <= 1.0).all(), (name, worst)


@pytest.mark.parametrize("kind,mutate,case", [("adam", "no-wd", "many130-adam"), ("adamax", "no-wd", "many130-adamax"),
                                              ("adamax", "no-eps", "many130-adamax"), ("adam", "step+1", "many130-adam")])
def test_bound_is_not_slack(kind, mutate, case):
    """A restatement that is wrong in one line leaves the bound by a wide margin on the SMALL 130-tensor list already."""
    worst = _run_case(OO.CASES[case], mutate=mutate)
    print(f"{case} with {mutate}: worst multiples {worst}")
    assert worst.max() > 10.0, (mutate, worst)
