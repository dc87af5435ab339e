"""The Polyak average of the weights inside the HIP optimiser step (csrc/optim.hip: the EMA instance of k_optim_update,
k_optim_ema_swap; training.HipAdam / HipAdamax with ``ema_decay``) on synthetic parameters, no model: the average must not
perturb the update, must follow the fp64 recurrence of tests/ema_oracle.py within the bound derived there, the device form must
equal the argument form, a skipped step must skip the average, the swap must be an exact in-place exchange, and the state must
round-trip.  Shapes: n % 4 != 0, a 2^16 chunk boundary with a short tail, three chunks, a parameter whose address is not a
multiple of 16 (element-by-element path) and one without a gradient (no chunk)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib, training  # noqa: E402

import ema_oracle as EO  # noqa: E402

DEV = "cuda:0"
SHAPES = [(7,), (1,), (48, 48), (65540,), (131075,)]
OFFSET_N = 1028          # a multiple of 4: only its ADDRESS keeps this parameter off the 16-byte path
FROZEN = (33,)
ARGS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
T = 5


def make_params(seed=11):
    """The five shapes, then a view one float into a larger buffer, then a parameter that never gets a gradient."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(DEV)) for s in SHAPES]
    big = (torch.randn(OFFSET_N + 4, generator=g) * 0.1).to(DEV)
    ps.append(torch.nn.Parameter(big[1:1 + OFFSET_N]))
    assert ps[-1].data_ptr() % 16 == 4 and ps[-1].is_contiguous()
    ps.append(torch.nn.Parameter((torch.randn(FROZEN, generator=g) * 0.1).to(DEV)))
    return ps


def grads_for(step, poison=False):
    """The gradients of one step (the same for every optimiser that runs it); step 2 is large enough for both clippings to bite."""
    g = torch.Generator().manual_seed(1000 + step)
    out = [torch.randn(p, generator=g) * (10.0 if step == 2 else 0.5) for p in SHAPES + [(OFFSET_N,)]]
    if poison:
        out[3][65537] = float("inf")
    return out


def set_grads(ps, step, poison=False):
    for p, gr in zip(ps, grads_for(step, poison)):      # (the last parameter stays without one)
        p.grad = gr.to(DEV)


def make(kind, **ema):
    ps = make_params()
    cls = training.HipAdam if kind == "adam" else training.HipAdamax
    return ps, cls(ps, **ARGS, **ema)


def snapshot(ps, opt, with_ema=True):
    names = ["exp_avg", opt.SECOND] + (["ema"] if with_ema else [])
    return ([p.detach().clone() for p in ps], [[opt.state[p][n].clone() for n in names] for p in ps])


def assert_same(a, b, what=""):
    (pa, sa), (pb, sb) = a, b
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x, y), (what, "param", i)
    for i, (x, y) in enumerate(zip(sa, sb)):
        for j, (u, v) in enumerate(zip(x, y)):
            assert torch.equal(u, v), (what, "state", i, j)


@pytest.mark.parametrize("kind", ["adam", "adamax"])
def test_ema_does_not_perturb_the_update(kind):
    """Same gradients, clipping 5.0 / 100.0, five steps, with and without the average: parameters, both state tensors, the clipped
    gradients and the returned norm are the same bits -- the EMA instance of the kernel only ADDS the average."""
    pa, oa = make(kind, ema_decay=0.9)
    pb, ob = make(kind)
    for step in range(T):
        set_grads(pa, step); set_grads(pb, step)
        na, nb = oa.fused_step(5.0, 100.0), ob.fused_step(5.0, 100.0)
        assert torch.equal(na, nb) and torch.isfinite(na), step
        assert_same(snapshot(pa, oa, False), snapshot(pb, ob, False), step)
        for i, (p, q) in enumerate(zip(pa[:-1], pb[:-1])):
            assert torch.equal(p.grad, q.grad), (step, i)
    assert all("ema" in oa.state[p] for p in pa) and not any("ema" in ob.state[p] for p in pb)
    assert "ema_updates" not in ob.state_dict()["param_groups"][0]


def _run_against_oracle(kind, decay, warmup, poison_at=None, clip=5.0):
    """T calls; the oracle advances an fp64 average from the device's own p' and its own w after every APPLIED step.  ``clip``: the
    value clipping -- it clamps an inf to the threshold, so the skip test runs without it.  Returns (optimiser, parameters,
    [oracle average], [M], applied)."""
    ps, opt = make(kind, ema_decay=decay, ema_warmup=warmup)
    e64 = [p.detach().cpu().double().numpy() for p in ps]                # the average starts as the parameters of the first step
    M = [float(np.abs(e).max()) for e in e64]
    frozen0 = ps[-1].detach().clone()
    applied = 0
    for step in range(T):
        poison = step == poison_at
        set_grads(ps, step, poison)
        before = snapshot(ps, opt) if (poison and step > 0) else None
        w_host = opt.ema_weight(opt.ema_updates)
        w = EO.weight_at(applied, decay, warmup)
        assert w_host == w, (step, w_host, w)                            # the optimiser's policy is the oracle's rule
        norm = opt.fused_step(clip, 100.0, skip_nonfinite=poison_at is not None)
        if poison:
            assert not torch.isfinite(norm)
            assert_same(snapshot(ps, opt), before, "skipped step")      # parameters, state AND the average: bitwise untouched
            opt.undo_step()
            assert opt.ema_updates == applied and opt._steps == applied
            assert opt.ema_weight(opt.ema_updates) == EO.weight_at(applied, decay, warmup)
            continue
        for i, p in enumerate(ps[:-1]):
            p_new = p.detach().cpu().double().numpy()
            e64[i] = EO.advance(e64[i], p_new, w)
            M[i] = max(M[i], float(np.abs(p_new).max()), float(opt.state[p]["ema"].abs().max()))
        applied += 1
    assert opt.ema_updates == applied
    assert torch.equal(ps[-1].detach(), frozen0) and torch.equal(opt.state[ps[-1]]["ema"], frozen0)      # no gradient: no chunk
    return opt, ps, e64, M, applied


def _assert_within_bound(opt, ps, e64, M, applied):
    for i, p in enumerate(ps[:-1]):
        err = np.abs(opt.state[p]["ema"].cpu().double().numpy() - e64[i]).max()
        lim = EO.bound(applied, M[i])
        print(f"param {i} shape {tuple(p.shape)}: max |ema - oracle| = {err:.3e}, bound {lim:.3e} (M = {M[i]:.3f})")
        assert err <= lim, (i, tuple(p.shape), err, lim)


@pytest.mark.parametrize("kind", ["adam", "adamax"])
@pytest.mark.parametrize("decay,warmup", [(0.5, False), (0.9, False), (0.999, True)])
def test_ema_follows_the_fp64_recurrence(kind, decay, warmup):
    """e' = e + (p' - e) * w on the device against the fp64 oracle driven by the device's own p' and the same float w: every
    element within 5 T 2^-24 M after T = 5 steps (tests/ema_oracle.py: three roundings per update, old error contracts).  The
    pre-update p, a wrong w or a missed tail element is off by more than 100 times that."""
    opt, ps, e64, M, applied = _run_against_oracle(kind, decay, warmup)
    assert applied == T
    _assert_within_bound(opt, ps, e64, M, applied)


@pytest.mark.parametrize("kind", ["adam", "adamax"])
def test_device_form_equals_argument_form(kind):
    """fused_step(hyper_dev = 4 doubles: hyper_values + ema_weight) -- what a captured step replays -- against the argument form
    over five steps with a learning rate that changes every step: parameters, state and average bitwise equal."""
    pa, oa = make(kind, ema_decay=0.9, ema_warmup=True)
    pb, ob = make(kind, ema_decay=0.9, ema_warmup=True)
    hyper = torch.zeros(4, dtype=torch.float64, device=DEV)
    for step in range(T):
        lr = 1e-3 * (1.0 + 0.25 * step)
        for o in (oa, ob):
            o.param_groups[0]["lr"] = lr
        set_grads(pa, step); set_grads(pb, step)
        na = oa.fused_step(5.0, 100.0)
        values = ob.hyper_values(lr, ob._steps + 1) + (ob.ema_weight(ob.ema_updates),)
        assert len(ob.hyper_values(lr, 1)) == 3
        hyper.copy_(torch.tensor(values, dtype=torch.float64))
        nb = ob.fused_step(5.0, 100.0, hyper_dev=hyper)
        assert torch.equal(na, nb), step
        assert_same(snapshot(pa, oa), snapshot(pb, ob), step)
    assert oa.ema_updates == ob.ema_updates == T
    with pytest.raises(_lib.GlowHipError):       # three words are the form without an average
        ob.fused_step(5.0, 100.0, hyper_dev=hyper[:3])


@pytest.mark.parametrize("kind", ["adam", "adamax"])
def test_skipped_step_leaves_the_average_alone(kind):
    """An inf in one gradient at the third step under skip_nonfinite: the device leaves the average untouched with parameters and
    state; after undo_step() the next w is the warm-up value of the count that was not advanced; the final average is the
    oracle's over the four applied steps."""
    opt, ps, e64, M, applied = _run_against_oracle(kind, 0.999, True, poison_at=2, clip=0.0)
    assert applied == T - 1
    _assert_within_bound(opt, ps, e64, M, applied)


def test_swap_is_an_exact_in_place_exchange():
    ps, opt = make("adam", ema_decay=0.9)
    for step in range(3):
        set_grads(ps, step)
        opt.fused_step(5.0, 100.0)
    p_old = [p.detach().clone() for p in ps]
    e_old = [opt.state[p]["ema"].clone() for p in ps]
    assert not any(torch.equal(a, b) for a, b in zip(p_old[:-1], e_old[:-1]))
    ptrs, versions, steps = [p.data_ptr() for p in ps], [p._version for p in ps], opt._steps

    def holds(now_p, now_e):
        for i, p in enumerate(ps[:-1]):
            assert torch.equal(p.detach(), now_p[i]) and torch.equal(opt.state[p]["ema"], now_e[i]), i
        assert torch.equal(ps[-1].detach(), p_old[-1]) and torch.equal(opt.state[ps[-1]]["ema"], e_old[-1])      # no gradient: left alone
        assert [p.data_ptr() for p in ps] == ptrs

    opt.swap_averaged()
    assert opt.swapped
    holds(e_old, p_old)
    assert all(p._version > v for p, v in zip(ps[:-1], versions))
    with pytest.raises(_lib.GlowHipError):
        opt.fused_step(5.0, 100.0)
    assert opt._steps == steps and opt.ema_updates == steps
    holds(e_old, p_old)
    opt.swap_averaged()
    assert not opt.swapped
    holds(p_old, e_old)

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with training.averaged_weights(opt):
            holds(e_old, p_old)
            raise Boom()
    assert not opt.swapped
    holds(p_old, e_old)
    set_grads(ps, 3)
    assert torch.isfinite(opt.fused_step(5.0, 100.0))      # and training goes on


@pytest.mark.parametrize("kind", ["adam", "adamax"])
def test_state_round_trip_rehomes_the_average(kind):
    """load_state_dict(state_dict()) mid-run moves exp_avg / exp_avg_sq AND the average into fresh flat buffers; with the gradients
    written in place (same addresses) the next steps must continue bitwise equal to a twin that was never interrupted."""
    pa, oa = make(kind, ema_decay=0.9, ema_warmup=True)
    pb, ob = make(kind, ema_decay=0.9, ema_warmup=True)
    for ps in (pa, pb):
        for p in ps[:-1]:
            p.grad = torch.zeros_like(p)
    for step in range(4):
        for ps in (pa, pb):
            for p, gr in zip(ps, grads_for(step)):
                p.grad.copy_(gr.to(DEV))
        oa.fused_step(5.0, 100.0); ob.fused_step(5.0, 100.0)
        if step == 1:
            old = oa.state[pa[0]]["ema"].data_ptr()
            oa.load_state_dict(oa.state_dict())
            assert oa.ema_updates == ob.ema_updates == 2 and oa.state[pa[0]]["ema"].data_ptr() != old
        assert_same(snapshot(pa, oa), snapshot(pb, ob), step)


def test_states_with_and_without_an_average_load():
    """A state without "ema" into an EMA optimiser: the average starts at the current parameters, its count at 0.  A state with
    "ema" into an optimiser without EMA: kept, ignored, and the update is the bits of a plain one."""
    pa, plain = make("adam")
    pb, with_ema = make("adam", ema_decay=0.9, ema_warmup=True)
    for step in range(2):
        set_grads(pa, step); set_grads(pb, step)
        plain.fused_step(5.0, 100.0); with_ema.fused_step(5.0, 100.0)
    sd_plain, sd_ema = plain.state_dict(), with_ema.state_dict()
    assert not any("ema" in s for s in sd_plain["state"].values()) and all("ema" in s for s in sd_ema["state"].values())
    assert sd_ema["param_groups"][0]["ema_updates"] == 2

    pc, oc = make("adam", ema_decay=0.9, ema_warmup=True)
    for p, q in zip(pc, pa):
        p.copy_(q.detach())
    oc.load_state_dict(sd_plain)
    assert oc.ema_updates == 0 and oc._steps == 2
    for p in pc:
        assert torch.equal(oc.state[p]["ema"], p.detach())

    pd, od = make("adam")
    for p, q in zip(pd, pa):
        p.copy_(q.detach())
    od.load_state_dict(sd_ema)
    kept = [od.state[p]["ema"].clone() for p in pd]
    set_grads(pa, 2); set_grads(pd, 2)
    assert torch.equal(plain.fused_step(5.0, 100.0), od.fused_step(5.0, 100.0))
    for p, q, k in zip(pa, pd, kept):
        assert torch.equal(p.detach(), q.detach()) and torch.equal(od.state[q]["ema"], k)


def test_ema_options_are_checked():
    ps = make_params()
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            training.HipAdam(ps, ema_decay=bad)
    with pytest.raises(_lib.GlowHipError):
        training.HipAdam(ps).swap_averaged()
