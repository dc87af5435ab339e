"""The optimiser step (csrc/optim.hip: k_optim_clip_sumsq, k_optim_update; training.HipAdam / HipAdamax) on synthetic tensors, no
model, against the fp64 restatement of tests/optim_oracle.py on EVERY element of the four arrays a step leaves behind (the clipped
gradient, exp_avg, exp_avg_sq / exp_inf, the parameter) within the per-element bound derived there, and the returned norm within
one rounding of the fp64 norm.  tests/test_optim_host.py shows on the host that the kernel's promised float32 arithmetic lies
inside that bound on each of these inputs, so nothing here is masked out.

Per step: read p, m, v back, upload the gradient, fused_step, then compare.  Shapes (optim_oracle.GEOMETRY): 1 .. 5 elements, the
trip boundary of the 16-byte loop at 256 threads (1020 / 1024 / 1028), a second chunk of one element (65535 / 65536 / 65537),
three chunks, a gradient and a parameter one float off a 16-byte address, and the state views that `_ensure_state` leaves
misaligned after every odd size; 130 / 64 / 65 small tensors for the 64-lane loop over the chunk sums."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib, training  # noqa: E402

import ema_oracle as EO  # noqa: E402
import optim_oracle as OO  # noqa: E402
from test_optim_host import step_f32  # noqa: E402

DEV = "cuda:0"
NORM_BOUND = 2.0 ** -24 * (1.0 + 2.0 ** -20)      # one rounding to float; the fp64 reduction's own error is below n 2^-53


def shifted(values):
    """A device copy of `values` that starts one float into a larger buffer: contiguous, 4 bytes past a 16-byte address."""
    n = values.numel()
    view = torch.zeros(n + 4, device=DEV)[1:1 + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def make(kind, geometry, placement=None, weight_decay=0.0, seed=0, frozen_at=None, **kw):
    """Parameters with optim_oracle's start values (``placement[i]``: "param" / "both" = a shifted view) and their optimiser.
    ``frozen_at``: a 33-element parameter that never gets a gradient, inserted at that position."""
    placement = placement or ("",) * len(geometry)
    ps = []
    for arr, place in zip(OO.params(geometry, seed), placement):
        t = torch.from_numpy(arr)
        ps.append(torch.nn.Parameter(shifted(t) if place in ("param", "both") else t.to(DEV)))
        assert place in ("param", "both") or ps[-1].data_ptr() % 16 == 0
    if frozen_at is not None:
        ps.insert(frozen_at, torch.nn.Parameter(torch.linspace(-1.0, 1.0, 33).to(DEV)))
    cls = training.HipAdam if kind == "adam" else training.HipAdamax
    h = OO.hyper(kind, 1, weight_decay=weight_decay)
    opt = cls(ps, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=weight_decay, **kw)
    opt._ensure_state()
    return ps, opt


def host(t):
    return t.detach().cpu().numpy().ravel().copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def read(opt, ps):
    """(p, m, v) of the parameters in `ps`, concatenated."""
    return tuple(OO.cat([host(f(p)) for p in ps]) for f in (lambda p: p, lambda p: opt.state[p]["exp_avg"], lambda p: opt.state[p][opt.SECOND]))


def upload(ps, grads, placement=None):
    placement = placement or ("",) * len(ps)
    for p, g, place in zip(ps, grads, placement):
        t = torch.from_numpy(g).view_as(p)
        p.grad = shifted(t) if place in ("grad", "both") else t.to(DEV)
        assert place in ("grad", "both") or p.grad.data_ptr() % 16 == 0


def check_norm(norm, grads, clip):
    ref = OO.total_norm(grads, clip)
    if math.isfinite(ref):
        assert math.isfinite(norm) and abs(norm - ref) <= NORM_BOUND * norm, (norm, ref)
    else:
        assert (math.isnan(norm) and math.isnan(ref)) or norm == ref, (norm, ref)
    return ref


def checked_step(kind, opt, ps, grads, clip, max_norm, placement=None, finite=True, label="", **kw):
    """One fused_step held to the oracle: the norm, then g, m, v, p on every element of the parameters `ps` (those with a gradient).
    ``finite=False``: the named non-finite cases -- device and oracle must be non-finite on the same elements, the rest within the
    bound.  Returns (norm, worst multiple per output, elements whose bits differ from the float32 restatement)."""
    p0, m0, v0 = read(opt, ps)
    upload(ps, grads, placement)
    g0 = OO.cat(grads)
    norm = float(opt.fused_step(clip, max_norm, **kw))
    check_norm(norm, grads, clip)
    group = opt.param_groups[0]
    h = dict(lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"], step=opt._steps,
             clip_value=clip, max_norm=max_norm)
    coef = OO.coef_from_norm(np.float32(norm), max_norm)
    p1, m1, v1 = read(opt, ps)
    got = (OO.cat([host(p.grad) for p in ps]), m1, v1, p1)
    ref, E = OO.step(kind, p0, g0, m0, v0, h, coef), OO.bound(kind, p0, g0, m0, v0, h, coef)
    if finite:
        assert all(np.isfinite(r).all() for r in ref) and all(np.isfinite(x).all() for x in got), label
    mult = np.array([OO.worst_multiple(a, b, e) for a, b, e in zip(got, ref, E)])
    f32 = step_f32(kind, p0, g0, m0, v0, h, coef)
    differ = int(sum(np.count_nonzero((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))) for a, b in zip(got, f32)))
    print(f"{label} step {opt._steps}: norm {norm:.9g} coef {float(coef):.9g}  worst multiple of the bound  g {mult[0]:.3f}  m {mult[1]:.3f}  "
          f"v {mult[2]:.3f}  p {mult[3]:.3f}  | {differ} of {4 * g0.size} values differ from the float32 restatement")
    assert (mult <= 1.0).all(), (label, opt._steps, mult)
    if coef == 1.0:              # norm clipping off or clamped at exactly 1: what is stored is the value-clamped input, bit for bit
        assert np.array_equal(bits(got[0]), bits(OO.clamp(g0, clip))), label
    return norm, mult, differ


def jump_to(opt, step):
    """Make the NEXT update number `step` by editing the state dict and loading it back (which also re-homes m and v)."""
    old = opt._flat[0].data_ptr()
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(float(step - 1))
    opt.load_state_dict(sd)
    assert opt._steps == step - 1 and opt._flat[0].data_ptr() != old


def run_case(case, placement=None, **kw):
    """The case's steps in order on a fresh optimiser; returns it with its parameters, the norms and the worst multiples."""
    ps, opt = make(case.kind, case.geometry, placement, case.weight_decay, case.seed, **kw)
    worst, norms, differ = np.zeros(4), [], 0
    for step in case.steps:
        if step != opt._steps + 1:
            jump_to(opt, step)
        norm, mult, d = checked_step(case.kind, opt, ps, case.grads(step), case.clip_value, case.max_norm, placement, label=case.name)
        assert opt._steps == step
        worst, differ = np.maximum(worst, mult), differ + d
        norms.append(norm)
    return ps, opt, norms, worst, differ


def chunk_rows(opt, ps):
    """(param, grad, m, v addresses, n) of every chunk, as `_chunk_table` builds them."""
    rows = []
    for p in ps:
        if p.grad is None:
            continue
        st = opt.state[p]
        base = (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st[opt.SECOND].data_ptr())
        for o in range(0, p.numel(), opt.CHUNK):
            rows.append(tuple(b + 4 * o for b in base) + (min(opt.CHUNK, p.numel() - o),))
    return rows


def test_geometry_puts_chunks_on_both_paths_of_both_launches():
    """From data_ptr(): the clip launch chooses by gradient address and length, the update launch by all four addresses -- the
    list has chunks on (16-byte, 16-byte), (16-byte, element: m / v misaligned after an odd size), (element by address alone,
    element) and a parameter off its address; a full 2^16 chunk and a 1-element second chunk among them."""
    ps, opt = make("adam", OO.GEOMETRY, OO.PLACEMENT)
    upload(ps, OO.grads(OO.GEOMETRY, 1), OO.PLACEMENT)
    rows = chunk_rows(opt, ps)
    assert len(rows) == 11 + 1 + 2 + 2 and opt.CHUNK == OO.CHUNK
    al = lambda a: a % 16 == 0
    clip_vec = [al(g) and n % 4 == 0 for (_, g, _, _, n) in rows]
    upd_vec = [al(p) and al(g) and al(m) and al(v) and n % 4 == 0 for (p, g, m, v, n) in rows]
    assert any(c and u and n == OO.CHUNK for c, u, (_, _, _, _, n) in zip(clip_vec, upd_vec, rows))
    assert any(c and not u and al(p) and not al(m) and not al(v) for c, u, (p, _, m, v, _) in zip(clip_vec, upd_vec, rows))
    assert any(not al(g) and n % 4 == 0 and al(p) for (p, g, _, _, n) in rows)           # the clip launch off the 16-byte path by address alone
    assert any(not al(p) and n % 4 == 0 and al(g) for (p, g, _, _, n) in rows)
    assert any(n == 1 for (*_, n) in rows) and sum(n for (*_, n) in rows) == sum(OO.GEOMETRY)
    opt.fused_step(5.0, 100.0)
    assert opt._n_chunks == len(rows)


ARITH = [n for n in OO.CASES if n.startswith("arith-")]
RANGE = [n for n in OO.CASES if n.startswith("range-")]
COUNTS = [n for n in OO.CASES if n.startswith(("many", "late-only-"))]


@pytest.mark.parametrize("name", ARITH)
def test_update_against_fp64_on_every_element(name):
    """Both kinds x weight_decay {0, 0.01} x (clip, max_norm) {(0,0), (5,0), (0,100), (5,100), (5,1e6): coef clamps to 1}; steps 1
    (zero state), 2 and -- through an edited state_dict -- 10^6 with betas (0.9, 0.9999); gradient scales 1e-4 / 0.5 / 300 in
    blocks, every 17th element zero, +-5, +-7.5, -0.0 and 0.0 in every tensor of 8 or more elements."""
    case = OO.CASES[name]
    _, opt, norms, worst, differ = run_case(case, OO.PLACEMENT)
    assert opt._n_chunks == 16 and opt._steps == 10 ** 6
    print(f"{name}: WORST  g {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}  p {worst[3]:.3f}  differ {differ}")


@pytest.mark.parametrize("name", RANGE)
def test_gradients_whose_squares_overflow_fp32(name):
    """Three elements of +-3e19: the sum of squares (2.7e39) exists only in fp64.  The norm is finite and one rounding from the
    fp64 norm, the step is applied and held to the oracle (with max_norm = 100 the coefficient is ~2e-18)."""
    case = OO.CASES[name]
    _, _, norms, worst, differ = run_case(case, OO.PLACEMENT)
    assert all(5e19 < n < 5.3e19 for n in norms), norms
    print(f"{name}: WORST  g {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}  p {worst[3]:.3f}  differ {differ}")


@pytest.mark.parametrize("name", COUNTS)
def test_norm_over_64_65_and_130_chunks(name):
    """The total norm is reduced by one wave, `for (i = lane; i < n_chunks; i += 64)`: exactly one trip (64 tensors), one trip and
    a single lane of the second (65), three trips (130), and 130 with non-zero gradients only in tensors 64 .. 129, where a norm
    from the first trip would be 0 and the coefficient 1 instead of ~0.1."""
    case = OO.CASES[name]
    _, opt, norms, worst, differ = run_case(case)
    assert opt._n_chunks == len(case.geometry)
    if case.gen == "late_only":
        assert norms[0] > 5.0 * case.max_norm
    print(f"{name}: WORST  g {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}  p {worst[3]:.3f}  differ {differ}")


@pytest.mark.parametrize("kind", OO.KINDS)
def test_16_byte_and_element_paths_give_the_same_bits(kind):
    """Same values, every tensor n % 4 == 0: once with all four addresses of every chunk on 16 bytes, once with parameters and
    gradients one float off (every chunk element by element in both launches).  Both held to the oracle; with max_norm = 0 (no
    dependence on the order of the norm's sum) p, m, v and the stored gradients are the same bits after each step."""
    for name in (f"aligned-{kind}-norm0", f"aligned-{kind}-norm100"):
        case = OO.CASES[name]
        both = ("both",) * len(case.geometry)
        pa, oa = make(kind, case.geometry, None, case.weight_decay, case.seed)
        pb, ob = make(kind, case.geometry, both, case.weight_decay, case.seed)
        for step in case.steps:
            checked_step(kind, oa, pa, case.grads(step), case.clip_value, case.max_norm, None, label=name + " 16-byte")
            assert all(a % 16 == 0 for row in chunk_rows(oa, pa) for a in row[:4])
            checked_step(kind, ob, pb, case.grads(step), case.clip_value, case.max_norm, both, label=name + " element")
            assert all(row[0] % 16 == 4 and row[1] % 16 == 4 for row in chunk_rows(ob, pb))
            if case.max_norm == 0:
                for x, y in zip(read(oa, pa) + (OO.cat([host(p.grad) for p in pa]),), read(ob, pb) + (OO.cat([host(p.grad) for p in pb]),)):
                    assert np.array_equal(bits(x), bits(y)), (name, step)


@pytest.mark.parametrize("kind", OO.KINDS)
def test_device_form_equals_argument_form_and_reruns_give_the_same_bits(kind):
    """Without EMA (tests/test_gpu_ema.py has the comparison with): fused_step(hyper_dev = the 3 doubles of hyper_values) against
    the argument form over three steps with a learning rate that changes every step, and a second argument-form run from the same
    state: parameters, both state tensors, stored gradients and the norm are the same bits in all three."""
    case = OO.CASES[f"arith-{kind}-wd0.01-clip5-norm100"]
    runs = [make(kind, case.geometry, OO.PLACEMENT, case.weight_decay, case.seed) for _ in range(3)]
    hyper = torch.zeros(3, dtype=torch.float64, device=DEV)
    for step in (1, 2, 3):
        lr = runs[0][1].defaults["lr"] * (1.0 + 0.25 * step)
        norms = []
        for i, (ps, opt) in enumerate(runs):
            opt.param_groups[0]["lr"] = lr
            upload(ps, case.grads(step), OO.PLACEMENT)
            if i == 1:
                values = opt.hyper_values(lr, opt._steps + 1)
                assert len(values) == 3
                hyper.copy_(torch.tensor(values, dtype=torch.float64))
                norms.append(opt.fused_step(case.clip_value, case.max_norm, hyper_dev=hyper))
            else:
                norms.append(opt.fused_step(case.clip_value, case.max_norm))
        assert torch.equal(norms[0], norms[1]) and torch.equal(norms[0], norms[2]) and torch.isfinite(norms[0])
        first = read(runs[0][1], runs[0][0]) + (OO.cat([host(p.grad) for p in runs[0][0]]),)
        for ps, opt in runs[1:]:
            for x, y in zip(first, read(opt, ps) + (OO.cat([host(p.grad) for p in ps]),)):
                assert np.array_equal(bits(x), bits(y)), step


@pytest.mark.parametrize("kind", OO.KINDS)
@pytest.mark.parametrize("ema", [False, True])
def test_parameter_without_gradient_between_two_that_have_one(kind, ema):
    """[1028 elements, 33 without a gradient, 7 elements]: the middle one keeps its bits, its zero state and (EMA on) its average;
    its neighbours are held to the oracle, and with EMA on their averages follow ema_oracle.advance from the device's own p' -- the
    pointer array of the averages is still parallel to a chunk table that skips a parameter."""
    case = OO.CASES[f"neighbours-{kind}"]
    ps, opt = make(kind, case.geometry, None, case.weight_decay, case.seed, frozen_at=1, **(dict(ema_decay=0.9) if ema else {}))
    frozen, active = ps[1], [ps[0], ps[2]]
    frozen0 = host(frozen)
    for step in case.steps:
        e0 = [host(opt.state[p]["ema"]) for p in active] if ema else None
        w = opt.ema_weight(opt.ema_updates) if ema else None
        checked_step(kind, opt, active, case.grads(step), case.clip_value, case.max_norm, label=case.name + (" ema" if ema else ""))
        assert opt._n_chunks == 2 and frozen.grad is None
        assert np.array_equal(bits(host(frozen)), bits(frozen0))
        assert not opt.state[frozen]["exp_avg"].any() and not opt.state[frozen][opt.SECOND].any()
        if ema:
            assert w == EO.weight_at(step - 1, 0.9, False)
            assert np.array_equal(bits(host(opt.state[frozen]["ema"])), bits(frozen0))
            for p, e in zip(active, e0):
                p1, e1 = host(p), host(opt.state[p]["ema"])
                ref = EO.advance(e, p1, w)
                lim = EO.bound(1, max(np.abs(e).max(), np.abs(p1).max(), np.abs(e1).max()))
                assert np.abs(e1 - ref).max() <= lim, (step, np.abs(e1 - ref).max(), lim)


def poisoned_call(kind, opt, ps, value, clip, max_norm, step):
    """A skipped step: one `value` in tensor 100 of the 130, skip_nonfinite on.  The norm is not finite; p, m, v (and the average)
    keep their bits; the gradients are the value-clamped input, the poison kept; undo_step() takes the counts back."""
    names = ["exp_avg", opt.SECOND] + (["ema"] if opt.ema_decay else [])
    before = [bits(host(p)) for p in ps] + [bits(host(opt.state[p][n])) for p in ps for n in names]
    grads = OO.poisoned_grads(OO.MANY, step, value)
    upload(ps, grads)
    steps, ema_t = opt._steps, opt.ema_updates
    norm = float(opt.fused_step(clip, max_norm, skip_nonfinite=True))
    check_norm(norm, grads, clip)
    assert not math.isfinite(norm) and opt._steps == steps + 1
    after = [bits(host(p)) for p in ps] + [bits(host(opt.state[p][n])) for p in ps for n in names]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    for p, g in zip(ps, grads):
        assert np.array_equal(bits(host(p.grad)), bits(OO.clamp(g, clip)))
    assert not np.isfinite(host(ps[OO.POISON_TENSOR].grad)[OO.POISON_ELEM])
    opt.undo_step()
    assert opt._steps == steps and opt.ema_updates == ema_t and float(opt.state[ps[0]]["step"]) == steps


@pytest.mark.parametrize("kind", OO.KINDS)
@pytest.mark.parametrize("ema", [False, True])
def test_nan_skips_the_step_and_the_next_one_continues(kind, ema):
    """NONFINITE_CASES "nan-skip": the clean step 1 of `many130`, a call with one NaN (clip 5, max_norm 10, skip on), undo_step(),
    then the clean step 2 -- held to the oracle AT STEP NUMBER 2, from the state the skipped call left alone."""
    case = OO.CASES[f"many130-{kind}"]
    ps, opt = make(kind, case.geometry, None, case.weight_decay, case.seed, **(dict(ema_decay=0.9, ema_warmup=True) if ema else {}))
    checked_step(kind, opt, ps, case.grads(1), case.clip_value, case.max_norm, label="nan-skip: before")
    poisoned_call(kind, opt, ps, np.nan, case.clip_value, case.max_norm, 2)
    assert np.isnan(host(ps[OO.POISON_TENSOR].grad)[OO.POISON_ELEM])
    checked_step(kind, opt, ps, case.grads(2), case.clip_value, case.max_norm, label="nan-skip: after")
    assert opt._steps == 2 and opt.ema_updates == (2 if ema else 0)


@pytest.mark.parametrize("kind", OO.KINDS)
def test_inf_is_clamped_by_the_value_clipping_and_skips_without_it(kind):
    """+inf in tensor 100.  With clip = 5 the clamp makes it 5: the norm is finite and the step is applied although skip is on
    (`inf-clamped`, a finite case).  NONFINITE_CASES "inf-unclamped-skip": with clip = 0 the norm is +inf and the step is skipped."""
    case = OO.CASES[f"inf-clamped-{kind}"]
    ps, opt = make(kind, case.geometry, None, case.weight_decay, case.seed)
    grads = case.grads(1)
    assert np.isposinf(grads[OO.POISON_TENSOR][OO.POISON_ELEM])
    norm, _, _ = checked_step(kind, opt, ps, grads, case.clip_value, case.max_norm, label=case.name, skip_nonfinite=True)
    assert math.isfinite(norm) and host(ps[OO.POISON_TENSOR].grad)[OO.POISON_ELEM] == np.float32(5.0) * OO.coef_from_norm(np.float32(norm), case.max_norm)
    poisoned_call(kind, opt, ps, np.inf, 0.0, case.max_norm, 2)
    assert opt._steps == 1


@pytest.mark.parametrize("kind", OO.KINDS)
@pytest.mark.parametrize("max_norm", [0.0, 10.0])
def test_nan_without_skip_is_torchs_semantics(kind, max_norm):
    """NONFINITE_CASES "nan-noskip": one NaN, skip off.  The norm is NaN; p, m and v are NaN exactly where the oracle's are and
    within the bound everywhere else -- with max_norm = 0 that is the one poisoned element, with max_norm > 0 the NaN coefficient
    reaches every element of every chunk, as clip_grad_norm_'s does."""
    ps, opt = make(kind, OO.MANY, None, 0.01)
    checked_step(kind, opt, ps, OO.grads(OO.MANY, 1), 5.0, max_norm, label="nan-noskip: before")
    norm, _, _ = checked_step(kind, opt, ps, OO.poisoned_grads(OO.MANY, 2, np.nan), 5.0, max_norm, finite=False, label=f"nan-noskip norm {max_norm:g}")
    assert math.isnan(norm)
    p1, m1, v1 = read(opt, ps)
    total = sum(OO.MANY)
    for a in (p1, m1, v1):
        assert np.count_nonzero(np.isnan(a)) == (total if max_norm > 0 else 1) and not np.isinf(a).any()
    where = sum(OO.MANY[:OO.POISON_TENSOR]) + OO.POISON_ELEM
    assert np.isnan(p1[where]) and np.isnan(m1[where]) and np.isnan(v1[where])


def test_refusals():
    """One set of hyper-parameters for all groups; contiguous gradients; fp32 parameters (torch itself refuses to attach a gradient
    of another type to an fp32 parameter, so a non-fp32 gradient can only arrive with a non-fp32 parameter)."""
    for key, other in (("lr", 5e-4), ("weight_decay", 0.01)):
        a, b = torch.nn.Parameter(torch.ones(8, device=DEV)), torch.nn.Parameter(torch.ones(8, device=DEV))
        opt = training.HipAdam([dict(params=[a]), dict(params=[b], **{key: other})], lr=1e-3)
        a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
        with pytest.raises(_lib.GlowHipError, match="one set of hyper-parameters"):
            opt.fused_step(5.0, 100.0)
        assert torch.equal(a.detach(), torch.ones(8, device=DEV)) and torch.equal(b.detach(), torch.ones(8, device=DEV))
    p = torch.nn.Parameter(torch.ones(4, 6, device=DEV))
    opt = training.HipAdamax([p])
    p.grad = torch.ones(6, 4, device=DEV).t()
    assert not p.grad.is_contiguous()
    with pytest.raises(_lib.GlowHipError, match="contiguous fp32"):
        opt.fused_step()
    assert torch.equal(p.detach(), torch.ones(4, 6, device=DEV))
    p.grad = torch.ones(4, 6, device=DEV)
    assert torch.isfinite(opt.fused_step())          # and the same optimiser goes on with a proper gradient
    q = torch.nn.Parameter(torch.ones(4, device=DEV, dtype=torch.float64))
    q.grad = torch.ones_like(q)
    with pytest.raises(_lib.GlowHipError, match="contiguous fp32 parameters"):
        training.HipAdam([q]).fused_step()
