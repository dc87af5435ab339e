"""fp64 restatement of the optimiser step of csrc/optim.hip (k_optim_clip_sumsq + k_optim_update: clip_grad_value_, clip_grad_norm_,
then torch.optim.Adam / Adamax in torch's single-tensor form), the per-element bound the device's fp32 result is held to, and the
seeded inputs the host and the GPU tests share.  numpy only; nothing here reads the package: tests/test_gpu_optim.py holds
training.HipAdam / HipAdamax to these lines, tests/test_optim_host.py holds these lines to torch's own optimisers on float64 and
shows that its float32 restatement of the update stays inside `bound` on every input the GPU tests use.

`hyper` everywhere: dict(lr, betas, eps, weight_decay, step, clip_value, max_norm); `step` is the 1-based number of the update."""
import math

import numpy as np

U = 2.0 ** -24                   # unit roundoff of fp32 (round to nearest)
FLOOR = 2.0 ** -126              # per rounding, absolute: holds under gradual underflow and under flush-to-zero
SECOND_ORDER = 1.0 + 2.0 ** -10  # the products of two of the first-order terms below

KINDS = ("adam", "adamax")


def _f32(x):
    return float(np.float32(x))


def constants(hyper, exact_constants=False):
    """The scalars of one update.  The kernel receives lr, beta1, beta2, 1 - beta1, 1 - beta2, eps and weight_decay as floats and
    forms step_size = float(lr / bc1) and float(sqrt(bc2)) itself; bc1 / bc2 are python-double arithmetic on the host (as torch's).
    ``exact_constants``: every one of them stays a double -- torch's optimisers on float64 parameters."""
    b1, b2 = (float(b) for b in hyper["betas"])
    step = int(hyper["step"])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    c = dict(lr=float(hyper["lr"]), beta1=b1, beta2=b2, omb1=1.0 - b1, omb2=1.0 - b2, eps=float(hyper["eps"]),
             wd=float(hyper["weight_decay"]))
    if not exact_constants:
        c = {k: _f32(x) for k, x in c.items()}
    c["step_size"] = c["lr"] / bc1
    c["bc2_sqrt"] = math.sqrt(bc2)
    if not exact_constants:
        c["step_size"], c["bc2_sqrt"] = _f32(c["step_size"]), _f32(c["bc2_sqrt"])
    c["clip"] = float(hyper.get("clip_value", 0.0) or 0.0)
    c["max_norm"] = float(hyper.get("max_norm", 0.0) or 0.0)
    return c


def clamp(g, clip_value):
    """clip_grad_value_: g < -c ? -c : (g > c ? c : g) -- NaN and -0.0 pass through; clip_value <= 0: off."""
    g = np.asarray(g)
    if not clip_value > 0:
        return g
    c = g.dtype.type(clip_value)
    return np.where(g < -c, -c, np.where(g > c, c, g))


def total_norm(grads, clip_value):
    """sqrt of the sum of squares of the clamped gradients of a list of float32 arrays, in fp64."""
    with np.errstate(all="ignore"):
        return math.sqrt(sum(float(np.sum(np.square(clamp(np.asarray(g, dtype=np.float64).ravel(), clip_value)))) for g in grads)) \
            if len(grads) else 0.0


def coef_from_norm(norm_f32, max_norm):
    """clip_grad_norm_'s coefficient as the kernel forms it from the float norm: two correctly rounded float32 operations, then
    `coef > 1 ? 1 : coef` (a NaN stays).  1 when the norm clipping is off."""
    if not max_norm > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        coef = np.float32(max_norm) / (np.float32(norm_f32) + np.float32(1e-6))
    return np.float32(1.0) if coef > np.float32(1.0) else np.float32(coef)


def _walk(kind, p, g, m, v, hyper, coef, exact_constants):
    """The update operation by operation in fp64, every intermediate kept (the bound needs them)."""
    assert kind in KINDS, kind
    c = constants(hyper, exact_constants)
    T = np.float64
    K = {k: T(x) for k, x in c.items()}
    p, g, m, v = (np.asarray(a).astype(T) for a in (p, g, m, v))      # float32 in: widened exactly (float64, the host test: as is)
    w = dict(c=c)
    with np.errstate(all="ignore"):
        w["gc"] = clamp(g, c["clip"])
        w["g1"] = w["gc"] * T(coef) if c["max_norm"] > 0 else w["gc"]
        if c["wd"] != 0:
            w["wdp"] = K["wd"] * p
            w["ge"] = w["g1"] + w["wdp"]
        else:
            w["ge"] = w["g1"]
        ge = w["ge"]
        w["d"] = ge - m
        w["t"] = w["d"] * K["omb1"]
        w["m1"] = m + w["t"]                                  # exp_avg.lerp_(grad, 1 - beta1)
        w["a"] = v * K["beta2"]
        if kind == "adam":
            w["b"] = K["omb2"] * ge
            w["cc"] = w["b"] * ge
            w["v1"] = w["a"] + w["cc"]                        # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            w["s"] = np.sqrt(w["v1"])
            w["q"] = w["s"] / K["bc2_sqrt"]
            w["den"] = w["q"] + K["eps"]
            w["r"] = w["m1"] / w["den"]
        else:
            w["b"] = np.abs(ge) + K["eps"]
            w["v1"] = np.where(w["a"] > w["b"], w["a"], w["b"])      # max(exp_inf * beta2, |grad| + eps), the kernel's a > b ? a : b
            w["r"] = w["m1"] / w["v1"]
        w["sr"] = K["step_size"] * w["r"]
        w["p1"] = p - w["sr"]                                 # param.addcdiv_(exp_avg, denom, value=-step_size)
    return w


def step(kind, p, g, m, v, hyper, coef, exact_constants=False):
    """One update in fp64 from fp32 inputs (`g`: the gradient as supplied, before either clipping).  Returns the four arrays the
    device leaves behind: (stored gradient, exp_avg, exp_avg_sq / exp_inf, parameter)."""
    w = _walk(kind, p, g, m, v, hyper, coef, exact_constants)
    return w["g1"], w["m1"], w["v1"], w["p1"]


def _rnd(x):
    """What one fp32 rounding of a result x can add."""
    return U * np.abs(x) + FLOOR


def bound(kind, p, g, m, v, hyper, coef):
    """First-order per-element bounds (E_g, E_m, E_v, E_p) on |device - step(...)|, walking the kernel's fp32 roundings: each adds
    u |result| + 2^-126, incoming errors are carried through every operation, the whole is multiplied by 1 + 2^-10 for the products
    of two such terms.  Inputs (p, g, m, v, coef and the constants) are floats and carry no error; the clamp is exact."""
    w = _walk(kind, p, g, m, v, hyper, coef, False)
    c = w["c"]
    with np.errstate(all="ignore"):
        E_g = _rnd(w["g1"]) if c["max_norm"] > 0 else np.zeros_like(w["g1"])
        E_ge = E_g + _rnd(w["wdp"]) + _rnd(w["ge"]) if c["wd"] != 0 else E_g
        E_d = E_ge + _rnd(w["d"])
        E_m = c["omb1"] * E_d + _rnd(w["t"]) + _rnd(w["m1"])
        age = np.abs(w["ge"])
        if kind == "adam":
            E_b = c["omb2"] * E_ge + _rnd(w["b"])
            E_c = age * E_b + np.abs(w["b"]) * E_ge + _rnd(w["cc"])      # = 2 omb2 |ge| E_ge + 2 u omb2 ge^2
            E_v = _rnd(w["a"]) + E_c + _rnd(w["v1"])
            s = w["s"]
            lin = np.where(s > 0, E_v / (2.0 * np.where(s > 0, s, 1.0)), np.inf)
            E_s = np.minimum(lin, np.sqrt(E_v)) + _rnd(s)                # |sqrt(x) - sqrt(y)| <= sqrt|x - y| holds at any size
            E_den = E_s / c["bc2_sqrt"] + _rnd(w["q"]) + _rnd(w["den"])
            E_r = E_m / w["den"] + np.abs(w["r"]) * E_den / w["den"] + _rnd(w["r"])
        else:
            E_v = np.maximum(_rnd(w["a"]), E_ge + _rnd(w["b"]))          # |max(a', b') - max(a, b)| <= max(|a' - a|, |b' - b|)
            E_r = E_m / w["v1"] + np.abs(w["r"]) * E_v / w["v1"] + _rnd(w["r"])
        E_p = c["step_size"] * E_r + _rnd(w["sr"]) + _rnd(w["p1"])
    return tuple(E * SECOND_ORDER for E in (E_g, E_m, E_v, E_p))


# ---------------------------------------------------------------------------------------------------------------------------
# Shared inputs.  Every generator is seeded and returns float32 numpy arrays; the GPU tests upload exactly these.

CHUNK = 1 << 16                  # training._HipOptimizer.CHUNK: elements per block of either launch
SIZES = (1, 3, 4, 5, 1020, 1024, 1028, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 4)
OFFSET_N = 1028                  # n % 4 == 0: only the ADDRESS (one float into a larger buffer) takes such a tensor off the 16-byte path
# the geometry of every arithmetic case: SIZES, then a tensor whose GRADIENT is a shifted view, then one whose PARAMETER is
GEOMETRY = SIZES + (OFFSET_N, OFFSET_N)
PLACEMENT = ("",) * len(SIZES) + ("grad", "param")
MANY = tuple(4 + (7 * i) % 37 for i in range(130))                  # 130 tensors of 4 .. 40 elements: 130 chunks, three wave trips
ALIGNED = (4, 1024, 1028, CHUNK, 2 * CHUNK + 4)                     # every n % 4 == 0: m / v views stay on 16-byte addresses
NEIGHBOURS = (1028, 7)                                              # the two tensors either side of one that has no gradient
SCALES = (1e-4, 0.5, 300.0)
BETAS = (0.9, 0.9999)
CLIPS = ((0.0, 0.0), (5.0, 0.0), (0.0, 100.0), (5.0, 100.0), (5.0, 1e6))      # the last: max_norm above any norm, coef clamps to 1
STEPS = (1, 2, 10 ** 6)          # from zero state, the next one, then a late one (both bias corrections ~ 1)
POISON_TENSOR, POISON_ELEM = 100, 3
assert min(MANY) == 4 and max(MANY) == 40 and len(SIZES) == 11 and MANY[POISON_TENSOR] > POISON_ELEM


def params(geometry, seed=0):
    """Start values, 0.1 * randn, one array per tensor."""
    rs = np.random.RandomState(9000 + seed)
    return [(0.1 * rs.randn(n)).astype(np.float32) for n in geometry]


def grads(geometry, step, seed=0):
    """Gradients of one step.  Blocks of 64 elements cycle through the scales 1e-4, 0.5 and 300 (the phase moves with tensor and
    step, so every tensor of more than 192 elements has all three at every step); every 17th element is an exact zero; tensors of
    8 elements or more carry +-5 exactly, +-7.5 (beyond a clip of 5), -0.0 and +0.0 at fixed places."""
    rs = np.random.RandomState((12345 + 7919 * int(step % 100003) + seed) % (2 ** 31))
    out = []
    for t, n in enumerate(geometry):
        i = np.arange(n)
        scale = np.asarray(SCALES)[(i // 64 + t + int(step % 3)) % 3]
        g = (rs.randn(n) * scale).astype(np.float32)
        g[(i + t) % 17 == 0] = 0.0
        if n >= 8:
            g[n - 7:n - 1] = np.array([5.0, -5.0, 7.5, -7.5, -0.0, 0.0], np.float32)
        out.append(g)
    return out


def huge_grads(geometry, step, seed=0):
    """The range case: `grads` with three elements of +-3e19 in the largest tensor (one per chunk): their squares overflow fp32
    (9e38) and not fp64."""
    out = grads(geometry, step, seed)
    big = int(np.argmax(geometry))
    out[big][[2, CHUNK + 1, out[big].size - 9]] = np.array([3e19, -3e19, 3e19], np.float32)
    return out


def late_only_grads(geometry, step, seed=0):
    """Non-zero gradients in tensors 64 .. only: a total norm taken from the first trip of the 64-lane loop alone would be 0."""
    out = grads(geometry, step, seed)
    for g in out[:64]:
        g[:] = 0.0
    return out


def poisoned_grads(geometry, step, value, seed=0):
    """`grads` with one element of tensor 100 replaced by `value` (NaN, +inf)."""
    out = grads(geometry, step, seed)
    out[POISON_TENSOR][POISON_ELEM] = value
    return out


def inf_grads(geometry, step, seed=0):
    return poisoned_grads(geometry, step, np.inf, seed)


GENERATORS = dict(grads=grads, huge=huge_grads, late_only=late_only_grads, inf=inf_grads)


class Case:
    """One input set whose fp64 reference is finite on every element: the optimiser's settings, the tensor sizes, the step numbers
    run in order (state carried from one to the next, zero at first) and the generator of each step's gradients."""

    def __init__(self, name, kind, geometry, weight_decay=0.0, clip_value=0.0, max_norm=0.0, steps=(1,), gen="grads", seed=0):
        self.name, self.kind, self.geometry, self.weight_decay = name, kind, tuple(geometry), weight_decay
        self.clip_value, self.max_norm, self.steps, self.gen, self.seed = clip_value, max_norm, tuple(steps), gen, seed

    def params(self):
        return params(self.geometry, self.seed)

    def grads(self, step):
        return GENERATORS[self.gen](self.geometry, step, self.seed)

    def hyper(self, step):
        return hyper(self.kind, step, self.clip_value, self.max_norm, self.weight_decay)


def _cases():
    out = []
    for kind in KINDS:
        for wd in (0.0, 0.01):                      # the arithmetic matrix, all on GEOMETRY
            for clip, max_norm in CLIPS:
                out.append(Case(f"arith-{kind}-wd{wd:g}-clip{clip:g}-norm{max_norm:g}", kind, GEOMETRY, wd, clip, max_norm, STEPS))
        for clip, max_norm in ((0.0, 0.0), (0.0, 100.0)):
            out.append(Case(f"range-{kind}-norm{max_norm:g}", kind, GEOMETRY, 0.01, clip, max_norm, (1, 2), gen="huge"))
        # chunk counts: three trips of the 64-lane loop, exactly one, one and a single lane of the second (also the steps around a
        # skipped one: tests/test_gpu_optim.py runs `many130` again with a poisoned call between its two steps)
        for n in (130, 64, 65):
            out.append(Case(f"many{n}-{kind}", kind, MANY[:n], 0.01, 5.0, 10.0, (1, 2)))
        out.append(Case(f"late-only-{kind}", kind, MANY, 0.0, 0.0, 1.0, (1,), gen="late_only"))
        out.append(Case(f"inf-clamped-{kind}", kind, MANY, 0.0, 5.0, 10.0, (1,), gen="inf"))      # +inf is clamped to 5: finite
        for max_norm in (0.0, 100.0):
            out.append(Case(f"aligned-{kind}-norm{max_norm:g}", kind, ALIGNED, 0.01, 5.0, max_norm, (1, 2)))
        out.append(Case(f"neighbours-{kind}", kind, NEIGHBOURS, 0.01, 5.0, 100.0, (1, 2)))
    return {c.name: c for c in out}


CASES = _cases()
# Input sets whose fp64 reference is itself non-finite, by name (tests/test_gpu_optim.py): the finite elements of these are still
# held to the oracle, the others must be non-finite exactly where the oracle's are -- no element is left out
NONFINITE_CASES = ("nan-skip", "inf-unclamped-skip", "nan-noskip")


def cat(arrays):
    return np.concatenate([np.asarray(a).ravel() for a in arrays]) if len(arrays) else np.zeros(0, np.float32)


def hyper(kind, step, clip_value=0.0, max_norm=0.0, weight_decay=0.0, lr=None, betas=BETAS, eps=1e-8):
    return dict(lr=(1e-3 if kind == "adam" else 2e-3) if lr is None else lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                step=int(step), clip_value=clip_value, max_norm=max_norm)


def worst_multiple(got, ref, E):
    """max over the elements of |got - ref| / E.  Elements where got and ref are the same non-finite value count as 0; an element
    that is non-finite on one side only, or differently, counts as inf."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        fin = np.isfinite(got) & np.isfinite(ref)
        same = (np.isnan(got) & np.isnan(ref)) | (~fin & (got == ref))
        diff = np.abs(got - ref)
        mult = np.where(fin, np.where(diff == 0, 0.0, diff / E), np.where(same, 0.0, np.inf))      # (E_g is 0 with the norm clipping off)
    return float(np.max(mult))
