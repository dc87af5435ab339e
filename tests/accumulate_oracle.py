"""numpy definition of gradient accumulation (csrc/accumulate.hip, glowhip_grad_accumulate): the three modes, per element, in
fp32 with one rounding per operation -- np.float32 adds, then ONE multiply -- and the composition over k micro-steps.

Comparison: `same_bits` compares int32 views, so signed zeros, infinities and the position of every NaN count.  The bit pattern OF
a NaN is left out: IEEE 754 does not fix the sign and payload of a NaN an operation generates (inf - inf gives 0xffc00000 on
x86 and 0x7fc00000 on the GPU), and nothing downstream reads it."""
import numpy as np

FIRST, ADD, FINISH = 0, 1, 2


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def first(g):
    """(grad, acc) after FIRST: acc = g, grad untouched."""
    g = _f32(g)
    return g.copy(), g.copy()


def add(g, acc):
    """(grad, acc) after ADD: acc = acc + g, grad untouched."""
    g, acc = _f32(g), _f32(acc)
    with np.errstate(all="ignore"):
        return g.copy(), (acc + g).astype(np.float32)


def finish(g, acc, scale):
    """(grad, acc) after FINISH: grad = (acc + g) * scale, acc untouched.  `scale` passes through a float32."""
    g, acc = _f32(g), _f32(acc)
    with np.errstate(all="ignore"):
        s = (acc + g).astype(np.float32)
        return (s * np.float32(scale)).astype(np.float32), acc.copy()


def apply(mode, g, acc, scale=1.0):
    if mode == FIRST:
        return first(g)
    if mode == ADD:
        return add(g, acc)
    if mode == FINISH:
        return finish(g, acc, scale)
    raise ValueError(mode)


def modes(k):
    """The mode of every micro-step of a round of k >= 2: FIRST, ADD x (k - 2), FINISH."""
    assert k >= 2
    return [FIRST] + [ADD] * (k - 2) + [FINISH]


def scale_for(k):
    """The float the model hands to FINISH: float32(1 / k), the division in doubles."""
    return np.float32(1.0 / k)


def compose(grads, scale=None):
    """The gradient k micro-steps leave behind: (((g0 + g1) + g2) + ... + g_{k-1}) * scale, every add and the one multiply
    rounded to fp32.  scale=None: `scale_for(k)`."""
    grads = [_f32(g) for g in grads]
    k = len(grads)
    scale = scale_for(k) if scale is None else scale
    acc = None
    for mode, g in zip(modes(k), grads):
        out, acc = apply(mode, g, acc, scale)
    return out


def bits(a):
    """int32 view of fp32 data with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(_f32(a))
    v = a.view(np.int32).copy()
    v[np.isnan(a)] = 0x7fc00000
    return v


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))
