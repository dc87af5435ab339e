"""Inputs, fp64 references and error bars of the log-likelihood accumulator tests (tests/test_gpu_objective.py on the GPU,
tests/test_objective_host.py on the CPU).  The only density formula is oracle.glow_oracle.gaussian_logps, evaluated and summed in
float64; this file adds the inputs, the bar and the classification of a case against the documented range of the accumulator
(csrc/common.h RANGE, include/glowhip.h glowhip_gaussian_logp):

    fine     every 256-element partial sum |v| < 2^14 nats      the Q31.32 word alone
    coarse   2^14 <= some |v| < 2^43                             whole nats counted above the flag bits: finite, exact
    beyond   some |v| >= 2^43                                    -inf / +inf by sign, flag bit 4 / 2

Everything here is built once per process and never written to."""
import functools

import numpy as np
import torch

from oracle import glow_oracle as O

import ycond_oracle as Y

U = 2.0 ** -24                      # unit roundoff of fp32
COARSE_MIN, COARSE_MAX, FINE_RANGE = 2.0 ** 14, 2.0 ** 43, 2.0 ** 31
REL = 1e-6                          # the range cases' bar against fp64 (the fp32 reference itself is ~1e-7 from it)

SHAPES = [(1, 1, 1, 1), (3, 1, 1, 255), (3, 1, 16, 16), (2, 1, 1, 257), (5, 3, 7, 11), (2, 12, 33, 31), (300, 2, 3, 5)]
ARGS = ["both", "mean", "logs", "neither"]


def _z(t, like):
    return torch.zeros_like(like) if t is None else t


def terms64(mean, logs, x):
    x = x.double()
    return O.gaussian_logps(_z(mean, x).double(), _z(logs, x).double(), x)


def logp64(mean, logs, x):
    """(N,) float64: the reference, oracle.glow_oracle.gaussian_logps in fp64 summed in fp64."""
    return terms64(mean, logs, x).flatten(1).sum(1)


def abs_terms64(mean, logs, x):
    """(N,) sum over elements of log(2 pi)/2 + |logs| + d^2 / (2 e^{2 logs}): from the oracle's value, -logps - logs is the sum of the
    two non-negative terms."""
    l = _z(logs, x).double()
    return (-terms64(mean, logs, x) - l + l.abs()).flatten(1).sum(1)


def partials64(mean, logs, x, chunk=256):
    """(N, ceil(CHW / chunk)) fp64 sums over consecutive elements of a sample: k_gaussian_logp's / k_split_tail's workgroups."""
    t = terms64(mean, logs, x).flatten(1)
    pad = (-t.shape[1]) % chunk
    return torch.nn.functional.pad(t, (0, pad)).view(t.shape[0], -1, chunk).sum(2)


def bar(mean, logs, x, inp=None):
    """Derived, per sample (as tests/test_gpu_ycond_shapes.py derives its head bound): an element's log-density comes from a handful of
    fp32 operations -- the difference and its square 3 u, expf 2 u, the quotient 1 u, two additions 2 u of the running magnitude --
    8 u of log(2 pi)/2 + |logs| + d^2 / (2 e^{2 logs}); the block sum is fp64; each workgroup partial is rounded to 2^-32 nats (half a
    unit: 2^-33); the fp32 store rounds the total (with `in`) once: u |total|."""
    total = logp64(mean, logs, x) + (0.0 if inp is None else inp.double())
    n_part = -(-x[0].numel() // 256)
    return 8 * U * abs_terms64(mean, logs, x) + n_part * 2.0 ** -33 + U * total.abs()


def classify(partials):
    """Per sample: 'fine' / 'coarse' / 'beyond' (see the table above), refusing inputs within 1 % of a threshold (the kernel's
    fp32 terms differ from fp64 by ~1e-7)."""
    m = partials.abs().max(dim=1).values
    for t in (COARSE_MIN, COARSE_MAX):
        assert not bool(((m > 0.99 * t) & (m < 1.01 * t)).any()), "a case sits on a threshold"
    return ["fine" if v < COARSE_MIN else "coarse" if v < COARSE_MAX else "beyond" for v in m.tolist()]


# ------------------------------------------------------------------------------------------------ 1. shapes and arguments
@functools.lru_cache(maxsize=None)
def logp_case(shape):
    g = torch.Generator().manual_seed(sum(shape) * 7 + shape[-1])
    x = torch.randn(shape, generator=g)
    mean = torch.randn(shape, generator=g) * 0.5
    logs = torch.randn(shape, generator=g) * 0.4
    inp = torch.randn(shape[0], generator=g) * 100.0
    return x, mean, logs, inp


def pick(args, mean, logs):
    return (mean if args in ("both", "mean") else None), (logs if args in ("both", "logs") else None)


def the_sample():
    """One (2, 3, 5) sample for the batch-position test (a row of the (300, 2, 3, 5) shape)."""
    g = torch.Generator().manual_seed(41)
    return [torch.randn(1, 2, 3, 5, generator=g) * s for s in (1.0, 0.5, 0.4)]


# ------------------------------------------------------------------------------------------------ 3. range on GaussianDiag.logp
# name: (batch, index of the extreme sample, what it holds, class, |sum| beyond 2^31)
RANGE_CASES = {
    "a": (4, 1, "one element 1e6", "coarse", True),
    "b": (4, 1, "all 3000", "coarse", True),
    "c": (4, 1, "all 1976", "coarse", False),
    "d": (300, 2, "all 3000", "coarse", True),
    "e": (4, 1, "one element 1e8", "beyond", True),      # beyond the documented range: must come back -inf, flag 4
}


@functools.lru_cache(maxsize=None)
def range_case(name):
    """(x, mean, logs, x_ordinary, i): samples of randn data under a random prior; sample i extreme with mean = logs = 0 there.
    x_ordinary: the same batch with ordinary data in sample i (the other samples' bits must not depend on it)."""
    n, i, what, _, _ = RANGE_CASES[name]
    g = torch.Generator().manual_seed(5)
    shape = (n, 4, 16, 16)
    x0 = torch.randn(shape, generator=g)
    mean = torch.randn(shape, generator=g) * 0.3
    logs = torch.randn(shape, generator=g) * 0.2
    mean[i], logs[i] = 0.0, 0.0
    x = x0.clone()
    if what.startswith("all"):
        x[i] = float(what.split()[1])
    else:
        x[i, 2, 7, 9] = float(what.split()[2])
    return x, mean, logs, x0, i


# ------------------------------------------------------------------------------------------------ 4. the Split2d routes
SPLIT_ROUTES = [("k_split_tail", 12, 4, 4), ("k_split_tail", 6, 3, 5), ("k_conv_tail", 12, 32, 32), ("k_conv_tail", 48, 8, 8),
                ("k_conv_tail_dma", 64, 16, 16)]
SPLIT_N, SPLIT_I, SPLIT_BIG = 3, 1, 1e6


@functools.lru_cache(maxsize=None)
def split_case(c, h, w):
    """(sd, x, x_ordinary): Split2d weights drawn as tests/test_gpu_sampler.py draws them, a batch of 3 whose sample 1 has one
    element of the dropped half z2 at 1e6 (z2 does not feed the convolution: mean and logs stay ordinary)."""
    g = torch.Generator().manual_seed(c * 100 + h)
    sd = {"conv2d_zeros.weight": torch.randn(c, c // 2, 3, 3, generator=g) * 0.05,
          "conv2d_zeros.bias": torch.randn(c, generator=g) * 0.3,
          "conv2d_zeros.logs": torch.randn(c, 1, 1, generator=g) * 0.1}
    x0 = torch.randn(SPLIT_N, c, h, w, generator=g)
    x = x0.clone()
    x[SPLIT_I, c // 2 + (c // 2) // 2, h // 2, w // 3] = SPLIT_BIG
    return sd, x, x0


def split_prior64(sd, x, dtype=torch.float64):
    """(mean, logs, z2) of the oracle's Split2d in `dtype`."""
    z1, z2 = O.split_channel(x.to(dtype), "simple")
    hh = O.conv2d_zeros(z1, sd["conv2d_zeros.weight"].to(dtype), sd["conv2d_zeros.bias"].to(dtype), sd["conv2d_zeros.logs"].to(dtype))
    mean, logs = O.split_channel(hh, "cross")
    return mean, logs, z2


# ------------------------------------------------------------------------------------------------ 4b / 5. whole models
CLASSES = 5
MODEL_KEY = dict(image=(32, 32), L=3, K=2, hidden=64, batch=4, seed="objective")


@functools.lru_cache(maxsize=None)
def model_case():
    """The 32x32, L 3, K 2, hidden 64 model of tests/test_gpu_sampler.py with its coupling and prior heads at zeros_std 1e-6 (as
    test_gpu_fused._range_case): with that file's 0.02, pixels scaled by 1e4 or a top latent of 1e6 drive sigmoid(h + 2) to 0 and
    the reference's own nll -- in fp64 too -- is inf; there would be no finite answer to hold the kernels to."""
    cfg = O.default_cfg(image_shape=(32, 32, 3), hidden_channels=64, K=2, L=3, batch=4)
    sd = O.seeded_state_dict(cfg, seed=1, zeros_std=1e-6, invconv_perturb=0.05)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(4, 3, 32, 32, generator=g)
    noise = torch.rand(4, 3, 32, 32, generator=g) / 256
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd, cfg)
    return cfg, sd, x, noise


def forward64(x, noise, sd, cfg, yo=None, dtype=torch.float64):
    with torch.no_grad():
        z, nll, _ = Y.glow_forward(x.to(dtype), noise.to(dtype), {k: v.to(dtype) for k, v in sd.items()}, cfg, None if yo is None else yo.to(dtype))
    return z, nll


def nats(nll, x):
    """|objective| in nats of an nll in bits/dim (less the constant -ln(256) CHW): what the accumulator holds."""
    return nll.abs() * float(np.log(2.0) * x[0].numel())


@functools.lru_cache(maxsize=None)
def head_case():
    """Class-conditional model (learn_top too) and pixels whose top latent has one element at 1e6 in sample 1: the oracle's decode
    of that latent.  Returns (cfg, sd with the head, pixels, y_onehot)."""
    cfg, sd, _, _ = model_case()
    C, hw = 3 * 2 ** (cfg["L"] + 1), 32 >> cfg["L"]
    sd = dict(sd)
    sd.update(Y.seeded_head_state(C, CLASSES, True))
    cfg = dict(cfg, learn_top=True, y_condition=True, weight_y=0.0)
    z = torch.randn(4, C, hw, hw, generator=torch.Generator().manual_seed(11))
    z[1, 0, 1, 2] = 1e6
    g = torch.Generator().manual_seed(12)
    eps = [torch.randn(4, *s, generator=g) for kind, _, s in O.flow_layout(cfg) if kind == "split"][::-1]
    with torch.no_grad():
        x = O.flow_decode(z, sd, cfg, eps)
    return cfg, sd, x, torch.eye(CLASSES)[torch.arange(4) % CLASSES]


def scaled_case():
    """Case 5: the model's own pixels scaled by 1e4."""
    cfg, sd, x, noise = model_case()
    return cfg, sd, x * 1e4, noise
