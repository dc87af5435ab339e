"""The top head (csrc/tophead.hip) at the shapes real models bring (-m gpu).  Every other test of the four head kernels runs the
tiny fixture (C = 24 channels on 16 pixels, 5 classes), where each strided loop makes at most one, partly empty trip.  The six
models here make every loop run a full wave, a ragged second trip and a second or third thread trip:

    id  image    L  hidden  top C x HW  classes  batch  learn_top  criterion  what it reaches
    S1  32x32    1  16       12 x 256    40      3      no         BCE        four full pixel trips
    S2  32x48    2  16       24 x 96     65      3      yes        CE         ragged second pixel trip; K one past a wave
    S3  64x64    3  32       48 x 64     40      5      yes        BCE        exactly one full wave of pixels
    S4  32x32    4  32       96 x 4     300      2      no         CE         K > 256: second thread trip of the logits loop
    S5  64x64    5  32      192 x 4      64      1      yes        CE         2C = 384 > 256; batch 1; K exactly one wave
    S6  128x128  6  64      384 x 4     300      3      yes        BCE        2C = 768: three trips of the prior loop

K = 1 FlowStep per level, affine coupling, invertible 1x1 convolutions, ActNorms initialised by the oracle; head parameters seeded
and non-zero (ycond_oracle.seeded_head_state), weight_y = 0.5.  Reference: tests/ycond_oracle.py in float64 under
O.STABLE_LOGDET, gradients from autograd (fp32 `det` underflows at C = 384, see test_gpu_train_deep.py).

Bounds.  Whole model: the project's own -- z, nll 1e-4; gradients and dx 2e-4 max|g| + 1e-7 (flow tensors with
test_gpu_train_deep.py's outlier rule: at most 1 % of the entries beyond it, none beyond 5 % of max|g|; head tensors with no
allowance, they have no ReLU kink); losses within ycond_oracle.logit_bound(sd, 1e-4); samples 1e-4.  Head alone: derived from
operand sizes where they are used (u = 2^-24, the unit roundoff of fp32); the whole-model bound cannot see the head at L >= 5, where
one dropped top element moves nll by ~4e-5 bits/dim.  Every check prints the worst observed multiple of its bound."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

import ycond_oracle as Y  # noqa: E402

DEV = "cuda:0"
CRIT = {"ce": "single_class", "bce": "multi_class"}
WEIGHT_Y = 0.5
U = 2.0 ** -24
HEAD = ("y_emb.", "classifier.", "learn_top.")

CASES = {
    "S1": dict(H=32, W=32, L=1, hidden=16, classes=40, batch=3, lt=False, crit="bce"),
    "S2": dict(H=32, W=48, L=2, hidden=16, classes=65, batch=3, lt=True, crit="ce", y=[64, 0, 33]),
    "S3": dict(H=64, W=64, L=3, hidden=32, classes=40, batch=5, lt=True, crit="bce"),
    "S4": dict(H=32, W=32, L=4, hidden=32, classes=300, batch=2, lt=False, crit="ce", y=[299, 70]),
    "S5": dict(H=64, W=64, L=5, hidden=32, classes=64, batch=1, lt=True, crit="ce", y=[63]),
    "S6": dict(H=128, W=128, L=6, hidden=64, classes=300, batch=3, lt=True, crit="bce"),
}
ALL = list(CASES)


def top_shape(c):
    return 3 * 2 ** (c["L"] + 1), c["H"] >> c["L"], c["W"] >> c["L"]


def split_shapes(c):
    """(C, H, W) of the half each Split2d drops, in decode order (deepest first)."""
    return [s for kind, _, s in O.flow_layout(dict(image_shape=[c["H"], c["W"], 3], K=1, L=c["L"])) if kind == "split"][::-1]


def case_labels(c):
    """CE: the targets of the table (class K - 1 among them, and a class >= 64 / >= 256 where K allows).  BCE: multi-hot rows of
    about 30 % ones, the second row all zero and the last all ones."""
    K, n = c["classes"], c["batch"]
    if c["crit"] == "ce":
        y = torch.tensor(c["y"])
        assert len(y) == n and int(y.max()) == K - 1 and (K <= 64 or int((y >= 64).sum()) > 0) and (K <= 256 or int((y >= 256).sum()) > 0)
        return y, torch.nn.functional.one_hot(y, K).float()
    yo = (torch.rand(n, K, generator=torch.Generator().manual_seed(9)) < 0.3).float()
    yo[1], yo[n - 1] = 0.0, 1.0
    return None, yo


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Weights, inputs, labels and every fp64 reference figure of a case; computed once, read by all tests, never written."""
    c = CASES[cid]
    C, h, w = top_shape(c)
    cfg = O.default_cfg(image_shape=(c["H"], c["W"], 3), hidden_channels=c["hidden"], K=1, L=c["L"], batch=c["batch"])
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=0.01)
    x = torch.rand(c["batch"], 3, c["H"], c["W"], generator=torch.Generator().manual_seed(4))
    noise = torch.rand(c["batch"], 3, c["H"], c["W"], generator=torch.Generator().manual_seed(5)) / 256
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd, cfg)
    assert tuple(sd["h_top"].shape) == (c["batch"], 2 * C, h, w)
    sd.update(Y.seeded_head_state(C, c["classes"], c["lt"]))
    cfg.update(learn_top=c["lt"], y_condition=True, weight_y=WEIGHT_Y)
    y, yo = case_labels(c)
    ref = Y.fp64_reference(x, noise, sd, cfg, yo, c["crit"], y=y)
    assert bool(torch.isfinite(ref["nll"]).all()) and all(float(ref["grad"][k].abs().max()) > 0 for k in sd
                                                           if k.startswith(HEAD) and k != "learn_top.weight")
    gen = torch.Generator().manual_seed(6)
    eps_top = torch.randn(c["batch"], C, h, w, generator=gen) * 0.6
    eps = [torch.randn(c["batch"], *s, generator=gen) * 0.6 for s in split_shapes(c)]
    O.STABLE_LOGDET = True
    try:
        sample = Y.glow_sample({k: v.double() for k, v in sd.items()}, cfg, yo.double(), eps_top.double(), [e.double() for e in eps])
    finally:
        O.STABLE_LOGDET = False
    return dict(cfg=cfg, sd=sd, sd64={k: v.double() for k, v in sd.items()}, x=x, noise=noise, y=y, yo=yo, ref=ref,
                eps_top=eps_top, eps=eps, sample=sample, D=3 * c["H"] * c["W"])


def hps_for(c, y_condition=True, classes=None):
    return util.AttrDict(dict(
        model=dict(image_shape=[c["H"], c["W"], 3], hidden_channels=c["hidden"], K=1, L=c["L"], actnorm_scale=1.0, n_bits_x=8,
                   weight_y=WEIGHT_Y),
        ablation=dict(learn_top=bool(c["lt"]) and y_condition, y_condition=y_condition, y_criterion=CRIT[c["crit"]],
                      lu_decomposition=False, flow_permutation="invconv", flow_coupling="affine"),
        optim=dict(num_batch_train=c["batch"]), dataset=dict(num_classes=classes or c["classes"]), device=dict(graph=[DEV])))


def make_glow(cid, y_condition=True, train=False):
    """A fresh model of the case on the GPU; ``y_condition=False``: the same flow weights under the plain N(0, 1) prior."""
    c, r = CASES[cid], reference(cid)
    np.random.seed(3)
    glow = G.Glow(hps_for(c, y_condition))
    glow.load_state_dict({k: v.clone() for k, v in r["sd"].items() if y_condition or not k.startswith(HEAD)}, strict=True)
    glow.set_actnorm_inited()
    glow = glow.to(DEV)
    return glow.train() if train else glow.eval()


def dev(t):
    return None if t is None else t.to(DEV)


def err(a, b):
    a = a.detach().cpu().double().reshape(b.shape)
    assert bool(torch.isfinite(a).all())
    return float((a - b.double()).abs().max())


def check_grads(glow, r, dx, what):
    """Every gradient against fp64 autograd; returns the worst multiple of the tight bound among (flow tensors, head tensors)."""
    ref = r["ref"]["grad"]
    rows = [] if dx is None else [("dL/dx", dx, r["ref"]["dx"])]
    for name, p in glow.named_parameters():
        if name in ("h_top", "learn_top.weight"):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name      # (learn_top.weight multiplies h_top == 0)
            continue
        assert p.grad is not None and name in ref, f"{what}: {name} has no gradient"
        rows.append((name, p.grad, ref[name]))
    assert float(ref["learn_top.weight"].abs().max()) == 0.0 if "learn_top.weight" in ref else True
    assert {n for n, _, _ in rows if n.startswith(HEAD)} == {k for k in r["sd"] if k.startswith(HEAD) and k != "learn_top.weight"}
    worst, fails = {False: ("", 0.0), True: ("", 0.0)}, []
    for name, got, want in rows:
        head = name.startswith(HEAD)
        e = (got.detach().cpu().double().reshape(want.shape) - want).abs()
        scale = float(want.abs().max())
        tight = 2e-4 * scale + 1e-7
        outliers = float((e > tight).double().mean())
        worst[head] = max(worst[head], (name, float(e.max()) / tight), key=lambda t: t[1])
        if not bool(torch.isfinite(got).all()) or outliers > (0.0 if head else 0.01) or float(e.max()) > 0.05 * scale + 1e-7:
            fails.append(f"{name}: max err {float(e.max()):.3e} = {float(e.max()) / tight:.2f} x the tight bound, {outliers:.2%} of "
                         f"the entries beyond it, max|g| {scale:.3e}")
    print(f"{what}: gradients, worst flow tensor {worst[False][0]} at {worst[False][1]:.3f} of 2e-4 max|g| + 1e-7, worst head tensor "
          f"{worst[True][0]} at {worst[True][1]:.3f}")
    assert not fails, f"{what}:\n" + "\n".join(fails)


# ----------------------------------------------------------------------------- 1. whole model
@pytest.mark.parametrize("cid", ALL)
def test_training_step_matches_the_fp64_oracle_on_both_routes(cid):
    c, r = CASES[cid], reference(cid)
    ref, lb = r["ref"], Y.logit_bound(r["sd"], 1e-4)
    x, noise, yo, y = dev(r["x"]), dev(r["noise"]), dev(r["yo"]), dev(r["y"])
    # (a) the reference's own step: normal_flow + the user's torch loss + loss.backward()
    glow = make_glow(cid, train=True)
    plan = glow.flow.plan_for(x)
    plan.launch_counts(reset=True)
    with torch.enable_grad():
        xd = x.clone().requires_grad_(True)
        z, nll, y_logits = glow.normal_flow(xd, yo, noise=noise)
        lg = G.Glow.generative_loss(nll)
        lc = G.Glow.single_class_loss(y_logits, y) if c["crit"] == "ce" else G.Glow.multi_class_loss(y_logits, yo)
        loss = lg + WEIGHT_Y * lc
        loss.backward()
    counts = plan.launch_counts(reset=True)
    ez, en, el = err(z, ref["z"]), err(nll, ref["nll"]), err(y_logits, ref["y_logits"])
    eloss, ecls = abs(float(loss) - ref["loss"]), abs(float(lc) - ref["loss_classes"])
    print(f"{cid} autograd route: z {ez / 1e-4:.3f} nll {en / 1e-4:.3f} of 1e-4; logits {el / lb:.3f} loss {eloss / lb:.3f} "
          f"classification loss {ecls / lb:.3f} of the logit bound {lb:.2e}; {counts}")
    assert counts.get("k_top_head_fwd") == 1 and counts.get("k_top_head_bwd") == 1, counts
    assert ez <= 1e-4 and en <= 1e-4 and tuple(y_logits.shape) == (c["batch"], c["classes"]) and el <= lb
    assert eloss <= lb and ecls <= lb
    check_grads(glow, r, xd.grad, f"{cid} autograd route")
    # (b) the direct route: criterion and weight_y inside the head kernel
    glow = make_glow(cid, train=True)
    plan = glow.flow.plan_for(x)
    plan.launch_counts(reset=True)
    loss_d = glow.loss_and_grads(x, noise=noise, y_onehot=yo, y=y, criterion=CRIT[c["crit"]])
    counts = plan.launch_counts(reset=True)
    lgen, lcls = glow.last_losses
    eloss, egen, ecls = abs(float(loss_d) - ref["loss"]), abs(float(lgen) - ref["loss_generative"]), abs(float(lcls) - ref["loss_classes"])
    print(f"{cid} direct route: generative loss {egen / 1e-4:.3f} of 1e-4; loss {eloss / lb:.3f} classification loss {ecls / lb:.3f} "
          f"of the logit bound; {counts}")
    assert counts.get("k_top_head_fwd") == 1 and counts.get("k_top_head_bwd") == 1, counts
    assert egen <= 1e-4 and eloss <= lb and ecls <= lb
    check_grads(glow, r, None, f"{cid} direct route")


# ----------------------------------------------------------------------------- 2-4. the head alone
@functools.lru_cache(maxsize=None)
def hip_forward(cid):
    """(z, nll, y_logits) of the conditional model and (z, nll) of the same flow under the plain prior, on the inference path."""
    r = reference(cid)
    x, noise = dev(r["x"]), dev(r["noise"])
    with torch.no_grad():
        z, nll, lg = make_glow(cid).normal_flow(x, dev(r["yo"]), noise=noise)
        plain = make_glow(cid, y_condition=False)
        zp, nllp, lgp = plain.normal_flow(x, None, noise=noise)
        assert lgp is None and not any(k.startswith("k_top_head") for k in plain.flow.plan_for(x).launch_counts())
    return z.cpu(), nll.cpu(), lg.cpu(), zp.cpu(), nllp.cpu()


@pytest.mark.parametrize("cid", ALL)
def test_head_log_density_against_the_plain_prior_on_the_same_flow(cid):
    """nll_cond - nll_plain = -[logp(z | mean, logs) - logp(z | 0, 0)] / (ln 2 D): the flow is the same launches on the same bits
    and cancels, so what is left is k_top_head_fwd against k_gaussian_logp (held to fp64 on its own, shapes, arguments and range,
    by tests/test_gpu_objective.py) and the fp64 densities of the HIP path's own z.

    Bound: both nll are fp32 outputs of a Q31.32 sum -- one rounding each plus the scaling, 4 u max|nll| -- and every top element's
    log-density is evaluated in fp32 from a handful of operations, each within a few u of the element's own size: 8 u = 2^-21
    times the sum of |logp| over both densities, in bits/dim.  The bound must stay 10 times below one average top element, so a
    single dropped element shows."""
    r = reference(cid)
    z, nll, _, zp, nllp = hip_forward(cid)
    assert torch.equal(z, zp)
    scale = math.log(2.0) * r["D"]
    zc = z.double()
    mean, logs = Y.prior(r["sd64"], r["cfg"], r["yo"].double())
    lp_c = O.gaussian_logps(mean, logs, zc)
    lp_0 = O.gaussian_logps(torch.zeros_like(zc), torch.zeros_like(zc), zc)
    want = -(lp_c.sum(dim=(1, 2, 3)) - lp_0.sum(dim=(1, 2, 3))) / scale
    got = nll.double() - nllp.double()
    bound = 4 * U * torch.maximum(nll.abs(), nllp.abs()).double() + 2.0 ** -21 * (lp_c.abs() + lp_0.abs()).sum(dim=(1, 2, 3)) / scale
    one = lp_c.abs().mean(dim=(1, 2, 3)) / scale
    ratio = float(((got - want).abs() / bound).max())
    print(f"{cid} head log-density: {ratio:.3f} of the bound (bound {float(bound.max()):.2e} bits/dim, one top element "
          f"{float(one.min()):.2e}, nll {[round(v, 4) for v in nll.tolist()]})")
    assert bool((10 * bound <= one).all()), (bound, one)
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0


@pytest.mark.parametrize("cid", ALL)
def test_head_logits_against_fp64_of_the_hip_latent(cid):
    """y_logits against the fp64 LinearZeros of mean_HW(z_hip).  The kernel rounds h once (1 u), adds C products and the bias in
    fp32 in order ((C + 1) u of sum |h_c w_kc| + |b_k|) and scales by expf(3 logs_k) (2 u): (C + 4) u exp(3 logs_k) (sum_c |h_c w_kc|
    + |b_k|), plus 2^-22 |logit| for the final product and the store."""
    c, r = CASES[cid], reference(cid)
    z, _, lg, _, _ = hip_forward(cid)
    C = top_shape(c)[0]
    sd = r["sd64"]
    h = z.double().mean(dim=(2, 3))
    w, b, s = sd["classifier.weight"], sd["classifier.bias"], torch.exp(3.0 * sd["classifier.logs"])
    want = (h @ w.t() + b) * s
    bound = (C + 4) * U * s * (h.abs() @ w.abs().t() + b.abs()) + 2.0 ** -22 * want.abs()
    assert tuple(lg.shape) == tuple(want.shape) == (c["batch"], c["classes"]) and bool(torch.isfinite(lg).all())
    ratio = float(((lg.double() - want).abs() / bound).max())
    print(f"{cid} head logits: {ratio:.3f} of the bound (max |logit| {float(want.abs().max()):.3f})")
    assert ratio <= 1.0


@pytest.mark.parametrize("cid", ALL)
def test_dense_prior_against_fp64(cid):
    """`Glow.prior` (k_top_prior) against the fp64 prior, both halves on every channel and every pixel.  The same form of bound with
    K terms in place of C; learn_top's share base_c = bias_c exp(3 logs_c) is one more term of the sum:
    (K + 4) u [exp(3 logs_c) (sum_k |y_k w_ck| + |b_c|) + |base_c|] + 2^-22 |value|."""
    c, r = CASES[cid], reference(cid)
    C, h, w = top_shape(c)
    K, sd, yo = c["classes"], r["sd64"], r["yo"].double()
    mean, logs = make_glow(cid).prior(dev(r["yo"]))
    assert tuple(mean.shape) == tuple(logs.shape) == (c["batch"], C, h, w)
    got = torch.cat([mean, logs], dim=1).cpu().double()
    m_ref, l_ref = Y.prior(sd, r["cfg"], yo)
    want = torch.cat([m_ref, l_ref], dim=1).expand(c["batch"], 2 * C, h, w)
    s = torch.exp(3.0 * sd["y_emb.logs"])
    terms = s * (yo.abs() @ sd["y_emb.weight"].abs().t() + sd["y_emb.bias"].abs())
    if c["lt"]:
        terms = terms + (sd["learn_top.bias"] * torch.exp(3.0 * sd["learn_top.logs"].reshape(-1))).abs()
    bound = ((K + 4) * U * terms).reshape(c["batch"], 2 * C, 1, 1) + 2.0 ** -22 * want.abs()
    assert bool(torch.isfinite(got).all())
    ratio = (got - want).abs() / bound
    print(f"{cid} dense prior: mean {float(ratio[:, :C].max()):.3f} logs {float(ratio[:, C:].max()):.3f} of the bound "
          f"(max |value| {float(want.abs().max()):.3f})")
    assert float(ratio.max()) <= 1.0


# ----------------------------------------------------------------------------- 5. sampling
# Rows of the batch whose sample has a reference.  S6's all-ones row sums 300 embeddings: its prior has logs up to 5.6, the draw a
# top latent of |z| up to 190, and the decode of that overflows in float64 itself (inf after the third Split2d) -- there is nothing
# to compare that row with; `test_dense_prior_against_fp64` holds its prior on every channel and pixel.
SAMPLE_ROWS = {"S2": [0, 1, 2], "S3": [0, 1, 2, 3, 4], "S6": [0, 1]}


@pytest.mark.parametrize("cid", list(SAMPLE_ROWS))
def test_conditional_sampling_matches_the_fp64_oracle(cid):
    r = reference(cid)
    rows = SAMPLE_ROWS[cid]
    assert [i for i in range(CASES[cid]["batch"]) if bool(torch.isfinite(r["sample"][i]).all())] == rows
    xs = make_glow(cid).reverse_flow(None, dev(r["yo"]), eps_std=0.6, eps=[dev(e) for e in r["eps"]], eps_top=dev(r["eps_top"]))
    assert tuple(xs.shape) == tuple(r["sample"].shape)
    e = err(xs[rows], r["sample"][rows])
    print(f"{cid} conditional sample: {e / 1e-4:.3f} of 1e-4 on rows {rows} (max |x| {float(r['sample'][rows].abs().max()):.2f})")
    assert e <= 1e-4


# ----------------------------------------------------------------------------- 6. repeatability
@pytest.mark.parametrize("cid", ["S4", "S6"])
def test_two_steps_from_the_same_state_give_the_same_bits(cid):
    c, r = CASES[cid], reference(cid)
    x, noise, yo, y = dev(r["x"]), dev(r["noise"]), dev(r["yo"]), dev(r["y"])
    glow = make_glow(cid, train=True)
    outs = []
    for _ in range(2):
        loss = glow.loss_and_grads(x, noise=noise, y_onehot=yo, y=y, criterion=CRIT[c["crit"]])
        outs.append((loss.clone(), [t.clone() for t in glow.last_losses],
                     {n: p.grad.clone() for n, p in glow.named_parameters() if p.grad is not None}))
    (la, ta, ga), (lb, tb, gb) = outs
    assert bool(torch.isfinite(la)) and torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ta, tb))
    assert set(ga) == set(gb) and {"y_emb.weight", "y_emb.logs", "classifier.weight", "classifier.logs"} <= set(ga)
    diff = [n for n in ga if not torch.equal(ga[n], gb[n])]
    print(f"{cid} repeatability: {len(ga)} gradients, {len(diff)} differ")
    assert not diff, diff


# ----------------------------------------------------------------------------- 7. refusals (host logic: check_head_desc)
def test_more_than_4096_classes_are_refused():
    c = dict(CASES["S2"], H=16, W=16, hidden=32, lt=False)      # (the tiny fixture's geometry with K = 1)
    np.random.seed(3)
    glow = G.Glow(hps_for(c, classes=4097))
    glow.set_actnorm_inited()
    glow = glow.to(DEV).eval()
    x = torch.rand(c["batch"], 3, 16, 16, device=DEV)
    yo = torch.zeros(c["batch"], 4097, device=DEV)
    with pytest.raises(G.GlowHipError, match="top head: K=4097 out of range"):
        glow.normal_flow(x, yo, noise=torch.zeros_like(x))
    assert not any(k.startswith("k_top_head") for k in glow.flow.plan_for(x).launch_counts())


def test_a_head_beyond_the_lds_is_refused():
    """(3 C + K) * 4 bytes must fit 48 KB.  No model shape gets there within 4096 classes, so the descriptor goes to
    glowhip_top_prior directly; the check comes before the launch.  Exactly 48 KB is accepted (a head with no parameters: the
    all-zero prior)."""
    C = 4096
    mean = torch.full((1, C, 1, 1), 7.0, device=DEV)
    logs = torch.full((1, C, 1, 1), 7.0, device=DEV)
    d = _lib.HeadDesc()
    d.K = 1
    rc = _lib.lib().glowhip_top_prior(d, None, 1, C, 1, _lib.ptr(mean), _lib.ptr(logs), _lib.stream_ptr(mean.device))
    with pytest.raises(G.GlowHipError, match="top head: C=4096, K=1 do not fit the head kernels' LDS"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert float(mean.min()) == 7.0 and float(logs.min()) == 7.0          # nothing ran
    d.K = 0
    _lib.check(_lib.lib().glowhip_top_prior(d, None, 1, C, 1, _lib.ptr(mean), _lib.ptr(logs), _lib.stream_ptr(mean.device)))
    torch.cuda.synchronize()
    assert float(mean.abs().max()) == 0.0 and float(logs.abs().max()) == 0.0
