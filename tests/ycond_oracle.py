"""CPU restatement of the class-conditional Glow (reference network/model.py:345-348, 362-379, 409-471, 508-538; LinearZeros
network/module.py:152-185) on top of oracle/glow_oracle.py, in torch so that autograd gives its gradients.  Pinned against the
vectors the real reference recorded (tests/golden/make_golden_ycond.py) by tests/test_ycond_host.py; the GPU tests use the
fixture itself."""
import numpy as np
import torch

from oracle import glow_oracle as O

TINY = dict(image_shape=[16, 16, 3], hidden_channels=32, K=2, L=2, actnorm_scale=1.0, n_bits_x=8, batch=4,
            flow_coupling="affine", flow_permutation="invconv")


def linear_zeros(x, sd, prefix):
    """network/module.py:152-185: (x W^T + b) * exp(3 logs)"""
    return (x @ sd[prefix + "weight"].t() + sd[prefix + "bias"]) * torch.exp(sd[prefix + "logs"] * 3.0)


def prior(sd, cfg, y_onehot):
    """network/model.py:362-379: h = h_top (== 0, detached) [-> learn_top] [+ y_emb(y_onehot)]; (mean, logs) = halves of h."""
    h = sd["h_top"].detach().clone()
    if cfg.get("learn_top", False):
        h = O.conv2d_zeros(h, sd["learn_top.weight"], sd["learn_top.bias"], sd["learn_top.logs"])
    if cfg.get("y_condition", False):
        assert y_onehot is not None
        h = h + linear_zeros(y_onehot, sd, "y_emb.").view(-1, h.shape[1], 1, 1)
    return O.split_channel(h, "simple")


def glow_forward(x, noise, sd, cfg, y_onehot=None):
    """network/model.py:409-452 with the dequantisation noise injected: (z, nll, y_logits)."""
    n_bins = 2 ** cfg["n_bits_x"]
    z = x + noise
    factor = x.shape[1] * O.count_pixels(x)
    objective = torch.zeros_like(x[:, 0, 0, 0]) + float(-np.log(n_bins)) * factor
    z, objective = O.flow_encode(z, objective, sd, cfg)
    mean, logs = prior(sd, cfg, y_onehot)
    objective = objective + O.gaussian_logp(mean, logs, z)
    y_logits = None
    if cfg.get("y_condition", False) and cfg.get("weight_y", 0.0) > 0:
        y_logits = linear_zeros(z.mean(dim=(2, 3)), sd, "classifier.")
    nll = (-objective) / float(np.log(2.0) * factor)
    return z, nll, y_logits


def classification_loss(y_logits, criterion, y=None, y_onehot=None):
    """network/model.py:508-538 (mean-reduced CrossEntropyLoss / BCEWithLogitsLoss)"""
    if criterion == "ce":
        return torch.nn.functional.cross_entropy(y_logits, y.long())
    return torch.nn.functional.binary_cross_entropy_with_logits(y_logits, y_onehot.to(y_logits.dtype))


def glow_sample(sd, cfg, y_onehot, eps_top, eps_list):
    """network/model.py:454-471 with z = None: z = mean + exp(logs) * eps_top, then decode with the injected split draws."""
    with torch.no_grad():
        mean, logs = prior(sd, cfg, y_onehot)
        z = O.gaussian_sample(mean, logs, eps_top)
        return O.flow_decode(z, sd, cfg, eps_list)


def logit_bound(sd, base):
    """`base` (a bound on |dz|) carried through the classifier: base * max(1, max_k exp(3 logs_k) * sum_c |W[k, c]|)."""
    w, logs = sd["classifier.weight"], sd["classifier.logs"]
    return base * max(1.0, float((torch.exp(3.0 * logs) * w.abs().sum(dim=1)).max()))


def seeded_head_state(C, classes, learn_top, seed=7):
    """Seeded, NON-zero parameters of the top head over a top latent of C channels (LinearZeros / Conv2dZeros initialise to zero,
    which would hide every head kernel): weights and biases randn * 0.1, every `logs` randn * 0.05; learn_top.weight small but
    non-zero (it multiplies h_top == 0, so its gradient must stay exactly zero).  Keys and shapes are the modules'."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    sd = {"y_emb.weight": rn(2 * C, classes) * 0.1, "y_emb.bias": rn(2 * C) * 0.1, "y_emb.logs": rn(2 * C) * 0.05,
          "classifier.weight": rn(classes, C) * 0.1, "classifier.bias": rn(classes) * 0.1, "classifier.logs": rn(classes) * 0.05}
    if learn_top:
        sd.update({"learn_top.weight": rn(2 * C, 2 * C, 3, 3) * 0.01, "learn_top.bias": rn(2 * C) * 0.1,
                   "learn_top.logs": rn(2 * C, 1, 1) * 0.05})
    return sd


def fp64_reference(x, noise, sd, cfg, y_onehot, crit, y=None):
    """The conditional training step in float64 under O.STABLE_LOGDET (fp32 `det` underflows at C = 384), gradients from
    autograd: dict(z, nll, y_logits, loss, loss_generative, loss_classes, grad={name: tensor}, dx).  `sd`, `x`, `noise` are the
    fp32 tensors the HIP path gets; they are widened exactly."""
    prev, O.STABLE_LOGDET = O.STABLE_LOGDET, True
    try:
        with torch.enable_grad():
            leaf = {k: v.double().requires_grad_(k != "h_top") for k, v in sd.items()}
            xr = x.double().requires_grad_(True)
            yo = y_onehot.double()
            z, nll, y_logits = glow_forward(xr, noise.double(), leaf, cfg, yo)
            loss_gen = nll.mean()
            loss_cls = classification_loss(y_logits, crit, y=y, y_onehot=yo)
            loss = loss_gen + float(cfg["weight_y"]) * loss_cls
            loss.backward()
    finally:
        O.STABLE_LOGDET = prev
    return dict(z=z.detach(), nll=nll.detach(), y_logits=y_logits.detach(), loss=loss.item(), loss_generative=loss_gen.item(),
                loss_classes=loss_cls.item(), grad={k: v.grad for k, v in leaf.items() if v.grad is not None}, dx=xr.grad)


def case_state(g, lt):
    """State dict of one fixture case: the shared one, without learn_top.* when that case has none."""
    return {k[3:]: v for k, v in g.items() if k.startswith("sd.") and (lt or not k.startswith("sd.learn_top."))}


CASES = [(lt, crit) for lt in (0, 1) for crit in ("ce", "bce")]
