"""CPU restatement of the full-latent encode on top of oracle/glow_oracle.py: the reference's encode loop (network/model.py:274-276)
with a look inside every Split2d (network/module.py:526-530) -- the dropped half z2, the prior (mean, logs) predicted from the
kept half, and the draw eps = (z2 - mean) * exp(-logs) that `flow_decode` takes back.  Pinned against the vectors the real
reference recorded (tests/golden/make_golden_latents.py) by tests/test_latents_host.py."""
import torch

from oracle import glow_oracle as O

G11 = dict(image_shape=[32, 32, 3], hidden_channels=32, K=2, L=3, actnorm_scale=1.0, n_bits_x=8, batch=4,
           flow_coupling="affine", flow_permutation="invconv", learn_top=False, y_condition=False)


def split_prior(z1, sd, prefix):
    """network/module.py:498-509: (mean, logs) = the even / odd channels of conv2d_zeros(z1)."""
    h = O.conv2d_zeros(z1, sd[prefix + "conv2d_zeros.weight"], sd[prefix + "conv2d_zeros.bias"], sd[prefix + "conv2d_zeros.logs"])
    return O.split_channel(h, "cross")


def split_eps(x, sd, prefix):
    """What one Split2d drops: dict(z2, mean, logs, eps)."""
    z1, z2 = O.split_channel(x, "simple")
    mean, logs = split_prior(z1, sd, prefix)
    return dict(z2=z2, mean=mean, logs=logs, eps=(z2 - mean) * torch.exp(-logs))


def flow_encode_latents(x, logdet, sd, cfg, prefix="flow.layers."):
    """(z, logdet, splits): `O.flow_encode` plus, per Split2d in DECODE order (deepest first), the dict of `split_eps`."""
    z, splits = x, []
    for kind, i, _ in O.flow_layout(cfg):
        if kind == "squeeze":
            z = O.squeeze2d(z, 2)
        elif kind == "step":
            z, logdet = O.flowstep(z, logdet, sd, f"{prefix}{i}.", cfg["flow_permutation"], cfg["flow_coupling"], reverse=False)
        else:
            splits.append(split_eps(z, sd, f"{prefix}{i}."))
            z, logdet = O.split2d(z, logdet, sd, f"{prefix}{i}.", reverse=False)
    return z, logdet, splits[::-1]


def g11_state(g):
    return {k[3:]: v for k, v in g.items() if k.startswith("sd.")}


def seeded_case(batch=4, seed=31):
    """The seeded config of the GPU checks: 32x32x3, hidden 64, K 4, L 3; Conv2dZeros ~ N(0, 0.02), perturbed invconv weights,
    ActNorm statistics from the batch.  Returns (cfg, sd, x, noise)."""
    cfg = O.default_cfg(image_shape=(32, 32, 3), hidden_channels=64, K=4, L=3, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=seed, zeros_std=0.02, invconv_perturb=0.05)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.floor(torch.rand(batch, 3, 32, 32, generator=g) * 256.0) / 256.0      # 8-bit pixel levels, as a dataset gives them
    noise = torch.rand(batch, 3, 32, 32, generator=g) / 256
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd, cfg)
    return cfg, sd, x, noise
