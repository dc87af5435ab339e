"""CPU reference of the differentiable decode: autograd through `O.flow_decode` in fp64 (oracle/glow_oracle.py is pure torch and
its decode has no no_grad), the seeded cases the GPU tests share, and the ReLU margin of a case.

Why a margin: the decode's gradient is piecewise constant in the ReLU masks of the coupling networks.  A hidden unit whose
pre-activation is within rounding of zero can take the other branch on the GPU, and one flipped mask changes everything downstream
of it in the sweep -- the fp32 oracle then disagrees with the fp64 oracle just as the kernels do.  A strict element-wise comparison
is therefore only meaningful for a seed whose smallest |pre-activation| (fp64, whole model) is well above the forward deviation;
`MIN_MARGIN` = 1e-5 is three times the 3e-6 DESIGN.md states for the forward."""
import functools

import numpy as np
import torch

from oracle import glow_oracle as O

import latents_oracle as LO

MIN_MARGIN = 1e-5


def image_hw(image):
    """(H, W) of ``image``: an int (square) or an (H, W) pair."""
    return (image, image) if isinstance(image, int) else (int(image[0]), int(image[1]))


def build_case(image, hidden, K, L, batch, seed, zeros_std, perm="invconv", coup="affine", tables=None, invconv_perturb=0.02):
    """(cfg, sd, z, eps, g_x): seeded weights + ActNorm init from the batch; the latents are the fp32 full-latent encode of that
    batch (no noise); g_x ~ N(0, 1).  ``image``: the side of a square image, or (H, W)."""
    H, W = image_hw(image)
    cfg = O.default_cfg(image_shape=(H, W, 3), hidden_channels=hidden, K=K, L=L, flow_permutation=perm, flow_coupling=coup,
                        batch=batch)
    sd = O.seeded_state_dict(cfg, seed=seed, zeros_std=zeros_std, invconv_perturb=invconv_perturb if perm == "invconv" else 0.0)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.floor(torch.rand(batch, 3, H, W, generator=g) * 256.0) / 256.0
    noise = torch.rand(batch, 3, H, W, generator=g) / 256
    gx = torch.randn(batch, 3, H, W, generator=g)
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd, cfg, perm_tables=tables)
        z, eps = encode_latents(x, sd, cfg, tables)
    return cfg, sd, z, eps, gx


def encode_latents(x, sd, cfg, tables=None):
    """(z, [eps] in decode order) of the oracle's encode, the dtype of x."""
    z, eps = x, []
    for kind, i, _ in O.flow_layout(cfg):
        p = f"flow.layers.{i}."
        if kind == "squeeze":
            z = O.squeeze2d(z, 2)
        elif kind == "step":
            z, _ = O.flowstep(z, 0.0, sd, p, cfg["flow_permutation"], cfg["flow_coupling"], reverse=False,
                              perm_tables=None if tables is None else tables[i])
        else:
            eps.append(LO.split_eps(z, sd, p)["eps"])
            z, _ = O.split2d(z, 0.0, sd, p, reverse=False)
    return z, eps[::-1]


def decode_margin(z, eps, sd, cfg, tables=None):
    """Smallest |pre-activation| of any ReLU of the decode (the dtype of the inputs): `O.flow_decode`'s walk with a look inside
    every coupling network."""
    m = float("inf")
    it = iter(eps)
    with torch.no_grad():
        for kind, i, _ in reversed(O.flow_layout(cfg)):
            p = f"flow.layers.{i}."
            if kind == "squeeze":
                z = O.unsqueeze2d(z, 2)
            elif kind == "step":
                z1, _ = O.split_channel(z, "simple")
                h = O.conv2d_actnorm(z1, sd[p + "f.0.weight"], sd[p + "f.0.actnorm.bias"], sd[p + "f.0.actnorm.logs"])
                m = min(m, float(h.abs().min()))
                h = O.conv2d_actnorm(torch.relu(h), sd[p + "f.2.weight"], sd[p + "f.2.actnorm.bias"], sd[p + "f.2.actnorm.logs"])
                m = min(m, float(h.abs().min()))
                z, _ = O.flowstep(z, 0.0, sd, p, cfg["flow_permutation"], cfg["flow_coupling"], reverse=True,
                                  perm_tables=None if tables is None else tables[i])
            else:
                z, _ = O.split2d(z, 0.0, sd, p, reverse=True, eps=next(it))
    return m


def decode_grads(z, eps, gx, sd, cfg, tables=None, dtype=torch.float64):
    """(x, g_z, [g_eps]) by autograd through `O.flow_decode` in ``dtype``."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    zl = z.to(dtype).requires_grad_(True)
    el = [e.to(dtype).requires_grad_(True) for e in eps]
    with torch.enable_grad():
        x = O.flow_decode(zl, sdd, cfg, el, perm_tables=tables)
        grads = torch.autograd.grad(x, [zl] + el, gx.to(dtype))
    return x.detach(), grads[0], list(grads[1:])


@functools.lru_cache(maxsize=None)
def reference(image, hidden, K, L, batch, seed, zeros_std, perm="invconv", coup="affine", stable=False, np_seed=None):
    """A case with its fp64 reference and margin, computed once per process and shared (callers must not modify it).
    ``np_seed``: the numpy seed under which a model with a fixed permutation draws its tables (perm != 'invconv')."""
    tables = perm_tables(image, hidden, K, L, batch, perm, coup, np_seed) if perm != "invconv" else None
    prev = O.STABLE_LOGDET
    O.STABLE_LOGDET = bool(stable)
    try:
        cfg, sd, z, eps, gx = build_case(image, hidden, K, L, batch, seed, zeros_std, perm, coup, tables)
        sd64 = {k: v.double() for k, v in sd.items()}
        margin = decode_margin(z.double(), [e.double() for e in eps], sd64, cfg, tables)
        x64, gz, geps = decode_grads(z, eps, gx, sd, cfg, tables)
    finally:
        O.STABLE_LOGDET = prev
    return dict(cfg=cfg, sd=sd, z=z, eps=eps, gx=gx, margin=margin, x=x64, gz=gz, geps=geps, tables=tables)


def perm_tables(image, hidden, K, L, batch, perm, coup, np_seed):
    """The tables a `Glow` of this config draws at construction under np.random.seed(np_seed) (no GPU involved)."""
    import pytorch_glow_amd as G
    from pytorch_glow_amd.misc import util
    H, W = image_hw(image)
    cfg = O.default_cfg(image_shape=(H, W, 3), hidden_channels=hidden, K=K, L=L, flow_permutation=perm, flow_coupling=coup, batch=batch)
    np.random.seed(np_seed)
    proto = G.Glow(hps_for(cfg, batch))
    return {i: (torch.as_tensor(getattr(l, perm).indices), torch.as_tensor(getattr(l, perm).indices_inverse))
            for i, l in enumerate(proto.flow.layers) if hasattr(l, perm)}


def hps_for(cfg, batch, device="cuda:0"):
    from pytorch_glow_amd.misc import util
    return util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False,
                      flow_permutation=cfg["flow_permutation"], flow_coupling=cfg["flow_coupling"]),
        optim=dict(num_batch_train=batch), dataset=dict(num_classes=1), device=dict(graph=[device])))


def beyond(a, ref):
    """(fraction of entries beyond the project's gradient bound 2e-4 max|ref| + 1e-7, worst error / max|ref|)."""
    a, ref = a.detach().cpu().double(), ref.double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    scale = float(ref.abs().max())
    err = (a - ref).abs()
    return float((err > 2e-4 * scale + 1e-7).double().mean()), float(err.max()) / max(scale, 1e-300)
