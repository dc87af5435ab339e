"""Gradient parity (-m gpu): the HIP training step (forward with tape + reverse sweep, through the C ABI and one
torch.autograd.Function) against torch autograd run on the CPU oracle with identical weights, inputs and noise.
Tolerance: |g_hip - g_ref| <= 2e-4 * max|g_ref| + 1e-7 per parameter tensor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

DEV = "cuda:0"


def hps_for(cfg, batch):
    return util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False,
                      flow_permutation=cfg["flow_permutation"], flow_coupling=cfg["flow_coupling"]),
        optim=dict(num_batch_train=batch), dataset=dict(num_classes=1), device=dict(graph=["cuda:0"])))


def oracle_grads(cfg, sd, x, noise, tables=None):
    with torch.enable_grad():
        leaf = {k: v.clone().requires_grad_(k != "h_top") for k, v in sd.items()}
        xr = x.clone().requires_grad_(True)
        z, nll, _ = O.glow_forward(xr, noise, leaf, cfg, perm_tables=tables)
        loss = nll.mean()
        loss.backward()
    return {k: v.grad for k, v in leaf.items() if v.grad is not None}, xr.grad, loss.item()


@pytest.mark.parametrize("coup,perm,hidden,image", [
    ("affine", "invconv", 32, 16),      # generic (direct) kernels everywhere
    ("additive", "reverse", 32, 16),
    ("affine", "invconv", 128, 32),     # MFMA forward kernels (f.0 halo, GEMM, tail) feeding the tape
    ("additive", "shuffle", 64, 32),
])
def test_glow_gradients_vs_autograd_oracle(coup, perm, hidden, image):
    batch = 3
    cfg = O.default_cfg(image_shape=(image, image, 3), hidden_channels=hidden, K=2, L=2, flow_permutation=perm,
                        flow_coupling=coup, batch=batch)
    np.random.seed(1)
    glow = G.Glow(hps_for(cfg, batch))
    g = torch.Generator().manual_seed(5)
    sd = {k: v.detach().clone() for k, v in glow.state_dict().items()}
    for k in sd:
        if k == "h_top":
            continue
        if k.endswith("invconv.weight"):
            c = sd[k].shape[0]
            sd[k] = torch.from_numpy(np.linalg.qr(np.random.randn(c, c))[0].astype("float32")) + 0.05 * torch.randn(c, c, generator=g)
        elif k.endswith("logs") or k.endswith("bias"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif ".f.4." in k or "conv2d_zeros" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.02
        else:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    tables = None
    if perm != "invconv":
        tables = {i: (getattr(l, perm).indices, getattr(l, perm).indices_inverse)
                  for i, l in enumerate(glow.flow.layers) if hasattr(l, perm)}
    glow = glow.to(DEV).train()
    x = torch.rand(batch, 3, image, image, generator=g)
    noise = torch.rand(batch, 3, image, image, generator=g) / 256
    ref, gx_ref, loss_ref = oracle_grads(cfg, sd, x, noise, tables)

    with torch.enable_grad():
        xd = x.to(DEV).requires_grad_(True)
        z, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    assert abs(loss.item() - loss_ref) < 1e-4
    worst = ("", 0.0)
    for name, p in glow.named_parameters():
        if name == "h_top":
            assert p.grad is None          # detached in the reference as well (model.py:372)
            continue
        assert p.grad is not None, name
        r = ref[name]
        err = (p.grad.cpu() - r).abs().max().item()
        bound = 2e-4 * r.abs().max().item() + 1e-7
        if err / bound > worst[1]:
            worst = (name, err / bound)
        assert err <= bound, f"{name}: err {err:.3e} vs bound {bound:.3e} (|g| max {r.abs().max().item():.3e})"
    egx = (xd.grad.cpu() - gx_ref).abs().max().item()
    assert egx <= 2e-4 * gx_ref.abs().max().item() + 1e-7, f"dL/dx err {egx:.3e}"
    print(f"worst parameter {worst[0]} at {worst[1]:.2f} of its bound; dL/dx err {egx:.2e}")


@pytest.mark.parametrize("coup,perm", [("affine", "invconv"), ("additive", "reverse")])
def test_glow_gradients_vs_the_reference_recorded_goldens(coup, perm):
    """the HIP training step against gradients recorded from the REFERENCE's own backward
    (tests/golden/g7_glow_tiny_grads.npz: tiny Glow, every parameter + dL/dx) -- N1's parity pinned directly, not through the
    oracle's autograd.  Same tolerance as the oracle comparison: 2e-4 max|g| + 1e-7 per tensor."""
    from conftest import load_golden, sub
    g = sub(load_golden("g7_glow_tiny"), f"{coup}_{perm}.")
    gr = sub(load_golden("g7_glow_tiny_grads"), f"{coup}_{perm}.")
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=32, K=2, L=2, flow_permutation=perm, flow_coupling=coup, batch=4)
    np.random.seed(5)
    glow = G.Glow(hps_for(cfg, 4))
    glow.load_state_dict(sub(g, "sd."))
    glow.set_actnorm_inited()
    if perm != "invconv":       # the fixed permutation tables are attributes, not parameters: the fixture's
        for i, layer in enumerate(glow.flow.layers):
            if hasattr(layer, perm):
                getattr(layer, perm).indices = g[f"indices.{i}"]
                getattr(layer, perm).indices_inverse = g[f"indices_inverse.{i}"]
    glow = glow.to(DEV).train()
    with torch.enable_grad():
        xd = g["x"].to(DEV).requires_grad_(True)
        _, nll, _ = glow.normal_flow(xd, None, noise=g["noise"].to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    assert abs(loss.item() - float(gr["loss"])) < 1e-4
    ref = sub(gr, "grad.")
    for name, p in glow.named_parameters():
        if name == "h_top":
            assert p.grad is None and name not in ref
            continue
        r = ref[name]
        err = (p.grad.cpu() - r).abs().max().item()
        assert err <= 2e-4 * r.abs().max().item() + 1e-7, f"{name}: err {err:.3e} (|g| max {r.abs().max().item():.3e})"
    egx = (xd.grad.cpu() - gr["dx"]).abs().max().item()
    assert egx <= 2e-4 * gr["dx"].abs().max().item() + 1e-7, f"dL/dx err {egx:.3e}"


def test_learned_top_prior_trains_on_the_hip_path():
    """VERDICT r4 missing #4: ablation.learn_top on the training path (network/model.py:362-379).  Forward (z, nll) and every
    gradient of mean(nll) -- learn_top.bias / .logs through the prior's own terms, everything else through the HIP sweep, which
    takes the learned mean / logs for d logp / d z -- against the vectors the REFERENCE recorded (g7_glow_tiny_learn_top.npz)."""
    from conftest import load_golden, sub
    g = load_golden("g7_glow_tiny_learn_top")
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=32, K=2, L=2, flow_permutation="invconv", flow_coupling="affine", batch=4)
    hps = hps_for(cfg, 4)
    hps.ablation.learn_top = True
    np.random.seed(7)
    glow = G.Glow(hps)
    glow.load_state_dict(sub(g, "sd."))
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    with torch.enable_grad():
        xd = g["x"].to(DEV).requires_grad_(True)
        z, nll, _ = glow.normal_flow(xd, None, noise=g["noise"].to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    assert (z.detach().cpu() - g["z"]).abs().max().item() < 1e-4 and (nll.detach().cpu() - g["nll"]).abs().max().item() < 1e-4
    ref = sub(g, "grad.")
    for name, p in glow.named_parameters():
        if name == "h_top":
            assert p.grad is None
            continue
        r = ref[name]
        got = p.grad.cpu() if p.grad is not None else torch.zeros_like(r)       # (learn_top.weight multiplies zeros: no gradient)
        err = (got - r).abs().max().item()
        assert err <= 2e-4 * r.abs().max().item() + 1e-7, f"{name}: err {err:.3e} (|g| max {r.abs().max().item():.3e})"
    assert float(ref["learn_top.bias"].abs().max()) > 0 and glow.learn_top.bias.grad is not None
    egx = (xd.grad.cpu() - g["dx"]).abs().max().item()
    assert egx <= 2e-4 * g["dx"].abs().max().item() + 1e-7, f"dL/dx err {egx:.3e}"
    # and the loop takes the autograd route for such a model (Glow.loss_and_grads is the fixed-prior fast path)
    from pytorch_glow_amd import parallel
    opt = torch.optim.Adam(glow.parameters(), lr=1e-5)
    l2, _ = parallel.train_step(glow, opt, g["x"].to(DEV), world=1)
    assert torch.isfinite(l2)


def test_train_steps_reduce_the_loss():
    """Three optimiser steps of the reference's training loop (trainer.py:123-150) on the HIP path: data-dependent
    ActNorm init, forward with tape, HIP backward, clip by value 5 / by norm 100, Adam -- the loss must fall and every
    parameter stay finite."""
    from pytorch_glow_amd import parallel
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = O.default_cfg(image_shape=(32, 32, 3), hidden_channels=128, K=2, L=2, batch=8)
    glow = G.Glow(hps_for(cfg, 8)).to(DEV).train()
    x = torch.rand(8, 3, 32, 32, device=DEV)
    with torch.no_grad():
        glow.normal_flow(x, None)                      # first training-mode forward: ActNorm init
    opt = torch.optim.Adam([p for p in glow.parameters()], lr=1e-3, betas=(0.9, 0.9999), eps=1e-8)
    losses = []
    for _ in range(4):
        loss, gnorm = parallel.train_step(glow, opt, x, world=1, max_grad_clip=5, max_grad_norm=100)
        losses.append(loss.item())
        assert torch.isfinite(gnorm)
    assert losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in glow.parameters())
    assert glow.h_top.grad is None


def _celeba_geometry_model(K, batch, seed=11):
    """Config-B channel geometry (64x64x3, L=3, hidden 512, affine + invconv) with a reduced K so the CPU autograd oracle
    finishes in seconds; bench-style seeded weights (Conv2dZeros ~ N(0, 0.002)) and data-dependent ActNorm init."""
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=seed, invconv_perturb=0.02)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    glow = G.Glow(hps_for(cfg, batch))
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    return cfg, sd, glow.to(DEV).train(), x, noise


def test_gradients_at_celeba_geometry_vs_autograd_oracle():
    """Same check on the headline model's layer shapes (C = 12/24/48, hidden 512, 32x32 / 16x16 / 8x8): these are the shapes
    that take the LDS-DMA GEMM, the DMA tail kernels and the split-K weight-gradient GEMMs.

    The yardstick is the oracle run in fp64.  With 2M hidden activations per layer a few ReLU pre-activations land within
    fp32 rounding of zero (measured: |x| = 6.9e-8 in layer 2's f.2, channel 81), and ANY fp32 implementation -- the fp32
    oracle included, which is off by 7e-3 of max|g| on such rows -- may take the other branch there: one flipped element
    changes one row of one weight gradient.  So: at most 1% of a parameter's entries may exceed the tight bound (a flip
    touches 1/512 of them), and none may exceed 5% of max|g|."""
    cfg, sd, glow, x, noise = _celeba_geometry_model(K=3, batch=4)
    ref, gx_ref, loss_ref = oracle_grads(cfg, {k: v.double() for k, v in sd.items()}, x.double(), noise.double())
    with torch.enable_grad():
        xd = x.to(DEV).requires_grad_(True)
        z, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    assert abs(loss.item() - loss_ref) < 1e-4
    for name, p in glow.named_parameters():
        if name == "h_top":
            continue
        r = ref[name]
        err = (p.grad.cpu().double() - r).abs()
        scale = r.abs().max().item()
        outliers = (err > 2e-4 * scale + 1e-7).double().mean().item()
        assert outliers <= 0.01, f"{name}: {outliers:.2%} of the entries off by more than 2e-4 of max|g| = {scale:.3e}"
        assert err.max().item() <= 0.05 * scale + 1e-7, f"{name}: max err {err.max().item():.3e}, max|g| {scale:.3e}"
    egx = (xd.grad.cpu().double() - gx_ref).abs()
    gscale = gx_ref.abs().max().item()
    assert (egx > 2e-4 * gscale + 1e-7).double().mean().item() <= 0.01 and egx.max().item() <= 0.05 * gscale, \
        f"dL/dx err {egx.max().item():.3e} vs max|g| {gscale:.3e}"


@pytest.mark.parametrize("image,batch", [(64, 28), (128, 7), (256, 2)])
def test_one_wave_kernel_taping_and_backward_instances_vs_fp64_autograd_oracle(image, batch):
    """the TAPING (MODE 1) and BACKWARD (MODE 2) instances of k_cnet1w against the fp64 autograd oracle
    itself -- not against k_cnet -- at hidden 512, L = 1, K = 1 on every level-1 width the configs run it at: 32-pixel rows
    (64x64 input, batch 28 = 224 tiles), 64-pixel rows (128x128, batch 7 = 224 tiles), 128-pixel rows (256x256, batch 2 =
    256 tiles); the instances asserted from the run-time launch counters.  Same rule as the celeba-geometry test above (a ReLU
    pre-activation within fp32 rounding of zero may flip one row of one weight gradient): at most 1 % of a tensor's entries
    beyond 2e-4 max|g| + 1e-7, none beyond 5 %.  Reference: network/model.py:82-117, network/trainer.py:123-150."""
    cfg = O.default_cfg(image_shape=(image, image, 3), K=1, L=1, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=31, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(31)
    x = torch.rand(batch, 3, image, image, generator=g)
    noise = torch.rand(batch, 3, image, image, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    glow = G.Glow(hps_for(cfg, batch))
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    ref, gx_ref, loss_ref = oracle_grads(cfg, {k: v.double() for k, v in sd.items()}, x.double(), noise.double())
    plan = glow.flow.plan_for(x.to(DEV))
    plan.launch_counts(reset=True)
    with torch.enable_grad():
        xd = x.to(DEV).requires_grad_(True)
        z, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    counts = plan.launch_counts(reset=True)
    # ("k_cnet(tape)" / "k_cnet(bwd)" count every fused coupling launch; the 1w keys say that cnet1w_sh.hip took it.)  At 128-pixel rows
    # the transposed network (12 channels in) has no fused backward instance -- its input tile with both halo rows needs two T units
    # per wave (cnet_select: upw = 2) -- so that sweep runs layer by layer on the exact-fp32 kernels: the gradients below are still
    # the taping k_cnet1w's tape against the fp64 oracle
    want_bwd = 0 if image == 256 else 1
    assert counts.get("k_cnet(tape)", 0) == 1 and counts.get("k_cnet1w(tape)", 0) == 1, counts
    assert counts.get("k_cnet(bwd)", 0) == want_bwd and counts.get("k_cnet1w(bwd)", 0) == want_bwd, counts
    assert abs(loss.item() - loss_ref) < 1e-4
    z_ref, nll_ref, _ = O.glow_forward(x, noise, sd, cfg)
    assert (z.detach().cpu() - z_ref).abs().max().item() <= 1e-4 and (nll.detach().cpu() - nll_ref).abs().max().item() <= 1e-4
    worst = ("", 0.0)
    for name, p in glow.named_parameters():
        if name == "h_top":
            continue
        r = ref[name]
        err = (p.grad.cpu().double() - r).abs()
        scale = r.abs().max().item()
        outliers = (err > 2e-4 * scale + 1e-7).double().mean().item()
        assert outliers <= 0.01, f"{name}: {outliers:.2%} of the entries off by more than 2e-4 of max|g| = {scale:.3e}"
        assert err.max().item() <= 0.05 * scale + 1e-7, f"{name}: max err {err.max().item():.3e}, max|g| {scale:.3e}"
        worst = max(worst, (name, err.max().item() / (2e-4 * scale + 1e-7)), key=lambda t: t[1])
    egx = (xd.grad.cpu().double() - gx_ref).abs()
    gscale = gx_ref.abs().max().item()
    assert (egx > 2e-4 * gscale + 1e-7).double().mean().item() <= 0.01 and egx.max().item() <= 0.05 * gscale, \
        f"dL/dx err {egx.max().item():.3e} vs max|g| {gscale:.3e}"
    print(f"{image}x{image} batch {batch}: worst {worst[0]} at {worst[1]:.2f} of the tight bound; dL/dx {egx.max().item():.2e} {counts}")


@pytest.mark.parametrize("coup,perm,hidden", [("additive", "reverse", 512), ("additive", "shuffle", 256), ("affine", "invconv", 256)])
def test_k_cnet_training_step_other_couplings_and_widths_vs_autograd_oracle(coup, perm, hidden):
    """The taping / backward k_cnet launches beyond the headline's affine + invconv at hidden 512: additive coupling (f.4 has C/2
    output channels, so the backward launch's first layer has C/2 inputs and its last C/2 outputs), permutations without a
    matrix, hidden 256.  Every gradient against autograd through the fp64 oracle; the kernels asserted from the launch counters."""
    K, batch = 2, 4
    cfg = O.default_cfg(K=K, batch=batch, hidden_channels=hidden, flow_coupling=coup, flow_permutation=perm)
    np.random.seed(3)
    glow = G.Glow(hps_for(cfg, batch))
    g = torch.Generator().manual_seed(29)
    sd = {k: v.detach().clone() for k, v in glow.state_dict().items()}
    for k in sd:
        if k == "h_top" or not sd[k].is_floating_point():
            continue
        if k.endswith("invconv.weight"):
            c = sd[k].shape[0]
            sd[k] = torch.from_numpy(np.linalg.qr(np.random.randn(c, c))[0].astype("float32")) + 0.02 * torch.randn(c, c, generator=g)
        elif k.endswith("logs") or k.endswith("bias"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif ".f.4." in k or "conv2d_zeros" in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.01
        elif ".f.2." in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * (1.0 / hidden) ** 0.5
        else:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    tables = None
    if perm != "invconv":
        tables = {i: (getattr(l, perm).indices, getattr(l, perm).indices_inverse)
                  for i, l in enumerate(glow.flow.layers) if hasattr(l, perm)}
    glow = glow.to(DEV).train()
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    ref, _, loss_ref = oracle_grads(cfg, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, x.double(), noise.double(),
                                    tables)
    with torch.enable_grad():
        z, nll, _ = glow.normal_flow(x.to(DEV), None, noise=noise.to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    counts = glow.flow.plan_for(x.to(DEV)).launch_counts()
    assert counts.get("k_cnet(tape)", 0) == 3 * K and counts.get("k_cnet(bwd)", 0) == 3 * K, counts
    assert abs(loss.item() - loss_ref) < 1e-4
    for name, p in glow.named_parameters():
        if name == "h_top" or p.grad is None:
            continue
        r = ref[name]
        err = (p.grad.cpu().double() - r).abs()
        scale = r.abs().max().item()
        outliers = (err > 2e-4 * scale + 1e-7).double().mean().item()
        assert outliers <= 0.01, f"{name}: {outliers:.2%} of the entries off by more than 2e-4 of max|g| = {scale:.3e}"
        assert err.max().item() <= 0.05 * scale + 1e-7, f"{name}: max err {err.max().item():.3e}, max|g| {scale:.3e}"


def test_log_scale_gradients_from_dw_with_dominant_actnorm_biases():
    """The backward k_cnet path derives d logs of the hidden ActNorms from the weight and bias gradients,
    d logs[r] = 3 (<W[r], dW[r]> + b[r] db[r]), instead of a pass over the activations.  The two terms cancel when |b| is large
    against the spread of the convolution output -- the regime a trained ActNorm can reach (not the data-dependent init, which
    centres the output).  Here half of the hidden channels get biases of +2.5 / -1.5 (in units of the output's std) and log-scales
    of +-0.1 on top of the init; bias and log-scale gradients of f.0 / f.2 against the fp64 oracle at the usual bound."""
    K, batch = 2, 4
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=17, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(17)
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    for k in list(sd):
        if (".f.0.actnorm." in k or ".f.2.actnorm." in k):
            v = sd[k]
            ch = torch.arange(v.numel()).reshape(v.shape)
            if k.endswith("bias"):      # bias is added before the scale exp(3 logs): shift in units of the output's std
                logs = sd[k.replace("bias", "logs")]
                shift = torch.where(ch % 4 == 0, 2.5, torch.where(ch % 4 == 1, -1.5, 0.0)) / torch.exp(3 * logs)
                sd[k] = v + shift.to(v.dtype)
    for k in list(sd):
        if (".f.0.actnorm.logs" in k or ".f.2.actnorm.logs" in k):
            v = sd[k]
            ch = torch.arange(v.numel()).reshape(v.shape)
            sd[k] = v + torch.where(ch % 2 == 0, 0.1, -0.1).to(v.dtype) / 3
    glow = G.Glow(hps_for(cfg, batch))
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    ref, _, loss_ref = oracle_grads(cfg, {k: v.double() for k, v in sd.items()}, x.double(), noise.double())
    with torch.enable_grad():
        z, nll, _ = glow.normal_flow(x.to(DEV), None, noise=noise.to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    assert glow.flow.plan_for(x.to(DEV)).launch_counts().get("k_cnet(bwd)", 0) == 3 * K
    assert abs(loss.item() - loss_ref) < 1e-4
    checked = 0
    for name, p in glow.named_parameters():
        if ".actnorm." not in name or not (".f.0." in name or ".f.2." in name):
            continue
        r = ref[name]
        err = (p.grad.cpu().double() - r).abs()
        scale = r.abs().max().item()
        outliers = (err > 2e-4 * scale + 1e-7).double().mean().item()
        assert outliers <= 0.01 and err.max().item() <= 0.05 * scale + 1e-7, \
            f"{name}: {outliers:.2%} beyond 2e-4 of max|g| = {scale:.3e}, max err {err.max().item():.3e}"
        checked += 1
    assert checked == 3 * K * 4


def test_forward_after_an_optimizer_step_matches_oracle():
    """The optimiser updates the parameters in place; the next forward must see them (derived data is re-packed from the
    live parameters every training step) and agree with the oracle evaluated on the SAME updated state_dict."""
    from pytorch_glow_amd import parallel
    cfg, sd, glow, x, noise = _celeba_geometry_model(K=3, batch=4)
    opt = torch.optim.Adam(list(glow.parameters()), lr=1e-4, betas=(0.9, 0.9999), eps=1e-8)
    xd = x.to(DEV)
    loss0, _ = parallel.train_step(glow, opt, xd, world=1, max_grad_clip=5, max_grad_norm=100)
    sd1 = {k: v.detach().cpu().clone() for k, v in glow.state_dict().items()}
    assert max((sd1[k] - sd[k]).abs().max().item() for k in sd if k != "h_top") > 5e-5      # the step moved them
    z_ref, nll_ref, _ = O.glow_forward(x, noise, sd1, cfg)
    assert torch.isfinite(nll_ref).all()
    for mode in ("eval", "train"):
        getattr(glow, mode)()
        z, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
        assert torch.isfinite(nll).all(), (mode, nll)
        assert (nll.cpu() - nll_ref).abs().max().item() < 1e-4, (mode, nll.cpu(), nll_ref)
        assert (z.cpu() - z_ref).abs().max().item() < 1e-4


def test_train_loop_follows_the_profile_schedule():
    """TrainLoop = the reference Trainer's per-step state (trainer.py:85-150): ActNorm init on the first batch, lr from the
    profile's scheduler written into the optimiser before each step, clipping thresholds from hps.ablation."""
    from pytorch_glow_amd import training
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = O.default_cfg(image_shape=(32, 32, 3), hidden_channels=128, K=2, L=2, batch=8)
    hps = hps_for(cfg, 8)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-4))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)
    glow = G.Glow(hps).to(DEV)
    loop = training.TrainLoop(glow, hps)
    x = torch.rand(8, 3, 32, 32, device=DEV)
    assert not glow.actnorm_inited()
    losses, lrs = [], []
    for _ in range(6):
        loss, _ = loop.step(x)
        losses.append(loss.item())
        lrs.append(loop.optimizer.param_groups[0]["lr"])
    assert glow.actnorm_inited() and loop.global_step == 6
    assert lrs[:5] == pytest.approx([1e-3 * (i + 1) / 5 for i in range(5)]) and lrs[5] == pytest.approx(1e-3 * (5 / 6) ** 0.5)
    assert losses[-1] < losses[0]


def test_inference_and_training_weight_images_do_not_go_stale():
    """glowhip_plan_pack_for refreshes only the images one kernel family reads (split-half for inference, exact-fp32 +
    transposed for training).  Alternating the two, and updating a parameter in place in between, must never leave a kernel
    with an old image."""
    cfg, sd, glow, x, noise = _celeba_geometry_model(K=2, batch=4)
    xd, nd = x.to(DEV), noise.to(DEV)
    glow.eval()
    z0, nll0, _ = glow.normal_flow(xd, None, noise=nd)                       # inference images
    glow.train()
    with torch.enable_grad():
        zt, nllt, _ = glow.normal_flow(xd, None, noise=nd)                   # training images only
        nllt.mean().backward()
    assert (nllt.detach() - nll0).abs().max().item() < 1e-5                  # two kernel families, same function
    glow.eval()
    z1, nll1, _ = glow.normal_flow(xd, None, noise=nd)                       # inference again
    assert torch.equal(z0, z1) and torch.equal(nll0, nll1)
    with torch.no_grad():                                                    # in-place update, as an optimiser does
        f = glow.flow.layers[1].f                                            # every packed weight of one coupling net
        f[0].weight.mul_(1.25); f[2].weight.mul_(1.25)
        f[4].weight.add_(0.004 * torch.randn_like(f[4].weight))
    sd2 = {k: v.detach().cpu().clone() for k, v in glow.state_dict().items()}
    z_ref, nll_ref, _ = O.glow_forward(x, noise, sd2, cfg)
    z2, nll2, _ = glow.normal_flow(xd, None, noise=nd)
    assert (z2 - z1).abs().max().item() > 1e-3                               # the update is visible at all
    assert (z2.cpu() - z_ref).abs().max().item() < 1e-4 and (nll2.cpu() - nll_ref).abs().max().item() < 1e-4
    glow.train()
    with torch.enable_grad():
        zt2, nllt2, _ = glow.normal_flow(xd, None, noise=nd)
    assert (nllt2.detach().cpu() - nll_ref).abs().max().item() < 1e-4


def test_tiny_gradients_behind_near_zero_tail_weights_purely_relative():
    """Early training, B = 64: dL/d(objective) = 1 / (B ln2 CHW) ~ 1.8e-6 and f.4 (Conv2dZeros) is still ~0, so the gradient that
    enters f.2's input-gradient GEMM as fp16 pairs is ~1e-8 .. 1e-10 -- below fp16's normal range unless it is pre-scaled
    (k_act_bwd_sh: 2^k = B ln2 CHW, undone exactly in the GEMM epilogue).  Checked here with NO absolute floor in the bound:
    config-B geometry (hidden 512, the split-half dgrad path), f.4 weights ~ N(0, 1e-5), and the loss divided by 16 on a
    batch of 4 so the gradients have the magnitude of a batch of 64."""
    K, batch = 2, 4
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=13, invconv_perturb=0.02, zeros_std=1e-5)
    g = torch.Generator().manual_seed(13)
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    glow = G.Glow(hps_for(cfg, batch))
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    ref, gx_ref, _ = oracle_grads(cfg, {k: v.double() for k, v in sd.items()}, x.double(), noise.double())
    with torch.enable_grad():
        z, nll, _ = glow.normal_flow(x.to(DEV), None, noise=noise.to(DEV))
        (G.Glow.generative_loss(nll) / 16.0).backward()
    checked = 0
    for name, p in glow.named_parameters():
        if not (".f.0." in name or ".f.2." in name):     # everything that lies behind f.2's input-gradient GEMM
            continue
        r = ref[name] / 16.0
        scale = r.abs().max().item()
        assert 0 < scale < 1e-3, (name, scale)            # these ARE the tiny gradients
        err = (p.grad.cpu().double() - r).abs()
        # A ReLU pre-activation within fp32 rounding of zero (this seed: ONE of 17 M, f.2 of the first step, +1.3e-7 in the fp64
        # oracle) may take the other side of the kink in any fp32 evaluation; the gradient is discontinuous there, and that one
        # pixel moves its f.2 row by ~1e-2 of max|g| (a row is a random-sign sum over 4096 pixels) and everything behind it by ~1e-3.
        # So: the bulk of the entries at 2e-4, the RMS at 1e-3, the worst entry at 5e-2 -- all relative to max|g|, no absolute floor
        # (a gradient flushed below fp16's range would be off by O(1) of max|g| in most entries).
        outliers = (err > 2e-4 * scale).double().mean().item()
        assert outliers <= 0.25, f"{name}: {outliers:.2%} of the entries off by more than 2e-4 of max|g| = {scale:.3e}"
        rms = err.pow(2).mean().sqrt().item()
        assert rms <= 1e-3 * scale, f"{name}: rms err {rms:.3e}, max|g| {scale:.3e}"
        assert err.max().item() <= 0.05 * scale, f"{name}: max err {err.max().item():.3e}, max|g| {scale:.3e}"
        checked += 1
    assert checked == 3 * K * 6


def test_training_step_runs_on_k_cnet_and_agrees_with_the_per_layer_kernels():
    """The training forward of a config-B FlowStep is the product path's two launches (k_cnet MODE 1 storing h1 / h2 and their
    sign bits from its epilogues, the finishing kernel storing hout, the step output and the next step's mixer output), its
    input-gradient chain ONE k_cnet launch on the transposed weight images (MODE 2: ReLU masks from the sign bits, g_u2 / g_u0
    stored for the weight-gradient GEMMs, bias gradients as row sums inside those GEMMs, log-scale gradients from dW and db):
    asserted from the launch counters, and compared -- z, nll, every gradient -- with the same step on the per-layer kernels
    (debug flags 0x40000000: forward, 0x80000000: backward), which the oracle tests above pin separately."""
    from pytorch_glow_amd import _lib
    K, batch = 2, 4
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=21, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    res = {}
    for flag in (_lib.DBG.TRAIN_PER_LAYER_FWD, _lib.DBG.TRAIN_PER_LAYER_BWD, 0):
        with _lib.debug_flags(flag):
            glow = G.Glow(hps_for(cfg, batch))
            glow.load_state_dict(sd)
            glow.set_actnorm_inited()
            glow = glow.to(DEV).train()
            with torch.enable_grad():
                z, nll, _ = glow.normal_flow(x.to(DEV), None, noise=noise.to(DEV))
                G.Glow.generative_loss(nll).backward()
            counts = glow.flow.plan_for(x.to(DEV)).launch_counts()
            res[flag] = (z.detach().cpu(), nll.detach().cpu(), {n: p.grad.cpu().double() for n, p in glow.named_parameters()
                                                                 if p.grad is not None}, counts)
    z0, n0, g0, c0 = res[_lib.DBG.TRAIN_PER_LAYER_FWD]
    assert c0.get("k_cnet(tape)", 0) == 0 and c0.get("k_cnet(bwd)", 0) == 0, c0
    for flag, want_bwd in ((_lib.DBG.TRAIN_PER_LAYER_BWD, 0), (0, 3 * K)):
        z1, n1, g1, c1 = res[flag]
        assert c1.get("k_cnet(tape)", 0) == 3 * K and c1.get("k_cnet(bwd)", 0) == want_bwd, (hex(flag), c1)
        assert (z1 - z0).abs().max().item() <= 2e-5 and (n1 - n0).abs().max().item() <= 2e-6
        for name, a in g0.items():
            scale = a.abs().max().item()
            err = (g1[name] - a).abs()
            assert err.pow(2).mean().sqrt().item() <= 1e-3 * scale + 1e-9 and err.max().item() <= 0.05 * scale + 1e-8, \
                (hex(flag), name, scale, err.max().item())


@pytest.mark.parametrize("image,L,batch", [(64, 3, 28), (32, 1, 112), (128, 1, 7)])
def test_training_launches_on_the_one_wave_kernel_agree_with_k_cnet(image, L, batch):
    """Round 5: where level 1 gives 224 or more 128-pixel tiles (batch 28 at config-B geometry) the TRAINING step's launches of its
    FlowSteps run on k_cnet1w (cnet1w_sh.hip):
      * the taping forward -- h1 / h2 stay in registers and go to the tape from the epilogue pipeline, two pixels of one row per
        4-byte store after a quad-permute, sign words as k_cnet writes them;
      * the input-gradient chain (the transposed network: 12 channels in, 6 out) -- ReLU masks read from those sign words a block
        ahead, g_u2 / g_u0 stored as fp32 for the weight-gradient GEMMs, the partial sums for k_chanmix_bwd in k_cnet's layout;
    and f.2's weight-gradient GEMM behind it reads 128 x 256 tiles with eight waves per workgroup (k_wgrad_gemm_ps512; debug switch
    0x80000: the 128-column kernel);
    evidence from the run-time counters (config-B geometry: 32-pixel rows, four per tile; and a 32 x 32 input with L = 1: 16-pixel rows,
    eight per tile, 224 tiles at batch 112; a 128 x 128 input with L = 1: 64-pixel rows, two per tile, 224 tiles at batch 7).  With the debug switches 0x10000 (no k_cnet1w at all) / 0x40000 (taping on k_cnet1w, backward
    on k_cnet) the same step runs on k_cnet MODE 1 / 2 (pinned against the fp64 oracle above): z, nll and every gradient agree."""
    from pytorch_glow_amd import _lib
    K = 2
    cfg = O.default_cfg(image_shape=(image, image, 3), K=K, L=L, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=23, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(23)
    x = torch.rand(batch, 3, image, image, generator=g)
    noise = torch.rand(batch, 3, image, image, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    res = {}
    for flag in (_lib.DBG.NO_CNET1W, _lib.DBG.NO_CNET1W_BWD, _lib.DBG.WGRAD_NARROW, 0):
        with _lib.debug_flags(flag):
            glow = G.Glow(hps_for(cfg, batch))
            glow.load_state_dict(sd)
            glow.set_actnorm_inited()
            glow = glow.to(DEV).train()
            with torch.enable_grad():
                xd = x.to(DEV).requires_grad_(True)
                z, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
                G.Glow.generative_loss(nll).backward()
            counts = glow.flow.plan_for(x.to(DEV)).launch_counts()
            grads = {n: p.grad.cpu().double() for n, p in glow.named_parameters() if p.grad is not None}
            grads["dx"] = xd.grad.cpu().double()
            res[flag] = (z.detach().cpu(), nll.detach().cpu(), grads, counts)
    z0, n0, g0, c0 = res[_lib.DBG.NO_CNET1W]
    assert c0.get("k_cnet(tape)", 0) == L * K and c0.get("k_cnet1w(tape)", 0) == 0 and c0.get("k_cnet1w(bwd)", 0) == 0, c0
    for flag, want_bwd in ((_lib.DBG.NO_CNET1W_BWD, 0), (_lib.DBG.WGRAD_NARROW, K), (0, K)):
        z1, n1, g1, c1 = res[flag]
        assert c1.get("k_cnet(tape)", 0) == L * K and c1.get("k_cnet1w(tape)", 0) == K and c1.get("k_cnet(bwd)", 0) == L * K, c1
        assert c1.get("k_cnet1w(bwd)", 0) == want_bwd, (hex(flag), c1)
        assert torch.isfinite(n1).all()
        assert (z1 - z0).abs().max().item() <= 2e-5 and (n1 - n0).abs().max().item() <= 2e-6 * max(1.0, n0.abs().max().item())
        for name, a in g0.items():
            scale = a.abs().max().item()
            err = (g1[name] - a).abs()
            assert err.pow(2).mean().sqrt().item() <= 1e-3 * scale + 1e-9 and err.max().item() <= 0.05 * scale + 1e-8, \
                (hex(flag), name, scale, err.max().item())


def test_grouped_weight_gradient_launches_agree_with_the_per_layer_kernels():
    """The weight-gradient GEMMs of a FlowStep behind the backward k_cnet run grouped: all three in one launch where the pixel axis
    is short (<= 512 k-tiles of 32 pixels), f.2's own kernel + f.4 / f.0 as a pair where it is long (level 1 from 17 images on).
    Batch 20 has both (level 1: 640 k-tiles, levels 2 / 3: 160 / 40): asserted from the launch counters, every gradient compared
    with the same step's per-layer backward (debug flag 0x80000000: plain fp32 tape reads, one GEMM per launch, which the oracle
    tests pin separately)."""
    from pytorch_glow_amd import _lib
    K, batch = 1, 20
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=33, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(33)
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    sd = O.glow_init_actnorm(x[:4], noise[:4], sd, cfg)
    res = {}
    for flag in (_lib.DBG.TRAIN_PER_LAYER_BWD, 0):
        with _lib.debug_flags(flag):
            glow = G.Glow(hps_for(cfg, batch))
            glow.load_state_dict(sd)
            glow.set_actnorm_inited()
            glow = glow.to(DEV).train()
            with torch.enable_grad():
                z, nll, _ = glow.normal_flow(x.to(DEV), None, noise=noise.to(DEV))
                G.Glow.generative_loss(nll).backward()
            counts = glow.flow.plan_for(x.to(DEV)).launch_counts()
            res[flag] = ({n: p.grad.cpu().double() for n, p in glow.named_parameters() if p.grad is not None}, counts)
    g0, c0 = res[_lib.DBG.TRAIN_PER_LAYER_BWD]
    g1, c1 = res[0]
    assert c0.get("k_wgrad(trio)", 0) == 0 and c0.get("k_wgrad(pair)", 0) == 0, c0
    assert c1.get("k_wgrad(pair)", 0) == K and c1.get("k_wgrad(trio)", 0) == 2 * K and c1.get("k_cnet(bwd)", 0) == 3 * K, c1
    for name, a in g0.items():
        scale = a.abs().max().item()
        err = (g1[name] - a).abs()
        assert err.pow(2).mean().sqrt().item() <= 1e-3 * scale + 1e-9 and err.max().item() <= 0.05 * scale + 1e-8, \
            (name, scale, err.max().item())


@pytest.mark.parametrize("kind", ["adam", "adamax"])
def test_hip_optimizer_matches_torch_optim(kind):
    """csrc/optim.hip against torch.optim.Adam / Adamax + clip_grad_value_ + clip_grad_norm_ (network/trainer.py:142-150) over
    five steps on tensors of awkward sizes (one longer than a 2^16 chunk): parameters, both state tensors and the returned
    gradient norm at 1e-6 relative; state_dict interchange both ways."""
    from pytorch_glow_amd import training
    g = torch.Generator().manual_seed(3)
    shapes = [(512, 24, 3, 3), (1, 512, 1, 1), (48, 48), (7,), (70001,)]
    p_ref = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(DEV)) for s in shapes]
    p_hip = [torch.nn.Parameter(p.detach().clone()) for p in p_ref]
    args = dict(lr=1e-3, betas=(0.9, 0.9999), eps=1e-8, weight_decay=0)
    o_ref = (torch.optim.Adam if kind == "adam" else torch.optim.Adamax)(p_ref, **args)
    o_hip = (training.HipAdam if kind == "adam" else training.HipAdamax)(p_hip, **args)
    rel = lambda a, b: ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
    for step in range(5):
        grads = [torch.randn(s, generator=g).to(DEV) * (10.0 if step == 2 else 0.5) for s in shapes]
        for p, q, gr in zip(p_ref, p_hip, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        torch.nn.utils.clip_grad_value_(p_ref, 5.0)
        n_ref = torch.nn.utils.clip_grad_norm_(p_ref, 100.0)
        o_ref.step()
        n_hip = o_hip.fused_step(5.0, 100.0)
        assert abs(n_hip.item() - n_ref.item()) <= 1e-5 * n_ref.item()
        for p, q in zip(p_ref, p_hip):
            assert rel(q.detach(), p.detach()) < 1e-6 and rel(q.grad, p.grad) < 1e-6
    second = "exp_avg_sq" if kind == "adam" else "exp_inf"
    for p, q in zip(p_ref, p_hip):
        assert rel(o_hip.state[q]["exp_avg"], o_ref.state[p]["exp_avg"]) < 1e-6
        assert rel(o_hip.state[q][second], o_ref.state[p][second]) < 1e-6
    # state_dict interchange: torch -> hip and hip -> torch, then one more identical step
    o_hip2 = (training.HipAdam if kind == "adam" else training.HipAdamax)([torch.nn.Parameter(p.detach().clone()) for p in p_ref], **args)
    o_hip2.load_state_dict(o_ref.state_dict())
    o_ref2 = (torch.optim.Adam if kind == "adam" else torch.optim.Adamax)([torch.nn.Parameter(p.detach().clone()) for p in p_ref], **args)
    o_ref2.load_state_dict(o_hip.state_dict())
    grads = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    for o in (o_ref, o_hip2, o_ref2):
        for p, gr in zip(o.param_groups[0]["params"], grads):
            p.grad = gr.clone()
        o.step()
    for a, b, c in zip(o_ref.param_groups[0]["params"], o_hip2.param_groups[0]["params"], o_ref2.param_groups[0]["params"]):
        assert rel(b.detach(), a.detach()) < 1e-6 and rel(c.detach(), a.detach()) < 1e-6


@pytest.mark.parametrize("kind", ["adam", "adamax"])
def test_hip_optimizer_survives_reloading_its_own_state(kind):
    """the cached device chunk table holds the state addresses too.  step -> load_state_dict(own state_dict()) moves
    exp_avg / exp_avg_sq into fresh flat buffers; with the gradients written IN PLACE (same addresses as before) the next step
    must update the new buffers, not the freed ones, and keep matching torch.optim."""
    from pytorch_glow_amd import training
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 12, 3, 3), (48, 48), (70001,)]
    p_ref = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(DEV)) for s in shapes]
    p_hip = [torch.nn.Parameter(p.detach().clone()) for p in p_ref]
    args = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    o_ref = (torch.optim.Adam if kind == "adam" else torch.optim.Adamax)(p_ref, **args)
    o_hip = (training.HipAdam if kind == "adam" else training.HipAdamax)(p_hip, **args)
    for p, q in zip(p_ref, p_hip):
        p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
    second = "exp_avg_sq" if kind == "adam" else "exp_inf"
    rel = lambda a, b: ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
    for step in range(4):
        for p, q, s in zip(p_ref, p_hip, shapes):
            gr = torch.randn(s, generator=g).to(DEV)
            p.grad.copy_(gr); q.grad.copy_(gr)               # in place: the gradient addresses never change
        o_ref.step()
        o_hip.step()
        if step == 1:
            o_hip.load_state_dict(o_hip.state_dict())        # re-homes the state in new flat buffers
        for p, q in zip(p_ref, p_hip):
            assert rel(q.detach(), p.detach()) < 1e-6, step
            assert rel(o_hip.state[q]["exp_avg"], o_ref.state[p]["exp_avg"]) < 1e-6, step
            assert rel(o_hip.state[q][second], o_ref.state[p][second]) < 1e-6, step


def test_training_overflow_is_skipped_on_device_then_rerun_on_exact_fp32():
    """the training forward carries h1 through f.2 as fp16 pairs (|v| < 65504).  With f.0's ActNorm scale blown
    up so that h1 ~ 3e5 (the fp32 reference stays finite) the step's loss and gradient norm come out non-finite; the fused
    optimiser must then leave every parameter and its state untouched ON THE DEVICE (no host sync in the step), and
    TrainLoop's deferred check must run the batch again with the plan on the exact-fp32 family: loss = the oracle's, a real
    update applied, plan back on the product family."""
    from pytorch_glow_amd import training
    torch.manual_seed(0)
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=128, K=1, L=1, batch=4)
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=1e-3)
    k0, k2 = "flow.layers.1.f.0.actnorm.logs", "flow.layers.1.f.2.actnorm.logs"
    sd[k0] = sd[k0] + float(np.log(3e5)) / 3.0
    sd[k2] = sd[k2] - float(np.log(3e5)) / 3.0
    hps = hps_for(cfg, 4)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)
    glow = G.Glow(hps)
    sd["h_top"] = torch.zeros_like(glow.h_top)
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(4, 3, 16, 16, generator=g)
    _, nll_ref, _ = O.glow_forward(x, torch.zeros_like(x), sd, cfg)
    assert torch.isfinite(nll_ref).all()
    loop = training.TrainLoop(glow, hps)
    before = {k: v.detach().clone() for k, v in glow.state_dict().items()}
    loss, gnorm = loop.step(x.to(DEV))
    assert not torch.isfinite(loss) and not torch.isfinite(gnorm), (loss, gnorm)       # (the test's own sync)
    after = glow.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "a skipped step must not touch the parameters"
    assert loop.range_fallbacks == 0                                   # not looked at yet: the check is deferred
    loop.flush()
    assert loop.range_fallbacks == 1 and loop.diverged_steps == 0
    loss2, gnorm2 = loop.last_rerun
    # dequantisation noise is drawn by the step (U(0, 1/256)): the oracle without noise is within 2e-2 bits/dim at this scale
    assert torch.isfinite(loss2) and abs(loss2.item() - nll_ref.mean().item()) < 5e-2, (loss2.item(), nll_ref.mean().item())
    after = glow.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if k != "h_top"), "the re-run applies the update"
    assert all(torch.isfinite(v).all() for v in after.values())
    assert glow.flow.plan_for(x.to(DEV)).family == 0 and loop.optimizer._steps == 1


def test_overflow_inside_a_graphed_training_step_is_skipped_and_rerun():
    """The range check around `training.GraphedTrainStep`: step 0 runs eagerly on a healthy model, then f.0's ActNorm scale is blown up
    in place (h1 ~ 3e5: beyond the fp16 pairs, finite in fp32) and step 1 is a graph replay -- the device-side skip sits inside the
    graph (parameters and optimiser state untouched, the step count taken back on the host before the next bias corrections), the
    deferred check finds the non-finite norm and re-runs the batch EAGERLY on the exact-fp32 family, and the loop carries on graphed
    (the plan is back on the product family, the weight images are re-derived inside the graph; if the eager call moved a workspace
    the stale graph is dropped, one step runs eagerly and the step is captured again -- never replayed over a stale pointer)."""
    from pytorch_glow_amd import training
    torch.manual_seed(0)
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=128, K=1, L=1, batch=4)
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=1e-3)
    hps = hps_for(cfg, 4)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)
    glow = G.Glow(hps)
    sd["h_top"] = torch.zeros_like(glow.h_top)
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(4, 3, 16, 16, generator=g).to(DEV)
    loop = training.TrainLoop(glow, hps, graph=True)
    loop.GRAPH_AFTER = 1
    loss0, norm0 = loop.step(x)
    assert torch.isfinite(loss0) and torch.isfinite(norm0) and loop._graphed is None
    params = dict(glow.named_parameters())
    with torch.no_grad():
        params["flow.layers.1.f.0.actnorm.logs"].add_(float(np.log(3e5)) / 3.0)
        params["flow.layers.1.f.2.actnorm.logs"].sub_(float(np.log(3e5)) / 3.0)
    before = {k: v.detach().clone() for k, v in glow.state_dict().items()}
    loss1, norm1 = loop.step(x)
    assert loop._graphed is not None and loop.graph_error is None, loop.graph_error
    assert not torch.isfinite(loss1) and not torch.isfinite(norm1), (loss1, norm1)
    after = glow.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "a skipped step must not touch the parameters"
    loop.flush()
    assert loop.range_fallbacks == 1 and loop.diverged_steps == 0 and loop.optimizer._steps == 2
    loss_r, norm_r = loop.last_rerun
    assert torch.isfinite(loss_r) and torch.isfinite(norm_r)
    after = glow.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if k != "h_top"), "the re-run applies the update"
    assert glow.flow.plan_for(x).family == 0
    # the eager re-run packed the plan again (for the other family): the loop notices (GraphedTrainStep.valid), runs one step eagerly
    # and captures again -- a replay of the old graph read freed host memory through its copy nodes when this was first tried; the
    # model still overflows, so every one of these steps is skipped and re-run again
    for _ in range(3):
        loss2, norm2 = loop.step(x)
        assert not torch.isfinite(norm2)
        loop.flush()
    assert loop.graph_error is None and loop.graph_recaptures >= 1, (loop.graph_error, loop.graph_recaptures)
    assert loop.range_fallbacks == 4 and loop.optimizer._steps == 5
    assert all(torch.isfinite(v).all() for v in glow.state_dict().values())


def test_direct_training_path_equals_the_autograd_route_bitwise():
    """VERDICT r4 #4c: `Glow.loss_and_grads` (HIP forward + reverse sweep called directly, gradients in the plan's persistent buckets,
    no autograd graph -- what parallel.train_step runs) against the reference-shaped route `normal_flow` + `loss.backward()`:
    same kernels, so the same bits -- for every gradient, and for the parameters after three optimiser steps of two loops that
    differ only in the route.  A second call of the direct path must overwrite its buckets in full (no accumulation)."""
    import copy
    from pytorch_glow_amd import training, parallel
    K, batch = 2, 8
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=31, invconv_perturb=0.02, zeros_std=0.01)
    hps = hps_for(cfg, batch)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)

    def fresh():
        glow = G.Glow(hps)
        sd2 = dict(sd); sd2["h_top"] = torch.zeros_like(glow.h_top)
        glow.load_state_dict(sd2)
        glow.set_actnorm_inited()
        return glow.to(DEV).train()

    g = torch.Generator().manual_seed(31)
    x = torch.rand(batch, 3, 64, 64, generator=g).to(DEV)
    noise = (torch.rand(batch, 3, 64, 64, generator=g) / 256).to(DEV)
    a, b = fresh(), fresh()
    with torch.enable_grad():
        _, nll, _ = a.normal_flow(x, None, noise=noise)
        la = G.Glow.generative_loss(nll)
        la.backward()
    lb = b.loss_and_grads(x, noise=noise)
    assert torch.equal(la.detach(), lb)
    ga = {n: p.grad for n, p in a.named_parameters() if p.grad is not None}
    gb = {n: p.grad for n, p in b.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb) and len(ga) > 60
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    first = {n: t.clone() for n, t in gb.items()}
    lb2 = b.loss_and_grads(x, noise=noise)                       # same inputs again: the buckets are overwritten, not added to
    assert torch.equal(lb, lb2) and all(torch.equal(first[n], p.grad) for n, p in b.named_parameters() if p.grad is not None)
    assert all(p.grad.data_ptr() == first_ptr for p, first_ptr in zip([p for _, p in b.named_parameters() if p.grad is not None],
                                                                        [gb[n].data_ptr() for n in gb]))
    # three steps of the loop, each route
    loops = [training.TrainLoop(m, hps) for m in (fresh(), fresh())]
    for step in range(3):
        xs = torch.rand(batch, 3, 64, 64, generator=g).to(DEV)
        outs = []
        for loop, direct in zip(loops, (True, False)):
            torch.manual_seed(100 + step)                        # the step draws its dequantisation noise from torch's generator
            loop.lr = loop.scheduler(global_step=loop.global_step)
            for group in loop.optimizer.param_groups:
                group["lr"] = loop.lr
            outs.append(parallel.train_step(loop.glow, loop.optimizer, xs, world=1, max_grad_clip=5, max_grad_norm=100, direct=direct))
            loop.global_step += 1
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (step, outs)
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)


def test_graphed_training_step_equals_the_eager_step_bitwise():
    """VERDICT r4 (missing #3): the training step of one rank as ONE hipGraph launch (`training.GraphedTrainStep`, what
    `TrainLoop(graph=True)` switches to after its eager warm-up steps): dequantisation draw, HIP forward with tape, reverse sweep,
    both clippings and the Adam update captured once -- learning rate and bias corrections read from device memory by the update
    kernel (glowhip_optim_step_dev), glowhip_plan_pack inside the graph.  Two loops from the same state, same batches, same seeds:
    one eager, one graphed from step 3 on -- loss, gradient norm and, after six steps under the noam schedule (the learning rate
    changes every step), every parameter and the optimiser state must be the same bits."""
    from pytorch_glow_amd import training
    K, batch = 2, 8
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=37, invconv_perturb=0.02, zeros_std=0.01)
    hps = hps_for(cfg, batch)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)

    def fresh():
        glow = G.Glow(hps)
        sd2 = dict(sd); sd2["h_top"] = torch.zeros_like(glow.h_top)
        glow.load_state_dict(sd2)
        glow.set_actnorm_inited()
        return glow.to(DEV).train()

    g = torch.Generator().manual_seed(37)
    loops = [training.TrainLoop(fresh(), hps, graph=False), training.TrainLoop(fresh(), hps, graph=True)]
    for step in range(6):
        xs = torch.rand(batch, 3, 64, 64, generator=g).to(DEV)
        outs = []
        for loop in loops:
            torch.manual_seed(200 + step)                        # the step draws its dequantisation noise from torch's generator
            loss, norm = loop.step(xs)
            outs.append((loss.clone(), norm.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (step, outs)
        assert torch.isfinite(outs[0][0]) and torch.isfinite(outs[0][1])
    for loop in loops:
        loop.flush()
    assert loops[1].graph_error is None and loops[1]._graphed is not None and loops[0]._graphed is None
    assert loops[0].optimizer._steps == loops[1].optimizer._steps == 6
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    sa, sb = loops[0].optimizer.state_dict()["state"], loops[1].optimizer.state_dict()["state"]
    for k in sa:
        for name in sa[k]:
            assert torch.equal(torch.as_tensor(sa[k][name]).cpu(), torch.as_tensor(sb[k][name]).cpu()), (k, name)


def _two_loops(seed, graph, range_check=True, K=2, batch=8):
    from pytorch_glow_amd import training
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=seed, invconv_perturb=0.02, zeros_std=0.01)
    hps = hps_for(cfg, batch)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)

    def fresh():
        glow = G.Glow(hps)
        sd2 = dict(sd); sd2["h_top"] = torch.zeros_like(glow.h_top)
        glow.load_state_dict(sd2)
        glow.set_actnorm_inited()
        return glow.to(DEV).train()

    return [training.TrainLoop(fresh(), hps, graph=g, range_check=range_check) for g in graph], batch


def test_graphed_steps_queued_far_ahead_of_the_device_read_their_own_learning_rate():
    """a replay's {lr, 1 - beta1^step, 1 - beta2^step} travel through PINNED host words, and a pinned-source copy
    reads them when the stream gets to it -- with one slot, a host several steps ahead of the device let step N read step N + 1's
    values.  Here the device is held back (a ~0.5 s spin kernel) while the host queues nine graphed steps under the noam warm-up
    (the learning rate and both bias corrections change every step) with no sync in between and the range check off (nothing bounds
    the host's lead but the slot ring itself): parameters and optimiser state must equal the eager loop's bit for bit."""
    loops, batch = _two_loops(41, graph=(False, True), range_check=False)
    g = torch.Generator().manual_seed(41)
    batches = [torch.rand(batch, 3, 64, 64, generator=g).to(DEV) for _ in range(12)]
    for loop in loops:
        for step, xs in enumerate(batches):
            if step == loop.GRAPH_AFTER and loop.graph:
                torch.cuda._sleep(1_000_000_000)                 # the host runs ahead from here on
            torch.manual_seed(300 + step)
            loop.step(xs)
        loop.flush()
    torch.cuda.synchronize()
    assert loops[1].graph_error is None and loops[1]._graphed is not None
    assert loops[0].optimizer._steps == loops[1].optimizer._steps == 12
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa), [k for k in pa if not torch.equal(pa[k], pb[k])][:5]
    sa, sb = loops[0].optimizer.state_dict()["state"], loops[1].optimizer.state_dict()["state"]
    assert all(torch.equal(torch.as_tensor(sa[k][n]).cpu(), torch.as_tensor(sb[k][n]).cpu()) for k in sa for n in sa[k])


def test_direct_step_binds_its_gradients_again_after_zero_grad_and_after_an_autograd_step():
    """`Glow.loss_and_grads` makes the plan's persistent bucket views the parameters' .grad; a caller that runs
    `optimizer.zero_grad()` (set_to_none) or one autograd-route step in between takes them away.  The next direct step must bind
    them again and the optimiser must rebuild its chunk table (a new token): after [direct, zero_grad, direct, autograd, direct] the
    parameters equal those of a loop that ran the same five batches on the autograd route throughout, bit for bit -- with stale
    bindings the third / fifth update applied old gradients or none."""
    from pytorch_glow_amd import parallel
    loops, batch = _two_loops(43, graph=(False, False))
    g = torch.Generator().manual_seed(43)
    routes = [(True, False), (True, True), (False, False), (True, False), (True, False)]      # (direct?, zero_grad after?)
    for step, (direct, zero) in enumerate(routes):
        xs = torch.rand(batch, 3, 64, 64, generator=g).to(DEV)
        for loop, d in zip(loops, (direct, False)):
            torch.manual_seed(400 + step)
            loop.lr = loop.scheduler(global_step=loop.global_step)
            for group in loop.optimizer.param_groups:
                group["lr"] = loop.lr
            parallel.train_step(loop.glow, loop.optimizer, xs, world=1, max_grad_clip=5, max_grad_norm=100, direct=d)
            loop.global_step += 1
        if zero:
            loops[0].optimizer.zero_grad()
            assert all(p.grad is None for p in loops[0].glow.parameters())
    plan = loops[0].glow._train_plan
    views = plan._pgrad[1]
    assert all(p.grad is v for p, v in zip(plan.trainable_parameters(), views))
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa), [k for k in pa if not torch.equal(pa[k], pb[k])][:5]


def test_log_scale_gradients_do_not_read_weight_gradients_after_their_bucket_is_handed_over():
    """on the backward-k_cnet path d logs of the hidden ActNorms is computed FROM the weight gradients, and those
    live in the per-level flat buckets a data-parallel run all-reduces in place, on a side stream, as soon as the level's
    gradient-ready event has passed.  The sweep must therefore have finished every read of a bucket before it records that
    bucket's event.  Simulated on one GPU: a side stream waits for each event and then CLOBBERS the bucket (what an in-place
    all-reduce + division does to it, only more so).  The log-scale gradients must equal those of an undisturbed backward bit
    for bit; the buckets of the levels above the last one are overwritten long before the sweep ends, so a sweep that reads
    them late fails deterministically."""
    K, batch = 2, 4
    cfg = O.default_cfg(K=K, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=23, invconv_perturb=0.02, zeros_std=0.01)
    g = torch.Generator().manual_seed(23)
    x = torch.rand(batch, 3, 64, 64, generator=g)
    noise = torch.rand(batch, 3, 64, 64, generator=g) / 256
    sd = O.glow_init_actnorm(x, noise, sd, cfg)
    glow = G.Glow(hps_for(cfg, batch))
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    side = torch.cuda.Stream(device=DEV)

    def run(clobber):
        glow.zero_grad(set_to_none=True)
        with torch.enable_grad():
            z, nll, _ = glow.normal_flow(x.to(DEV), None, noise=noise.to(DEV))
            G.Glow.generative_loss(nll).backward()
        buckets = glow.flow.pop_grad_buckets()
        assert buckets is not None and len(buckets) == 3 + 1          # one per level + the small one
        if clobber:
            with torch.cuda.stream(side):
                for flat, ready in buckets[:-1]:
                    side.wait_event(ready)
                    flat.fill_(float("nan"))
            torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in glow.named_parameters() if p.grad is not None}

    clean = run(False)
    assert glow.flow.plan_for(x.to(DEV)).launch_counts().get("k_cnet(bwd)", 0) >= 3 * K
    hit = run(True)
    checked = 0
    for name, gc in clean.items():
        if name.endswith(("f.0.weight", "f.2.weight", "f.4.weight", "conv2d_zeros.weight")):
            assert torch.isnan(hit[name]).all(), name         # (the views into the buckets: the clobber did land)
            continue
        assert torch.equal(hit[name], gc), f"{name} was computed from a bucket that had already been handed over"
        checked += name.endswith("actnorm.logs")
    assert checked >= 3 * K * 3
