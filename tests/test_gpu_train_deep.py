"""Training the six-level (256x256-style) stack (-m gpu): the deepest level has C = 384 channels, which the channel mixer's
backward takes on k_chanmix_bwd_wide (csrc/backward.hip: 32 pixels x 32 channels per workgroup, grid = pixel blocks x channel
slices) instead of k_chanmix_bwd, whose three C x 65 LDS arrays stop at C = 192.

The reference cannot serve as the yardstick at C = 384 -- its fp32 torch.det underflows there (test_deep_multiscale_configs_vs_oracle)
-- so gradients are compared with the autograd oracle under O.STABLE_LOGDET (sum of log-pivots), run in fp64.  Tolerance: the
project's gradient bound (tests/test_gpu_grad.py): |g - g_ref| <= 2e-4 max|g_ref| + 1e-7, at most 1 % of a tensor's
entries beyond it (a ReLU pre-activation within fp32 rounding of zero may flip one row of one weight gradient), none beyond
0.05 max|g_ref|; loss within 1e-4.  Reference: network/model.py:82-117, network/trainer.py:123-150."""
import contextlib
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

DEV = "cuda:0"
WIDE = "k_chanmix_bwd_wide"


@contextlib.contextmanager
def stable_logdet():
    O.STABLE_LOGDET = True
    try:
        yield
    finally:
        O.STABLE_LOGDET = False


def hps_for(cfg, batch):
    return util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False,
                      flow_permutation=cfg["flow_permutation"], flow_coupling=cfg["flow_coupling"]),
        optim=dict(num_batch_train=batch), dataset=dict(num_classes=1), device=dict(graph=["cuda:0"])))


def train_hps(cfg, batch, lr):
    hps = hps_for(cfg, batch)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=lr, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=lr / 10))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)
    return hps


def deep_model(image, batch, hidden, perm="invconv", coup="affine"):
    """K = 1, L = 6: C = 12, 24, 48, 96, 192, 384 -- weights, batch and ActNorm init as test_deep_multiscale_configs_vs_oracle builds them."""
    cfg = O.default_cfg(image_shape=(image, image, 3), hidden_channels=hidden, K=1, L=6, flow_permutation=perm,
                        flow_coupling=coup, batch=batch)
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=0.01)
    x = torch.rand(batch, 3, image, image, generator=torch.Generator().manual_seed(4))
    noise = torch.rand(batch, 3, image, image, generator=torch.Generator().manual_seed(5)) / 256
    np.random.seed(5)
    proto = G.Glow(hps_for(cfg, batch))      # (the fixed permutation tables are attributes of the modules, drawn at construction)
    tables = None
    if perm != "invconv":
        tables = {i: (torch.as_tensor(getattr(l, perm).indices), torch.as_tensor(getattr(l, perm).indices_inverse))
                  for i, l in enumerate(proto.flow.layers) if hasattr(l, perm)}
    with torch.no_grad():
        sd = O.glow_init_actnorm(x, noise, sd, cfg, perm_tables=tables)

    def fresh(hps=None):
        np.random.seed(5)                     # same tables as `proto`
        glow = G.Glow(hps or hps_for(cfg, batch))
        glow.load_state_dict(sd)
        glow.set_actnorm_inited()
        return glow.to(DEV).train()

    return cfg, sd, x, noise, tables, fresh


def fp64_oracle_grads(cfg, sd, x, noise, tables):
    with stable_logdet(), torch.enable_grad():
        leaf = {k: v.double().requires_grad_(k != "h_top") for k, v in sd.items()}
        xr = x.double().requires_grad_(True)
        _, nll, _ = O.glow_forward(xr, noise.double(), leaf, cfg, perm_tables=tables)
        loss = nll.mean()
        loss.backward()
    return {k: v.grad for k, v in leaf.items() if v.grad is not None}, xr.grad, loss.item()


def wide_steps(sd):
    return sum(1 for k, v in sd.items() if re.fullmatch(r"flow\.layers\.\d+\.actnorm\.bias", k) and v.numel() > 192)


def check_against_fp64_oracle(cfg, sd, x, noise, tables, glow, what):
    ref, gx_ref, loss_ref = fp64_oracle_grads(cfg, sd, x, noise, tables)
    assert all(torch.isfinite(v).all() for v in ref.values()) and torch.isfinite(gx_ref).all()
    plan = glow.flow.plan_for(x.to(DEV))
    plan.launch_counts(reset=True)
    with torch.enable_grad():
        xd = x.to(DEV).requires_grad_(True)
        _, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
        loss = G.Glow.generative_loss(nll)
        loss.backward()
    counts = plan.launch_counts(reset=True)
    worst = ("", 0.0)
    rows = [("dL/dx", xd.grad, gx_ref)]
    for name, p in glow.named_parameters():
        if name == "h_top":
            continue
        assert p.grad is not None and name in ref, name
        rows.append((name, p.grad, ref[name]))
    failures = []
    for name, got, r in rows:
        err = (got.detach().cpu().double().reshape(r.shape) - r).abs()
        scale = r.abs().max().item()
        tight = 2e-4 * scale + 1e-7
        outliers = (err > tight).double().mean().item()
        worst = max(worst, (name, err.max().item() / tight), key=lambda t: t[1])
        if not torch.isfinite(got).all() or outliers > 0.01 or err.max().item() > 0.05 * scale + 1e-7:
            failures.append(f"{name}: max err {err.max().item():.3e}, {outliers:.2%} beyond 2e-4 max|g|, max|g| {scale:.3e}")
    print(f"{what}: loss {loss.item():.6f} vs {loss_ref:.6f}; worst {worst[0]} at {worst[1]:.3f} of the tight bound; {counts}")
    assert not failures, failures
    assert abs(loss.item() - loss_ref) < 1e-4
    # one launch of the wide kernel per C = 384 FlowStep (K = 1: one) -- so the C = 192 step did not take it
    assert wide_steps(sd) == 1 and counts.get(WIDE, 0) == 1, counts


@pytest.mark.parametrize("image,batch,hidden", [
    (128, 3, 64),      # C = 384 on 2x2 pixels: 12 pixels, one partial pixel block (every lane mask live); C = 192 on 4x4
    (256, 5, 128),     # C = 384 on 4x4: 80 pixels = full blocks + a partial one, blocks spanning image boundaries; C = 192 on 8x8
])
def test_six_level_gradients_vs_fp64_autograd_oracle(image, batch, hidden):
    """Every parameter gradient and dL/dx of the L = 6 stack (affine coupling, invertible 1x1 convolutions: the matrix instance of
    k_chanmix_bwd_wide with dW, the ActNorm gradients and W^-1 / log-det at C = 384 from the LU kernel)."""
    cfg, sd, x, noise, tables, fresh = deep_model(image, batch, hidden)
    check_against_fp64_oracle(cfg, sd, x, noise, tables, fresh(), f"{image}x{image} batch {batch} hidden {hidden}")


def test_six_level_gradients_shuffle_additive_vs_fp64_autograd_oracle():
    """The gather instance of k_chanmix_bwd_wide (matrix == nullptr, gather_inv): flow_permutation = shuffle, additive coupling, the
    permutation tables taken from the modules."""
    cfg, sd, x, noise, tables, fresh = deep_model(128, 3, 64, perm="shuffle", coup="additive")
    assert tables
    check_against_fp64_oracle(cfg, sd, x, noise, tables, fresh(), "128x128 shuffle / additive")


# 68 images x 2x2 pixels = 272 pixels at C = 384: nine 32-pixel blocks on the level's eight accumulator copies -- more blocks than
# copies, so the launch adds with fp64 atomics (not plain stores) and blocks 0 and 8 add into the same copy; the last block is partial
SHARED_BATCH = 68


def test_six_level_direct_step_equals_the_autograd_route_bitwise():
    """`Glow.loss_and_grads` against `normal_flow` + `loss.backward()` on one six-level model: same kernels, same bits, for the
    loss and every gradient.  Batch 68 on purpose: two workgroups of k_chanmix_bwd_wide add into one accumulator copy (see
    SHARED_BATCH), so the comparison covers the atomic route as well -- sums of fp32 values in fp64 are exact in any order."""
    cfg, sd, x, noise, tables, fresh = deep_model(128, SHARED_BATCH, 64)
    a, b = fresh(), fresh()
    xd, nd = x.to(DEV), noise.to(DEV)
    pa, pb = a.flow.plan_for(xd), b.flow.plan_for(xd)
    pa.launch_counts(reset=True); pb.launch_counts(reset=True)
    with torch.enable_grad():
        _, nll, _ = a.normal_flow(xd, None, noise=nd)
        la = G.Glow.generative_loss(nll)
        la.backward()
    lb = b.loss_and_grads(xd, noise=nd)
    assert pa.launch_counts().get(WIDE, 0) == 1 and pb.launch_counts().get(WIDE, 0) == 1
    assert torch.isfinite(la) and torch.equal(la.detach(), lb)
    ga = {n: p.grad for n, p in a.named_parameters() if p.grad is not None}
    gb = {n: p.grad for n, p in b.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb) and len(ga) >= 6 * 12
    for n in ga:
        assert torch.isfinite(ga[n]).all() and torch.equal(ga[n], gb[n]), n
    first = {n: t.clone() for n, t in gb.items()}
    lb2 = b.loss_and_grads(xd, noise=nd)       # again: the wide level's accumulator copies are zeroed per step, nothing adds up
    assert torch.equal(lb, lb2) and all(torch.equal(first[n], p.grad) for n, p in b.named_parameters() if p.grad is not None)


def test_six_level_graphed_training_step_equals_the_eager_step_bitwise():
    """Two `TrainLoop`s from the same state and batches, one eager, one replaying ONE hipGraph per step from step 3 on (the wide
    mixer backward, its accumulators' memset and the finalize jobs inside the graph): loss, gradient norm and, after five steps,
    every parameter must be the same bits.  Batch as above (shared accumulator copies)."""
    from pytorch_glow_amd import training
    cfg, sd, x, noise, tables, fresh = deep_model(128, SHARED_BATCH, 64)
    hps = train_hps(cfg, SHARED_BATCH, 1e-4)
    loops = [training.TrainLoop(fresh(hps), hps, graph=False), training.TrainLoop(fresh(hps), hps, graph=True)]
    xd = x.to(DEV)
    for step in range(5):
        outs = []
        for loop in loops:
            torch.manual_seed(300 + step)        # the step draws its dequantisation noise from torch's generator
            loss, norm = loop.step(xd)
            outs.append((loss.clone(), norm.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (step, outs)
        assert torch.isfinite(outs[0][0]) and torch.isfinite(outs[0][1])
    for loop in loops:
        loop.flush()
    assert loops[1].graph_error is None and loops[1]._graphed is not None and loops[0]._graphed is None
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert max((pa[k].cpu() - sd[k]).abs().max().item() for k in sd if k != "h_top") > 5e-5      # the steps moved them


def test_six_level_train_loop_reduces_the_loss():
    """Ten `TrainLoop` steps (data-dependent ActNorm init, forward with tape, HIP backward, both clippings, Adam under the noam
    schedule) on a freshly constructed six-level model: the loss must fall, every parameter stay finite, and a forward after the
    last step agree with the oracle evaluated on the updated state_dict."""
    from pytorch_glow_amd import training
    torch.manual_seed(0)
    np.random.seed(0)
    batch = 3
    cfg = O.default_cfg(image_shape=(128, 128, 3), hidden_channels=64, K=1, L=6, batch=batch)
    hps = train_hps(cfg, batch, 1e-3)
    glow = G.Glow(hps).to(DEV)
    loop = training.TrainLoop(glow, hps)
    x = torch.rand(batch, 3, 128, 128, generator=torch.Generator().manual_seed(4))
    noise = torch.rand(batch, 3, 128, 128, generator=torch.Generator().manual_seed(5)) / 256
    xd = x.to(DEV)
    plan = glow.flow.plan_for(xd)
    plan.launch_counts(reset=True)
    losses = []
    for _ in range(10):
        loss, gnorm = loop.step(xd)
        losses.append(loss.item())
        assert torch.isfinite(gnorm)
    loop.flush()
    assert plan.launch_counts().get(WIDE, 0) >= 10
    assert glow.actnorm_inited() and loop.global_step == 10
    assert losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in glow.parameters())
    sd1 = {k: v.detach().cpu().clone() for k, v in glow.state_dict().items()}
    with stable_logdet(), torch.no_grad():
        z_ref, nll_ref, _ = O.glow_forward(x, noise, sd1, cfg)
    assert torch.isfinite(nll_ref).all()
    for mode in ("eval", "train"):
        getattr(glow, mode)()
        z, nll, _ = glow.normal_flow(xd, None, noise=noise.to(DEV))
        assert (nll.cpu() - nll_ref).abs().max().item() < 1e-4, (mode, nll.cpu(), nll_ref)
        assert (z.cpu() - z_ref).abs().max().item() < 1e-4
