"""`-m gpu`: the forward-only parameter pack as ONE launch (csrc/pack.hip k_pack_fused) and Split2d's z1 read in place by the
squeeze folded into k_chanmix (no compaction copy).  Every check is BITWISE against a route that already existed: the per-kind
pack launches (DBG.PACK_UNFUSED) and the unfused squeeze / copy / mixer launches (DBG.NO_MIXER_FUSION).  Hidden is 512 throughout: the product kernels and their weight images are built for it.
Reference: network/module.py:76-82,356-363 (ActNorm / invconv log-det terms), network/model.py:105-139 (FlowStep), :263-276 (encode)."""
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.network import model as M
from oracle import glow_oracle as O
from test_gpu_parity import dev, make_glow

pytestmark = pytest.mark.gpu
DBG = _lib.DBG


def _state(cfg, seed):
    """Seeded weights with every derived quantity of the pack non-trivial: Conv2dZeros weights / biases / logs and all ActNorm
    biases / logs away from zero, invconv matrices away from orthogonal (row swaps in the LU)."""
    sd = O.seeded_state_dict(cfg, seed=seed, zeros_std=0.02, invconv_perturb=0.05)
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in sd.items():
        if k.endswith(".logs") or k.endswith("actnorm.bias") or (k.endswith(".bias") and (".f.4." in k or "conv2d_zeros" in k)):
            sd[k] = v + 0.05 * torch.randn(v.shape, generator=g)
    return sd


def _glow(hw, L, K, batch, seed):
    cfg = O.default_cfg(image_shape=(hw[0], hw[1], 3), hidden_channels=512, K=K, L=L, batch=batch)
    sd = _state(cfg, seed)
    return make_glow(cfg, sd, batch), cfg, sd


def _images(batch, hw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, 3, hw[0], hw[1], generator=g)
    return x, torch.rand(batch, 3, hw[0], hw[1], generator=g) / 256


def _pack_into_fresh_buffer(plan, use, flags):
    """`packed` of a pack into a buffer that held 0xA5 bytes before (nothing may rely on what a buffer held)."""
    plan.packed = torch.full_like(plan.packed, 0xA5)
    plan.launch_counts(reset=True)
    with _lib.debug_flags(flags):
        plan.pack(use, merge=False)
    torch.cuda.synchronize()
    return plan.packed.clone(), plan.launch_counts(reset=True)


@pytest.mark.parametrize("image,L,K", [(64, 3, 2), (32, 2, 3)])
def test_fused_pack_leaves_the_bytes_of_the_per_kind_launches(image, L, K):
    """The same plan packed into two fresh buffers, by k_pack_fused and by the per-kind launch sequence: EVERY byte of `packed` is
    equal -- weight images, scale tables, per-step log|det W| and konst slots, the log-det total in packed[0], the zero block, and the
    tables themselves (the segment table travels on both routes).  64x64 L=3 has C = 12 / 24 / 48 jobs, 32x32 L=2 only C = 12 / 24:
    other block counts per job.  A second fused pack of the same buffer reproduces it (the arrival counter is back at zero)."""
    glow, cfg, sd = _glow((image, image), L, K, 2, seed=41)
    x, _ = _images(2, (image, image), 1)
    plan = glow.flow.plan_for(dev(x))
    fused, cf = _pack_into_fresh_buffer(plan, plan.PACK_INFERENCE, 0)
    plain, cp = _pack_into_fresh_buffer(plan, plan.PACK_INFERENCE, DBG.PACK_UNFUSED)
    assert cf.get("pack:k_pack_fused") == 1 and "pack:k_step_prepare_small" not in cf, cf
    assert cp.get("pack:k_step_prepare_small") == 1 and "pack:k_pack_fused" not in cp, cp
    diff = (fused != plain).nonzero().flatten()
    assert diff.numel() == 0, (diff.numel(), diff[:8].tolist())
    total = fused[:8].view(torch.float64).item()
    assert total != 0.0 and total == total, total            # packed[0]: the plan-wide log-det constant
    assert not fused[8:256].any()                             # the zero block
    plan.pack(plan.PACK_INFERENCE, merge=False)               # `plan.packed` is the per-kind buffer: fused on top of it
    torch.cuda.synchronize()
    assert torch.equal(plan.packed, fused)


def test_which_packs_take_the_one_launch():
    """The route from the run-time counters: forward-only packs of the 12 / 24 / 48-wide plans take k_pack_fused; a pack that also
    serves decode (INVERSE: W^-1), a training pack, and a plan with a C = 96 level (no one-wave LU for it) keep today's launches."""
    glow, cfg, sd = _glow((64, 64), 3, 2, 2, seed=42)
    plan = glow.flow.plan_for(dev(_images(2, (64, 64), 1)[0]))

    def counts(p, use):
        p.launch_counts(reset=True)
        p.pack(use, merge=False)
        return p.launch_counts(reset=True)

    c = counts(plan, plan.PACK_INFERENCE)
    assert c.get("pack:k_pack_fused") == 1 and not any(k.startswith("pack:k_step_prepare") for k in c), c
    for use in (plan.PACK_INFERENCE | plan.PACK_INVERSE, plan.PACK_TRAINING, plan.PACK_INFERENCE | plan.PACK_TRAINING):
        c = counts(plan, use)
        assert c.get("pack:k_step_prepare_batched") == 1 and "pack:k_pack_fused" not in c, (use, c)
    wide, _, _ = _glow((128, 128), 4, 1, 1, seed=43)
    pw = wide.flow.plan_for(dev(_images(1, (128, 128), 1)[0]))
    c = counts(pw, pw.PACK_INFERENCE)
    assert c.get("pack:k_step_prepare_batched") == 1 and "pack:k_pack_fused" not in c, c
    torch.cuda.synchronize()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_repack_after_an_in_place_update_equals_a_fresh_plan(graph):
    """Pack, forward, change EVERY parameter in place, pack, forward: bitwise the result of a fresh model (fresh plan, fresh buffer)
    with the new parameters -- nothing of the first pack survives in the second (images, scale tables, log-det total, counter).
    Eager launches, and the captured graph replayed after the update."""
    batch = 2
    glow, cfg, sd = _glow((64, 64), 3, 2, batch, seed=44)
    x, noise = _images(batch, (64, 64), 2)
    x, noise = dev(x), dev(noise)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        if graph:
            gf = glow.capture_forward(x, repack=True)
            z0, n0 = (t.clone() for t in gf())
        else:
            z0, n0, _ = glow.normal_flow(x, None, noise=noise, repack=True)
        for p in glow.flow.parameters():
            p.mul_(1.0 + 0.02 * torch.randn(p.shape, generator=g).to(p.device)).add_(0.003)
        if graph:
            z1, n1 = (t.clone() for t in gf())
            noise = gf.noise.clone()
        else:
            plan = glow.flow.plan_for(x)
            plan.launch_counts(reset=True)
            z1, n1, _ = glow.normal_flow(x, None, noise=noise, repack=True)
            assert plan.launch_counts(reset=True).get("pack:k_pack_fused") == 1
        fresh = make_glow(cfg, {k: v.detach().cpu() for k, v in glow.state_dict().items()}, batch)
        zf, nf, _ = fresh.normal_flow(x, None, noise=noise)
        with _lib.debug_flags(DBG.PACK_UNFUSED):
            zu, nu, _ = fresh.normal_flow(x, None, noise=noise, repack=True)
    assert torch.isfinite(n1).all() and not torch.equal(n1, n0)
    assert torch.equal(z1, zf) and torch.equal(n1, nf)
    assert torch.equal(z1, zu) and torch.equal(n1, nu)


@pytest.mark.parametrize("hw,K", [((48, 80), 1), ((48, 80), 2), ((64, 64), 2)])
def test_folded_squeeze_and_z1_in_place_equal_the_separate_launches_bitwise(hw, K):
    """Behind a Split2d the squeeze folded into the mixer reads z1 where it lies, through the batch stride of the undivided tensor
    (no compaction copy): float input with the in-kernel noise draw, uint8 input, an explicit noise tensor, and bound latents -- each the same BITS
    as under DBG.NO_MIXER_FUSION (squeeze kernel, copy, mixer as separate launches).  48x80: non-square, 24x40 and 12x20 levels on
    the per-layer kernels; with K = 1 the level-2 step is the plan's last layer, whose squeeze does not fold (so z1 is copied); with
    K = 2 it folds and reads z1 in place; 64x64 the same on the k_cnet path."""
    L, batch = 2, 3
    folds = L if K > 1 else L - 1
    glow, cfg, sd = _glow(hw, L, K, batch, seed=46)
    x, noise = _images(batch, hw, 5)
    u8 = (x * 255).round().to(torch.uint8).to(x.device)
    x, noise, u8 = dev(x), dev(noise), u8.to("cuda:0")
    plan = glow.flow.plan_for(x)

    def run(flags, inp, nz, latents):
        torch.manual_seed(11)                                   # (the in-kernel draw is keyed by torch's seed and a call count:
        M.reset_dequant_stream()                                #  both runs of a pair draw call 0 of the same seed)
        bufs = plan.latent_buffers(batch) if latents else None
        with _lib.debug_flags(flags), torch.no_grad():
            plan.launch_counts(reset=True)
            z, nll, _ = glow.normal_flow(inp, None, noise=nz, eps_out=bufs)
            counts = plan.launch_counts(reset=True)
        return z.clone(), nll.clone(), [b.clone() for b in (bufs or [])], counts

    for what, inp, nz, latents in [("float + in-kernel draw", x, None, False), ("uint8", u8, None, False),
                                   ("explicit noise", x, noise, False), ("uint8 + explicit noise", u8, noise, False),
                                   ("latents bound", x, noise, True)]:
        z, nll, e, c = run(0, inp, nz, latents)
        zu, nllu, eu, cu = run(DBG.NO_MIXER_FUSION, inp, nz, latents)
        assert c.get("squeeze(folded)") == folds and c.get("split2d:z1 in place", 0) == folds - 1, (what, c)
        assert "squeeze(folded)" not in cu and "split2d:z1 in place" not in cu, (what, cu)
        assert torch.isfinite(nll).all(), what
        assert torch.equal(z, zu) and torch.equal(nll, nllu), what
        assert len(e) == len(eu) == (L - 1 if latents else 0) and all(torch.equal(a, b) for a, b in zip(e, eu)), what
