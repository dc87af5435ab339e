"""`-m gpu`: whole models with ``lu_decomposition=True`` (every FlowStep's 1x1 convolution kept as P L U factors,
csrc/invconv_lu.hip) -- forward, round trips, class-conditional forward, captured forward, gradients against the fp64 autograd
oracle (tests/plu_oracle.py: W built from l, u, log_s as fp64 leaves and fed to oracle.glow_oracle under the dense key), the
training loop eager and captured, and a step under a one-rank RCCL group.  The reference raises at network/module.py:336-337, so
there is nothing of its to record: the dense route of this project, on the same fp32 W, is the bitwise twin.

Model: 16x16x3, L = 3, K = 2, affine coupling, hidden 32 (the smallest model of tests/test_gpu_grad.py): widths 12, 24 and 48."""
import os

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd.misc import util
from oracle import glow_oracle as O
import plu_oracle as PLU
from test_gpu_parity import DEV, dev

pytestmark = pytest.mark.gpu
BATCH, IMAGE = 3, 16
CFG = O.default_cfg(image_shape=(IMAGE, IMAGE, 3), hidden_channels=32, K=2, L=3, flow_permutation="invconv",
                    flow_coupling="affine", batch=BATCH)


def hps_for(lu, batch=BATCH):
    return util.AttrDict(dict(
        model=dict(image_shape=[IMAGE, IMAGE, 3], hidden_channels=32, K=2, L=3, actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=lu, flow_permutation="invconv", flow_coupling="affine"),
        optim=dict(num_batch_train=batch), dataset=dict(num_classes=1), device=dict(graph=["cuda:0"])))


_SD = {}


def lu_state_dict():
    """Seeded parameters away from every special value (test_gpu_grad.py's recipe), the dense 1x1 weights Q + 0.05 randn factored
    by the snapshot helper: the state dict of the LU model, on the host.  Built once."""
    if not _SD:
        np.random.seed(1)
        dense = G.Glow(hps_for(False))
        g = torch.Generator().manual_seed(5)
        sd = {k: v.detach().clone() for k, v in dense.state_dict().items()}
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
        _SD["sd"] = util.lu_state_dict_from_dense(sd)
        _SD["x"] = torch.rand(BATCH, 3, IMAGE, IMAGE, generator=g)
        _SD["noise"] = torch.rand(BATCH, 3, IMAGE, IMAGE, generator=g) / 256
    return _SD["sd"], _SD["x"], _SD["noise"]


def lu_glow(train=False, hps=None, inited=True):
    sd, _, _ = lu_state_dict()
    np.random.seed(2)
    glow = G.Glow(hps or hps_for(True))
    sd = {k: v.clone() for k, v in sd.items()}
    sd["h_top"] = torch.zeros_like(glow.h_top)          # (its leading dimension is the batch size of the hps)
    glow.load_state_dict(sd, strict=True)
    if inited:
        glow.set_actnorm_inited()
    glow = glow.to(DEV)
    return glow.train() if train else glow.eval()


def dense_twin(glow, hps):
    """The dense model with the LU model's parameters and, for every 1x1 convolution, the fp32 W its kernels assemble."""
    np.random.seed(2)
    twin = G.Glow(hps)
    sd = {}
    for k, v in glow.state_dict().items():
        if ".invconv." not in k:
            sd[k] = v.detach().cpu().clone()
    for name, m in glow.named_modules():
        if isinstance(m, G.Invertible1x1ConvLU):
            sd[name + ".weight"] = m.weight.cpu()
    twin.load_state_dict(sd, strict=True)
    twin.set_actnorm_inited()
    return twin.to(DEV).eval()


_REF = {}


def oracle():
    if not _REF:
        sd, x, noise = lu_state_dict()
        _REF["r"] = PLU.glow_grads(CFG, sd, x, noise)
    return _REF["r"]


def test_forward_equals_the_dense_twin_bitwise_and_the_oracle():
    _, x, noise = lu_state_dict()
    glow = lu_glow()
    _, _, nll_ref, z_ref = oracle()
    with torch.no_grad():
        z, nll, _ = glow.normal_flow(dev(x), None, noise=dev(noise))
        twin = dense_twin(glow, hps_for(False))
        zt, nllt, _ = twin.normal_flow(dev(x), None, noise=dev(noise))
    assert torch.equal(z, zt), "the same kernels read the same fp32 W"
    for what, v in (("lu", nll), ("dense twin", nllt)):
        err = (v.cpu().double() - nll_ref).abs().max().item()
        print(f"nll {what}: max |err| {err:.2e}")
        assert err <= 1e-4, (what, err)
    assert (z.cpu().double() - z_ref).abs().max().item() <= 1e-4
    plan = glow.flow.plan_for(dev(x))
    c = plan.launch_counts()
    assert c.get("pack:invconv_lu", 0) >= 6 and not [k for k in c if k.startswith("pack:lu:")], c


def test_data_dependent_init_pass_on_an_lu_model():
    """The first training-mode forward of an LU model: glowhip_plan_actnorm_init packs from C with the assemble launch in front,
    so the mixers of the init pass read the assembled W.  Every ActNorm against the fp64 oracle's init pass on the dense W (2e-5, the
    tolerance of the dense init test in tests/test_gpu_parity.py), then z and nll of that forward (1e-4)."""
    sd, x, noise = lu_state_dict()
    with torch.no_grad():
        post = O.glow_init_actnorm(x.double(), noise.double(), PLU.dense_state_dict(sd), CFG)
        z_ref, nll_ref, _ = O.glow_forward(x.double(), noise.double(), post, CFG)
        glow = lu_glow(train=True, inited=False)
        assert not glow.actnorm_inited()
        z, nll, _ = glow.normal_flow(dev(x), None, noise=dev(noise))
    assert all(m.bias_inited and m.logs_inited for m in glow.modules() if isinstance(m, G.ActNorm))
    checked = 0
    for k, v in glow.state_dict().items():
        if "actnorm" in k:
            err = (v.cpu().double() - post[k]).abs().max().item()
            assert err <= 2e-5, (k, err)
            checked += 1
        elif ".invconv." in k:
            assert torch.equal(v.cpu(), sd[k]), k      # the init pass writes no factor
    assert checked == 6 * 6
    assert (z.cpu().double() - z_ref).abs().max().item() <= 1e-4
    assert (nll.cpu().double() - nll_ref).abs().max().item() <= 1e-4


def test_round_trips():
    _, x, noise = lu_state_dict()
    glow = lu_glow()
    xd = dev(x)
    with torch.no_grad():
        z, _, eps = glow.flow.encode(xd, 0., return_eps=True)
        back = glow.flow.decode(z, eps=eps)
        assert (back - xd).abs().max().item() <= 1e-4
        lat = glow.encode_latents(xd, noise=dev(noise))
        rec = glow.decode_latents(lat)
        assert (rec - (xd + dev(noise))).abs().max().item() <= 1e-4
        rec0 = glow.decode_latents(glow.encode_latents(xd, dequantize=False))
        assert (rec0 - xd).abs().max().item() <= 1e-4


def test_class_conditional_forward():
    from test_ycond_host import ycond_hps
    hps = ycond_hps(learn_top=True, device="cuda:0", batch=4)
    hps.ablation.lu_decomposition = True
    np.random.seed(4)
    torch.manual_seed(4)
    glow = G.Glow(hps)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).eval()
    assert any(isinstance(m, G.Invertible1x1ConvLU) for m in glow.modules())
    g = torch.Generator().manual_seed(8)
    x = dev(torch.rand(4, 3, 16, 16, generator=g))
    noise = dev(torch.rand(4, 3, 16, 16, generator=g) / 256)
    yo = torch.nn.functional.one_hot(torch.tensor([0, 3, 1, 4]), 5).float().to(DEV)
    hd = ycond_hps(learn_top=True, device="cuda:0", batch=4)
    with torch.no_grad():
        z, nll, logits = glow.normal_flow(x, yo, noise=noise)
        twin = dense_twin(glow, hd)
        zt, nllt, logitst = twin.normal_flow(x, yo, noise=noise)
    assert torch.isfinite(nll).all() and logits is not None and torch.isfinite(logits).all()
    assert torch.equal(z, zt) and torch.equal(logits, logitst)
    assert (nll - nllt).abs().max().item() <= 1e-4


def test_captured_forward_equals_the_eager_one_bitwise():
    _, x, _ = lu_state_dict()
    glow = lu_glow()
    xd = dev(x)
    with torch.no_grad():
        gf = glow.capture_forward(xd, repack=True)
        z1, n1 = (t.clone() for t in gf())
        ze, ne, _ = glow.normal_flow(xd, None, noise=gf.noise.clone())
        assert torch.equal(z1, ze) and torch.equal(n1, ne)
        # an optimiser-style in-place update of a factor: the next replay assembles the new W
        glow.flow.layers[1].invconv.log_s.mul_(1.05)
        z2, n2 = (t.clone() for t in gf())
        ze2, ne2, _ = glow.normal_flow(xd, None, noise=gf.noise.clone())
        assert torch.equal(z2, ze2) and torch.equal(n2, ne2) and not torch.equal(z2, z1)


@pytest.mark.parametrize("route", ["direct", "autograd"])
def test_gradients_against_the_fp64_autograd_oracle(route):
    _, x, noise = lu_state_dict()
    ref, loss_ref, _, _ = oracle()
    glow = lu_glow(train=True)
    if route == "direct":
        loss = glow.loss_and_grads(dev(x), noise=dev(noise))
    else:
        with torch.enable_grad():
            _, nll, _ = glow.normal_flow(dev(x), None, noise=dev(noise))
            loss = G.Glow.generative_loss(nll)
            loss.backward()
    assert abs(loss.item() - loss_ref) < 1e-4
    worst = ("", 0.0)
    seen = 0
    for name, p in glow.named_parameters():
        if name == "h_top":
            continue
        assert p.grad is not None, name
        r = ref[name]
        gp = p.grad.cpu().double()
        err = (gp - r).abs().max().item()
        bound = 2e-4 * r.abs().max().item() + 1e-7
        if err / bound > worst[1]:
            worst = (name, err / bound)
        assert err <= bound, f"{name}: err {err:.3e} vs bound {bound:.3e} (|g| max {r.abs().max().item():.3e})"
        if name.endswith("invconv.l"):
            assert not torch.triu(gp).any(), name
            seen += 1
        if name.endswith("invconv.u"):
            assert not torch.tril(gp).any(), name
    assert seen == 6
    print(f"{route}: worst parameter {worst[0]} at {worst[1]:.3f} of its bound")
    plan = glow.flow.plan_for(dev(x))
    c = plan.launch_counts()
    assert c.get("k_invconv_lu_backward") == 1 and not [k for k in c if k.startswith("pack:lu:")], c


def test_training_loop_eager_and_captured_same_bits():
    from pytorch_glow_amd import training
    batch = 4
    hps = hps_for(True, batch)
    hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
    hps.ablation.update(max_grad_clip=5, max_grad_norm=100)
    loops = [training.TrainLoop(lu_glow(train=True, hps=hps), hps, graph=False),
             training.TrainLoop(lu_glow(train=True, hps=hps), hps, graph=True)]
    start = {k: v.detach().clone() for k, v in loops[0].glow.state_dict().items()}
    g = torch.Generator().manual_seed(41)
    for step in range(5):
        xs = torch.rand(batch, 3, IMAGE, IMAGE, generator=g).to(DEV)
        outs = []
        for loop in loops:
            torch.manual_seed(300 + step)
            loss, norm = loop.step(xs)
            outs.append((loss.clone(), norm.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (step, outs)
        assert torch.isfinite(outs[0][0]) and torch.isfinite(outs[0][1])
        pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
        assert all(torch.equal(pa[k], pb[k]) for k in pa), step
    for loop in loops:
        loop.flush()
    assert loops[1].graph_error is None and loops[1]._graphed is not None and loops[0]._graphed is None
    end = loops[1].glow.state_dict()
    moved = 0
    for k, v in end.items():
        if k.endswith("invconv.p") or k.endswith("invconv.sign_s"):
            assert torch.equal(v, start[k]), k
        elif k.endswith("invconv.l"):
            assert torch.equal(torch.triu(v), torch.triu(start[k])), k
            moved += int(not torch.equal(v, start[k]))
        elif k.endswith("invconv.u"):
            assert torch.equal(torch.tril(v), torch.tril(start[k])), k
            moved += int(not torch.equal(v, start[k]))
        elif k.endswith("invconv.log_s"):
            moved += int(not torch.equal(v, start[k]))
    assert moved == 18, "every l, u and log_s takes part in the update"


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_step_under_a_one_rank_rccl_group():
    """One training step with the gradient exchange forced through RCCL over a one-rank group, in a fresh child process: l, u and
    log_s travel in the small bucket."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="%d", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
import pytorch_glow_amd as G
from pytorch_glow_amd import parallel, training
from test_gpu_lu_param_model import hps_for, lu_glow
hps = hps_for(True, 4)
hps.optim.update(optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8), lr_scheduler="noam",
                 lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5))
hps.ablation.update(max_grad_clip=5, max_grad_norm=100)
glow = lu_glow(train=True, hps=hps)
before = {k: v.detach().clone() for k, v in glow.state_dict().items()}
x = torch.rand(4, 3, 16, 16, device="cuda:0")
parallel.FORCE_EXCHANGE = True
loop = training.TrainLoop(glow, hps, rank=0, world=1)
l0, n0 = loop.step(x)
loop.flush()
torch.cuda.synchronize()
assert torch.isfinite(l0) and torch.isfinite(n0)
plan = glow.flow.plan_for(x)
lay = plan._bucket_layout()
small = len(lay["sizes"]) - 1
names = [(n, b) for (i, n, p), (b, off) in zip(plan._grad_fields(), lay["slots"]) if n.startswith("lu_")]
assert len(names) == 18 and all(b == small for _, b in names), names
inv = glow.flow.layers[1].invconv
assert inv.l.grad is not None and inv.u.grad is not None and inv.log_s.grad is not None
assert not torch.equal(inv.log_s, before["flow.layers.1.invconv.log_s"]), "log_s did not move"
assert parallel._SIDE_STREAMS, "the RCCL bucket path did not run"
print("RCCL_LU_OK", dist.get_backend(), dist.get_world_size())
dist.destroy_process_group()
''' % (root, root, _free_port())
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "RCCL_LU_OK nccl 1" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
