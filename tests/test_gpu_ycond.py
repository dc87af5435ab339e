"""Class-conditional Glow on the HIP path (-m gpu): the top head (csrc/tophead.hip) against the vectors the REAL reference
recorded for the tiny model (tests/golden/g10_glow_tiny_ycond.npz: {learn_top off, on} x {CE, BCE}).

Bounds: z, nll 1e-4 absolute (what test_learned_top_prior_trains_on_the_hip_path holds the same model to); y_logits within the
z bound carried through the classifier, 1e-4 * max(1, max_k exp(3 logs_k) sum_c |W[k, c]|); every gradient and dx within
2e-4 * max|g| + 1e-7 per tensor (tests/test_gpu_grad.py); decoded images 1e-4 (tests/test_gpu_parity.py, G7 dec_x)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from conftest import load_golden, sub  # noqa: E402

import ycond_oracle as Y  # noqa: E402
from test_ycond_host import ycond_hps  # noqa: E402

DEV = "cuda:0"
CRIT = {"ce": "single_class", "bce": "multi_class"}


def build(g, lt, weight_y=None, train=False):
    hps = ycond_hps(learn_top=bool(lt), weight_y=float(g["weight_y"]) if weight_y is None else weight_y, device=DEV)
    np.random.seed(3)
    glow = G.Glow(hps)
    glow.load_state_dict(Y.case_state(g, lt), strict=True)
    glow.set_actnorm_inited()
    glow = glow.to(DEV)
    return glow.train() if train else glow.eval()


def labels(g, crit):
    return g[f"y_onehot_{crit}"].to(DEV), torch.from_numpy(g["y"]).to(DEV)


def err(a, b):
    return float((a.detach().cpu().double() - b.double()).abs().max())


def check_grads(glow, ref, tag):
    for name, p in glow.named_parameters():
        if name in ("h_top", "learn_top.weight"):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name      # (learn_top.weight multiplies h_top == 0)
            continue
        r = ref[name]
        assert p.grad is not None, f"{tag}: {name} has no gradient"
        e = err(p.grad, r)
        bound = 2e-4 * float(r.abs().max()) + 1e-7
        print(f"{tag} {name}: err {e:.3e} bound {bound:.3e}")
        assert e <= bound, f"{tag} {name}: err {e:.3e} > {bound:.3e}"


@pytest.mark.parametrize("lt,crit", Y.CASES)
def test_conditional_forward_matches_the_reference(lt, crit):
    g = load_golden("g10_glow_tiny_ycond")
    c = sub(g, f"lt{lt}_{crit}.")
    glow = build(g, lt)
    yo, _ = labels(g, crit)
    z, nll, y_logits = glow.normal_flow(g["x"].to(DEV), yo, noise=g["noise"].to(DEV))
    lb = Y.logit_bound(Y.case_state(g, lt), 1e-4)
    print(f"lt{lt}_{crit}: z {err(z, g['z']):.2e} nll {err(nll, c['nll']):.2e} logits {err(y_logits, c['y_logits']):.2e} (bound {lb:.2e})")
    assert err(z, g["z"]) <= 1e-4 and err(nll, c["nll"]) <= 1e-4
    assert tuple(y_logits.shape) == (4, 5) and err(y_logits, c["y_logits"]) <= lb
    # the checked path (Glow.forward in eval / no_grad; it draws its own dequantisation noise) returns logits too, and the
    # prior is the reference's
    z2, nll2, lg2 = glow(x=g["x"].to(DEV), y_onehot=yo)
    assert z2.shape == z.shape and tuple(lg2.shape) == (4, 5) and bool(torch.isfinite(lg2).all()) and bool(torch.isfinite(nll2).all())
    mean, logs = glow.prior(yo)
    m_ref, l_ref = Y.prior(Y.case_state(g, lt), dict(Y.TINY, learn_top=bool(lt), y_condition=True), g[f"y_onehot_{crit}"])
    assert err(mean, m_ref) <= 2e-6 and err(logs, l_ref) <= 2e-6
    with pytest.raises(AssertionError):
        glow.normal_flow(g["x"].to(DEV), None, noise=g["noise"].to(DEV))


def test_no_logits_without_a_classifier_weight():
    g = load_golden("g10_glow_tiny_ycond")
    glow = build(g, 1, weight_y=0.0)
    yo, _ = labels(g, "ce")
    z, nll, y_logits = glow.normal_flow(g["x"].to(DEV), yo, noise=g["noise"].to(DEV))
    assert y_logits is None and err(nll, g["lt1_ce.nll"]) <= 1e-4
    counts = glow.flow.plan_for(g["x"].to(DEV)).launch_counts()
    assert counts.get("k_top_head_fwd", 0) >= 1


@pytest.mark.parametrize("lt,crit", Y.CASES)
def test_conditional_gradients_match_the_reference_on_both_routes(lt, crit):
    g = load_golden("g10_glow_tiny_ycond")
    c = sub(g, f"lt{lt}_{crit}.")
    ref, wy = sub(c, "grad."), float(g["weight_y"])
    yo, y = labels(g, crit)
    # (a) the reference's own step: normal_flow + the user's torch loss + loss.backward()
    glow = build(g, lt, train=True)
    with torch.enable_grad():
        xd = g["x"].to(DEV).requires_grad_(True)
        z, nll, y_logits = glow.normal_flow(xd, yo, noise=g["noise"].to(DEV))
        lg = G.Glow.generative_loss(nll)
        lc = G.Glow.single_class_loss(y_logits, y) if crit == "ce" else G.Glow.multi_class_loss(y_logits, yo)
        loss = lg + wy * lc
        loss.backward()
    assert abs(float(loss) - float(c["loss"])) <= 1e-4 and abs(float(lc) - float(c["loss_classes"])) <= Y.logit_bound(Y.case_state(g, lt), 1e-4)
    check_grads(glow, ref, f"autograd lt{lt}_{crit}")
    e = err(xd.grad, c["dx"])
    assert e <= 2e-4 * float(c["dx"].abs().max()) + 1e-7, f"dx err {e:.3e}"
    # (b) the direct route: criterion and weight_y inside the head kernel
    glow = build(g, lt, train=True)
    loss_d = glow.loss_and_grads(g["x"].to(DEV), noise=g["noise"].to(DEV), y_onehot=yo, y=y if crit == "ce" else None, criterion=CRIT[crit])
    lgen, lcls = glow.last_losses
    assert abs(float(loss_d) - float(c["loss"])) <= 1e-4 and abs(float(lgen) - float(c["loss_generative"])) <= 1e-4
    assert abs(float(lcls) - float(c["loss_classes"])) <= Y.logit_bound(Y.case_state(g, lt), 1e-4)
    check_grads(glow, ref, f"direct lt{lt}_{crit}")
    buckets = glow.flow.pop_grad_buckets()
    assert buckets is not None and glow.y_emb.weight.grad.untyped_storage().data_ptr() == buckets[-1][0].untyped_storage().data_ptr()


def test_routes_agree_bitwise_without_a_classifier_term_and_runs_repeat_bitwise():
    g = load_golden("g10_glow_tiny_ycond")
    yo, y = labels(g, "bce")
    x, noise = g["x"].to(DEV), g["noise"].to(DEV)
    a, b = build(g, 1, weight_y=0.0, train=True), build(g, 1, weight_y=0.0, train=True)
    with torch.enable_grad():
        _, nll, lg = a.normal_flow(x, yo, noise=noise)
        la = G.Glow.generative_loss(nll)
        la.backward()
    assert lg is None
    lb = b.loss_and_grads(x, noise=noise, y_onehot=yo, criterion="multi_class")
    assert torch.equal(la.detach(), lb)
    ga = {n: p.grad for n, p in a.named_parameters() if p.grad is not None}
    gb = {n: p.grad for n, p in b.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb) and "y_emb.weight" in ga and "learn_top.logs" in ga and "classifier.weight" not in ga
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    # two runs, same bits: forward (z, nll, logits) and backward (every gradient), classifier term included
    outs = []
    for _ in range(2):
        m = build(g, 1, train=True)
        loss = m.loss_and_grads(x, noise=noise, y_onehot=yo, criterion="multi_class")
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        m.eval()
        z, nll, lg = m.normal_flow(x, yo, noise=noise)
        outs.append((loss.clone(), grads, z, nll, lg))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(outs[0][i], outs[1][i]) for i in (2, 3, 4))
    assert "classifier.weight" in outs[0][1] and all(torch.equal(outs[0][1][n], outs[1][1][n]) for n in outs[0][1])


@pytest.mark.parametrize("lt,crit", Y.CASES)
def test_conditional_sampling_and_reconstruction(lt, crit):
    g = load_golden("g10_glow_tiny_ycond")
    c = sub(g, f"lt{lt}_{crit}.")
    glow = build(g, lt)
    yo, _ = labels(g, crit)
    xs = glow.reverse_flow(None, yo, eps_std=0.6, eps=[c["sample_eps1"].to(DEV)], eps_top=c["sample_eps0"].to(DEV))
    xr = glow.reverse_flow(g["z"].to(DEV), yo, eps_std=0.6, eps=[c["recon_eps0"].to(DEV)])
    print(f"lt{lt}_{crit}: sample {err(xs, c['sample_x']):.2e} recon {err(xr, c['recon_x']):.2e}")
    assert err(xs, c["sample_x"]) <= 1e-4 and err(xr, c["recon_x"]) <= 1e-4
    other = torch.roll(yo, 1, dims=1) if crit == "ce" else 1.0 - yo
    xo = glow.reverse_flow(None, other, eps_std=0.6, eps=[c["sample_eps1"].to(DEV)], eps_top=c["sample_eps0"].to(DEV))
    assert float((xo - xs).abs().max()) > 1e-3          # another label, the same draws: another image
    from pytorch_glow_amd.network import Inferer
    inf = Inferer(hps=glow.hps, graph=glow, devices=[DEV], data_device=DEV)
    torch.manual_seed(5); i1 = inf.sample(z=None, y_onehot=yo, eps_std=0.6)
    torch.manual_seed(5); i2 = inf.sample(z=None, y_onehot=yo, eps_std=0.6)
    torch.manual_seed(5); i3 = inf.sample(z=None, y_onehot=other, eps_std=0.6)
    assert i1.shape == (4, 3, 16, 16) and torch.equal(i1, i2) and float((i1 - i3).abs().max()) > 1e-3
    with pytest.raises(AssertionError):
        inf.sample(z=None, y_onehot=None)


def test_an_overflowing_prior_is_flagged_never_finite():
    g = load_golden("g10_glow_tiny_ycond")
    glow = build(g, 0)
    yo, _ = labels(g, "ce")
    with torch.no_grad():
        glow.y_emb.logs.fill_(40.0)            # exp(120) overflows fp32: the prior's mean / logs become +-inf
    x = g["x"].to(DEV)
    z, nll, _ = glow.normal_flow(x, yo, noise=g["noise"].to(DEV))
    assert not bool(torch.isfinite(nll).any()), nll
    st = glow.flow.plan_for(x).status(4)
    assert bool((st != 0).all()), st


def test_the_head_is_one_launch_each_way():
    g = load_golden("g10_glow_tiny_ycond")
    x, noise = g["x"].to(DEV), g["noise"].to(DEV)
    yo, y = labels(g, "ce")
    glow = build(g, 1)
    plan = glow.flow.plan_for(x)
    plan.launch_counts(reset=True)
    glow.normal_flow(x, yo, noise=noise)
    c = plan.launch_counts(reset=True)
    assert c.get("k_top_head_fwd") == 1 and "k_top_head_bwd" not in c
    glow.train()
    glow.loss_and_grads(x, noise=noise, y_onehot=yo, y=y, criterion="single_class")
    c = plan.launch_counts(reset=True)
    assert c.get("k_top_head_fwd") == 1 and c.get("k_top_head_bwd") == 1 and c.get("k_top_head_reduce", 0) <= 1
    # an unconditional model launches none of them
    hps = ycond_hps(device=DEV)
    hps.ablation.y_condition = False
    np.random.seed(3)
    plain = G.Glow(hps)
    plain.load_state_dict({k: v for k, v in Y.case_state(g, 0).items() if not k.startswith(("y_emb.", "classifier."))})
    plain.set_actnorm_inited()
    plain = plain.to(DEV).train()
    pp = plain.flow.plan_for(x)
    pp.launch_counts(reset=True)
    plain.loss_and_grads(x, noise=noise)
    c = pp.launch_counts()
    assert not any(k.startswith("k_top_head") for k in c), c


class _Labelled(torch.utils.data.Dataset):
    """Two visibly different classes: the label shifts the image's brightness."""

    def __init__(self, n=32):
        gen = torch.Generator().manual_seed(0)
        self.y = torch.arange(n) % 5
        base = torch.rand(1, 3, 16, 16, generator=gen)
        self.x = (0.6 * base + 0.05 * torch.rand(n, 3, 16, 16, generator=gen) + 0.06 * self.y.view(-1, 1, 1, 1).float()).clamp(0, 1)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        multi = torch.nn.functional.one_hot(self.y[i], 5).float()
        multi[(int(self.y[i]) + 2) % 5] = 1.0
        return {"x": self.x[i], "y": self.y[i], "y_onehot": multi}


def _train_hps(criterion, learn_top=False, y_condition=True):
    hps = ycond_hps(learn_top=learn_top, criterion=criterion, device=DEV, batch=8)
    hps.ablation.y_condition = y_condition
    hps.optim.update(num_epochs=12, interval_scalar=1, interval_snapshot=8, interval_valid=5, interval_sample=7,
                     optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8), lr_scheduler_args=dict(warmup_steps=20, min_lr=1e-5))
    return hps


@pytest.mark.parametrize("criterion", ["single_class", "multi_class"])
def test_trainer_trains_a_conditional_model_with_the_captured_step(tmp_path, criterion):
    from pytorch_glow_amd.network import Trainer
    hps = _train_hps(criterion)
    util.manual_seed(3)
    glow = G.Glow(hps).to(DEV)
    opt = training.build_optimizer(hps, glow.parameters())
    trainer = Trainer(hps=hps, result_subdir=str(tmp_path), step=0, graph=glow, optimizer=opt, scheduler=None, devices=[DEV],
                      dataset=_Labelled(), data_device=DEV)
    losses, cls = [], []
    orig = trainer.loop.step

    def step(x, **kw):
        r = orig(x, **kw)
        losses.append(float(r[0])); cls.append(float(glow.last_losses[1]))
        return r

    trainer.loop.step = step
    trainer.train(max_steps=12)
    assert len(losses) == 12 and all(np.isfinite(losses)) and all(np.isfinite(cls)), (losses, cls)
    assert trainer.loop.graph_error is None and (trainer.loop._graphed is not None or trainer.loop.graph_recaptures > 0), trainer.loop.graph_error
    assert min(losses[-2:]) < losses[0], losses
    assert "loss/classification_loss" in trainer.writer.scalars if hasattr(trainer.writer, "scalars") else True
    # a reference-format snapshot of the conditional model loads back and samples
    snap = os.path.join(str(tmp_path), util.get_model_name(8))
    assert os.path.exists(snap)
    other = G.Glow(hps)
    st = util.load_model(str(tmp_path), 8, other, device="cpu")
    assert st["step"] == 8 and "y_emb.weight" in other.state_dict() and float(other.y_emb.weight.abs().max()) > 0
    other = other.to(DEV).eval()
    yo = torch.eye(5, device=DEV)[torch.arange(8) % 5]
    img = other(z=None, y_onehot=yo, eps_std=0.5, reverse=True)
    assert img.shape == (8, 3, 16, 16) and bool(torch.isfinite(img).all())


@pytest.mark.parametrize("criterion,lt,ycond", [("multi_class", True, True), ("single_class", False, True), (None, True, False)])
def test_graphed_conditional_step_equals_the_eager_step_bitwise(criterion, lt, ycond):
    """Two loops from the same state, same batches, labels and seeds: one eager, one captured from TrainLoop.GRAPH_AFTER on (both on
    the direct route) -- loss, gradient norm, every parameter and the optimiser state the same bits.  The third case is a
    learn_top-only model, which now takes the direct and the captured step too."""
    hps = _train_hps(criterion or "single_class", learn_top=lt, y_condition=ycond)
    g = load_golden("g10_glow_tiny_ycond")
    sd = {k: v for k, v in Y.case_state(g, int(lt)).items() if ycond or not k.startswith(("y_emb.", "classifier."))}

    def fresh():
        np.random.seed(3)
        glow = G.Glow(hps)
        sd2 = dict(sd); sd2["h_top"] = torch.zeros_like(glow.h_top)
        glow.load_state_dict(sd2)
        glow.set_actnorm_inited()
        return glow.to(DEV).train()

    data = _Labelled()
    loops = [training.TrainLoop(fresh(), hps, graph=False), training.TrainLoop(fresh(), hps, graph=True)]
    assert loops[0].criterion == (criterion if ycond else None)
    for step in range(6):
        idx = torch.arange(8) + 8 * (step % 4)
        xs = data.x[idx].to(DEV)
        kw = {}
        if ycond:
            items = [data[int(i)] for i in idx]
            kw["y_onehot"] = (torch.stack([it["y_onehot"] for it in items]) if criterion == "multi_class"
                              else torch.eye(5)[data.y[idx]]).to(DEV)
            kw["y"] = data.y[idx].to(DEV) if criterion == "single_class" else None
        outs = []
        for loop in loops:
            torch.manual_seed(300 + step)
            loss, norm = loop.step(xs, **kw)
            outs.append((loss.clone(), norm.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (step, outs)
        assert torch.isfinite(outs[0][0]) and torch.isfinite(outs[0][1])
    for loop in loops:
        loop.flush()
    assert loops[1].graph_error is None and loops[1]._graphed is not None and loops[0]._graphed is None, loops[1].graph_error
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    sa, sb = loops[0].optimizer.state_dict()["state"], loops[1].optimizer.state_dict()["state"]
    for k in sa:
        for name in sa[k]:
            assert torch.equal(torch.as_tensor(sa[k][name]).cpu(), torch.as_tensor(sb[k][name]).cpu()), (k, name)


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_conditional_step_under_a_one_rank_rccl_group():
    """A conditional training step with the gradient exchange forced through RCCL over a one-rank group, in a fresh child
    process started before any GPU call here could matter to it (a process group per pytest process would leak)."""
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
from test_ycond_host import ycond_hps
hps = ycond_hps(learn_top=True, criterion="multi_class", device="cuda:0")
glow = G.Glow(hps).to("cuda:0")
x = torch.rand(4, 3, 16, 16, device="cuda:0")
yo = (torch.rand(4, 5, device="cuda:0") > 0.5).float()
parallel.FORCE_EXCHANGE = True
loop = training.TrainLoop(glow, hps, rank=0, world=1)
l0, n0 = loop.step(x, y_onehot=yo)
l1, n1 = loop.step(x, y_onehot=yo)
loop.flush()
torch.cuda.synchronize()
assert torch.isfinite(l0) and torch.isfinite(l1) and torch.isfinite(n1)
assert glow.y_emb.weight.grad is not None and glow.classifier.weight.grad is not None and glow.learn_top.bias.grad is not None
assert float(glow.y_emb.weight.abs().max()) > 0, "y_emb did not move"
assert parallel._SIDE_STREAMS, "the RCCL bucket path did not run"
print("RCCL_YCOND_OK", dist.get_backend(), dist.get_world_size())
dist.destroy_process_group()
''' % (root, root, _free_port())
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "RCCL_YCOND_OK nccl 1" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
