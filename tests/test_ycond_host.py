"""Class-conditional Glow (ablation.y_condition) without a GPU: module surface, the CPU restatement of the head
(tests/ycond_oracle.py) against the vectors the REAL reference recorded (tests/golden/make_golden_ycond.py), and the host
logic that carries labels through Trainer / TrainLoop / the gradient buckets / a 2-rank gloo group.

Bounds: those tests/test_oracle_golden.py holds the oracle to on the same tiny model -- z 2e-5, nll and the generative loss
2e-6, decoded image 5e-5; y_logits and the classification loss within the z bound carried through the classifier (both losses
are 1-Lipschitz in the logits); gradients within 2e-4 * max|g| + 1e-7 per tensor (fp32 torch on both sides)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib, parallel, training
from pytorch_glow_amd._plan import FlowPlan
from pytorch_glow_amd.misc import util
from conftest import load_golden, sub

import ycond_oracle as Y


def ycond_hps(learn_top=False, weight_y=0.5, device="cpu", criterion="single_class", batch=4, num_classes=5):
    return util.AttrDict(dict(
        profile="ycond",
        model=dict(image_shape=[16, 16, 3], hidden_channels=32, K=2, L=2, actnorm_scale=1.0, n_bits_x=8, weight_y=weight_y),
        ablation=dict(learn_top=learn_top, y_condition=True, y_criterion=criterion, lu_decomposition=False,
                      flow_permutation="invconv", flow_coupling="affine", max_grad_clip=5, max_grad_norm=100, seed=1),
        optim=dict(optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8), lr_scheduler="noam",
                   lr_scheduler_args=dict(warmup_steps=10, min_lr=1e-5), num_batch_train=batch, num_epochs=100,
                   interval_scalar=1, interval_snapshot=10 ** 6, interval_valid=10 ** 6, interval_sample=10 ** 6, num_sample=2),
        dataset=dict(num_classes=num_classes, num_workers=0), device=dict(graph=[device], data=[device]),
        general=dict(result_dir=".", warm_start=True, pre_trained="", resume_run_id="", resume_step="")))


def cfg_for(g, lt):
    return dict(Y.TINY, learn_top=bool(lt), y_condition=True, weight_y=float(g["weight_y"]))


@pytest.mark.parametrize("lt", [0, 1])
def test_conditional_glow_constructs_with_the_reference_state_dict(lt):
    g = load_golden("g10_glow_tiny_ycond")
    np.random.seed(3)
    glow = G.Glow(ycond_hps(learn_top=bool(lt)))
    mine = sorted("{}|{}".format(k, ",".join(str(d) for d in v.shape)) for k, v in glow.state_dict().items())
    assert mine == [str(s) for s in g[f"keys_lt{lt}"]]
    assert isinstance(glow.y_emb, G.LinearZeros) and isinstance(glow.classifier, G.LinearZeros)
    glow.load_state_dict(Y.case_state(g, lt), strict=True)      # a reference-written conditional state dict loads as it is
    with pytest.raises(AssertionError):
        glow.prior(None)                                        # the reference's assertion (network/model.py:377)


@pytest.mark.parametrize("lt,crit", Y.CASES)
def test_cpu_restatement_reproduces_the_reference(lt, crit):
    g = load_golden("g10_glow_tiny_ycond")
    c = sub(g, f"lt{lt}_{crit}.")
    cfg, sd = cfg_for(g, lt), Y.case_state(g, lt)
    yo, y, wy = g[f"y_onehot_{crit}"], torch.from_numpy(g["y"]), float(g["weight_y"])
    with torch.enable_grad():
        leaf = {k: v.clone().requires_grad_(k != "h_top") for k, v in sd.items()}
        x = g["x"].clone().requires_grad_(True)
        z, nll, y_logits = Y.glow_forward(x, g["noise"], leaf, cfg, yo)
        loss_gen = nll.mean()
        loss_cls = Y.classification_loss(y_logits, crit, y=y, y_onehot=yo)
        loss = loss_gen + wy * loss_cls
        loss.backward()
    err = lambda a, b: float((a.detach().double() - b.double()).abs().max())
    lb = Y.logit_bound(sd, 2e-5)
    print(f"lt{lt}_{crit}: z {err(z, g['z']):.2e} nll {err(nll, c['nll']):.2e} logits {err(y_logits, c['y_logits']):.2e} (bound {lb:.2e})")
    assert err(z, g["z"]) <= 2e-5 and err(nll, c["nll"]) <= 2e-6 and err(loss_gen, c["loss_generative"]) <= 2e-6
    assert err(y_logits, c["y_logits"]) <= lb and err(loss_cls, c["loss_classes"]) <= lb
    ref = sub(c, "grad.")
    assert set(ref) == {k for k in sd if k not in ("h_top", "learn_top.weight")} and leaf["h_top"].grad is None
    if lt:
        assert bool(c["learn_top_weight_grad_is_zero"]) and float(leaf["learn_top.weight"].grad.abs().max()) == 0.0
    for k, want in ref.items():
        assert err(leaf[k].grad, want) <= 2e-4 * float(want.abs().max()) + 1e-7, k
    assert err(x.grad, c["dx"]) <= 2e-4 * float(c["dx"].abs().max()) + 1e-7
    # conditional sample (top draw + one per Split2d, all recorded) and reconstruction from z
    xs = Y.glow_sample(sd, cfg, yo, c["sample_eps0"], [c["sample_eps1"]])
    assert err(xs, c["sample_x"]) <= 5e-5
    from oracle import glow_oracle as O
    xr = O.glow_reverse(g["z"], sd, cfg, [c["recon_eps0"]])
    assert err(xr, c["recon_x"]) <= 5e-5


def test_y_logits_are_absent_without_a_classifier_weight():
    g = load_golden("g10_glow_tiny_ycond")
    cfg = dict(cfg_for(g, 0), weight_y=0.0)
    _, _, y_logits = Y.glow_forward(g["x"], g["noise"], Y.case_state(g, 0), cfg, g["y_onehot_ce"])
    assert y_logits is None
    glow = G.Glow(ycond_hps(weight_y=0.0))
    assert "cl_w" not in glow._head_parts() and "ye_w" in glow._head_parts()


# ----------------------------------------------------------------------------- host logic
class _Labelled(torch.utils.data.Dataset):
    def __init__(self, n=8, with_y=True, with_onehot=True):
        gen = torch.Generator().manual_seed(0)
        self.x = torch.rand(n, 3, 16, 16, generator=gen)
        self.y = torch.arange(n) % 5
        self.with_y, self.with_onehot = with_y, with_onehot

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        item = {"x": self.x[i]}
        if self.with_y:
            item["y"] = self.y[i]
        if self.with_onehot:
            item["y_onehot"] = torch.nn.functional.one_hot(self.y[i], 5).float()
        return item


def _trainer(tmp_path, criterion, dataset):
    from pytorch_glow_amd.network.trainer import Trainer
    hps = ycond_hps(criterion=criterion)
    glow = G.Glow(hps)
    return Trainer(hps=hps, result_subdir=str(tmp_path), step=0, graph=glow, optimizer=torch.optim.Adam(glow.parameters(), lr=1e-4),
                   scheduler=None, devices=["cpu"], dataset=dataset, data_device="cpu")


def test_trainer_extracts_labels_as_the_reference(tmp_path):
    tr = _trainer(tmp_path, "single_class", _Labelled())
    batch = next(iter(tr.data_loader))
    y, yo = tr.labels_of(batch)
    assert torch.equal(y, batch["y"]) and yo.shape == (4, 5) and torch.equal(yo.argmax(1), y) and float(yo.sum()) == 4.0
    with pytest.raises(AssertionError, match='Single-class criterion needs "y" in batch data'):
        tr.labels_of({"x": batch["x"], "y_onehot": batch["y_onehot"]})
    tr = _trainer(tmp_path, "multi_class", _Labelled())
    y, yo = tr.labels_of(batch)
    assert y is None and torch.equal(yo, batch["y_onehot"])
    with pytest.raises(AssertionError, match='Multi-class criterion needs "y_onehot" in batch data'):
        tr.labels_of({"x": batch["x"], "y": batch["y"]})
    with pytest.raises(AssertionError, match="Unsupported criterion: focal"):
        _trainer(tmp_path, "focal", _Labelled())
    # 'multi_class' is BCE over a multi-hot target here (the reference's table calls single_class_loss, which raises for one)
    lg, multi = torch.randn(4, 5), torch.tensor([[1., 0, 1, 0, 0]] * 4)
    assert torch.equal(tr.criterion_dict["multi_class"](lg, multi), G.Glow.multi_class_loss(lg, multi))


def test_train_loop_forwards_labels(monkeypatch):
    hps = ycond_hps(criterion="multi_class")
    glow = G.Glow(hps)
    seen = {}

    def fake_step(glow_, opt, x, **kw):
        seen.update(kw, x=x)
        return torch.zeros(()), torch.zeros(())

    def fake_init(glow_, x, rank, world, init_fn=None, y_onehot=None):
        seen["init_y_onehot"] = y_onehot
        glow_.set_actnorm_inited()

    monkeypatch.setattr(parallel, "train_step", fake_step)
    monkeypatch.setattr(parallel, "data_dependent_init", fake_init)
    loop = training.TrainLoop(glow, hps, optimizer=torch.optim.Adam(glow.parameters(), lr=1e-4))
    x, yo = torch.rand(4, 3, 16, 16), torch.eye(5)[:4]
    loop.step(x, y_onehot=yo)
    assert seen["y_onehot"] is yo and seen["y"] is None and seen["criterion"] == "multi_class" and seen["init_y_onehot"] is yo
    assert loop.criterion == "multi_class"
    # the deferred range check keeps the labels with their batch
    stash = training.TrainLoop._stash
    assert "y_onehot" in stash.__code__.co_varnames and "y" in stash.__code__.co_varnames


@pytest.mark.parametrize("lt,wy", [(False, 0.5), (True, 0.5), (True, 0.0)])
def test_head_parameters_sit_in_the_last_gradient_bucket(lt, wy):
    glow = G.Glow(ycond_hps(learn_top=lt, weight_y=wy))
    plan = FlowPlan.__new__(FlowPlan)                       # host bookkeeping only: no C plan, no device
    plan.layers = list(glow.flow.layers)
    plan._head_parts = tuple(glow._head_parts().items())
    fields, lay = plan._grad_fields(), plan._bucket_layout()
    head = [(f, slot) for f, slot in zip(fields, lay["slots"]) if f[0] < 0]
    names = [f[1] for f, _ in head]
    want = (["lt_bias", "lt_logs"] if lt else []) + ["ye_w", "ye_b", "ye_logs"] + (["cl_w", "cl_b", "cl_logs"] if wy > 0 else [])
    assert names == want and set(names) <= set(_lib.HEAD_PARAMS)
    last = len(lay["sizes"]) - 1
    assert all(slot[0] == last for _, slot in head)
    ends = [slot[1] + f[2].numel() for f, slot in head]
    assert max(ends) <= lay["sizes"][last] and all(slot[1] % 64 == 0 for _, slot in head)
    params = {id(p) for p in plan.trainable_parameters()}
    assert id(glow.y_emb.weight) in params and (id(glow.classifier.weight) in params) == (wy > 0)
    if lt:
        assert id(glow.learn_top.bias) in params and id(glow.learn_top.weight) not in params      # (it multiplies h_top == 0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _label_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = load_golden("g10_glow_tiny_ycond")
        x = parallel.shard_batch(g["x"], world, rank)
        yo = parallel.shard_batch(g["y_onehot_bce"], world, rank)
        noise = parallel.shard_batch(g["noise"], world, rank)
        sd = Y.case_state(g, 1)
        with torch.no_grad():
            _, nll, lg = Y.glow_forward(x, noise, dict(sd, h_top=sd["h_top"][:x.shape[0]]), cfg_for(g, 1), yo)
        ret[rank] = dict(n=x.shape[0], yo=yo, nll=parallel.gather_nll(nll, world), logits=parallel.gather_nll(lg, world))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_labels_are_sharded_with_x():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_label_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    g = load_golden("g10_glow_tiny_ycond")
    c = sub(g, "lt1_bce.")
    for r in (0, 1):
        assert ret[r]["n"] == 2 and torch.equal(ret[r]["yo"], g["y_onehot_bce"][2 * r:2 * r + 2])
        # every sample met ITS label: the gathered per-sample nll / logits are the global batch's (a label off by one rank would
        # move the nll by the prior's shift, orders of magnitude above this bound)
        assert float((ret[r]["nll"] - c["nll"]).abs().max()) <= 2e-6
        assert float((ret[r]["logits"] - c["y_logits"]).abs().max()) <= Y.logit_bound(Y.case_state(g, 1), 2e-5)
