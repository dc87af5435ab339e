"""The Polyak average through the model's training paths: the eager and the captured step (training.TrainLoop, GraphedTrainStep
with a fourth hyper word) keep the same average to the bit; an evaluation under `training.averaged_weights` sees exactly the
weights `util.averaged_state_dict` extracts from a snapshot, moves no address and costs the captured step no recapture; and
`Builder.build(training=False)` with ``hps.general.use_ema`` loads the average.  Model and batches as in
test_gpu_grad.py::test_graphed_training_step_equals_the_eager_step_bitwise."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib, training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from pytorch_glow_amd.network import Builder  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

DEV = "cuda:0"
K, BATCH, STEPS = 2, 8, 6


def make_hps():
    cfg = O.default_cfg(K=K, batch=BATCH)
    hps = util.AttrDict(dict(
        profile="ema", model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                                  actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False, flow_permutation=cfg["flow_permutation"],
                      flow_coupling=cfg["flow_coupling"], max_grad_clip=5, max_grad_norm=100),
        optim=dict(num_batch_train=BATCH, optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                   lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5), ema_decay=0.9),
        dataset=dict(num_classes=1), device=dict(graph=["cuda:0"], data=["cuda:0"]),
        general=dict(result_dir=".", warm_start=True, pre_trained="", resume_run_id="", resume_step="")))
    return cfg, hps


def fresh_glow(hps, sd=None):
    glow = G.Glow(hps)
    if sd is not None:
        sd = dict(sd); sd["h_top"] = torch.zeros_like(glow.h_top)
        glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    return glow.to(DEV)


def batch_of(step):
    return torch.rand(BATCH, 3, 64, 64, generator=torch.Generator().manual_seed(3700 + step)).to(DEV)


def step_both(loops, step):
    xs = batch_of(step)
    outs = []
    for loop in loops:
        torch.manual_seed(200 + step)                        # the step draws its dequantisation noise from torch's generator
        loss, norm = loop.step(xs)
        outs.append((loss.clone(), norm.clone()))
    return outs


def opt_state(loop):
    return {k: {n: torch.as_tensor(v).detach().cpu().clone() for n, v in st.items()} for k, st in loop.optimizer.state_dict()["state"].items()}


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Six steps of an eager and a graphed loop with ema_decay = 0.9 (run once for the module), what test 7 compares -- copies taken
    right after the sixth step -- and a snapshot of the graphed loop written at that point."""
    cfg, hps = make_hps()
    sd = O.seeded_state_dict(cfg, seed=37, invconv_perturb=0.02, zeros_std=0.01)
    with torch.no_grad():
        loops = [training.TrainLoop(fresh_glow(hps, sd).train(), hps, graph=False), training.TrainLoop(fresh_glow(hps, sd).train(), hps, graph=True)]
        outs = [step_both(loops, step) for step in range(STEPS)]
        for loop in loops:
            loop.flush()
        after6 = dict(outs=outs, params=[{k: v.detach().cpu().clone() for k, v in loop.glow.state_dict().items()} for loop in loops],
                      state=[opt_state(loop) for loop in loops], steps=[loop.optimizer._steps for loop in loops],
                      ema_updates=[loop.optimizer.ema_updates for loop in loops], graph_error=loops[1].graph_error,
                      graphed=[loop._graphed is not None for loop in loops])
        subdir = str(tmp_path_factory.mktemp("ema_snapshot"))
        util.save_model(subdir, STEPS, loops[1].glow, loops[1].optimizer, seconds=0.0, is_best=False)
    return dict(hps=hps, loops=loops, after6=after6, snapshot=os.path.join(subdir, util.get_model_name(STEPS)))


def test_eager_and_captured_steps_keep_the_same_average(trained):
    a = trained["after6"]
    assert a["graph_error"] is None and a["graphed"] == [False, True]
    assert a["steps"] == [STEPS, STEPS] and a["ema_updates"] == [STEPS, STEPS]
    for step, (eager, graphed) in enumerate(a["outs"]):
        assert torch.equal(eager[0], graphed[0]) and torch.equal(eager[1], graphed[1]), (step, eager, graphed)
        assert torch.isfinite(eager[0]) and torch.isfinite(eager[1])
    pa, pb = a["params"]
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    sa, sb = a["state"]
    assert sa.keys() == sb.keys() and len(sa) > 60
    moved = 0
    for k in sa:
        assert set(sa[k]) == set(sb[k]) and "ema" in sa[k]
        for name in sa[k]:
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)
    names = [n for n, _ in trained["loops"][0].glow.named_parameters()]
    for k in sa:      # the average is a real one: it trails the parameters that moved
        moved += int(not torch.equal(sa[k]["ema"], pa[names[k]]))
    assert moved > 60


def test_evaluation_under_the_average_keeps_the_captured_step(trained):
    hps, loops = trained["hps"], trained["loops"]
    eager, graphed = loops
    x = batch_of(100)
    noise = torch.rand(BATCH, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV) / 256
    for loop in loops:
        loop.glow.eval()
    nll_of = lambda glow: glow.normal_flow(x, None, noise=noise)[1].clone()
    live_before = nll_of(graphed.glow)
    recaptures, the_graph = graphed.graph_recaptures, graphed._graphed
    ptrs = [p.data_ptr() for p in graphed.glow.parameters()]
    with training.averaged_weights(graphed.optimizer):
        nll_swapped = nll_of(graphed.glow)
        assert graphed._graphed.valid()
        with pytest.raises(_lib.GlowHipError):
            graphed._graphed(x, 1e-4)
        for call in (lambda: graphed.step(x), graphed.flush):      # nothing of the loop trains -- or re-runs a batch -- while swapped
            with pytest.raises(_lib.GlowHipError):
                call()
        assert graphed.global_step == STEPS
    state = torch.load(trained["snapshot"], map_location="cpu")
    other = fresh_glow(hps).eval()
    other.load_state_dict(util.averaged_state_dict(state, other))
    nll_loaded = nll_of(other)
    assert torch.equal(nll_swapped, nll_loaded)
    assert not torch.equal(nll_swapped, live_before)
    assert torch.equal(nll_of(graphed.glow), live_before)            # swapped back: the live weights' bits
    assert [p.data_ptr() for p in graphed.glow.parameters()] == ptrs
    assert graphed.optimizer._steps == STEPS and graphed.optimizer.ema_updates == STEPS
    # the seventh step: a replay of the SAME captured graph, equal to the eager twin's
    (l0, n0), (l1, n1) = step_both(loops, STEPS)
    for loop in loops:
        loop.flush()
    assert graphed.graph_error is None and graphed.graph_recaptures == recaptures and graphed._graphed is the_graph
    assert graphed._graphed.valid()
    assert torch.equal(l0, l1) and torch.equal(n0, n1) and torch.isfinite(l0)
    pa, pb = eager.glow.state_dict(), graphed.glow.state_dict()
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    sa, sb = opt_state(eager), opt_state(graphed)
    for k in sa:
        for name in sa[k]:
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)


@pytest.mark.parametrize("use_ema", [True, False])
def test_builder_loads_the_average_for_inference(trained, use_ema, tmp_path):
    _, hps = make_hps()
    hps.general.update(pre_trained=trained["snapshot"], result_dir=str(tmp_path), use_ema=use_ema)
    built = Builder(hps).build(training=False)
    assert built["step"] == STEPS and built["optimizer"] is None
    state = torch.load(trained["snapshot"], map_location="cpu")
    params = list(built["graph"].named_parameters())
    assert len(params) > 60
    for i, (name, p) in enumerate(params):
        want = state["optimizer"]["state"][i]["ema"] if use_ema else state["graph"][name]
        assert torch.equal(p.detach().cpu(), want), (i, name)
    differ = sum(int(not torch.equal(state["optimizer"]["state"][i]["ema"], state["graph"][n])) for i, (n, _) in enumerate(params))
    assert differ > 60


def test_trainer_evaluates_under_the_average(tmp_path):
    """`Trainer.train` with hps.optim.ema_eval on one rank: every interval_valid / interval_sample block runs between a swap in and
    a swap out (the parameters ARE the average inside), nothing but the two swaps surrounds them -- no flush of the deferred range
    check, which on several ranks would be a collective issued by rank 0 alone -- training goes on afterwards on the captured
    step, and the snapshot carries the average.  ema_eval without ema_decay is refused when the Trainer is built."""
    from pytorch_glow_amd.network import Trainer

    class Synthetic(torch.utils.data.Dataset):
        def __init__(self):
            g = torch.Generator().manual_seed(0)
            base = torch.rand(1, 3, 16, 16, generator=g)
            self.x = (base + 0.05 * torch.rand(32, 3, 16, 16, generator=g)).clamp(0, 1)

        def __len__(self):
            return self.x.shape[0]

        def __getitem__(self, i):
            return {"x": self.x[i]}

    def small_hps(**optim):
        hps = util.AttrDict(dict(
            profile="ema", model=dict(image_shape=[16, 16, 3], hidden_channels=32, K=2, L=2, actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
            ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False, flow_permutation="invconv",
                          flow_coupling="affine", max_grad_clip=5, max_grad_norm=100, seed=1),
            optim=dict(optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8), lr_scheduler="noam",
                       lr_scheduler_args=dict(warmup_steps=20, min_lr=1e-5), num_batch_train=8, num_epochs=8, interval_scalar=1,
                       interval_snapshot=4, interval_valid=3, interval_sample=5, num_sample=2, **optim),
            dataset=dict(num_classes=1, num_workers=0), device=dict(graph=["cuda:0"], data=["cuda:0"]),
            general=dict(result_dir=str(tmp_path), warm_start=False, pre_trained="", resume_run_id="", resume_step="")))
        return hps

    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(hps=small_hps(ema_eval=True), dataset=Synthetic(), **Builder(small_hps(ema_eval=True)).build())

    hps = small_hps(ema_decay=0.9, ema_eval=True)
    util.manual_seed(3)
    state = Builder(hps).build()
    trainer = Trainer(hps=hps, dataset=Synthetic(), **state)
    opt = trainer.loop.optimizer
    assert opt is state["optimizer"] and opt.ema_decay == 0.9
    probe = max(opt.param_groups[0]["params"], key=lambda p: p.numel())
    events = []
    swap, flush, forward = opt.swap_averaged, trainer.loop.flush, trainer.graph.forward

    def swap_logged():
        before = (probe.detach().clone(), opt.state[probe]["ema"].clone()) if "ema" in opt.state[probe] else None
        swap()
        events.append(("swap", trainer.step, opt.swapped,
                       before is not None and torch.equal(probe.detach(), before[1]) and torch.equal(opt.state[probe]["ema"], before[0])))

    opt.swap_averaged = swap_logged
    trainer.loop.flush = lambda: (events.append(("flush", trainer.step)), flush())[1]
    trainer.graph.forward = lambda *a, **k: (events.append(("eval", trainer.step, opt.swapped)), forward(*a, **k))[1]
    trainer.train()
    assert trainer.step == 8 and not opt.swapped and opt.ema_updates == opt._steps == 8
    # validation at steps 3 and 6 (two model calls each), sampling at step 5 (one): each block between its two swaps, the model calls
    # inside under the average; the only flushes are the snapshot's (step 4, before the swap-free save) and the final one
    want = []
    for step, calls in ((3, 2), (5, 1), (6, 2)):
        want += [("swap", step, True, True)] + [("eval", step, True)] * calls + [("swap", step, False, True)]
    assert [e for e in events if e[0] != "flush"] == want, events
    assert [e for e in events if e[0] == "flush"] == [("flush", 4), ("flush", 8)], events
    assert trainer.loop.graph_error is None and (trainer.loop._graphed is not None or trainer.loop.graph_recaptures > 0)
    snap = torch.load(os.path.join(state["result_subdir"], util.get_model_name(4)), map_location="cpu", weights_only=False)
    assert set(snap) == set(util.SNAPSHOT_KEYS) and all("ema" in st for st in snap["optimizer"]["state"].values())
    assert snap["optimizer"]["param_groups"][0]["ema_updates"] == 5
    averaged = util.averaged_state_dict(snap, trainer.graph)
    assert sum(int(not torch.equal(averaged[k], snap["graph"][k])) for k in averaged) > 20
