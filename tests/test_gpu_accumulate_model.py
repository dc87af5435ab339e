"""Gradient accumulation through the model (-m gpu): `Glow.loss_and_grads(accumulate=k)`, `parallel.train_step`, the captured step and
`training.TrainLoop` with ``hps.optim.accumulate_steps``, held to tests/accumulate_oracle.py -- the composition of the k gradients
that k plain calls on the slices produce, to the bit -- and to fp64 autograd on the full batch.  Model: the small training
configuration of tests/test_gpu_grad.py (64x64x3, L = 3, hidden 512, K = 2, seeded weights) unless a test says otherwise."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib, _plan, parallel, training  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402

import accumulate_oracle as AO  # noqa: E402

DEV = "cuda:0"
K = 2
NUM_CLASSES = 5


def make_hps(batch, ycond=False, lu=False, cfg=None, **optim):
    cfg = cfg or O.default_cfg(K=K, batch=batch)
    return util.AttrDict(dict(
        model=dict(image_shape=cfg["image_shape"], hidden_channels=cfg["hidden_channels"], K=cfg["K"], L=cfg["L"],
                   actnorm_scale=1.0, n_bits_x=8, weight_y=0.5 if ycond else 0.0),
        ablation=dict(learn_top=False, y_condition=ycond, y_criterion="single_class", lu_decomposition=lu,
                      flow_permutation=cfg["flow_permutation"], flow_coupling=cfg["flow_coupling"], max_grad_clip=5, max_grad_norm=100),
        optim=dict(num_batch_train=batch, optimizer="adam", optimizer_args=dict(lr=1e-4, betas=[0.9, 0.9999], eps=1e-8),
                   lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5), **optim),
        dataset=dict(num_classes=NUM_CLASSES if ycond else 1), device=dict(graph=["cuda:0"])))


_SD = {}


def seeded(seed):
    """The flow's seeded state (tests/test_gpu_grad.py's), built once per seed; the batch size plays no part in it."""
    if seed not in _SD:
        _SD[seed] = O.seeded_state_dict(O.default_cfg(K=K, batch=8), seed=seed, invconv_perturb=0.02, zeros_std=0.01)
    return _SD[seed]


def fresh(hps, seed=31):
    """A model with the seeded flow on the device, in training mode, ActNorm marked initialised; a class-conditional head gets
    small seeded weights (the reference zero-initialises it: its gradients would be trivial)."""
    sd = seeded(seed)
    if hps.ablation.lu_decomposition:
        sd = util.lu_state_dict_from_dense(sd)
    np.random.seed(2)
    glow = G.Glow(hps)
    sd = {k: v.clone() for k, v in sd.items()}
    sd["h_top"] = torch.zeros_like(glow.h_top)
    if hps.ablation.y_condition:
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in glow.named_parameters():
            if name.startswith(("y_emb.", "classifier.")):
                sd[name] = torch.randn(p.shape, generator=g) * 0.05
    glow.load_state_dict(sd, strict=True)
    glow.set_actnorm_inited()
    return glow.to(DEV).train()


def batch_of(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, 64, 64, generator=g).to(DEV)
    noise = (torch.rand(n, 3, 64, 64, generator=g) / 256).to(DEV)
    y = torch.randint(0, NUM_CLASSES, (n,), generator=g).to(DEV)
    return x, noise, y


def grads_of(glow):
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in glow.named_parameters() if p.grad is not None}


def opt_state(loop):
    return {k: {n: torch.as_tensor(v).detach().cpu().clone() for n, v in st.items()} for k, st in loop.optimizer.state_dict()["state"].items()}


def same_tensor(a, b):
    return AO.same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


@pytest.mark.parametrize("n,k,kind", [(8, 4, "dense"), (6, 3, "class_conditional"), (4, 2, "lu")])
def test_accumulated_gradient_is_the_composition_of_the_micro_gradients(n, k, kind):
    """k plain calls on the slices, gradients cloned after each; then ONE accumulating call on the whole batch: every .grad is the
    oracle's composition of those k gradients, bit for bit, the loss is the mean of the k losses (and so are the two terms)."""
    ycond = kind == "class_conditional"
    hps = make_hps(n, ycond=ycond, lu=kind == "lu")
    glow = fresh(hps)
    x, noise, y = batch_of(n, seed=500 + n)
    labels = lambda lo, hi: dict(y_onehot=torch.eye(NUM_CLASSES, device=DEV)[y[lo:hi]], y=y[lo:hi], criterion="single_class") if ycond else {}
    micro, losses, terms = [], [], []
    for lo, hi in training.micro_slices(n, k):
        losses.append(glow.loss_and_grads(x[lo:hi], noise=noise[lo:hi], **labels(lo, hi)).clone())
        terms.append(tuple(None if t is None else t.clone() for t in glow.last_losses))
        micro.append(grads_of(glow))
    assert len(micro[0]) > 60 and all(torch.isfinite(l) for l in losses)
    ptrs = {name: p.grad.data_ptr() for name, p in glow.named_parameters() if p.grad is not None}
    loss = glow.loss_and_grads(x, noise=noise, accumulate=k, **labels(0, n))
    got = grads_of(glow)
    assert set(got) == set(micro[0])
    for name in got:
        want = AO.compose([m[name] for m in micro])
        assert AO.same_bits(got[name], want), name
    assert {name: p.grad.data_ptr() for name, p in glow.named_parameters() if p.grad is not None} == ptrs      # the same views
    assert torch.equal(loss, torch.stack(losses).mean())
    assert torch.equal(glow.last_losses[0], torch.stack([t[0] for t in terms]).mean())
    if ycond:
        assert torch.equal(glow.last_losses[1], torch.stack([t[1] for t in terms]).mean())
        assert any(np.abs(got[name]).max() > 0 for name in got if name.startswith("classifier."))
    else:
        assert glow.last_losses[1] is None
    if kind == "lu":
        assert any(name.endswith("invconv.l") for name in got) and not any(name.endswith("invconv.weight") for name in got)
    # a plain call afterwards is a plain call: the buckets are overwritten in full
    glow.loss_and_grads(x[:n // k], noise=noise[:n // k], **labels(0, n // k))
    again = grads_of(glow)
    assert all(AO.same_bits(again[name], micro[0][name]) for name in again)
    # noise=None: one draw of micro-batch shape per micro-step, in order
    torch.manual_seed(77)
    loss_drawn = glow.loss_and_grads(x, accumulate=k, **labels(0, n))
    drawn = grads_of(glow)
    torch.manual_seed(77)
    b = n // k
    draws = torch.cat([torch.empty((b,) + tuple(x.shape[1:]), device=DEV).uniform_(0, 1. / 256) for _ in range(k)])
    loss_given = glow.loss_and_grads(x, noise=draws, accumulate=k, **labels(0, n))
    given = grads_of(glow)
    assert torch.equal(loss_drawn, loss_given) and all(AO.same_bits(drawn[name], given[name]) for name in drawn)


def test_accumulated_gradient_against_fp64_autograd_on_the_full_batch():
    """The oracle route of test_gpu_grad.py::test_glow_gradients_vs_autograd_oracle (its recipe for the weights, its MFMA-forward
    configuration: 32x32, hidden 128, K = 2, L = 2, affine + invconv), the oracle run in fp64 on the FULL batch of 6: first the plain
    step of the full batch, then the accumulated one (k = 3), every tensor within 2e-4 max|g| + 1e-7 with no outlier allowance.
    Seed 21 was chosen on the oracle side: of seeds 5 .. 59 it keeps the fp64 ReLU pre-activations farthest from zero (min |h| =
    1.2e-6, an order above fp32 rounding of the O(1) activations), so no fp32 implementation takes another ReLU branch."""
    seed, batch, image, k = 21, 6, 32, 3
    cfg = O.default_cfg(image_shape=(image, image, 3), hidden_channels=128, K=2, L=2, batch=batch)
    np.random.seed(seed)
    glow = G.Glow(make_hps(batch, cfg=cfg))
    g = torch.Generator().manual_seed(seed)
    sd = {name: v.detach().clone() for name, v in glow.state_dict().items()}
    for name in sd:
        if name == "h_top":
            continue
        if name.endswith("invconv.weight"):
            c = sd[name].shape[0]
            sd[name] = torch.from_numpy(np.linalg.qr(np.random.randn(c, c))[0].astype("float32")) + 0.05 * torch.randn(c, c, generator=g)
        elif name.endswith("logs") or name.endswith("bias"):
            sd[name] = torch.randn(sd[name].shape, generator=g) * 0.1
        elif ".f.4." in name or "conv2d_zeros" in name:
            sd[name] = torch.randn(sd[name].shape, generator=g) * 0.02
        else:
            sd[name] = torch.randn(sd[name].shape, generator=g) * 0.05
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    x = torch.rand(batch, 3, image, image, generator=g)
    noise = torch.rand(batch, 3, image, image, generator=g) / 256
    with torch.enable_grad():
        leaf = {name: v.double().requires_grad_(name != "h_top") for name, v in sd.items()}
        _, nll, _ = O.glow_forward(x.double(), noise.double(), leaf, cfg)
        loss_ref = nll.mean()
        loss_ref.backward()
    ref = {name: v.grad for name, v in leaf.items() if v.grad is not None}

    def held(what):
        worst = ("", 0.0)
        for name, p in glow.named_parameters():
            if name == "h_top":
                continue
            r = ref[name]
            err = (p.grad.cpu().double() - r).abs().max().item()
            bound = 2e-4 * r.abs().max().item() + 1e-7
            worst = max(worst, (name, err / bound), key=lambda t: t[1])
            assert err <= bound, f"{what}: {name}: err {err:.3e} vs bound {bound:.3e}"
        print(f"{what}: worst {worst[0]} at {worst[1]:.3f} of its bound")

    loss = glow.loss_and_grads(x.to(DEV), noise=noise.to(DEV))
    assert abs(loss.item() - loss_ref.item()) < 1e-4
    held("plain step, batch 6")
    loss = glow.loss_and_grads(x.to(DEV), noise=noise.to(DEV), accumulate=k)
    assert abs(loss.item() - loss_ref.item()) < 1e-4
    held("accumulated step, 3 x 2")


def _count_accumulate_calls(monkeypatch):
    calls = []
    real = _plan.FlowPlan.accumulate_grads

    def counted(self, mode, scale=1.0):
        calls.append((int(mode), float(scale), self.family))
        return real(self, mode, scale)

    monkeypatch.setattr(_plan.FlowPlan, "accumulate_grads", counted)
    return calls


def test_off_is_off(monkeypatch):
    """accumulate_steps absent, 0 and 1: three loops, three steps, the same bits in loss, norm, parameters and optimiser state, and
    the plan's accumulate method never entered (no accumulator allocated)."""
    calls = _count_accumulate_calls(monkeypatch)
    batch = 8
    runs = []
    for optim in (dict(), dict(accumulate_steps=0), dict(accumulate_steps=1)):
        hps = make_hps(batch, **optim)
        loop = training.TrainLoop(fresh(hps), hps)
        outs = []
        for step in range(3):
            x, _, _ = batch_of(batch, seed=600 + step)
            torch.manual_seed(100 + step)
            loss, norm = loop.step(x)
            outs.append((loss.clone(), norm.clone()))
        loop.flush()
        plan = loop.glow.flow.plan_for(x)
        assert plan.grad_accumulators() is None and getattr(plan, "_gacc", None) is None
        runs.append((outs, {n: v.detach().cpu().clone() for n, v in loop.glow.state_dict().items()}, opt_state(loop)))
    assert calls == []
    for outs, params, state in runs[1:]:
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(outs, runs[0][0]))
        assert all(torch.equal(params[n], runs[0][1][n]) for n in params)
        assert all(torch.equal(state[i][n], runs[0][2][i][n]) for i in state for n in state[i])
    assert all(torch.isfinite(o[0]) and torch.isfinite(o[1]) for o in runs[0][0])


@pytest.mark.parametrize("ema", [False, True])
def test_captured_accumulating_step_equals_the_eager_one_bitwise(ema, monkeypatch):
    """The pattern of test_gpu_grad.py::test_graphed_training_step_equals_the_eager_step_bitwise with accumulate_steps = 2: batch 8,
    six steps under the noam schedule, one loop eager and one captured from step 3 on (the graph holds both micro-steps, the two
    combine launches and the update) -- loss, norm, parameters, optimiser state and the Polyak average the same bits."""
    calls = _count_accumulate_calls(monkeypatch)
    batch, steps = 8, 6
    hps = make_hps(batch, accumulate_steps=2, **(dict(ema_decay=0.9) if ema else {}))
    loops = [training.TrainLoop(fresh(hps, seed=37), hps, graph=False), training.TrainLoop(fresh(hps, seed=37), hps, graph=True)]
    assert [loop.accumulate for loop in loops] == [2, 2]
    for step in range(steps):
        x, _, _ = batch_of(batch, seed=3700 + step)
        outs = []
        for loop in loops:
            torch.manual_seed(200 + step)
            loss, norm = loop.step(x)
            outs.append((loss.clone(), norm.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (step, outs)
        assert torch.isfinite(outs[0][0]) and torch.isfinite(outs[0][1])
    for loop in loops:
        loop.flush()
    assert loops[1].graph_error is None, loops[1].graph_error
    assert loops[1]._graphed is not None and loops[1]._graphed.accumulate == 2 and loops[0]._graphed is None
    assert loops[1]._graphed.x.shape[0] == batch and loops[1]._graphed.valid()
    assert loops[0].optimizer._steps == loops[1].optimizer._steps == steps
    assert loops[0].global_step == loops[1].global_step == steps and loops[1].range_fallbacks == 0
    # eager: 2 launches per step; captured: 3 eager steps, then ONE capture that enqueues the two launches once for all replays
    half = float(np.float32(0.5))
    assert calls == [(AO.FIRST, 1.0, 0), (AO.FINISH, half, 0)] * (steps + 3 + 1)
    pa, pb = loops[0].glow.state_dict(), loops[1].glow.state_dict()
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    sa, sb = opt_state(loops[0]), opt_state(loops[1])
    assert sa.keys() == sb.keys() and len(sa) > 60
    for i in sa:
        assert set(sa[i]) == set(sb[i]) and ("ema" in sa[i]) == ema
        for name in sa[i]:
            assert torch.equal(sa[i][name], sb[i][name]), (i, name)
    if ema:
        assert loops[0].optimizer.ema_updates == loops[1].optimizer.ema_updates == steps


def test_overflow_in_the_second_micro_batch_skips_the_step_and_reruns_all_of_it(monkeypatch):
    """The model of test_gpu_grad.py::test_training_overflow_is_skipped_on_device_then_rerun_on_exact_fp32 with f.0's ActNorm scale
    raised by 300 (h1 ~ 3e2: inside the fp16 pairs' range for pixels in [0, 1]) and a batch whose SECOND micro-batch alone is scaled
    by 1 000 (h1 ~ 3e5: beyond the range, finite in fp32).  The accumulated norm is non-finite, the update is skipped on the device,
    and the deferred check re-runs BOTH micro-batches on the exact-fp32 family, on the plan and tape of the micro-batch."""
    calls = _count_accumulate_calls(monkeypatch)
    forwards = []
    real_forward = _plan.FlowPlan.glow_forward_train

    def logged(self, x, *a, **kw):
        forwards.append((x.shape[0], self.family))
        return real_forward(self, x, *a, **kw)

    monkeypatch.setattr(_plan.FlowPlan, "glow_forward_train", logged)
    torch.manual_seed(0)
    cfg = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=128, K=1, L=1, batch=4)
    sd = O.seeded_state_dict(cfg, seed=3, zeros_std=1e-3)
    k0, k2 = "flow.layers.1.f.0.actnorm.logs", "flow.layers.1.f.2.actnorm.logs"
    sd[k0] = sd[k0] + float(np.log(3e2)) / 3.0
    sd[k2] = sd[k2] - float(np.log(3e2)) / 3.0
    hps = make_hps(4, cfg=cfg, accumulate_steps=2)
    glow = G.Glow(hps)
    sd["h_top"] = torch.zeros_like(glow.h_top)
    glow.load_state_dict(sd)
    glow.set_actnorm_inited()
    glow = glow.to(DEV).train()
    x = torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(9))
    x[2:] *= 1000.0
    _, nll_ref, _ = O.glow_forward(x, torch.zeros_like(x), sd, cfg)
    assert torch.isfinite(nll_ref).all()                               # the fp32 reference handles the whole batch
    x = x.to(DEV)
    assert torch.isfinite(glow.loss_and_grads(x[:2]))                  # the first micro-batch alone is in range ...
    assert not torch.isfinite(glow.loss_and_grads(x[2:]))              # ... the second alone is not
    del forwards[:]
    loop = training.TrainLoop(glow, hps)
    before = {n: v.detach().clone() for n, v in glow.state_dict().items()}
    loss, gnorm = loop.step(x)
    assert not torch.isfinite(loss) and not torch.isfinite(gnorm), (loss, gnorm)
    after = glow.state_dict()
    assert all(torch.equal(before[n], after[n]) for n in before), "a skipped step must not touch the parameters"
    assert loop.range_fallbacks == 0 and forwards == [(2, 0), (2, 0)] and [c[0] for c in calls] == [AO.FIRST, AO.FINISH]
    loop.flush()
    assert loop.range_fallbacks == 1 and loop.diverged_steps == 0
    exact = _plan.FlowPlan.FAMILY_EXACT_FP32
    assert forwards == [(2, 0), (2, 0), (2, exact), (2, exact)], forwards            # k micro-steps again, micro-batch shape, exact fp32
    assert [(c[0], c[2]) for c in calls] == [(AO.FIRST, 0), (AO.FINISH, 0), (AO.FIRST, exact), (AO.FINISH, exact)]
    loss2, gnorm2 = loop.last_rerun
    assert torch.isfinite(loss2) and torch.isfinite(gnorm2)
    assert abs(loss2.item() - nll_ref.mean().item()) < 5e-2 * max(1.0, abs(nll_ref.mean().item()))
    after = glow.state_dict()
    assert any(not torch.equal(before[n], after[n]) for n in before if n != "h_top"), "the re-run applies the update"
    assert all(torch.isfinite(v).all() for v in after.values())
    assert glow.flow.plan_for(x).family == 0
    assert loop.optimizer._steps == 1 and loop.global_step == 1        # what a loop without the overflow would count


def test_accumulating_step_needs_less_memory_than_the_plain_step_of_the_batch():
    """Batch 16 as one step and as 4 x 4: after two warm-up steps the peak of allocated bytes over a step is lower with accumulation
    (the tape, the training workspace and the head buffers are a micro-batch's; the accumulators are one more copy of the gradients)."""
    batch = 16
    peaks, tapes = {}, {}
    for k in (1, 4):
        hps = make_hps(batch, **(dict(accumulate_steps=k) if k > 1 else {}))
        loop = training.TrainLoop(fresh(hps), hps)
        x, _, _ = batch_of(batch, seed=900)
        for _ in range(2):
            loop.step(x)
        loop.flush()
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, _ = loop.step(x)
        torch.cuda.synchronize()
        peaks[k] = (torch.cuda.max_memory_allocated(), base)
        assert torch.isfinite(loss)
        plan = loop.glow.flow.plan_for(x)
        tapes = {n: int(_lib.lib().glowhip_plan_tape_bytes(plan._h, n)) for n in (4, 16)}
        loop.flush()
        del loop, plan
        gc.collect()
        torch.cuda.empty_cache()
    print(f"peak allocated bytes over one step at batch 16: plain {peaks[1][0]} (resident before the step {peaks[1][1]}), "
          f"4 x 4 {peaks[4][0]} (resident {peaks[4][1]}); glowhip_plan_tape_bytes: batch 4 {tapes[4]}, batch 16 {tapes[16]}")
    assert tapes[4] < tapes[16]
    assert peaks[4][0] < peaks[1][0], peaks


def test_exchange_sees_final_gradients_once_per_optimiser_step(monkeypatch):
    """`parallel.allreduce_buckets` replaced by a recorder: one call per optimiser step, every bucket with the ONE event recorded
    behind the last combine, and after that event the bucket contents are the final .grad values."""
    n, k = 8, 4
    hps = make_hps(n)
    glow = fresh(hps)
    opt = training.build_optimizer(hps, glow.parameters())
    seen = []

    def recorder(buckets, world=None, average=True):
        events = {id(ev) for _, ev in buckets}
        for _, ev in buckets:
            ev.synchronize()
        seen.append((len(buckets), events, [flat.clone() for flat, _ in buckets], [flat.data_ptr() for flat, _ in buckets]))

    monkeypatch.setattr(parallel, "allreduce_buckets", recorder)
    x, _, _ = batch_of(n, seed=950)
    for step in range(2):
        torch.manual_seed(40 + step)
        loss, norm = parallel.train_step(glow, opt, x, world=1, accumulate=k)       # (no clipping: the update leaves the gradients alone)
        assert torch.isfinite(loss) and torch.isfinite(norm)
        assert len(seen) == step + 1
    plan = glow.flow.plan_for(x)
    flats, grads = plan._pgrad[0], plan._pgrad[1]
    count, events, copies, ptrs = seen[-1]
    assert count == len(flats) == glow.flow.L + 1 and len(events) == 1
    assert sorted(ptrs) == sorted(f.data_ptr() for f in flats)
    by_ptr = dict(zip(ptrs, copies))
    params = plan.trainable_parameters()
    assert len(params) == len(grads) > 60
    for p, gview in zip(params, grads):
        assert p.grad is gview
        flat = next(f for f in flats if f.data_ptr() <= gview.data_ptr() < f.data_ptr() + 4 * f.numel())
        off = (gview.data_ptr() - flat.data_ptr()) // 4
        assert same_tensor(by_ptr[flat.data_ptr()][off:off + gview.numel()].view_as(gview), p.grad)
    assert glow.flow.pop_grad_buckets() is None                         # handed over once


def test_refusals():
    n = 8
    hps = make_hps(n, accumulate_steps=2, ema_decay=0.9)
    glow = fresh(hps)
    x, noise, _ = batch_of(n, seed=960)
    with pytest.raises(ValueError, match="8 % 3"):
        glow.loss_and_grads(x, noise=noise, accumulate=3)
    with pytest.raises(ValueError):
        glow.loss_and_grads(x, noise=noise, accumulate=0)
    opt = training.build_optimizer(hps, glow.parameters())
    with pytest.raises(ValueError, match="direct route"):
        parallel.train_step(glow, opt, x, accumulate=2, direct=False)
    with pytest.raises(ValueError, match="direct route"):
        parallel.train_step(glow, torch.optim.Adam(glow.parameters(), lr=1e-4), x, accumulate=2)
    # an uninitialised ActNorm: the data-dependent init belongs to the full batch, not to a micro-batch
    cold = fresh(hps)
    cold.set_actnorm_inited(False)
    with pytest.raises(_lib.GlowHipError, match="not initialised"):
        cold.loss_and_grads(x, noise=noise, accumulate=2)
    assert not cold.actnorm_inited()
    # a training step under swapped averaged weights raised before and still raises
    loop = training.TrainLoop(glow, hps, optimizer=opt)
    loop.step(x)
    loop.flush()
    steps = opt._steps
    with training.averaged_weights(opt):
        with pytest.raises(_lib.GlowHipError, match="swapped"):
            loop.step(x)
        with pytest.raises(_lib.GlowHipError, match="swapped"):
            parallel.train_step(glow, opt, x, accumulate=2)
    assert opt._steps == steps and loop.global_step == 1
    loss, norm = loop.step(x)
    loop.flush()
    assert torch.isfinite(loss) and torch.isfinite(norm) and opt._steps == steps + 1
