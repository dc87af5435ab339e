"""world_size=2 gloo tests (CPU) of the N>1 path: sharding, step-0 init + flat parameter broadcast, scalar loss
all-reduce, nll gather.  The per-rank compute is injected (CPU oracle) because the HIP path needs a GPU; what is
under test is the exchange logic of pytorch-glow_amd/parallel.py."""
import os

import numpy as np
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pytorch_glow_amd as G
from pytorch_glow_amd import parallel
from pytorch_glow_amd.misc import util
from oracle import glow_oracle as O

CFG = O.default_cfg(image_shape=(16, 16, 3), hidden_channels=16, K=2, L=2, batch=2)


def tiny_glow():
    hps = util.AttrDict(dict(
        model=dict(image_shape=[16, 16, 3], hidden_channels=16, K=2, L=2, actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False, flow_permutation="invconv",
                      flow_coupling="affine"),
        optim=dict(num_batch_train=2), dataset=dict(num_classes=1), device=dict(graph=["cpu"])))
    return G.Glow(hps)


def oracle_init(glow, x):
    sd = {k: v.detach().clone() for k, v in glow.state_dict().items()}
    with torch.no_grad():
        post = O.glow_init_actnorm(x, torch.zeros_like(x), sd, CFG)
    glow.load_state_dict(post)


def worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)            # ranks start with DIFFERENT weights
        import numpy as np
        np.random.seed(100 + rank)
        glow = tiny_glow()
        xg = torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(0))   # same global batch everywhere
        x = parallel.shard_batch(xg, world, rank)
        assert x.shape[0] == 2 and torch.equal(x, xg[2 * rank:2 * rank + 2])
        parallel.data_dependent_init(glow, x, rank, world, init_fn=oracle_init)
        assert all(m.bias_inited for m in glow.modules() if isinstance(m, G.ActNorm))
        sd = {k: v.detach().clone() for k, v in glow.state_dict().items()}
        with torch.no_grad():
            _, nll, _ = O.glow_forward(x, torch.zeros_like(x), sd, CFG)
        total = parallel.reduce_loss(nll.clone(), world)
        allnll = parallel.gather_nll(nll, world)
        ret[rank] = dict(sd=sd, nll=nll, total=total, allnll=allnll)
    finally:
        dist.destroy_process_group()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_shard_bounds():
    assert parallel.shard_bounds(512, 8, 3) == (192, 256)
    assert parallel.shard_bounds(64, 1, 0) == (0, 64)
    with pytest.raises(AssertionError):
        parallel.shard_bounds(50, 8, 0)


@pytest.mark.timeout(300)
def test_world2_init_broadcast_and_loss_allreduce():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(worker, args=(world, free_port(), ret), nprocs=world, join=True)
    r0, r1 = ret[0], ret[1]
    # (1) after the step-0 exchange both ranks hold rank 0's parameters, ActNorm statistics included
    for k in r0["sd"]:
        assert torch.equal(r0["sd"][k], r1["sd"][k]), k
    # ... and those statistics come from rank 0's shard only (reference trainer.py:112-115)
    xg = torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(0))
    torch.manual_seed(100)
    import numpy as np
    np.random.seed(100)
    ref = tiny_glow()
    oracle_init(ref, xg[:2])
    for k, v in ref.state_dict().items():
        assert torch.allclose(v, r0["sd"][k], atol=1e-6), k
    # (2) the all-reduced loss equals the single-process loss over the global batch
    with torch.no_grad():
        sd4 = dict(r0["sd"], h_top=torch.zeros(4, *r0["sd"]["h_top"].shape[1:]))
        _, nll_all, _ = O.glow_forward(xg, torch.zeros_like(xg), sd4, dict(CFG, batch=4))
    assert torch.allclose(r0["total"], nll_all.sum(), atol=1e-4) and torch.equal(r0["total"], r1["total"])
    # (3) gathered per-sample nll is in rank order
    assert torch.allclose(r0["allnll"], nll_all, atol=1e-5) and torch.equal(r0["allnll"], r1["allnll"])
    assert torch.allclose(r0["nll"], nll_all[:2], atol=1e-5) and torch.allclose(r1["nll"], nll_all[2:], atol=1e-5)


def grad_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(7)
        m = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
        m[1].bias.requires_grad_(False)                      # a parameter without gradient (like h_top)
        xg = torch.arange(40, dtype=torch.float32).reshape(8, 5) / 10
        x = parallel.shard_batch(xg, world, rank)
        with torch.enable_grad():
            m(x).pow(2).mean().backward()                    # local mean over the shard
        parallel.allreduce_gradients(m, world)               # -> gradient of the GLOBAL mean
        ret[rank] = [None if p.grad is None else p.grad.clone() for p in m.parameters()]
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_gradient_allreduce_equals_global_batch_gradient():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(grad_worker, args=(world, free_port(), ret), nprocs=world, join=True)
    torch.manual_seed(7)
    m = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    m[1].bias.requires_grad_(False)
    xg = torch.arange(40, dtype=torch.float32).reshape(8, 5) / 10
    with torch.enable_grad():
        m(xg).pow(2).mean().backward()
    for r in (0, 1):
        for got, p in zip(ret[r], m.parameters()):
            if p.grad is None:
                assert got is None
            else:
                assert torch.allclose(got, p.grad, atol=1e-6)


class _StubFlow:
    output_shapes = [[-1, 2, 2, 2]]


class _StubGraph(torch.nn.Module):
    """CPU stand-in for Glow in the Inferer's data-parallel bookkeeping test: z = a fixed linear image of x."""
    def __init__(self):
        super().__init__()
        self.h_top = torch.nn.Parameter(torch.zeros(2, 4, 2, 2), requires_grad=False)
        self.flow = _StubFlow()

    def forward(self, x=None, **kw):
        return x[:, :2, :2, :2] * 2.0 + 1.0, None, None


def inferer_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorch_glow_amd.network import Inferer
        from pytorch_glow_amd.misc import util
        hps = util.AttrDict(dict(dataset=dict(num_classes=3, num_workers=0), ablation=dict(y_condition=False)))
        g = torch.Generator().manual_seed(3)
        xs = torch.rand(8, 3, 4, 4, generator=g); ys = (torch.rand(8, 3, generator=g) > 0.5).float()
        mine = list(range(rank * 4, rank * 4 + 4))                  # each rank sees its half of the data set
        data = [{"x": xs[i], "y_onehot": ys[i]} for i in mine]
        inf = Inferer(hps, _StubGraph(), devices=["cpu"], data_device="cpu")
        ret[rank] = inf.compute_attribute_delta(data, shuffle=False, world=world)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_attribute_delta_equals_single_process():
    """Ranks accumulate over different batches; one all-reduce of sums and counts at the end gives every rank the deltaz of
    the whole data set (checked against the oracle's restatement)."""
    from oracle import glow_oracle as O
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(inferer_worker, args=(world, free_port(), ret), nprocs=world, join=True)
    g = torch.Generator().manual_seed(3)
    xs = torch.rand(8, 3, 4, 4, generator=g); ys = (torch.rand(8, 3, generator=g) > 0.5).float()
    zs = (xs[:, :2, :2, :2] * 2.0 + 1.0).numpy()
    want = O.attribute_delta(zs, ys.numpy(), batch_size=2)
    for r in (0, 1):
        assert np.abs(ret[r] - want).max() < 1e-6


def test_bench_launches_its_own_ranks_dry_run():
    """`python bench.py --gpus 2` with no launcher around it spawns its two ranks itself (before touching any GPU), the ranks
    rendezvous on 127.0.0.1, run the timed-loop protocol (warm-up, barrier, K steps, barrier, MAX over ranks) and rank 0
    prints ONE JSON line carrying n_gpus = 2 and the observed world size.  --dry-run-cpu swaps RCCL for gloo and the step
    for an empty one, so the launcher and the collective sequence are exercised where there is no GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-run-cpu", "--full", "--steps", "3",
                          "--warmup", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_world_size"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["allreduce_check"] == 3.0     # 1 + 2: both ranks took part in the step's collective
    # the N-rank line's diagnostics: per-rank step times gathered in rank order (the dry run adds the rank to each so
    # the order shows), their min / max, and the timed flat all-reduce -- the same parallel.* helpers the RCCL run calls
    mr = rec["multi_rank"]
    assert mr["world"] == 2 and mr["backend"] == "gloo" and len(mr["per_rank_device_ms_per_step"]) == 2
    assert mr["per_rank_device_ms_per_step"][1] > mr["per_rank_device_ms_per_step"][0] + 0.5
    assert mr["ms_per_step_rank_min"] == min(mr["per_rank_device_ms_per_step"]) and mr["ms_per_step_rank_max"] == max(mr["per_rank_device_ms_per_step"])
    ar = mr["gradient_allreduce_flat"]
    assert ar["bytes"] == 4 << 16 and ar["world"] == 2 and ar["allreduce_ms"] > 0 and ar["busbw_GBps"] == pytest.approx(ar["algbw_GBps"], rel=0.05)
    # a failing rank takes the job down with a non-zero exit code instead of hanging the others
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=dict(env, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert bad.returncode != 0


def test_bench_eight_rank_launch_dry_run():
    """The launch the driver's 8-GPU tier makes -- `bench.py --gpus 8`: eight children spawned before anything touches a GPU, one
    rendezvous on 127.0.0.1, the timed-loop protocol, ONE JSON line with n_gpus = 8 and all eight ranks in the step's collective
    (sum of rank + 1 over 8 ranks = 36) -- exercised on gloo where there is no GPU (VERDICT r3 #6b)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-run-cpu", "--steps", "2",
                          "--warmup", "1"], capture_output=True, text=True, timeout=600, env=dict(env, OMP_NUM_THREADS="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["rccl_world_size"] == 8 and rec["allreduce_check"] == 36.0 and rec["scaling"] == "weak"


def bucket_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(11)
        m = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.Linear(8, 4), torch.nn.Linear(4, 2))
        xg = torch.arange(48, dtype=torch.float32).reshape(8, 6) / 7
        x = parallel.shard_batch(xg, world, rank)
        with torch.enable_grad():
            m(x).pow(2).mean().backward()
        # the layout FlowPlan.glow_backward uses: gradients are VIEWS into flat buckets (weights per "level", small ones last,
        # 64-element aligned slots), handed over in the order the sweep finishes them
        params = list(m.parameters())
        groups = [[params[4]], [params[2]], [params[0]], [params[1], params[3], params[5]]]
        buckets = []
        for grp in groups:
            sizes = [(p.numel() + 63) // 64 * 64 for p in grp]
            flat = torch.full((sum(sizes),), float(rank + 1))            # (padding holds junk: it must not leak anywhere)
            off = 0
            for p, n in zip(grp, sizes):
                flat[off:off + p.numel()] = p.grad.reshape(-1)
                p.grad = flat[off:off + p.numel()].view_as(p)
                off += n
            buckets.append((flat, None))
        ref = [p.grad.clone() for p in params]
        parallel.allreduce_buckets(buckets, world)                        # in place, bucket by bucket
        got = [p.grad.clone() for p in params]
        for p, g0 in zip(params, ref):                                    # the one-flat-buffer path on the same local gradients
            p.grad = g0
        parallel.allreduce_gradients(m, world)
        ret[rank] = (got, [p.grad.clone() for p in params])
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_bucketed_allreduce_equals_flat_allreduce():
    """VERDICT r2 #4a: the per-level gradient buckets (all-reduced one by one as the backward sweep leaves each level) give the
    same averaged gradients as the single flat all-reduce, and both equal the global-batch gradient."""
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(bucket_worker, args=(world, free_port(), ret), nprocs=world, join=True)
    torch.manual_seed(11)
    m = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.Linear(8, 4), torch.nn.Linear(4, 2))
    xg = torch.arange(48, dtype=torch.float32).reshape(8, 6) / 7
    with torch.enable_grad():
        m(xg).pow(2).mean().backward()
    for r in (0, 1):
        bucketed, flat = ret[r]
        for b, f, p in zip(bucketed, flat, m.parameters()):
            assert torch.equal(b, f)
            assert torch.allclose(b, p.grad, atol=1e-6)


def _sampler_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorch_glow_amd.network.trainer import _ShardSampler
        torch.manual_seed(1234 + 77 * rank)      # ranks of an unseeded run draw DIFFERENT torch seeds
        s = _ShardSampler(list(range(40)), global_batch=8, rank=rank, world=world, seed=None)
        ret[rank] = dict(seed=s.seed, epoch0=list(iter(s)), epoch1=list(iter(s)))
    finally:
        dist.destroy_process_group()


def test_world2_unseeded_sampler_agrees_on_rank0s_seed():
    """without a profile seed every rank used its own torch.initial_seed(), the per-epoch permutations
    differed and the 'positions [r*per, (r+1)*per) of the same global batch' sharding overlapped / omitted samples.  Now rank 0's
    draw is broadcast: equal seeds, disjoint shards that together are each epoch's 40 // 8 global batches."""
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_sampler_worker, args=(2, free_port(), ret), nprocs=2, join=True)
    a, b = ret[0], ret[1]
    assert a["seed"] == b["seed"] == (1234 % (2 ** 31))
    for ep in ("epoch0", "epoch1"):
        assert len(a[ep]) == len(b[ep]) == 20 and not (set(a[ep]) & set(b[ep])) and len(set(a[ep]) | set(b[ep])) == 40
    assert a["epoch0"] != a["epoch1"]
