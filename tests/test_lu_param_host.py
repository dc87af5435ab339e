"""Host checks (no GPU) of the LU-parameterised invertible 1x1 convolution: the module surface (`Invertible1x1ConvLU`, the
state-dict helper, `Glow(hps)` with ``lu_decomposition=True``), the yardstick of the GPU tests (tests/plu_oracle.py) and the
data-parallel step-0 exchange of the modules' buffers.  The reference has no implementation to compare with: it raises at
network/module.py:336-337."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pytorch_glow_amd as G
from pytorch_glow_amd import parallel
from pytorch_glow_amd.misc import util
import lu_oracle as LU
import plu_oracle as PLU

U24 = 2.0 ** -24


def lu_hps(lu=True, device="cpu", **abl):
    a = dict(learn_top=False, y_condition=False, lu_decomposition=lu, flow_permutation="invconv", flow_coupling="affine")
    a.update(abl)
    return util.AttrDict(dict(
        model=dict(image_shape=[16, 16, 3], hidden_channels=16, K=2, L=2, actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=a, optim=dict(num_batch_train=2), dataset=dict(num_classes=1), device=dict(graph=[device])))


def module_factors(m):
    f = {n: getattr(m, n).detach().numpy() for n in PLU.NAMES}
    return f


def factor_rounding_bound(f):
    """(C + 2) 2^-24 (|L||U_f|): the fp32 rounding of the factors (one per entry of L and U_f, C terms per product)."""
    return (f["l"].shape[0] + 2) * U24 * PLU.abs_product(f)


def test_state_dict_keys_shapes_and_kinds():
    C = 12
    m = G.Invertible1x1ConvLU(C)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(p=(C, C), sign_s=(C,), l=(C, C), u=(C, C), log_s=(C,))
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert sorted(n for n, _ in m.named_parameters()) == ["l", "log_s", "u"]
    assert sorted(n for n, _ in m.named_buffers()) == ["p", "sign_s"]
    p = sd["p"].numpy()
    assert ((p == 0) | (p == 1)).all() and (p.sum(0) == 1).all() and (p.sum(1) == 1).all()
    assert set(np.unique(sd["sign_s"].numpy())) <= {-1.0, 1.0}
    assert not torch.triu(sd["l"]).any() and not torch.tril(sd["u"]).any()
    assert G.network.Invertible1x1ConvLU is G.Invertible1x1ConvLU


@pytest.mark.parametrize("C", [2, 12, 48, 96])
def test_initialisation_is_the_dense_draw(C):
    np.random.seed(11 + C)
    dense = G.Invertible1x1Conv(C)
    after_dense = np.random.get_state()
    np.random.seed(11 + C)
    draw = np.linalg.qr(np.random.randn(C, C))[0]
    np.random.seed(11 + C)
    m = G.Invertible1x1ConvLU(C)
    after_lu = np.random.get_state()
    assert after_dense[0] == after_lu[0] and np.array_equal(after_dense[1], after_lu[1]) and after_dense[2:] == after_lu[2:]
    f = module_factors(m)
    bound = factor_rounding_bound(f)
    assert (np.abs(PLU.assemble(f) - draw) <= bound).all()
    # the read-only dense view: the same matrix, rounded to fp32 once more
    w = m.weight
    assert w.dtype == torch.float32 and not w.requires_grad
    assert (np.abs(w.numpy().astype(np.float64) - draw) <= bound + U24 * np.abs(draw)).all()
    assert np.array_equal(dense.weight.detach().numpy(), draw.astype(np.float32))
    with pytest.raises(AttributeError):
        m.weight = w


def test_dense_constructor_still_raises_and_names_the_class():
    with pytest.raises(NotImplementedError, match="Invertible1x1ConvLU"):
        G.Invertible1x1Conv(4, lu_decomposition=True)


@pytest.mark.parametrize("family", LU.ALL)
def test_from_weight_factors_a_given_matrix(family):
    W = LU.matrix(family, 24)
    m = G.Invertible1x1ConvLU.from_weight(torch.from_numpy(np.array(W)))
    f = module_factors(m)
    assert (np.abs(PLU.assemble(f) - W.astype(np.float64)) <= factor_rounding_bound(f)).all()
    g = PLU.params(family, 24)
    assert all(np.array_equal(f[n], g[n]) for n in PLU.NAMES)      # the oracle's factorisation is the module's


def test_snapshot_helper_loads_a_dense_state_dict_strictly():
    np.random.seed(3)
    torch.manual_seed(3)
    dense = G.Glow(lu_hps(lu=False))
    sd = {k: v.detach().clone() for k, v in dense.state_dict().items()}
    for k in sd:
        if k.endswith("invconv.weight"):
            sd[k] = sd[k] + 0.05 * torch.randn_like(sd[k])
    conv = util.lu_state_dict_from_dense(sd)
    assert not any(k.endswith("invconv.weight") for k in conv) and all(k in conv for k in sd if not k.endswith("invconv.weight"))
    lu = G.Glow(lu_hps())
    lu.load_state_dict(conv, strict=True)
    n = 0
    for name, mod in lu.named_modules():
        if isinstance(mod, G.Invertible1x1ConvLU):
            f = module_factors(mod)
            W = sd[name + ".weight"].numpy().astype(np.float64)
            assert (np.abs(PLU.assemble(f) - W) <= factor_rounding_bound(f)).all(), name
            n += 1
    assert n == 4
    for k, v in lu.state_dict().items():
        if ".invconv." not in k:
            assert torch.equal(v, sd[k]), k


def test_glow_builds_with_lu_decomposition_and_has_no_dense_weight():
    glow = G.Glow(lu_hps())
    names = [n for n, _ in glow.named_parameters()]
    assert not any(n.endswith("invconv.weight") for n in names)
    steps = [l for l in glow.flow.layers if isinstance(l, G.FlowStep)]
    assert len(steps) == 4 and all(isinstance(s.invconv, G.Invertible1x1ConvLU) for s in steps)
    assert sum(n.endswith("invconv.log_s") for n in names) == 4
    # other permutations ignore the flag
    rev = G.Glow(lu_hps(flow_permutation="reverse"))
    assert not any(".invconv." in n for n, _ in rev.named_parameters())
    assert isinstance(G.FlowStep(12, 16, lu_decomposition=False).invconv, G.Invertible1x1Conv)


CASES = sorted(set(PLU.standalone_cases()) | set(PLU.plan_cases()))


@pytest.mark.parametrize("family,C", CASES, ids=[f"{f}-{C}" for f, C in CASES])
def test_oracle_conditioning(family, C):
    """The yardstick of the GPU tests: the two fp64 inverse routes agree, and sum(log_s) agrees with slogdet of the assembled
    matrix, to 1e-2 of the bounds the kernels are held to."""
    r_inv, r_ld = PLU.conditioning_ratios(PLU.params(family, C))
    print(f"PLU-ORACLE {family}-{C} inverse {r_inv:.2e} logdet {r_ld:.2e}")
    assert r_inv <= 1e-2 and r_ld <= 1e-2, (family, C, r_inv, r_ld)


def test_oracle_backward_matches_autograd():
    """plu_oracle.backward (closed form) against torch autograd through the assembled matrix, fp64."""
    f = PLU.params("orth", 12)
    rs = np.random.RandomState(0)
    dW = rs.randn(12, 12)
    dl, du, ds, *_ = PLU.backward(f, dW, 0.75)
    with torch.enable_grad():
        leaf = {n: torch.from_numpy(np.array(f[n], dtype=np.float64)).requires_grad_(n in ("l", "u", "log_s")) for n in PLU.NAMES}
        W = PLU.dense_state_dict({"a.invconv." + n: v for n, v in leaf.items()})["a.invconv.weight"]
        ((W * torch.from_numpy(dW)).sum() + 0.75 * leaf["log_s"].sum()).backward()
    assert np.allclose(leaf["l"].grad.numpy(), dl, atol=1e-12) and np.allclose(leaf["u"].grad.numpy(), du, atol=1e-12)
    assert np.allclose(leaf["log_s"].grad.numpy(), ds, atol=1e-12)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)
        np.random.seed(100 + rank)               # ranks draw DIFFERENT matrices, permutations and signs
        glow = G.Glow(lu_hps())
        before = {k: v.detach().clone() for k, v in glow.state_dict().items()}
        x = torch.rand(2, 3, 16, 16)
        parallel.data_dependent_init(glow, x, rank, world, init_fn=lambda g, xx: g.set_actnorm_inited())
        ret[rank] = dict(before=before, after={k: v.detach().clone() for k, v in glow.state_dict().items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_step0_init_sends_the_lu_buffers():
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_init_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    r0, r1 = ret[0], ret[1]
    differed = False
    for k in r0["after"]:
        assert torch.equal(r0["after"][k], r1["after"][k]), k
        assert torch.equal(r0["after"][k], r0["before"][k]), k          # rank 0's values, untouched
        if k.endswith("invconv.p") or k.endswith("invconv.sign_s"):
            differed = differed or not torch.equal(r0["before"][k], r1["before"][k])
    assert differed, "the two ranks drew the same permutations and signs: the test shows nothing"


def _flat_sent_by_broadcast(module, monkeypatch):
    sent = []
    monkeypatch.setattr(dist, "broadcast", lambda t, src=0: sent.append(t.clone()))
    parallel.broadcast_parameters(module, src=0, world=2)
    assert len(sent) == 1
    return sent[0]


def test_broadcast_of_a_model_without_lu_modules_is_the_parameter_list(monkeypatch):
    """No LU module: the ONE flat tensor broadcast_parameters sends is cat(parameters()), as it always was."""
    glow = G.Glow(lu_hps(lu=False))
    flat = _flat_sent_by_broadcast(glow, monkeypatch)
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in glow.parameters()]))


def test_broadcast_of_an_lu_model_appends_the_buffers(monkeypatch):
    glow = G.Glow(lu_hps())
    flat = _flat_sent_by_broadcast(glow, monkeypatch)
    params = [p.detach().reshape(-1) for p in glow.parameters()]
    bufs = [b.reshape(-1) for m in glow.modules() if isinstance(m, G.Invertible1x1ConvLU) for b in (m.p, m.sign_s)]
    assert len(bufs) == 8 and torch.equal(flat, torch.cat(params + bufs))


def test_plu_factors_refuses_a_singular_matrix():
    with pytest.raises(ValueError, match="singular"):
        G.Invertible1x1ConvLU.from_weight(torch.ones(3, 3))
