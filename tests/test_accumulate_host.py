"""Gradient accumulation, everything that needs no GPU: the one definition of the micro-batch cut, the numpy oracle held to fp64,
the profile key ``hps.optim.accumulate_steps``, and the refusals of glowhip_grad_accumulate that come before any device call.
The kernel and the model are held to tests/accumulate_oracle.py by test_gpu_accumulate.py / test_gpu_accumulate_model.py."""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib, parallel, training
from pytorch_glow_amd.misc import util

import accumulate_oracle as AO


def test_micro_slices_cover_the_batch_exactly():
    assert training.micro_slices is parallel.micro_slices          # ONE definition
    for n in range(2, 65):
        for k in range(1, n + 1):
            if n % k:
                with pytest.raises(ValueError, match=f"{n} % {k}"):
                    training.micro_slices(n, k)
                continue
            cuts = training.micro_slices(n, k)
            assert len(cuts) == k and cuts[0][0] == 0 and cuts[-1][1] == n
            assert all(hi - lo == n // k for lo, hi in cuts)
            assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            training.micro_slices(8, bad)


@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_oracle_composition_is_the_fp64_mean_to_k_roundings(k):
    """k - 1 fp32 adds, one fp32 multiply by float32(1 / k): each rounds by at most 2^-24 relative to a partial sum that is at most
    sum |g_i|, so |composition - mean| <= ((k - 1) + 2) 2^-24 sum|g| / k (+ second order) -- below k 2^-24 sum|g| for every k >= 2."""
    rng = np.random.default_rng(100 + k)
    n = 20000
    mags = 10.0 ** rng.uniform(-6, 3, size=(k, n))
    grads = (mags * rng.choice([-1.0, 1.0], size=(k, n))).astype(np.float32)
    got = AO.compose(list(grads))
    assert got.dtype == np.float32
    mean = grads.astype(np.float64).sum(0) / k
    bound = k * 2.0 ** -24 * np.abs(grads.astype(np.float64)).sum(0)
    err = np.abs(got.astype(np.float64) - mean)
    assert (err <= bound).all(), (err / bound).max()
    # the modes compose as their definitions say
    g, a = AO.first(grads[0])
    assert AO.same_bits(a, grads[0]) and AO.same_bits(g, grads[0])
    g, a2 = AO.add(grads[1], a)
    assert AO.same_bits(a2, grads[0] + grads[1]) and AO.same_bits(g, grads[1])
    g, a3 = AO.finish(grads[1], a, 0.5)
    assert AO.same_bits(a3, a) and AO.same_bits(g, (grads[0] + grads[1]) * np.float32(0.5))
    assert AO.modes(k) == [AO.FIRST] + [AO.ADD] * (k - 2) + [AO.FINISH]
    assert (AO.FIRST, AO.ADD, AO.FINISH) == (_lib.ACC_FIRST, _lib.ACC_ADD, _lib.ACC_FINISH)


def test_oracle_comparison_sees_signed_zeros_and_nan_positions():
    a = np.array([0.0, 1.0, np.nan, np.inf], dtype=np.float32)
    assert AO.same_bits(a, a.copy())
    assert not AO.same_bits(a, np.array([-0.0, 1.0, np.nan, np.inf], dtype=np.float32))
    assert not AO.same_bits(a, np.array([0.0, np.nan, np.nan, np.inf], dtype=np.float32))
    assert not AO.same_bits(a, np.array([0.0, 1.0, np.nan, -np.inf], dtype=np.float32))
    other = a.copy()
    other.view(np.int32)[2] = -0x400000           # 0xffc00000: another NaN at the same place
    assert AO.same_bits(a, other)


def _hps(**optim):
    return util.AttrDict(dict(
        model=dict(image_shape=[16, 16, 3], hidden_channels=32, K=1, L=2, actnorm_scale=1.0, n_bits_x=8, weight_y=0.0),
        ablation=dict(learn_top=False, y_condition=False, lu_decomposition=False, flow_permutation="invconv", flow_coupling="affine"),
        optim=dict(num_batch_train=16, optimizer="adam", optimizer_args=dict(lr=1e-3, betas=[0.9, 0.999], eps=1e-8),
                   lr_scheduler="noam", lr_scheduler_args=dict(warmup_steps=5, min_lr=1e-5), **optim),
        dataset=dict(num_classes=1, num_workers=0), device=dict(graph=["cpu"], data=["cpu"])))


def test_profile_key_is_accepted_and_validated():
    for name in ("celeba", "test"):
        assert "accumulate_steps" not in util.load_profile(name).optim      # beyond the reference's schema: its profiles have none
    assert util.accumulate_steps(_hps()) == 1
    assert util.accumulate_steps(_hps(accumulate_steps=None)) == 1
    assert util.accumulate_steps(_hps(accumulate_steps=0)) == 1
    assert util.accumulate_steps(_hps(accumulate_steps=1)) == 1
    assert util.accumulate_steps(_hps(accumulate_steps=4)) == 4
    assert util.accumulate_steps(_hps(accumulate_steps=4), world=2) == 4      # 16 = 2 * 4 * 2
    assert util.accumulate_steps(_hps(accumulate_steps=0), world=16) == 1
    with pytest.raises(ValueError, match=r"num_batch_train = 16 .* 2 \* 16 = 32"):
        util.accumulate_steps(_hps(accumulate_steps=16), world=2)
    with pytest.raises(ValueError, match=r"num_batch_train = 16 .* 1 \* 3 = 3"):
        util.accumulate_steps(_hps(accumulate_steps=3), world=1)
    for bad in (-1, 2.0, "4", True):
        with pytest.raises(ValueError, match="accumulate_steps"):
            util.accumulate_steps(_hps(accumulate_steps=bad))


def test_train_loop_and_trainer_read_the_key():
    from pytorch_glow_amd.network import Trainer
    for optim, want in ((dict(), 1), (dict(accumulate_steps=0), 1), (dict(accumulate_steps=1), 1), (dict(accumulate_steps=4), 4)):
        hps = _hps(**optim)
        loop = training.TrainLoop(G.Glow(hps), hps)
        assert loop.accumulate == want
        assert loop._accumulate_kw() == (dict(accumulate=want) if want > 1 else {})       # off: the step is called as it always was
    hps = _hps(accumulate_steps=3)
    with pytest.raises(ValueError, match=r"num_batch_train = 16 .* 1 \* 3 = 3"):
        Trainer(hps, result_subdir=".", step=0, graph=None, optimizer=None, scheduler=None, devices=["cpu"], dataset=None,
                data_device="cpu")
    hps = _hps(accumulate_steps=4)
    with pytest.raises(ValueError, match=r"num_batch_train = 16 .* 8 \* 4 = 32"):
        Trainer(hps, result_subdir=".", step=0, graph=None, optimizer=None, scheduler=None, devices=["cpu"], dataset=None,
                data_device="cpu", rank=0, world=8)


def test_train_step_refuses_accumulation_off_the_direct_route():
    hps = _hps()
    glow = G.Glow(hps)
    opt = training.build_optimizer(hps, glow.parameters())
    x = torch.rand(4, 3, 16, 16)                                       # a host batch is not the direct route
    with pytest.raises(ValueError, match="direct route"):
        parallel.train_step(glow, opt, x, accumulate=2)
    with pytest.raises(ValueError, match="direct route"):
        parallel.train_step(glow, opt, x, accumulate=2, direct=False)


def _segs(entries):
    return (_lib.GradSeg * max(len(entries), 1))(*[_lib.GradSeg(g, a, n) for g, a, n in entries])


def test_grad_accumulate_refusals_need_no_device():
    """Every refusal comes before any device call: the pointers here are made-up addresses that nothing ever reads."""
    lib = G.lib()
    err = lambda: lib.glowhip_last_error().decode()
    call = lambda entries, n, mode, scale: lib.glowhip_grad_accumulate(_segs(entries), n, mode, scale, None)
    good = (0x10000, 0x20000, 8)
    assert ctypes.sizeof(_lib.GradSeg) == 24
    assert call([], 0, _lib.ACC_ADD, 1.0) == 0                                    # n_segs = 0: OK, no launch
    assert lib.glowhip_grad_accumulate(None, 0, _lib.ACC_FIRST, 0.0, None) == 0
    assert call([(0, 0, 0), (0x10000, 0, 0)], 2, _lib.ACC_ADD, 1.0) == 0         # nothing but empty segments: OK, no launch
    assert call([good] * 17, 17, _lib.ACC_ADD, 1.0) == -1 and "n_segs 17" in err()
    assert call([good], -1, _lib.ACC_ADD, 1.0) == -1 and "n_segs -1" in err()
    assert call([good, (0x10000, 0x20000, -5)], 2, _lib.ACC_ADD, 1.0) == -1 and "n = -5" in err()
    assert call([(0, 0x20000, 4)], 1, _lib.ACC_FIRST, 1.0) == -1 and "null pointer" in err()
    assert call([good, (0x10000, 0, 4)], 2, _lib.ACC_FINISH, 1.0) == -1 and "null pointer" in err()
    assert call([(0x10002, 0x20000, 4)], 1, _lib.ACC_ADD, 1.0) == -1 and "4-byte aligned" in err()
    assert call([good], 1, 3, 1.0) == -1 and "mode 3" in err()
    assert call([good], 1, -1, 1.0) == -1 and "mode -1" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call([good], 1, _lib.ACC_FINISH, bad) == -1 and "non-finite scale" in err()
    assert lib.glowhip_grad_accumulate(None, 1, _lib.ACC_ADD, 1.0, None) == -1 and "null segment table" in err()
