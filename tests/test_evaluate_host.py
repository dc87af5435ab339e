"""CPU checks of the held-out evaluation (-m "not gpu"): the host bookkeeping of the level split, the fp64 oracle's own
properties (tests/evaluate_oracle.py), the profile key ``hps.optim.interval_eval`` and the evaluator's draw numbering against a
stub plan.  The kernels are held to the same oracle by tests/test_gpu_evaluate.py and tests/test_gpu_evaluate_model.py."""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib
from pytorch_glow_amd.misc import util
from pytorch_glow_amd.network import evaluate as EV
from pytorch_glow_amd.network import model as gmodel

import evaluate_oracle as EO

D = 3 * 64 * 64


def _layer(d, kind, C, H, W, fake):
    d.kind, d.C, d.H, d.W = kind, C, H, W
    if kind == _lib.LAYER_SPLIT2D:      # host bookkeeping never follows the pointers: any non-null address will do
        d.f4_w = d.f4_bias = d.f4_logs = fake


def test_level_count_is_host_bookkeeping():
    lib = G.lib()
    assert lib.glowhip_plan_level_count(None) == 0
    keep = ctypes.create_string_buffer(64)
    fake = ctypes.addressof(keep)
    d = (_lib.LayerDesc * 2)()
    _layer(d[0], _lib.LAYER_SQUEEZE, 3, 8, 8, fake)
    _layer(d[1], _lib.LAYER_SQUEEZE, 12, 4, 4, fake)
    h = lib.glowhip_plan_create(d, 2)
    assert h and lib.glowhip_plan_level_count(h) == 1
    assert lib.glowhip_plan_level_scratch_bytes(h, 5) == 1 * 9 * 5 * 8
    lib.glowhip_plan_destroy(h)
    # squeeze, split, squeeze, split, squeeze: two Split2d layers, three levels
    d = (_lib.LayerDesc * 5)()
    _layer(d[0], _lib.LAYER_SQUEEZE, 3, 16, 16, fake)
    _layer(d[1], _lib.LAYER_SPLIT2D, 12, 8, 8, fake)
    _layer(d[2], _lib.LAYER_SQUEEZE, 6, 8, 8, fake)
    _layer(d[3], _lib.LAYER_SPLIT2D, 24, 4, 4, fake)
    _layer(d[4], _lib.LAYER_SQUEEZE, 12, 4, 4, fake)
    h = lib.glowhip_plan_create(d, 5)
    assert h, lib.glowhip_last_error()
    assert lib.glowhip_plan_level_count(h) == 3
    assert lib.glowhip_plan_level_scratch_bytes(h, 4) == 3 * 9 * 4 * 8
    # binding is host bookkeeping too: refused without both buffers, accepted with them, (NULL, NULL, 0) unbinds
    assert lib.glowhip_plan_bind_level_terms(h, None, fake, 64) != 0
    assert b"null terms or scratch" in lib.glowhip_last_error()
    assert lib.glowhip_plan_bind_level_terms(h, fake, fake, 64) == 0
    assert lib.glowhip_plan_bind_level_terms(h, None, None, 0) == 0
    lib.glowhip_plan_destroy(h)


def test_eval_state_mirror_matches_the_header():
    # 2 + 2 + 3*2 + 16*2 words, two doubles, two int32, two counters, 256 bins
    assert ctypes.sizeof(_lib.EvalState) == 8 * (2 + 2 + 6 + 32 + 2 + 1 + 2 + 256)
    assert _lib.EvalState.sum_level.offset == 80 and _lib.EvalState.lo.offset == 80 + 256
    assert _lib.EvalState.bins.offset == 352 and _lib.EvalState.under.offset == 360 and _lib.EvalState.hist.offset == 376


def test_fold_refusals_come_before_any_device_call():
    lib = G.lib()
    keep = ctypes.create_string_buffer(64)
    p = ctypes.addressof(keep)
    assert lib.glowhip_eval_fold(None, p, None, 1, 4, 0, 1.0, None, p, 0, None) != 0
    assert lib.glowhip_eval_fold(p, p, None, 0, 4, 0, 1.0, None, p, 0, None) != 0 and b"draws" in lib.glowhip_last_error()
    assert lib.glowhip_eval_fold(p, p, p, 1, 4, 17, 1.0, None, p, 0, None) != 0 and b"n_levels" in lib.glowhip_last_error()
    assert lib.glowhip_eval_fold(p, p, None, 1, 4, 0, 0.0, None, p, 0, None) != 0 and b"dims" in lib.glowhip_last_error()
    assert lib.glowhip_eval_fold(p, p, None, 1, 0, 0, 1.0, None, p, 0, None) == 0      # an empty batch: nothing to launch
    assert lib.glowhip_eval_reset(p, 17, 0, 0.0, 1.0, None) != 0
    assert lib.glowhip_eval_reset(p, 3, 257, 0.0, 1.0, None) != 0
    assert lib.glowhip_eval_reset(p, 3, 8, 2.0, 2.0, None) != 0 and b"range" in lib.glowhip_last_error()


# ------------------------------------------------------------------------------------------------ the oracle's own properties
def test_one_draw_is_the_plain_figure():
    o = np.random.RandomState(1).uniform(-26000, -24000, size=(1, 37)).astype(np.float32)
    bpd, single = EO.per_image(o, D)
    want = -o[0].astype(np.float64) / (EO.LN2 * D)
    assert np.array_equal(bpd, want) and np.array_equal(single, want)


def test_jensen_holds_per_image_and_large_objectives_do_not_underflow():
    rs = np.random.RandomState(2)
    o = (-25000.0 + rs.uniform(-60, 60, size=(5, 257))).astype(np.float32)
    o[:, 7] = -25000.0      # an image whose draws are all equal: the two figures coincide
    bpd, single = EO.per_image(o, D)
    assert np.isfinite(bpd).all() and np.isfinite(single).all()
    assert (bpd <= single + 1e-15).all()
    assert abs(bpd[7] - single[7]) <= 1e-15 * abs(single[7])
    # exp(-25000) underflows fp64; the max-subtracted form is within the spread of the draws
    assert (bpd >= -(o.astype(np.float64).max(axis=0)) / (EO.LN2 * D) - 1e-12).all()
    # against exact rational-free arithmetic in longdouble on the shifted values
    ol = o.astype(np.longdouble)
    ref = -(ol.max(axis=0) + np.log(np.exp(ol - ol.max(axis=0)).sum(axis=0)) - np.log(np.longdouble(5))) / (np.longdouble(EO.LN2) * D)
    assert np.abs(bpd - ref.astype(np.float64)).max() <= 1e-12


def test_fixed_point_totals_do_not_depend_on_partition_or_order():
    rs = np.random.RandomState(3)
    vals = rs.uniform(2.5, 5.5, size=257)
    whole = EO.fixed_total(vals)
    parts_a = EO.fixed_total(vals[:100]) + EO.fixed_total(vals[100:200]) + EO.fixed_total(vals[200:])
    perm = rs.permutation(257)
    parts_b = EO.fixed_total(vals[perm][200:]) + EO.fixed_total(vals[perm][:64]) + EO.fixed_total(vals[perm][64:200])
    parts_c = sum(EO.fixed_total(vals[i:i + 1]) for i in reversed(range(257)))
    assert whole == parts_a == parts_b == parts_c
    assert abs(whole / EO.FIX - vals.sum()) <= 257 * 2.0 ** -33 + 1e-9


def test_oracle_fold_flags_non_finite_images_and_bins_edges():
    o = np.full((2, 6), -25000.0, dtype=np.float32)
    o[1, 1], o[0, 3], o[1, 4] = np.nan, np.inf, -np.inf
    f = EO.fold(o, D, hist=(16, 0.0, 8.0))
    assert f["flagged"] == 3 and f["count"] == 3 and np.isnan(f["bpd32"][[1, 3, 4]]).all()
    assert f["sum_bpd"] == 3 * EO.q(f["bpd32"][0])
    assert EO.hist_slot(0.0, 16, 0.0, 8.0) == 0 and EO.hist_slot(8.0, 16, 0.0, 8.0) == "over"
    assert EO.hist_slot(2.5, 16, 0.0, 8.0) == 5 and EO.hist_slot(np.nextafter(2.5, 0.0), 16, 0.0, 8.0) == 4
    assert EO.hist_slot(-1e-9, 16, 0.0, 8.0) == "under"


def test_level_terms_of_the_oracle_add_up_to_its_objective():
    cfg = EO.O.default_cfg(image_shape=(16, 16, 3), hidden_channels=16, K=2, L=3, batch=2)
    sd = EO.O.seeded_state_dict(cfg, seed=4, zeros_std=0.02, invconv_perturb=0.05)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 16, 16, generator=g)
    noise = torch.rand(2, 3, 16, 16, generator=g) / 256
    terms, offset, obj = EO.level_terms(x, noise, sd, cfg)
    assert terms.shape == (3, 2) and EO.n_levels(cfg) == 3
    _, _, obj_ref = EO.O.glow_forward(x.double(), noise.double(), {k: v.double() for k, v in sd.items()}, cfg)
    assert (obj - obj_ref).abs().max().item() <= 1e-9 * obj_ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ profile key
def _hps(**optim):
    return util.AttrDict(dict(optim=dict(num_batch_train=16, **optim)))


def test_profile_schema_accepts_interval_eval():
    for name in ("celeba", "test"):
        assert "interval_eval" not in util.load_profile(name).optim      # beyond the reference's schema: its profiles have none
    assert util.interval_eval(_hps()) == 0
    assert util.interval_eval(_hps(interval_eval=None)) == 0
    assert util.interval_eval(_hps(interval_eval=0)) == 0
    assert util.interval_eval(_hps(interval_eval=250)) == 250
    for bad in (-1, 2.5, "10", True):
        with pytest.raises(ValueError, match="interval_eval"):
            util.interval_eval(_hps(interval_eval=bad))


# ------------------------------------------------------------------------------------------------ draw numbering
class _StubPlan:
    """Records what the evaluator asks of a plan; computes nothing."""
    n_levels, out_chw, FAMILY_EXACT_FP32, family = 2, (4, 2, 2), 1, 0

    def __init__(self):
        self.calls, self.streams = [], []

    def head_call(self, n, y):
        raise AssertionError("no head attached")

    def set_dequant_stream(self, seed, call):
        self.streams.append((seed, call))

    def set_dequant_rng(self, seed, enable):
        self.streams.append(("off", enable))

    def glow_forward(self, x, noise, pm, pl, ps, n_bits, out=None, head=None, level_terms=None):
        assert noise is None
        self.calls.append((self.streams[-1], x.shape[0], level_terms is not None))
        return out


def test_draw_numbering_follows_batch_order_and_leaves_the_global_stream_alone(monkeypatch):
    plan = _StubPlan()

    class _Flow:
        def plan_for(self, x, device=None):
            return plan

    class _Glow:
        hps = util.AttrDict(dict(model=dict(n_bits_x=8)))
        flow = _Flow()

        def _attach_head(self, p):
            return False

    monkeypatch.setattr(_lib, "require_device_tensor", lambda t, what="", allow_uint8=False: t)
    torch.manual_seed(11)
    gmodel.dequant_position(advance=True)
    before = gmodel.dequant_position()
    ev = EV.Evaluator(_Glow(), draws=3, levels=True, seed=5)
    key = EV.stream_seed(5)
    assert key == 5      # rank 0 of a single-process run: the seed itself
    for b, n in enumerate((4, 4, 3)):
        ev._forward_draws(torch.zeros(n, 3, 4, 4), None, b, key)
    assert [c[0] for c in plan.calls] == [(5, b * 3 + k) for b in range(3) for k in range(3)]
    assert [c[1] for c in plan.calls] == [4] * 6 + [3] * 3 and all(c[2] for c in plan.calls)
    assert plan.streams[-1] == ("off", False)      # the plan does not keep drawing with the evaluator's stream
    assert gmodel.dequant_position() == before
