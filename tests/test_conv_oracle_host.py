"""CPU checks of tests/conv_oracle.py, the yardstick tests/test_gpu_conv_kernels.py holds the exact-fp32 convolution kernels to:

  * the fp64 reference equals float64 torch.nn.functional.conv2d plus the same epilogue within 1e-12 of the element's sum of magnitudes;
  * the launchers' routing rules, written out again in the oracle, give every instance the GPU file expects;
  * every `exact` set meets the two conditions of its family (integers times the row granule, partial sums below 2^24 granules);
  * an fp32 emulation of the promised arithmetic (one rounding per accumulated product in the kernel's k order, the split-K slices
    summed in order, the pre-scaled FIRST image, the epilogue in the kernel's order) equals the reference on every `exact` set and
    stays inside the bound on every `random` set the GPU file runs;
  * each single fault of conv_oracle.FAULTS / TAIL_FAULTS leaves the bound (`random`) and the exact value (`exact`) on every case it
    applies to;
  * the tail's row map is a bijection onto the channels, its modes equal the model's coupling / split arithmetic in float64, and the
    launcher's cost model, written out again, gives every (MT, TP) and every DMA width the GPU file expects.
A large case is looked at on its first and last image (conv_oracle.host_images); its route is that of the whole case."""
import numpy as np
import pytest
import torch

import conv_oracle as C

f64 = np.float64
CASES = C.all_cases()
IDS = [c["name"] for c in CASES]
HOST_WORST = {}
_cache = {}


def setup(c, fam):
    """(operands, images, route, ref, bound, A), computed once per case and family and shared"""
    key = (c["name"], fam)
    if key not in _cache:
        d, images, rt = C.build(c, fam), C.host_images(c), C.route(c)
        ref, bound, A = C.reference(c, d, images, rt.get("S", 1))
        _cache.clear()      # (one entry: the tests of a case run next to each other)
        _cache[key] = (d, images, rt, ref, bound, A)
    return _cache[key]


def test_case_names_are_unique_and_instances_complete():
    assert len(set(IDS)) == len(IDS)
    seen = {c["instance"] for c in CASES} | {"k_conv_first MB=%d" % c["MB"] for c in CASES if c["op"] == C.FIRST}
    assert set(C.EXPECTED_INSTANCES) <= seen, set(C.EXPECTED_INSTANCES) - seen
    for c in C.wide_refusals():
        assert not C.wide_supported(c["Cin"], c["H"], c["W"], c["Cout"], c["ks"]) or c.get("transposed")
    for c in C.first_refusals():
        assert not C.first_supported(c["Cin"], c["H"], c["W"], c["Cout"])
    for c in CASES:
        ok = C.wide_supported(c["Cin"], c["H"], c["W"], c["Cout"], c["ks"]) if c["op"] == C.WIDE else (
            C.first_supported(c["Cin"], c["H"], c["W"], c["Cout"]) if c["op"] == C.FIRST else True)
        assert ok, c["name"]


def test_route_thresholds():
    w = lambda **k: C.wide_route(dict(dict(N=1, Cin=64, Cout=64, H=8, W=8, ks=3), **k))
    assert w(scratch=4 * 4096)["S"] == 4 and w(scratch=4 * 4096 - 1)["S"] == 3 and w(scratch=2 * 4096)["S"] == 2 and w(scratch=4096)["S"] == 1 and w()["S"] == 1
    assert w(N=5, H=16, W=76, scratch=1 << 30)["grid"] == [95, 3, 1] and w(N=6, H=16, W=64, scratch=1 << 30)["grid"] == [96, 1, 1]
    assert w(Cin=53, scratch=1 << 30)["S"] == 1 and w(Cin=54, scratch=1 << 30)["S"] == 4
    big = dict(N=16, H=32, W=32, Cout=512)
    assert w(ks=1, Cin=32, **big)["kernel"] == "k_conv_wide<1,128>" and w(ks=1, Cin=64, **big)["kernel"] == "k_gemm_glds"
    assert w(ks=1, Cin=64, N=15, H=32, W=32, Cout=512)["kernel"] == "k_conv_wide<1,64>" and w(Cin=6, **big)["kernel"] == "k_conv_wide<3,128>"
    assert C.first_max_cin(4, 16) == 168 and C.first_max_cin(1, 128) == 54      # 192 input channels fit no geometry's LDS window


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_reference_equals_float64_conv2d(c):
    d = C.build(c, "random")
    images = C.host_images(c)
    ref, _, A = C.reference(c, d, images)
    x = torch.from_numpy(d["x"][images]).double()
    w = torch.from_numpy(d["w"]).double()
    if c.get("transposed"):
        w = w.permute(1, 0, 2, 3).flip(2, 3)
    y = torch.nn.functional.conv2d(x, w, padding=c["ks"] // 2)
    t = lambda k: torch.from_numpy(d[k]).double().view(1, -1, 1, 1)
    for k in ("bias", "post_bias", "fold_bias"):
        if d[k] is not None:
            y = y + t(k)
    if d["post_scale"] is not None:
        y = y * t("post_scale")
    elif d["post_logs"] is not None:
        y = y * torch.exp(3.0 * t("post_logs"))
    if d["fold_logs"] is not None:
        y = y * torch.exp(3.0 * t("fold_logs"))
    if c["relu"]:
        y = torch.relu(y)
    assert np.all(np.abs(y.numpy().reshape(ref.shape) - ref) <= 1e-12 * (A * 8 + 1e-30) + 1e-12 * np.abs(ref))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_fp32_emulation_inside_bound_and_exact(c):
    for fam in c["families"]:
        d, images, rt, ref, bound, A = setup(c, fam)
        got = C.emulate(c, d, images, rt)
        if fam == "exact":
            C.check_exact(c, d, A)
            assert np.array_equal(got.astype(f64), ref), (c["name"], int((got.astype(f64) != ref).sum()), "values differ")
        else:
            HOST_WORST[c["instance"]] = max(HOST_WORST.get(c["instance"], 0.0), C.worst(got, ref, bound))
            assert C.inside(got, ref, bound), (c["name"], C.worst(got, ref, bound))


@pytest.mark.parametrize("fault", sorted(C.FAULTS))
def test_single_fault_leaves_the_bound(fault):
    hit = 0
    for c in CASES:
        for fam in c["families"]:
            d, images, rt = C.build(c, fam), C.host_images(c), C.route(c)
            rt.setdefault("S", 1)
            bad = C.FAULTS[fault](c, d, images, rt)
            if bad is None:
                continue
            ref, bound, _ = C.reference(c, d, images, rt["S"])
            hit += 1
            if fam == "exact":
                assert not np.array_equal(bad, ref), (fault, c["name"], "exact set does not notice")
            else:
                assert not C.inside(bad, ref, bound), (fault, c["name"], "random set stays inside the bound")
    assert hit >= 2, (fault, "applies to", hit, "sets")


def test_zz_report_host_yardstick():
    for k in sorted(HOST_WORST):
        print(f"host emulation, worst multiple of the bound: {k:36s} {HOST_WORST[k]:.3f}")
    assert HOST_WORST and max(HOST_WORST.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the tail convolution
# ---------------------------------------------------------------------------------------------------------------------
TAILS = C.tail_cases()
TIDS = [c["name"] for c in TAILS]


def test_tail_row_map_and_routes():
    assert len(set(TIDS)) == len(TIDS)
    for Cout in range(1, 100):
        for paired in ((0, 1) if Cout % 2 == 0 else (0,)):
            rows = [C.tail_row_channel(m, Cout, paired) for m in range(16 * C.tail_mt(Cout, paired))]
            assert sorted(r for r in rows if r >= 0) == list(range(Cout)), (Cout, paired)      # every channel once, the rest empty
    assert [C.tail_row_channel(m, 8, 1) for m in range(8)] == [0, 2, 1, 3, 4, 6, 5, 7]
    assert [C.tail_mt(c, 1) for c in (2, 10, 12, 24, 48, 96)] == [1, 1, 1, 2, 3, 6] and [C.tail_mt(c, 0) for c in (1, 6, 17, 56)] == [1, 1, 2, 4]
    for c in C.tail_refusals():
        assert C.tail_route(c).get("refused"), c
    seen = {c["instance"] for c in TAILS}
    for mt in (1, 2):
        for tp in (16, 32, 64, 128):
            assert "k_conv_tail<MT=%d,TP=%d>" % (mt, tp) in seen
    assert any(i.startswith("k_conv_tail<MT=3") for i in seen)
    for W in (8, 16, 32, 64, 128):
        assert any(i.startswith("k_conv_tail_dma") and i.endswith("W=%d>" % W) for i in seen), W
    # a 128-wide map has no register-staged tile; without the zero block (or with the DMA kernels switched off) it is refused
    assert not any(C.tp_ok_reg(tp, 1, 128) for tp in (16, 32, 64, 128)) and C.tp_ok_dma(128, 1, 128, 32, False)


@pytest.mark.parametrize("c", TAILS[::4], ids=TIDS[::4])
def test_tail_modes_equal_the_model_arithmetic(c):
    """conv + epilogue against float64 torch with the coupling / split arithmetic of oracle/glow_oracle.py's formulas"""
    from oracle import glow_oracle as O
    d, rt = C.build_tail(c, "random"), C.tail_route(c)
    ref = C.tail_reference(c, d, rt)
    N, Cout, H, W = c["N"], c["Cout"], c["H"], c["W"]
    h = torch.nn.functional.conv2d(torch.from_numpy(d["x"]).double(), torch.from_numpy(d["w"]).double(), padding=1)
    if d["bias"] is not None:
        h = (h + torch.from_numpy(d["bias"]).double().view(1, -1, 1, 1)) * torch.from_numpy(d["post_scale"]).double().view(1, -1, 1, 1)
    close = lambda a, b: np.allclose(a.reshape(-1), np.asarray(b).reshape(-1), rtol=1e-11, atol=1e-13)
    assert close(ref["hout"][0], h.numpy())
    z = torch.from_numpy(d["z2"]).double().view(N, -1, H, W)
    mode = c["mode"]
    if mode in C.PAIRED_MODES:
        A_, B_ = O.split_channel(h, "cross")
        if mode.startswith("affine"):
            s = torch.sigmoid(B_ + 2.0)
            z2 = (z + A_) * s if mode == "affine_fwd" else z / s - A_
            t = torch.log(s).flatten(1).sum(1) * (1 if mode == "affine_fwd" else -1)
        elif mode == "split_fwd":
            t = O.gaussian_logp(A_, B_, z)
            z2 = (z - A_) * torch.exp(-B_)
            assert close(O.gaussian_sample(A_, B_, z2).numpy(), z.numpy())      # the implied draw is what split_rev takes back
        else:
            z2, t = O.gaussian_sample(A_, B_, z), None
        if t is not None:
            assert close(ref["term"][0], t.numpy())
    else:
        z2 = h if mode == "plain" else (z + h if mode == "add_fwd" else z - h)
    assert close(ref["z2_out"][0], z2.numpy())


@pytest.mark.parametrize("c", TAILS, ids=TIDS)
def test_tail_fp32_emulation_inside_bound_and_exact(c):
    rt = C.tail_route(c)
    for fam in c["families"]:
        d = C.build_tail(c, fam)
        ref, got = C.tail_reference(c, d, rt), C.emulate_tail(c, d, rt)
        if fam == "exact":
            _, A = C.conv_sums(d["x"], d["w"].astype(f64), 3)
            C.check_exact(c, d, A)
            for k in C.tail_exact_outputs(c):
                assert np.array_equal(got[k].astype(f64), ref[k][0]), (c["name"], k)
        for k in ref:
            assert np.all(np.isfinite(ref[k][0])) and np.all(np.isfinite(ref[k][1])), (c["name"], fam, k)
            w = C.worst(got[k], *ref[k])
            if fam == "random":
                key = "%s %s %s" % (c["instance"].split("<")[0], c["mode"], k)
                HOST_WORST[key] = max(HOST_WORST.get(key, 0.0), w)
            assert C.inside(got[k], *ref[k]), (c["name"], fam, k, w)


@pytest.mark.parametrize("fault", sorted(C.TAIL_FAULTS))
def test_tail_single_fault_leaves_the_bound(fault):
    hit = 0
    for c in TAILS:
        rt = C.tail_route(c)
        for fam in c["families"]:
            d = C.build_tail(c, fam)
            bad = C.TAIL_FAULTS[fault](c, d, rt)
            if bad is None:
                continue
            ref = C.tail_reference(c, d, rt)
            hit += 1
            keys = [k for k in C.tail_outputs(c) if k in ref] or ["hout"]
            if fam == "exact":
                keys = [k for k in keys if k in C.tail_exact_outputs(c)] or ["hout"]
                if fault == "plus2_dropped":
                    continue      # (hout does not see the sigmoid: the random sets hold this one)
                assert any(not np.array_equal(bad[k][0], ref[k][0]) for k in keys), (fault, c["name"], "exact set does not notice")
            else:
                assert any(not C.inside(bad[k][0], *ref[k]) for k in keys), (fault, c["name"], "random set stays inside the bound")
    assert hit >= 2, (fault, "applies to", hit, "sets")


def test_zzz_report_tail_yardstick():
    for k in sorted(HOST_WORST):
        if k.startswith("k_conv_tail"):
            print(f"host emulation, worst multiple of the bound: {k:44s} {HOST_WORST[k]:.3f}")
    assert max(HOST_WORST.values()) <= 1.0
