"""Every HBM-bound gradient kernel of the training sweep on its own (csrc/backward.hip: the coupling tail, the split prior, the
ReLU / ActNorm masks, the channel-mixer backward in its three launch forms with the add_part gather of csrc/cnet_fin.h, the top
prior, flipT, logs_from_dw and the fp64-accumulator finalisation), launched through the testing hook glowhip_debug_bwd -- which
calls the launchers the backward sweep calls -- on operands laid out here, against the fp64 reference of tests/bwd_oracle.py on
EVERY output element:

  * `exact` input sets (every product and partial sum in every order an fp32 number): the kernel must return the reference value
    for value;
  * `random` input sets (realistic magnitudes): every element within the bound derived in bwd_oracle from the kernel's roundings,
    no outliers allowed.

tests/test_bwd_oracle_host.py shows on the CPU that the promised arithmetic lies inside that bound and that eleven single faults
leave it.

Every launch: every operand and output sits between 0xA5 guards, all intact afterwards; each case runs twice into fresh buffers --
elementwise outputs and plain-store accumulators bitwise equal, atomic accumulators each within the bound; the route (kernel, grid,
threads per channel, w_lds, LDS bytes, pixel blocks, reduction blocks, plain stores) is asserted from what the launcher reports
(glowhip_bwd_info).  Accumulators are zeroed here as the sweep zeroes them; the add_part scratch is sized as the sweep sizes it and
every slot the gather must not use holds NaN.

Worst multiple of the bound per op and route, `random` sets, measured on an MI355X (printed by the last test):
  route                               elementwise outputs              fp64 accumulators
  k_coupling_bwd4 affine              g_y2 0.763  g_pre 0.708          d b 0.111  d logs 0.171
  k_coupling_bwd4 additive            g_pre 0.993 (one rounding)       d b 0.105  d logs 0.147
  k_coupling_bwd affine               g_y2 0.695  g_pre 0.702          d b 0.181  d logs 0.291
  k_coupling_bwd additive             g_pre 0.993                      d b 0.297  d logs 0.464
  k_split_bwd                         g_z2 0.611  g_pre 0.712          d b 0.243  d logs 0.245
  k_act_bwd, 1 .. 32 threads / ch.    g_u 0.968                        d b 0.234  d logs 0.271
  k_act_bwd, 64 / 128 / >= 256        g_u 0.985 / 0.986 / 0.996        d b, d logs <= 0.001
  k_act_bwd1                          g_u 0.998                        d b 0.700  d logs 0.672
  k_chanmix_bwd matrix                g_x 0.597                        dW 0.065  d b 0.010  d logs 0.009
  k_chanmix_bwd matrix, w_lds         g_x 0.565                        dW 0.039  d b 0.017  d logs 0.015
  k_chanmix_bwd matrix, w_lds, add    g_x 0.285                        dW 0.028  d b 0.007  d logs 0.008
  k_chanmix_bwd gather / pass-through g_x 0.993 / 0.996                d b 0.034  d logs 0.022
  k_chanmix_bwd_reduce                g_x 0.314  reduced dW 0.996      dW 0.014  d b 0.006  d logs 0.008
  k_chanmix_bwd_wide matrix           g_x 0.037                        dW 0.119  d b 0.004  d logs 0.005
  k_chanmix_bwd_wide gather           g_x 0.998                        d b 0.078  d logs 0.074
  k_prior_bwd 0.808   k_logs_from_dw 0.946   k_gld_from_nll 0.989   k_sum_gld 0.000   k_grad_finalize_batched 0.914 (plain) 0.994 (winv)
  `exact` sets: 4 238 037 values compared, none differing.
(Outputs that are one rounding of an exact value sit just below 1 as they must; the accumulator bounds are worst cases in the
segment length, so sums of many terms use little of them.)"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib  # noqa: E402

import bwd_oracle as B  # noqa: E402

DEV = "cuda:0"
GUARD = 4096
EINVAL = -1
WORST = {}          # "op / route" -> worst multiple of the bound seen (reported by the last test)
EXACT = [0, 0]      # exact values compared, differing
f32, f64 = np.float32, np.float64
L = _lib


class Buf:
    """`nbytes` of device memory between two 0xA5 guards; the payload starts 0xA5 too unless `data` (numpy) is given.
    off: the payload starts that many bytes behind the 4096-aligned address (misaligned operands)."""

    def __init__(self, nbytes=0, data=None, off=0):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes
        self.nbytes, self.off = nbytes, off
        self.raw = torch.full((2 * GUARD + off + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        if data is not None and nbytes:
            self.raw[GUARD + off:GUARD + off + nbytes] = torch.from_numpy(data.view(np.uint8).reshape(-1)).to(DEV)
        self.ptr = self.raw.data_ptr() + GUARD + off
        assert (self.raw.data_ptr() & 255) == 0

    def intact(self):
        return bool((self.raw[:GUARD + self.off] == 0xA5).all()) and bool((self.raw[GUARD + self.off + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return bool((self.raw == 0xA5).all())

    def host(self, dtype):
        return self.raw[GUARD + self.off:GUARD + self.off + self.nbytes].cpu().numpy().view(dtype).copy()


def call(probe):
    info = L.BwdInfo()
    rc = L.lib().glowhip_debug_bwd(ctypes.byref(probe), ctypes.byref(info), L.stream_ptr(DEV))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this run
        pytest.exit(f"device error after glowhip_debug_bwd: {e}", returncode=3)
    return rc, info


def ok(probe):
    rc, info = call(probe)
    assert rc == 0, L.lib().glowhip_last_error()
    return info


def intact(*bufs):
    return all(b.intact() for b in bufs if b is not None)


def compare(route, name, fam, got, ref, key):
    """the assertion of every output: value for value (`exact`) or every element within the bound (`random`)"""
    r, b = ref
    got = np.asarray(got).reshape(r.shape)
    if fam == "exact":
        differ = int((got.astype(f64) != r).sum())
        EXACT[0] += got.size
        EXACT[1] += differ
        assert differ == 0, (name, key, route, differ, "of", got.size, "values differ from the fp64 reference")
        return
    w = B.worst(got, r, b)
    print(f"{name} [{fam}] {route} {key}: worst multiple of the bound {w:.3f}")
    WORST[route + " " + key] = max(WORST.get(route + " " + key, 0.0), w)
    assert B.inside(got, r, b), (name, key, route, int((~(np.abs(got.astype(f64) - r) <= b)).sum()), "elements outside the bound; worst multiple", w)


def halves(t1, t2):
    """(N, Ch, HW) x 2 -> the (N, 2 Ch, HW) tensor whose second half the sweep's pointers address"""
    return np.concatenate([t1, t2], axis=1)


def ids(cases):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# coupling tail
# ---------------------------------------------------------------------------------------------------------------------
def run_coupling(case, d):
    N, Ch, Cout, HW = case["N"], case["Ch"], case["Cout"], case["HW"]
    mis = case["misalign"]
    hout, z = Buf(data=d["hout"], off=4 if mis == "hout" else 0), Buf(data=halves(d["z1"], d["z2"]))
    g = Buf(data=halves(d["g1"], d["g2"]))
    gy = g if case["inplace"] else Buf(N * 2 * Ch * HW * 4)
    gpre, e4, gld = Buf(N * Cout * HW * 4, off=4 if mis == "gpre" else 0), Buf(data=d["e4"]), Buf(data=d["gld"])
    stride = 2 * Cout if case["copies"] > 1 else 0
    acc = Buf(data=np.zeros(((case["copies"] - 1) * stride + 2 * Cout), f64))
    p = L.BwdProbe()
    p.op, p.N, p.C, p.C2, p.HW, p.flag, p.acc_copies, p.acc_stride = L.BWD_COUPLING, N, Ch, Cout, HW, case["affine"], case["copies"], stride
    half = Ch * HW * 4
    p.src[0], p.src[1], p.src[2], p.src[3], p.src[4] = hout.ptr, z.ptr + half, g.ptr + half, e4.ptr, gld.ptr
    p.bs[0] = p.bs[1] = 2 * Ch * HW
    p.dst[0], p.dst[1], p.acc[0], p.acc[1] = gy.ptr + half, gpre.ptr, acc.ptr, acc.ptr + Cout * 8
    info = ok(p)
    assert intact(hout, z, g, gy, gpre, e4, gld, acc), case["name"]
    gyh = gy.host(f32).reshape(N, 2, Ch * HW)
    first = g.host(f32).reshape(N, 2, Ch * HW)[:, 0] if case["inplace"] else gyh[:, 0]
    assert first.tobytes() == (d["g1"].reshape(N, -1) if case["inplace"] else np.full((N, Ch * HW * 4), 0xA5, np.uint8)).tobytes(), "the first half was written"
    a = acc.host(f64)
    a = np.stack([a[k * stride:k * stride + 2 * Cout] for k in range(case["copies"])]).sum(axis=0)
    return dict(gy2=gyh[:, 1].copy(), gpre=gpre.host(f32), acc_b=a[:Cout], acc_l=a[Cout:]), info


@pytest.mark.parametrize("case", B.coupling_cases(), ids=ids(B.coupling_cases()))
def test_coupling_tail_equals_fp64(case):
    N, Ch, HW = case["N"], case["Ch"], case["HW"]
    for fam in case["families"]:
        d = B.build_coupling(case, fam)
        got, info = run_coupling(case, d)
        again, _ = run_coupling(case, d)
        ref = B.coupling_ref(case, d)
        if case["vec4"]:
            route = "k_coupling_bwd4 " + ("affine" if case["affine"] else "additive")
            assert info.kernel == L.BWI_COUPLING4 and list(info.grid) == [-(-Ch * HW // 1024), N, 1] and info.threads_per_channel == HW // 4, case["name"]
        else:
            route = "k_coupling_bwd " + ("affine" if case["affine"] else "additive")
            assert info.kernel == L.BWI_COUPLING1 and list(info.grid) == [-(-HW // 256), Ch, N], case["name"]
        for k in ("gy2", "gpre"):
            assert got[k].tobytes() == again[k].tobytes(), (case["name"], fam, k, "two runs differ")
        for k in ref:
            compare(route, case["name"], fam, got[k], ref[k], k)
        for k in ("acc_b", "acc_l"):
            assert B.inside(again[k], *ref[k]), (case["name"], fam, k, "second run outside the bound")


# ---------------------------------------------------------------------------------------------------------------------
# split prior
# ---------------------------------------------------------------------------------------------------------------------
def run_split(case, d):
    N, Ch, HW = case["N"], case["Ch"], case["HW"]
    r = B.rng_of("z1", case["name"])
    hout, z = Buf(data=d["hout"]), Buf(data=halves(r.normal(size=(N, Ch, HW)).astype(f32), d["z2"]))
    gz, gpre, e4, gld = Buf(N * 2 * Ch * HW * 4), Buf(N * 2 * Ch * HW * 4), Buf(data=d["e4"]), Buf(data=d["gld"])
    acc = Buf(data=np.zeros(4 * Ch, f64))
    p = L.BwdProbe()
    p.op, p.N, p.C, p.HW = L.BWD_SPLIT, N, Ch, HW
    half = Ch * HW * 4
    p.src[0], p.src[1], p.src[3], p.src[4] = hout.ptr, z.ptr + half, e4.ptr, gld.ptr
    p.bs[0] = p.bs[1] = 2 * Ch * HW
    p.dst[0], p.dst[1], p.acc[0], p.acc[1] = gz.ptr + half, gpre.ptr, acc.ptr, acc.ptr + 2 * Ch * 8
    info = ok(p)
    assert intact(hout, z, gz, gpre, e4, gld, acc), case["name"]
    gzh = gz.host(np.uint8).reshape(N, 2, half)
    assert (gzh[:, 0] == 0xA5).all(), "the first half of the gradient was written"
    a = acc.host(f64)
    return dict(gz2=gzh[:, 1].copy().view(f32), gpre=gpre.host(f32), acc_b=a[:2 * Ch], acc_l=a[2 * Ch:]), info


@pytest.mark.parametrize("case", B.split_cases(), ids=ids(B.split_cases()))
def test_split_prior_equals_fp64(case):
    d = B.build_split(case, "random")
    got, info = run_split(case, d)
    again, _ = run_split(case, d)
    ref = B.split_ref(case, d)
    assert info.kernel == L.BWI_SPLIT and list(info.grid) == [-(-case["HW"] // 256), case["Ch"], case["N"]], case["name"]
    for k in ("gz2", "gpre"):
        assert got[k].tobytes() == again[k].tobytes(), (case["name"], k, "two runs differ")
    for k in ref:
        compare("k_split_bwd", case["name"], "random", got[k], ref[k], k)
    for k in ("acc_b", "acc_l"):
        assert B.inside(again[k], *ref[k]), (case["name"], k, "second run outside the bound")


# ---------------------------------------------------------------------------------------------------------------------
# ReLU / ActNorm
# ---------------------------------------------------------------------------------------------------------------------
def run_act(case, d):
    N, Cm, HW = case["N"], case["Cm"], case["HW"]
    g, h, e, acc = Buf(data=d["g"]), Buf(data=d["h"]), Buf(data=d["e"]), Buf(data=np.zeros(2 * Cm, f64))
    p = L.BwdProbe()
    p.op, p.N, p.C, p.HW = L.BWD_ACT, N, Cm, HW
    p.src[0], p.src[3], p.dst[0], p.acc[0], p.acc[1] = h.ptr, e.ptr, g.ptr, acc.ptr, acc.ptr + Cm * 8
    info = ok(p)
    assert intact(g, h, e, acc), case["name"]
    a = acc.host(f64)
    return dict(gu=g.host(f32), acc_b=a[:Cm], acc_l=a[Cm:]), info


@pytest.mark.parametrize("case", B.act_cases(), ids=ids(B.act_cases()))
def test_relu_actnorm_equals_fp64(case):
    N, Cm, HW = case["N"], case["Cm"], case["HW"]
    for fam in case["families"]:
        d = B.build_act(case, fam)
        got, info = run_act(case, d)
        again, _ = run_act(case, d)
        ref = B.act_ref(case, d)
        if case["vec4"]:
            tpc = HW // 4
            route = "k_act_bwd tpc %s" % ("1..32" if tpc < 64 else "64" if tpc == 64 else "128" if tpc == 128 else ">=256")
            assert info.kernel == L.BWI_ACT4 and list(info.grid) == [-(-Cm * HW // 1024), N, 1] and info.threads_per_channel == tpc, case["name"]
        else:
            route = "k_act_bwd1"
            assert info.kernel == L.BWI_ACT1 and list(info.grid) == [-(-HW // 256), Cm, N], case["name"]
        assert got["gu"].tobytes() == again["gu"].tobytes(), (case["name"], fam, "two runs differ")
        for k in ref:
            compare(route, case["name"], fam, got[k], ref[k], k)
        for k in ("acc_b", "acc_l"):
            assert B.inside(again[k], *ref[k]), (case["name"], fam, k, "second run outside the bound")


# ---------------------------------------------------------------------------------------------------------------------
# channel mixer
# ---------------------------------------------------------------------------------------------------------------------
def run_mixer(case, d, add=True, inplace=None, expect_rc=0):
    """One launch_chanmix_bwd on fresh buffers -> (outputs, info, per-copy accumulators)."""
    N, C, HW, copies = case["N"], case["C"], case["HW"], case["copies"]
    inplace = case["inplace"] if inplace is None else inplace
    x, gy, bias, scale = Buf(data=d["x"]), Buf(data=d["gy"]), Buf(data=d["bias"]), Buf(data=d["scale"])
    gx = gy if inplace else Buf(N * C * HW * 4)
    mat = Buf(data=d["matrix"], off=4 if case["misalign_w"] else 0) if case["mode"] == "matrix" else None
    inv = Buf(data=d["inv"]) if case["mode"] == "gather" else None
    stride = C * C + 2 * C
    acc = Buf(data=np.zeros(copies * stride, f64))
    p = L.BwdProbe()
    p.op, p.N, p.C, p.HW, p.acc_copies, p.acc_stride = L.BWD_CHANMIX, N, C, HW, copies, stride
    p.src[0], p.src[1], p.src[2], p.src[3] = x.ptr, gy.ptr, bias.ptr, scale.ptr
    p.src[4], p.src[5] = (mat.ptr if mat else None), (inv.ptr if inv else None)
    p.bs[0] = p.bs[1] = C * HW
    p.dst[0], p.acc[0], p.acc[1], p.acc[2] = gx.ptr, acc.ptr, acc.ptr + C * C * 8, acc.ptr + (C * C + C) * 8
    scratch = None
    if case["add"] and add:
        geo = B.case_geometry(case)
        assert d["scratch"].size == geo["MS"] * N * geo["Cout"] * HW + 2 * geo["MS"] * geo["tiles"] * geo["Cout"] * geo["W"]
        scratch = Buf(data=d["scratch"])
        p.src[6], p.add_scale = scratch.ptr, float(d["add_scale"])
        for i, v in enumerate((geo["Cout"], geo["MS"], geo["tiles"], geo["R"], geo["NI"], geo["lpxt"], geo["H"], geo["W"])):
            p.add[i] = v
    parts, dws = [Buf(data=t) for t in d["partials"]], [Buf(j["Mreal"] * j["Nreal"] * 4) for j in case["jobs"]]
    p.n_jobs = len(case["jobs"])
    for i, j in enumerate(case["jobs"]):
        p.job[i].a, p.job[i].out = parts[i].ptr, dws[i].ptr
        for k, name in enumerate(("splits", "Mpad", "Npad", "Mreal", "Nreal", "mode")):
            p.job[i].n[k] = j[name]
    rc, info = call(p)
    assert rc == expect_rc, (rc, L.lib().glowhip_last_error())
    assert intact(x, gy, gx, bias, scale, mat, inv, acc, scratch, *parts, *dws), case["name"]
    if rc:
        assert (inplace or gx.untouched()) and not acc.host(f64).any() and gy.host(f32).tobytes() == d["gy"].tobytes(), "a refused launch wrote"
        return None, info, None
    a = acc.host(f64).reshape(copies, stride)
    s = a.sum(axis=0)
    out = dict(gx=gx.host(f32), acc_b=s[C * C:C * C + C], acc_l=s[C * C + C:], dw=[t.host(f32) for t in dws])
    if case["mode"] == "matrix":
        out["acc_w"] = s[:C * C]
    else:
        assert not a[:, :C * C].any(), "a gather wrote dW"
    return out, info, a


def check_mixer(case, families=None):
    C, copies, blocks = case["C"], case["copies"], case["blocks"]
    for fam in families or case["families"]:
        d = B.build_mixer(case, fam)
        got, info, a = run_mixer(case, d)
        again, _, a2 = run_mixer(case, d)
        ref = B.mixer_ref(case, d)
        plain = blocks <= copies
        route = {"plain": "k_chanmix_bwd", "reduce": "k_chanmix_bwd_reduce", "wide": "k_chanmix_bwd_wide"}[case["kernel"]] + \
            " %s%s%s" % (case["mode"], " w_lds" if case["w_lds"] else "", " add" if case["add"] else "")
        want = {"plain": L.BWI_CHANMIX, "reduce": L.BWI_CHANMIX_REDUCE, "wide": L.BWI_CHANMIX_WIDE}[case["kernel"]]
        assert (info.kernel, info.w_lds, info.lds_bytes, info.mix_blocks, info.rblocks, info.plain_stores) == \
            (want, case["w_lds"], case["lds"], blocks, case["rblocks"], int(plain)), (case["name"], info.kernel, info.w_lds, info.lds_bytes, info.mix_blocks,
                                                                                      info.rblocks, info.plain_stores)
        grid = [blocks, -(-C // 32), 1] if case["kernel"] == "wide" else [blocks + case["rblocks"] * len(case["jobs"]), 1, 1]
        assert list(info.grid) == grid and info.launches == (2 if case["jobs"] and case["kernel"] != "reduce" else 1), case["name"]
        assert got["gx"].tobytes() == again["gx"].tobytes(), (case["name"], fam, "two runs differ")
        if plain:      # every pixel block owns its copy: stores, the same bytes every run, and nothing in the copies beyond
            assert a.tobytes() == a2.tobytes(), (case["name"], fam, "plain-store accumulators differ between two runs")
            assert not a[blocks:].any(), (case["name"], "an accumulator copy beyond the pixel blocks was written")
        for k in ref:
            compare(route, case["name"], fam, got[k], ref[k], k)
            if k != "gx":
                assert B.inside(again[k].reshape(ref[k][0].shape), *ref[k]), (case["name"], fam, k, "second run outside the bound")
        for job, part, dw, dw2 in zip(case["jobs"], d["partials"], got["dw"], again["dw"]):
            assert dw.tobytes() == dw2.tobytes()
            compare("split-K reduction beside the mixer", case["name"], fam, dw, B.reduce_ref(job, part), "dw")


@pytest.mark.parametrize("case", B.mixer_cases(), ids=ids(B.mixer_cases()))
def test_mixer_narrow_equals_fp64(case):
    check_mixer(case)


@pytest.mark.parametrize("case", B.mixer_reduce_cases(), ids=ids(B.mixer_reduce_cases()))
def test_mixer_with_reductions_equals_fp64(case):
    """k_chanmix_bwd_reduce (C = 96: the reductions as a launch of their own, the same outputs)"""
    check_mixer(case)


@pytest.mark.parametrize("case", B.mixer_add_cases(), ids=ids(B.mixer_add_cases()))
def test_mixer_add_part_equals_fp64(case):
    """the six gather instantiations: halos at MS = 1, 2, 4, none at MS = 2, 4, and the generic one (MS = 1 without halos)"""
    check_mixer(case)
    # channels >= add_C of the staged gradient do not see the gather: as a pass-through (no matrix, no table) g_x = g e
    ident = dict(case, mode="identity")
    d = B.build_mixer(ident, "random")
    with_add, _, _ = run_mixer(ident, d)
    without, _, _ = run_mixer(ident, d, add=False)
    aC = case["add"]["C"]
    w, wo = (t["gx"].reshape(case["N"], case["C"], case["HW"]) for t in (with_add, without))
    assert w[:, aC:].tobytes() == wo[:, aC:].tobytes(), "channels >= add_C differ from the run without add_part"
    assert (w[:, :aC] != wo[:, :aC]).any() and np.isfinite(w).all()


@pytest.mark.parametrize("case", B.mixer_wide_cases(), ids=ids(B.mixer_wide_cases()))
def test_mixer_wide_equals_fp64(case):
    check_mixer(case)


def test_mixer_wide_refuses_in_place_and_add_part():
    case = B.mixer_wide_cases()[0]
    d = B.build_mixer(case, "random")
    run_mixer(case, d, inplace=True, expect_rc=EINVAL)
    geo = B.add_geometry(case["N"], 2, 2, 2, 1, 1, 6)
    withadd = dict(case, add=dict(H=2, W=2, R=2, NI=1, MS=1, C=6))
    d["scratch"], d["add_scale"] = B.build_scratch(geo, B.rng_of("wide add"), "random"), f32(1.0)
    run_mixer(withadd, d, expect_rc=EINVAL)


# ---------------------------------------------------------------------------------------------------------------------
# top prior, flipT, logs_from_dw, finalize
# ---------------------------------------------------------------------------------------------------------------------
def run_prior(case, d):
    N, per = case["N"], case["per"]
    z, gld, gz = Buf(data=d["z"]), Buf(data=d["gld"]), Buf(N * per * 4)
    mean, logs = (Buf(data=d[k]) if case["ml"] != "null" else None for k in ("mean", "logs"))
    gin = Buf(data=d["gz_in"]) if case["gz_in"] else None
    p = L.BwdProbe()
    p.op, p.N, p.per = L.BWD_PRIOR, N, per
    p.bs[0] = per if case["ml"] == "sample" else 0
    p.src[0], p.src[1], p.src[2], p.src[4], p.src[5] = z.ptr, (mean.ptr if mean else None), (logs.ptr if logs else None), gld.ptr, (gin.ptr if gin else None)
    p.dst[0] = gz.ptr
    info = ok(p)
    assert intact(z, gld, gz, mean, logs, gin), case["name"]
    return gz.host(f32), info


@pytest.mark.parametrize("case", B.prior_cases(), ids=ids(B.prior_cases()))
def test_top_prior_equals_fp64(case):
    d = B.build_prior(case, "random")
    got, info = run_prior(case, d)
    again, _ = run_prior(case, d)
    assert info.kernel == L.BWI_PRIOR and list(info.grid) == [-(-case["per"] // 256), case["N"], 1]
    assert got.tobytes() == again.tobytes()
    compare("k_prior_bwd", case["name"], "random", got, B.prior_ref(case, d)["gz"], "gz")


@pytest.mark.parametrize("shape", B.FLIP_CASES, ids=["%dx%dx%d" % s for s in B.FLIP_CASES])
def test_weight_flipT_bitwise(shape):
    Cout, Cin, k = shape
    w = B.rng_of("flip", shape).normal(size=(Cout, Cin, k, k)).astype(f32)
    src, dst = Buf(data=w), Buf(w.nbytes)
    p = L.BwdProbe()
    p.op, p.C, p.C2, p.ksize = L.BWD_FLIP, Cout, Cin, k
    p.src[0], p.dst[0] = src.ptr, dst.ptr
    ok(p)
    assert intact(src, dst) and dst.host(f32).tobytes() == B.flip_ref(w).tobytes()


def test_logs_from_dw_equals_fp64():
    data = [B.build_logs(rows, K) for rows, K in B.LOGS_JOBS]
    outs = []
    for _ in range(2):
        bufs = [{k: Buf(data=d[k]) for k in ("w", "dw", "b", "db")} for d in data]
        out = [Buf(rows * 4) for rows, _ in B.LOGS_JOBS]
        p = L.BwdProbe()
        p.op, p.n_jobs = L.BWD_LOGS_FROM_DW, len(data)
        for i, (rows, K) in enumerate(B.LOGS_JOBS):
            j = p.job[i]
            j.a, j.b, j.c, j.d, j.out = bufs[i]["w"].ptr, bufs[i]["dw"].ptr, bufs[i]["b"].ptr, bufs[i]["db"].ptr, out[i].ptr
            j.n[0], j.n[1] = rows, K
        ok(p)
        assert intact(*out, *[b for bb in bufs for b in bb.values()])
        outs.append([o.host(f32) for o in out])
    for d, a, b in zip(data, *outs):
        assert a.tobytes() == b.tobytes()
        compare("k_logs_from_dw", "logs_from_dw", "random", a, B.logs_ref(d), "out")


def run_finalize(N, d):
    nll, gld, gsum = Buf(data=d["nll"]), Buf(N * 4), Buf(8)
    accs = [Buf(data=a) for a in d["acc"]]
    winvs = [Buf(data=w) if w is not None else None for w in d["winv"]]
    outs = [Buf(j["n"] * 4) for j in d["jobs"]]
    p = L.BwdProbe()
    p.op, p.N, p.inv, p.n_jobs = L.BWD_FINALIZE, N, d["inv"], len(d["jobs"])
    p.src[0], p.dst[0], p.acc[0] = nll.ptr, gld.ptr, gsum.ptr
    for i, j in enumerate(d["jobs"]):
        q = p.job[i]
        q.a, q.b, q.out = accs[i].ptr, (winvs[i].ptr if winvs[i] else None), (outs[i].ptr if j["out"] else None)
        q.n[0], q.n[1], q.n[2], q.stride, q.add_mul = j["n"], j["C"], j["copies"], j["stride"], j["add_mul"]
    ok(p)
    assert intact(nll, gld, gsum, *accs, *winvs, *outs)
    for j, o in zip(d["jobs"], outs):
        assert j["out"] or o.untouched(), "the job without an output wrote"
    return gld.host(f32), gsum.host(f64)[0], [o.host(f32) for o in outs]


@pytest.mark.parametrize("N", B.FINALIZE_N)
def test_finalize_equals_fp64(N):
    for fam in ("exact", "random"):
        d = B.build_finalize(N, fam)
        gld, gsum, outs = run_finalize(N, d)
        gld2, gsum2, outs2 = run_finalize(N, d)
        assert gld.tobytes() == gld2.tobytes() and gsum == gsum2 and all(a.tobytes() == b.tobytes() for a, b in zip(outs, outs2))
        compare("k_gld_from_nll", "finalize-N%d" % N, fam, gld, B.gld_ref(d), "gld")
        G, mag = gld.astype(f64).sum(), np.abs(gld.astype(f64)).sum()
        compare("k_sum_gld", "finalize-N%d" % N, fam, np.array([gsum]), (np.array([G]), B.bnd(B.F64 * np.array([mag]))), "gsum")
        for j, got, rb in zip(d["jobs"], outs, B.finalize_ref(d, gld)):
            if rb:
                compare("k_grad_finalize_batched " + ("winv" if j["winv"] else "plain"), "finalize-N%d" % N, fam, got, rb, "out")


def test_hook_refuses_what_it_cannot_launch():
    """an unknown op, a null operand, more jobs than the table holds: GLOWHIP_EINVAL, nothing launched"""
    g, acc = Buf(data=np.ones((1, 4, 4), f32)), Buf(data=np.zeros(8, f64))
    p = L.BwdProbe()
    p.op, p.N, p.C, p.HW = 99, 1, 4, 4
    assert call(p)[0] == EINVAL
    p.op = L.BWD_ACT      # h and e missing
    p.dst[0], p.acc[0], p.acc[1] = g.ptr, acc.ptr, acc.ptr + 32
    assert call(p)[0] == EINVAL
    p.op, p.n_jobs = L.BWD_LOGS_FROM_DW, L.BWD_MAX_JOBS + 1
    assert call(p)[0] == EINVAL
    assert g.host(f32).tobytes() == np.ones(16, f32).tobytes() and not acc.host(f64).any() and intact(g, acc)


def test_zz_report():
    """Prints the worst multiple of the bound per op and route and the count of `exact` values compared (the figures of the module
    docstring); asserts nothing that the tests above have not."""
    for name in sorted(WORST):
        print(f"worst multiple of the bound  {name:60s} {WORST[name]:.3f}")
    print(f"exact values compared: {EXACT[0]}, differing: {EXACT[1]}")
    assert EXACT[1] == 0
