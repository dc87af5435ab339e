"""Every exact-fp32 convolution kernel on its own (csrc/conv_mfma.hip: k_conv_wide<1|3, 64|128> with its split-K form and
k_splitk_finish, k_gemm_glds; csrc/conv_mfma_first.hip: k_conv_first<BN, W> in its nine instances with MB = 1, 2, 4;
csrc/conv_direct.hip: k_conv_direct<1|3>; the REPACK_WIDE / REPACK_FIRST image jobs of csrc/pack.hip with the folded ActNorm and the
transposed source), launched through the testing hook glowhip_debug_conv -- which builds the weight image with the plan's repack job
and calls the launchers the plan calls -- on synthetic operands, against the fp64 reference of tests/conv_oracle.py on EVERY output
element:

  * `exact` input sets (every product and partial sum in every order an fp32 number): the kernel must return the reference value
    for value, whatever its order of accumulation;
  * `random` input sets (realistic magnitudes, rows at 1, 1e-3, 1e-7): every element within the bound derived in conv_oracle from
    the kernel's roundings, no outliers allowed.

tests/test_conv_oracle_host.py shows on the CPU that the promised arithmetic lies inside that bound and that fifteen single faults
(nine on the wide / first / direct kernels, six on the tail) leave it.

Every launch: the instance (kernel, tile, split-K slices, MB, grid, launches, image size) is asserted from what the launcher
reports (glowhip_conv_info) against the launchers' rules written out again in conv_oracle; every operand, the weight image, the
split-K scratch (exactly the floats the launcher was told of) and the output sit between 0xA5 guards, all intact afterwards; each
case runs twice into fresh buffers and must give the same bytes.  Split-K launches are also compared with the one-launch result of
the same operands; an input that is the first half of a tensor twice as wide, NaN behind, must give the bytes of the contiguous one.

The tail convolution (csrc/conv_mfma_tail.hip k_conv_tail<MT, ...> and k_pack_tail, csrc/conv_mfma_tail_dma.h k_conv_tail_dma<..., W>
and the shared tail_epilogue) runs in its seven modes under every forced pixel tile with the out-channel split on and off, with
hout, z2_out and the finalised per-sample term compared on every element; z2_in / z2_out inside tensors twice as wide with NaN /
0xA5 in the gap; the in-kernel draw of TAIL_SPLIT_REV stays with the sampler tests.

Worst multiple of the bound per instance, `random` sets, measured on an MI355X / the fp32 emulation of the host file (printed by
the last test of either file):
  k_conv_wide<3,64> 0.253 / 0.253   <1,64> 0.107 / 0.107   <3,128> 0.129 / 0.101   <1,128> 0.148 / 0.148   k_gemm_glds 0.089 / 0.073
  k_conv_wide + k_splitk_finish 0.004 / 0.004 (long K: the bound's worst-case term dwarfs what random data uses of it)
  k_conv_first<64,8> 0.074 / 0.074  <64,16> 0.063 / 0.067  <64,32> 0.072 / 0.075  <64,64> 0.036 / 0.036  <128,8> 0.105 / 0.097
               <128,16> 0.101 / 0.093  <128,32> 0.055 / 0.042  <128,128> 0.071 / 0.076  (<128,64> runs its `exact` set only)
  k_conv_direct<1> 0.559 / 0.559    <3> 0.363 / 0.363
  k_conv_tail      hout <= 0.057 / 0.057   add z2_out 0.995 / 0.995 (one rounding of an exact sum)   affine z2_out 0.449 / 0.449
                   split_fwd z2_out 0.060 / 0.062   split_rev z2_out 0.082 / 0.100   term: affine 0.013 / 0.010, split 0.006 / 0.006
  k_conv_tail_dma  hout <= 0.009 / 0.009   add z2_out 0.989 / 0.989   affine z2_out 0.102 / 0.102   split z2_out 0.008 / 0.009
                   term <= 0.002 / 0.001
  `exact` sets: 137 412 266 values compared, none differing.
(Where the MI355X and the emulation agree to three digits the kernel's order of accumulation is the emulated one on that element.)"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib as L  # noqa: E402

import conv_oracle as C  # noqa: E402

DEV = "cuda:0"
GUARD = 4096
EINVAL = -1
WORST = {}          # instance -> worst multiple of the bound seen (reported by the last test)
EXACT = [0, 0]      # exact values compared, differing
SEEN = set()        # instances asserted from glowhip_conv_info
BLOCK = 1 << 23     # output elements per comparison block
f32, f64 = np.float32, np.float64
OPS = {C.WIDE: L.CONV_WIDE, C.FIRST: L.CONV_FIRST, C.DIRECT: L.CONV_DIRECT}


class Buf:
    """`nbytes` of device memory between two 0xA5 guards; the payload starts 0xA5 too unless `data` (numpy) is given"""

    def __init__(self, nbytes=0, data=None):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes
        self.nbytes = nbytes
        self.raw = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        if data is not None and nbytes:
            self.raw[GUARD:GUARD + nbytes] = torch.from_numpy(data.view(np.uint8).reshape(-1)).to(DEV)
        self.ptr = self.raw.data_ptr() + GUARD
        assert (self.raw.data_ptr() & 255) == 0

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return bool((self.raw == 0xA5).all())

    def host(self, dtype):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).copy()


def call(probe):
    info = L.ConvInfo()
    rc = L.lib().glowhip_debug_conv(ctypes.byref(probe), ctypes.byref(info), L.stream_ptr(DEV))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this run
        pytest.exit(f"device error after glowhip_debug_conv: {e}", returncode=3)
    return rc, info


def tab(d, k):
    return None if d[k] is None else Buf(data=d[k])


def launch(c, d, xwide=None, scratch="case"):
    """one launch of case c on operands d; returns (y Buf, info, all buffers).  scratch: "case" (what the case says) or None"""
    N, Cin, Cout, H, W = c["N"], c["Cin"], c["Cout"], c["H"], c["W"]
    HW = H * W
    xwide = c.get("xwide", False) if xwide is None else xwide
    x = d["x"].reshape(N, Cin, HW)
    if xwide:
        x = np.concatenate([x, np.full_like(x, np.nan)], axis=1)
    p = L.ConvProbe()
    p.op, p.N, p.Cin, p.H, p.W, p.Cout, p.ksize, p.relu, p.transposed = OPS[c["op"]], N, Cin, H, W, Cout, c["ks"], int(c["relu"]), int(c.get("transposed", 0))
    p.x_bs = (2 if xwide else 1) * Cin * HW
    rt = C.route(c)
    bufs = dict(x=Buf(data=x), w=Buf(data=d["w"]), y=Buf(N * Cout * HW * 4))
    for k in ("bias", "post_bias", "post_logs", "post_scale", "fold_bias", "fold_logs"):
        bufs[k] = tab(d, k)
        setattr(p, k, bufs[k].ptr if bufs[k] else None)
    p.x, p.w, p.y = bufs["x"].ptr, bufs["w"].ptr, bufs["y"].ptr
    if c["op"] == C.FIRST or (c["op"] == C.WIDE and not c.get("transposed")):
        rc, info = call(p)                                  # no image: the size alone
        assert rc == 0 and info.image_bytes == rt["image_bytes"] and info.kernel == 0 and bufs["y"].untouched(), c["name"]
        bufs["image"] = Buf(rt["image_bytes"])
        p.image = bufs["image"].ptr
    floats = c.get("scratch") if scratch == "case" else None
    if floats:
        bufs["scratch"] = Buf(floats * 4)
        p.scratch, p.scratch_floats = bufs["scratch"].ptr, floats
    rc, info = call(p)
    assert rc == 0, (c["name"], L.lib().glowhip_last_error())
    for k, b in bufs.items():
        assert b is None or b.intact(), (c["name"], k, "guard overwritten")
    for k in ("x", "w"):
        assert bufs[k].host(np.uint8).tobytes() == np.ascontiguousarray(x if k == "x" else d["w"]).tobytes(), (c["name"], k, "operand changed")
    return bufs["y"], info, bufs


def assert_route(c, info, rt):
    name = c["name"]
    assert info.launches == rt["launches"] and list(info.grid) == rt["grid"], (name, info.launches, list(info.grid), rt)
    if c["op"] == C.WIDE:
        glds = rt["kernel"] == "k_gemm_glds"
        assert info.kernel == (L.CVI_GEMM_GLDS if glds else L.CVI_WIDE) and info.ksize == c["ks"] and info.tile == rt["tile"] and info.splits == rt["S"], (name, rt)
        assert info.image_bytes == rt["image_bytes"]
    elif c["op"] == C.FIRST:
        assert info.kernel == L.CVI_FIRST and info.tile == rt["tile"] and info.mb == rt["MB"] and info.image_bytes == rt["image_bytes"], (name, info.tile, info.mb, rt)
        SEEN.add("k_conv_first MB=%d" % info.mb)
    else:
        assert info.kernel == L.CVI_DIRECT and info.ksize == c["ks"], name
    SEEN.add(rt["kernel"])


def compare(c, d, fam, y, rt):
    """every output element against the fp64 reference, a block of images at a time"""
    N, Cout, HW = c["N"], c["Cout"], c["H"] * c["W"]
    got = y.host(f32).reshape(N, Cout, HW)
    step = max(1, BLOCK // (Cout * HW))
    for n0 in range(0, N, step):
        images = list(range(n0, min(N, n0 + step)))
        ref, bound, A = C.reference(c, d, images, rt.get("S", 1))
        g = got[images]
        if fam == "exact":
            C.check_exact(c, d, A)
            differ = int((g.astype(f64) != ref).sum())
            EXACT[0] += g.size
            EXACT[1] += differ
            assert differ == 0, (c["name"], rt["kernel"], differ, "of", g.size, "values differ from the fp64 reference; first at", np.argwhere(g.astype(f64) != ref)[0])
        else:
            w = C.worst(g, ref, bound)
            WORST[rt["kernel"]] = max(WORST.get(rt["kernel"], 0.0), w)
            assert C.inside(g, ref, bound), (c["name"], rt["kernel"], int((~(np.abs(g.astype(f64) - ref) <= bound)).sum()), "elements outside the bound; worst multiple", w)
    return got


def run_case(c):
    rt = C.route(c)
    for fam in c["families"]:
        d = C.build(c, fam)
        y, info, bufs = launch(c, d)
        assert_route(c, info, rt)
        y2, _, _ = launch(c, d)
        assert torch.equal(y.raw, y2.raw), (c["name"], fam, "two runs differ")
        del y2
        if "scratch" in bufs and rt["S"] == 1:
            assert bufs["scratch"].untouched(), (c["name"], "scratch written without split-K")
        got = compare(c, d, fam, y, rt)
        print(f"{c['name']} [{fam}] {rt['kernel']}: worst multiple of the bound so far {WORST.get(rt['kernel'], 0.0):.3f}")
        if rt.get("S", 1) > 1:                               # the same operands in one launch
            y1, info1, _ = launch(c, d, scratch=None)
            assert info1.splits == 1 and info1.launches == 1
            one = y1.host(f32).reshape(got.shape)
            if fam == "exact":
                assert one.tobytes() == got.tobytes(), (c["name"], "split-K and one launch differ on an exact set")
            else:
                ref, b_s, _ = C.reference(c, d, None, rt["S"])
                _, b_1, _ = C.reference(c, d, None, 1)
                assert C.inside(one, ref, b_1) and np.all(np.abs(one.astype(f64) - got) <= b_s + b_1), (c["name"], "split-K and one launch apart")
        if c.get("xwide"):                                   # NaN behind every sample's channels: never read
            assert np.isfinite(got).all(), c["name"]
            yc, _, _ = launch(c, d, xwide=False)
            assert torch.equal(y.raw, yc.raw), (c["name"], fam, "strided and contiguous input differ")


WIDE_CASES, FIRST_CASES, DIRECT_CASES = C.wide_cases(), C.first_cases(), C.direct_cases()
ids = lambda cases: [c["name"] for c in cases]


@pytest.mark.parametrize("c", WIDE_CASES, ids=ids(WIDE_CASES))
def test_wide_equals_fp64(c):
    run_case(c)


@pytest.mark.parametrize("c", FIRST_CASES, ids=ids(FIRST_CASES))
def test_first_equals_fp64(c):
    run_case(c)


@pytest.mark.parametrize("c", DIRECT_CASES, ids=ids(DIRECT_CASES))
def test_direct_equals_fp64(c):
    run_case(c)


def test_direct_scale_wins_over_logs():
    """post_scale and post_logs both given: the table is used, value for value what the scale alone gives"""
    c = next(c for c in DIRECT_CASES if c["epi"] == "scale+logs" and c["ks"] == 3 and c["H"] > 1 and "random" in c["families"])
    d = C.build(c, "random")
    y, _, _ = launch(c, d)
    d2 = dict(d, post_logs=None)
    y2, _, _ = launch(c, d2)
    assert torch.equal(y.raw, y2.raw)


REFUSALS = C.wide_refusals() + C.first_refusals() + C.direct_refusals()


@pytest.mark.parametrize("c", REFUSALS, ids=["refuse-%s%d-Cin%d-Cout%d-%dx%d%s" % (c["op"], c["ks"], c["Cin"], c["Cout"], c["H"], c["W"], "-T" if c.get("transposed") else "")
                                             for c in REFUSALS])
def test_refused_shapes_launch_nothing(c):
    N, Cin, Cout, HW = c["N"], c["Cin"], c["Cout"], c["H"] * c["W"]
    x, w, y, image = Buf(N * Cin * HW * 4), Buf(Cin * Cout * 25 * 4), Buf(N * Cout * HW * 4), Buf(1 << 20)
    p = L.ConvProbe()
    p.op, p.N, p.Cin, p.H, p.W, p.Cout, p.ksize, p.relu, p.transposed = OPS[c["op"]], N, Cin, c["H"], c["W"], Cout, c["ks"], 1, int(c.get("transposed", 0))
    p.x_bs, p.x, p.w, p.y, p.image = Cin * HW, x.ptr, w.ptr, y.ptr, image.ptr
    rc, info = call(p)
    assert rc == EINVAL and info.kernel == 0 and info.launches == 0 and L.lib().glowhip_last_error()
    assert x.untouched() and w.untouched() and y.untouched() and image.untouched()
    p.image = None
    assert call(p)[0] == EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# the tail convolution: every mode x forced tile x out-channel split, both kernels, ragged channels, strided z2, hout, the term
# ---------------------------------------------------------------------------------------------------------------------
TAIL_CASES = C.tail_cases()


def launch_tail(c, d, hout=None):
    """one launch of tail case c under its switches; returns ({output: numpy}, info, z2_out Buf)"""
    N, Cin, Cout, H, W, mode = c["N"], c["Cin"], c["Cout"], c["H"], c["W"], c["mode"]
    HW, paired = H * W, c["mode"] in C.PAIRED_MODES
    Cz = Cout // 2 if paired else Cout
    hout = c["hout"] if hout is None else hout
    rt = C.tail_route(c)
    p = L.ConvProbe()
    p.op, p.N, p.Cin, p.H, p.W, p.Cout, p.ksize, p.mode, p.x_bs = L.CONV_TAIL, N, Cin, H, W, Cout, 3, C.MODES.index(mode), Cin * HW
    wide = 2 if c["z2wide"] else 1
    bufs = dict(x=Buf(data=d["x"]), w=Buf(data=d["w"]), bias=tab(d, "bias"), post_scale=tab(d, "post_scale"))
    if mode != "plain":
        z = d["z2"] if wide == 1 else np.concatenate([d["z2"], np.full_like(d["z2"], np.nan)], axis=1)
        bufs["z2_in"] = Buf(data=z)
        p.z2_in, p.z2_in_bs = bufs["z2_in"].ptr, wide * Cz * HW
    if c["z2out"] or mode != "split_fwd":
        bufs["z2_out"] = Buf(N * wide * Cz * HW * 4)
        p.z2_out, p.z2_out_bs = bufs["z2_out"].ptr, wide * Cz * HW
    if hout:
        bufs["hout"] = Buf(N * Cout * HW * 4)
        p.hout = bufs["hout"].ptr
    if c["zeros"]:
        bufs["zeros"] = Buf(data=np.zeros(16, f32))
        p.zeros = bufs["zeros"].ptr
    want_term = c.get("acc", True) and mode in ("affine_fwd", "affine_rev", "split_fwd")
    if want_term:
        bufs["acc"], bufs["term"] = Buf(16 * N), Buf(4 * N)
        p.acc, p.term = bufs["acc"].ptr, bufs["term"].ptr
    p.x, p.w = bufs["x"].ptr, bufs["w"].ptr
    p.bias, p.post_scale = (bufs["bias"].ptr if bufs["bias"] else None), (bufs["post_scale"].ptr if bufs["post_scale"] else None)
    with L.debug_flags(c["flags"]):
        rc, info = call(p)
        assert rc == 0 and info.image_bytes == rt["image_bytes"] and info.kernel == 0, (c["name"], rc, info.image_bytes, rt)
        bufs["image"] = Buf(rt["image_bytes"])
        p.image = bufs["image"].ptr
        rc, info = call(p)
    assert rc == 0, (c["name"], L.lib().glowhip_last_error())
    for k, b in bufs.items():
        assert b is None or b.intact(), (c["name"], k, "guard overwritten")
    assert bufs["x"].host(np.uint8).tobytes() == d["x"].tobytes() and bufs["w"].host(np.uint8).tobytes() == d["w"].tobytes(), (c["name"], "operand changed")
    got = {}
    if "z2_out" in bufs:
        zo = bufs["z2_out"].host(f32).reshape(N, wide, Cz * HW)
        assert zo[:, 1:].tobytes() == b"\xa5" * (zo[:, 1:].size * 4), (c["name"], "the gap of the wider z2_out was written")
        got["z2_out"] = zo[:, 0].reshape(N, Cz, HW).copy()
    if hout:
        got["hout"] = bufs["hout"].host(f32).reshape(N, Cout, HW)
    if want_term:
        got["term"] = bufs["term"].host(f32)
    return got, info, rt


def assert_tail_route(c, info, rt):
    assert info.kernel == (L.CVI_TAIL_DMA if rt["dma"] else L.CVI_TAIL) and info.tile == rt["tile"] and info.mb == rt["MT"] and info.splits == rt["WK"], (c["name"], rt)
    assert list(info.grid) == rt["grid"] and info.paired == rt["paired"] and info.launches == 1 and info.image_bytes == rt["image_bytes"], (c["name"], list(info.grid), rt)
    SEEN.add(rt["kernel"])


def compare_tail(c, fam, got, ref, rt):
    assert sorted(got) == sorted(C.tail_outputs(c)), (c["name"], sorted(got))
    for k in got:
        r, b = ref[k]
        g = got[k].reshape(r.shape)
        if fam == "exact" and k in C.tail_exact_outputs(c):
            differ = int((g.astype(f64) != r).sum())
            EXACT[0] += g.size
            EXACT[1] += differ
            assert differ == 0, (c["name"], rt["kernel"], k, differ, "of", g.size, "values differ from the fp64 reference")
        else:
            key = "%s %s %s" % (rt["kernel"].split("<")[0], c["mode"], k)
            w = C.worst(g, r, b)
            if fam == "random":
                WORST[key] = max(WORST.get(key, 0.0), w)
            assert C.inside(g, r, b), (c["name"], fam, rt["kernel"], k, int((~(np.abs(g.astype(f64) - r) <= b)).sum()), "elements outside the bound; worst multiple", w)


@pytest.mark.parametrize("c", TAIL_CASES, ids=ids(TAIL_CASES))
def test_tail_equals_fp64(c):
    for fam in c["families"]:
        d = C.build_tail(c, fam)
        got, info, rt = launch_tail(c, d)
        assert_tail_route(c, info, rt)
        again, _, _ = launch_tail(c, d)
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (c["name"], fam, k, "two runs differ")
        compare_tail(c, fam, got, C.tail_reference(c, d, rt), rt)
        if c["hout"]:                                        # the tape output changes nothing else
            bare, _, _ = launch_tail(c, d, hout=False)
            for k in bare:
                assert got[k].tobytes() == bare[k].tobytes(), (c["name"], fam, k, "differs without hout")


@pytest.mark.parametrize("tp", (16, 64))
def test_tail_dma_and_register_kernels_agree(tp):
    """the same operands with the zero block (LDS-DMA kernel), without it and under GLOWHIP_DBG_TAIL_NO_DMA (register-staged kernel both
    times: the same bytes).  The two kernels walk the channels in different orders (chunks of 16 against chunks of 32, tap-major inside a
    chunk), so between them the exact set must agree to the byte and the random set inside the two bounds added."""
    plain, dma, nodma = [c for c in TAIL_CASES if c.get("twin") and c["flags"] & 0xff == tp]
    assert not plain["zeros"] and dma["zeros"] and not dma["flags"] & C.DBG_NO_DMA and nodma["flags"] & C.DBG_NO_DMA
    for fam in ("exact", "random"):
        d = C.build_tail(plain, fam)
        assert all(C.build_tail(c, fam)["x"].tobytes() == d["x"].tobytes() for c in (dma, nodma))
        a, ia, ra = launch_tail(plain, d)
        b, ib, rb = launch_tail(dma, d)
        e, ie, re_ = launch_tail(nodma, d)
        assert ia.kernel == L.CVI_TAIL and ib.kernel == L.CVI_TAIL_DMA and ie.kernel == L.CVI_TAIL and ia.tile == ib.tile == ie.tile == tp
        ref = C.tail_reference(plain, d, ra)
        for k in a:
            assert a[k].tobytes() == e[k].tobytes(), (fam, k, "the register kernel differs under NO_DMA")
            if fam == "exact" and k == "hout":
                assert a[k].tobytes() == b[k].tobytes(), (fam, k)
            assert np.all(np.abs(a[k].astype(f64) - b[k].reshape(a[k].shape)) <= 2 * ref[k][1].reshape(a[k].shape)), (fam, k, "the two kernels are apart")


TAIL_REFUSALS = C.tail_refusals()


@pytest.mark.parametrize("c", TAIL_REFUSALS, ids=["refuse-tail-%s-Cin%d-Cout%d-%dx%d-f%x%s" % (c["mode"], c["Cin"], c["Cout"], c["H"], c["W"], c["flags"], "-zeros" if c["zeros"] else "")
                                                  for c in TAIL_REFUSALS])
def test_tail_refused_shapes_launch_nothing(c):
    N, Cin, Cout, HW = c["N"], c["Cin"], c["Cout"], c["H"] * c["W"]
    bufs = [Buf(N * Cin * HW * 4), Buf(Cin * Cout * 9 * 4), Buf(N * Cout * HW * 4), Buf(N * Cout * HW * 4), Buf(1 << 20), Buf(N * Cout * HW * 4)]
    zeros = Buf(data=np.zeros(16, f32))
    p = L.ConvProbe()
    p.op, p.N, p.Cin, p.H, p.W, p.Cout, p.ksize, p.mode, p.x_bs = L.CONV_TAIL, N, Cin, c["H"], c["W"], Cout, 3, C.MODES.index(c["mode"]), Cin * HW
    p.x, p.w, p.z2_in, p.z2_out, p.image, p.hout = [b.ptr for b in bufs]
    p.z2_in_bs = p.z2_out_bs = Cout * HW
    p.zeros = zeros.ptr if c["zeros"] else None
    with L.debug_flags(c["flags"]):
        rc, info = call(p)
    assert rc == EINVAL and info.kernel == 0 and L.lib().glowhip_last_error()
    assert all(b.untouched() for b in bufs), "a refused call wrote something"


def test_zz_report_instances_and_worst_multiples():
    for k in sorted(WORST):
        print(f"worst multiple of the bound: {k:36s} {WORST[k]:.3f}")
    print(f"`exact` sets: {EXACT[0]} values compared, {EXACT[1]} differing; instances seen: {sorted(SEEN)}")
    missing = (set(C.EXPECTED_INSTANCES) | set(C.tail_expected_instances())) - SEEN
    assert not missing, ("instances never launched", sorted(missing))
    assert EXACT[0] > 0 and EXACT[1] == 0
