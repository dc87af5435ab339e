"""The split-half MFMA kernels of the coupling network, each instance on its own: k_cnet<HID, MS, UPW, PXT, NG, MODE> (csrc/cnet_sh.hip)
and k_cnet1w (csrc/cnet1w_sh.hip) in their forward / inverse (MODE 0) and taping (MODE 1) forms, and the three SH2 weight images of
csrc/pack.hip they read (REPACK_SH2_FIRST / _GEMM / _TAIL; plain, k-permuted, from a transposed copy, with ActNorm folded in),
launched through the testing hook glowhip_debug_sh2 -- which fills the RepackJob / CnetArgs fields the plan fills and calls the
pack code and the launcher the plan calls -- on operands laid out here, against the fp64 reference of tests/sh2_oracle.py on EVERY
output element:

  * `exact-w` / `exact-a` input sets (the arithmetic csrc/sh.h promises is the true sum; tests/test_sh2_oracle_host.py asserts the
    conditions): the partial sums, gathered as the finishing kernel gathers them, the fp16 tape and every sign bit (exact zeros
    included: the expected bit is h > 0) must equal the reference value for value.  This is what sees a lost cross product;
  * `random` input sets: every element within the bound derived in sh2_oracle from sh.h, no outliers; a sign bit is compared where
    the reference pre-activation is farther from zero than its bound (the rest: below 0.1 %, asserted on the host);
  * images without a fold bit for bit against the layout written out in numpy; with a fold, decoded, within 3 u |w'| plus the split's
    own error of the fp64 w e^{3 logs}; padding rows, groups and k exactly zero.

Every launch: every operand and output sits between 0xA5 guards, the strided input's gaps hold 0xA5, all intact afterwards; the
scratch is sized as the plan sizes it and pre-filled with NaN, tape and masks with 0xFF: every slot the layout assigns is written,
every other slot (the halo rows no pixel reads, the plan's surplus) is untouched; each case runs twice into fresh buffers, bitwise
equal; the instance, grid and hand-over tiling are asserted from what the launcher reports (glowhip_sh2_info).  k_cnet1w's launches
also run on k_cnet (NO_CNET1W / NO_CNET1W_BWD): on the exact sets hpart, g_u and sign words of the two agree bit for bit; the halo
slots hup / hdn (k_cnet1w adds a halo row's three taps to one another, k_cnet adds them to a +0) and the fp16 tape agree but for the sign
of a zero.  The last test fails if an instantiated
forward or taping instance, or an image kind in one of its forms, was never seen.

Backward launches (MODE 2: all twelve GH_CNT instances and k_cnet1w's) run the same way: the sign words are laid out by the oracle
(random bits, all-ones and all-zeros words) and must come back unchanged, g_u2 / g_u0 (fp32) and the partial sums are held to the
masked reference on the flipped, transposed weights.  Taping and backward launches also run at half and twice the in_scale /
out_scale csrc/plan_train.hip derives.  k_dn_gemm's three instances run through DN_MIX and DN_NET with each of their epilogues.

The six k_cnet<*, *, 2, 64> instances could not be launched (two T units per wave need NU4 * KS > 8; a 64-pixel tile's unit holds
two row tiles, so NU4 <= 8 and KS = 1 from NU4 = 5 on): the host enumeration through the hook confirms it, and they were removed.

Worst multiple of the bound per route, `random` sets, measured on an MI355X (printed by the last test):
  route                                               h (partial sums gathered)      tape h1        tape h2
  k_cnet<512, *, 1, 128>       mode 0 / mode 1        3.7e-06 .. 6.0e-06 / 6.2e-06   0.87 .. 0.93   0.16 .. 0.21
  k_cnet<512, *, 1, 64>        mode 0 / mode 1        3.3e-06 .. 5.7e-06 / 5.5e-06   0.74 .. 0.92   0.10 .. 0.24
  k_cnet<256, *, 1, 128>       mode 0 / mode 1        5.3e-06 .. 9.1e-06 / 1.3e-05   0.93           0.37
  k_cnet<256, *, 1, 64>        mode 0 / mode 1        5.1e-06 .. 1.4e-05 / 1.2e-05   0.89 .. 0.93   0.25 .. 0.34
  k_cnet<128, *, 1, 128 / 64>  mode 0 / mode 1        1.1e-05 .. 2.8e-05 / 1.7e-05   0.71 .. 0.86   0.20 .. 0.37
  k_cnet<64, 1, 1 / 2, 128>    mode 0                 5.9e-05 / 2.3e-05
  k_cnet<*, *, 2, 128>         mode 0 (Cout = 48)     2.6e-06 .. 1.0e-05
  k_cnet<*, *, 1, 64, 2>       mode 0 (Cout = 96)     1.4e-06 .. 4.3e-06
  k_cnet1w<512, 10, 4>         mode 0 / mode 1        5.6e-06 / 5.6e-06              0.93           0.22
  images with a fold (decoded against fp64 w e^{3 logs}): 0.90 at worst; without: bit for bit
  `exact` sets: 6 597 120 values compared, none differing.  Run time of this file: 27 s (99 tests; two thirds of it is the fp64
  reference on the host).
(h: the bound is the worst case of 3 K fp32 additions, K up to 4608, so a kernel that sums in fp32 with round to nearest uses 1e-5 of
it -- the `random` sets see layout and operand faults, the `exact` sets the arithmetic.  The fp16 tape is one rounding of the bound's
2^-11 |v|: it sits just below 1 as it must.)"""
import ctypes
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib  # noqa: E402

import sh2_oracle as S  # noqa: E402

DEV = "cuda:0"
GUARD = 4096
EINVAL = -1
WORST = {}
EXACT = [0, 0]
SEEN_INST, SEEN_IMAGE = set(), set()
TWIN = {}
T0 = time.time()
f16, f32, f64 = np.float16, np.float32, np.float64
L = _lib
CASES = S.cnet_cases()


class Buf:
    """`nbytes` of device memory between two 0xA5 guards; the payload holds `fill` bytes unless `data` (numpy) is given"""

    def __init__(self, nbytes=0, data=None, fill=0xA5):
        if data is not None:
            data = np.ascontiguousarray(data)
            nbytes = data.nbytes
        self.nbytes = nbytes
        self.raw = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        if data is not None and nbytes:
            self.raw[GUARD:GUARD + nbytes] = torch.from_numpy(data.view(np.uint8).reshape(-1)).to(DEV)
        elif fill != 0xA5:
            self.raw[GUARD:GUARD + nbytes] = fill
        self.ptr = self.raw.data_ptr() + GUARD
        assert (self.raw.data_ptr() & 255) == 0

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())

    def host(self, dtype=np.uint8):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).copy()


class Strided:
    """(N, per) fp32 rows at a batch stride of `bs` floats between guards; the gaps hold 0xA5 and must keep it"""

    def __init__(self, N, per, bs, data):
        self.N, self.per, self.bs = N, per, bs
        h = np.full(N * bs, np.frombuffer(b"\xa5" * 4, f32)[0], f32)
        for n in range(N):
            h[n * bs:n * bs + per] = np.asarray(data[n], f32).reshape(-1)
        self.src = h
        self.buf = Buf(data=h)
        self.ptr = self.buf.ptr

    def intact(self):
        return self.buf.intact() and self.buf.host(f32).tobytes() == self.src.tobytes()


def call(probe):
    info = L.Sh2Info()
    rc = L.lib().glowhip_debug_sh2(ctypes.byref(probe), ctypes.byref(info), L.stream_ptr(DEV))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this run
        pytest.exit(f"device error after glowhip_debug_sh2: {e}", returncode=3)
    return rc, info


def pack(kind, w, kperm=False, fold_bias=None, fold_logs=None, transposed=False):
    """one image through the hook -> (Buf holding it, info); the image buffer starts as 0xA5"""
    w = np.ascontiguousarray(w, f32)
    Cout, Cin = (w.shape[1], w.shape[0]) if transposed else w.shape[:2]
    p = L.Sh2Probe()
    p.op, p.kind, p.Cin, p.Cout, p.kperm, p.transposed = L.SH2_IMAGE, kind, Cin, Cout, int(kperm), int(transposed)
    rc, info = call(p)
    assert rc == 0, L.lib().glowhip_last_error()
    wb, img = Buf(data=w), Buf(info.image_bytes)
    fb = Buf(data=fold_bias) if fold_bias is not None else None
    fl = Buf(data=fold_logs) if fold_logs is not None else None
    flip = Buf(w.nbytes) if transposed else None
    p.w, p.image, p.fold_bias, p.fold_logs, p.flip = wb.ptr, img.ptr, fb.ptr if fb else None, fl.ptr if fl else None, flip.ptr if flip else None
    rc, info = call(p)
    assert rc == 0, L.lib().glowhip_last_error()
    assert all(b.intact() for b in (wb, img, fb, fl, flip) if b is not None), "a guard of the image launch was written"
    assert wb.host(f32).tobytes() == w.tobytes(), "the weight was written"
    if transposed:
        assert flip.host(f32).tobytes() == S.flip_t(w).tobytes(), "the transposed copy"
    return img, info


def ids(cases):
    return [c["name"] for c in cases]


def note(route, w):
    WORST[route] = max(WORST.get(route, 0.0), w)


# ---------------------------------------------------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.IMAGE_CASES, ids=["%s %dx%d %s" % ({3: "gemm", 4: "first", 5: "tail"}[c["kind"]], c["Cout"], c["Cin"], c["form"]) for c in S.IMAGE_CASES])
def test_image_equals_the_layout(c):
    w, fb, fl, kperm, tr = S.image_operands(c)
    img, info = pack(c["kind"], w, kperm, fb, fl, tr)
    again, _ = pack(c["kind"], w, kperm, fb, fl, tr)
    got = img.host().tobytes()
    assert got == again.host().tobytes(), "two runs differ"
    ref = S.image_ref(c["kind"], w, kperm, fb, fl, tr)
    assert (info.Kp, info.M, info.image_bytes) == (ref["Kp"], ref["M"], len(got))
    worst, pad_zero, in_range = S.image_fold_check(c["kind"], got, w, kperm, fb, fl, tr)
    print(f"image {c}: worst multiple of the bound {worst:.3f}")
    assert pad_zero and in_range and worst <= 1.0, (c, worst, pad_zero, in_range)
    if fl is None:
        assert got == S.image_bytes(ref), (c, "the image differs from the layout written out in numpy")
    else:
        note("image %s folded" % {3: "gemm", 4: "first", 5: "tail"}[c["kind"]], worst)
        # the same fold with logs = 0 multiplies by expf(0) = 1: bit for bit again
        z = np.zeros_like(fl)
        img0, _ = pack(c["kind"], w, kperm, fb, z, tr)
        assert img0.host().tobytes() == S.image_bytes(S.image_ref(c["kind"], w, kperm, fb, z, tr)), (c, "logs = 0")
    for form in c["form"].split("+"):
        SEEN_IMAGE.add((c["kind"], form))


# ---------------------------------------------------------------------------------------------------------------------
# k_cnet / k_cnet1w
# ---------------------------------------------------------------------------------------------------------------------
def cnet_images(c, d):
    ng = S.groups(c["Cout"])
    cg = c["Cout"] // ng
    if c["bwd"]:      # as the plan builds them: from the transposed, flipped copy of the forward weights, the logs alone folded in
        w0, _ = pack(S.FIRST, S.flip_t(d["w0"]), False, None, d["l0"], transposed=True)
        w2, _ = pack(S.GEMM, S.flip_t(d["w2"]), True, None, d["l2"], transposed=True)
        return w0, w2, pack(S.TAIL, S.flip_t(d["w4"]), True, transposed=True)[0]
    w0, _ = pack(S.FIRST, d["w0"], False, d["b0"], d["l0"])
    w2, _ = pack(S.GEMM, d["w2"], True, d["b2"], d["l2"])
    parts = [pack(S.TAIL, d["w4"][g * cg:(g + 1) * cg], True)[0].host() for g in range(ng)]      # one image per group, one after the other
    return w0, w2, Buf(data=np.concatenate(parts))


def run_cnet(c, d, images, expect_rc=0, scratch_floats=None, masks=True, scale=None):
    N, Cin, H, W, hid, Cout = (c[k] for k in ("N", "Cin", "H", "W", "hid", "Cout"))
    HW, P = H * W, N * H * W
    w0, w2, w4 = images
    x = Strided(N, Cin * HW, Cin * HW + c.get("bs_extra", 0), d["z1"])
    plan_floats = S.scratch_floats_plan(N, H, W, Cout)
    scratch = Buf(4 * (plan_floats if scratch_floats is None else scratch_floats), fill=0xFF)
    p = L.Sh2Probe()
    p.op, p.N, p.Cin, p.H, p.W, p.hidden, p.Cout, p.mode = L.SH2_CNET, N, Cin, H, W, hid, Cout, S.AFFINE_FWD if Cout == 2 * Cin else S.ADD_FWD
    p.x, p.x_bs, p.w0, p.w2, p.w4, p.scratch, p.scratch_floats = x.ptr, x.bs, w0.ptr, w2.ptr, w4.ptr, scratch.ptr, scratch.nbytes // 4
    tape, bwd = None, bool(c.get("bwd"))
    if c.get("tape") or bwd:
        # taping: fp16 tape and sign words out; backward: sign words in (laid out by the oracle: the first layer reads mask2), fp32 g_u2 / g_u0 out
        words = [Buf(data=S.mask_encode(d[k])) for k in ("mk2", "mk1")] if bwd else [Buf(4 * (hid // 32) * P, fill=0xFF) for _ in range(2)]
        tape = [Buf((4 if bwd else 2) * hid * P, fill=0xFF), Buf((4 if bwd else 2) * hid * P, fill=0xFF)] + words
        p.tape_h1, p.tape_h2, p.bwd = tape[0].ptr, tape[1].ptr, int(bwd)
        if masks:
            p.mask1, p.mask2 = tape[2].ptr, tape[3].ptr
        p.in_scale, p.out_scale = scale or S.scales(c)[0]
    with L.debug_flags(c.get("flags", 0)):
        rc, info = call(p)
    assert rc == expect_rc, (c["name"], rc, L.lib().glowhip_last_error())
    assert x.intact() and all(b.intact() for b in (w0, w2, w4, scratch) + tuple(tape or ())), (c["name"], "a guard, a gap or an input was written")
    if rc:
        assert (scratch.host() == 0xFF).all() and all((b.host() == 0xFF).all() for b in tape or ()), (c["name"], "a refused launch wrote")
        return None, info
    res = dict(scratch=scratch.host(f32))
    if tape:
        res.update(tape1=tape[0].host(f32 if bwd else f16), tape2=tape[1].host(f32 if bwd else f16), mask1=tape[2].host(np.uint16), mask2=tape[3].host(np.uint16))
    if bwd:
        assert res["mask1"].tobytes() == S.mask_encode(d["mk2"]).tobytes() and res["mask2"].tobytes() == S.mask_encode(d["mk1"]).tobytes(), "the backward wrote its sign words"
    return res, info


def compare(route, name, fam, key, got, ref, bound):
    got = np.asarray(got).reshape(ref.shape)
    if fam != "random":
        differ = int((got.astype(f64) != ref).sum())
        EXACT[0] += got.size
        EXACT[1] += differ
        assert differ == 0, (name, fam, key, differ, "of", got.size, "values differ from the fp64 reference")
        return
    err = np.abs(got.astype(f64) - ref)
    w = float(np.max(err / bound))
    print(f"{name} [{fam}] {key}: worst multiple of the bound {w:.2e}")
    note(route + " " + key, w)
    assert np.isfinite(got).all() and (err <= bound).all(), (name, key, "elements outside the bound; worst multiple", w)


def twins_agree(g, a, b, k):
    """k_cnet and k_cnet1w on the same exact set: bit for bit (hpart, g_u, sign words) -- except the sign of a zero in the fp16 tape and,
    in the scratch, in the halo slots hup / hdn alone: k_cnet1w adds a halo row's three taps to one another, k_cnet adds them to a +0, so where all three are -0 (a zero T value
    times the negative row scale) one stores -0 and the other +0"""
    if k == "scratch":
        ua, ub = a.view(np.uint32).copy(), b.view(np.uint32).copy()
        halo = np.zeros(ua.size, bool)
        halo[g["MS"] * g["N"] * g["Cout"] * g["HW"]:g["floats"]] = True
        for u in (ua, ub):
            u[halo & (u == 0x80000000)] = 0
        return bool((ua == ub).all())
    if a.dtype == f16:      # the fp16 tape: the two store a zero activation with either sign (equal values; the cause was not traced)
        ua, ub = a.view(np.uint16).copy(), b.view(np.uint16).copy()
        ua[ua == 0x8000] = 0
        ub[ub == 0x8000] = 0
        return bool((ua == ub).all())
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_cnet_equals_fp64(c):
    N, H, W, hid, Cout = (c[k] for k in ("N", "H", "W", "hid", "Cout"))
    P = N * H * W
    route = "%s<%s>" % ("k_cnet1w" if c["inst"][0] == S.K_CNET1W else "k_cnet", ",".join(str(v) for v in c["inst"][1:]))
    runs = [(fam, None) for fam in S.FAMILIES]
    if c["tape"] or c["bwd"]:                # the neighbouring powers of two of in_scale / out_scale (the host test holds these sets to the exact conditions)
        runs += [(fam, sc) for sc in S.scales(c)[1:] for fam in S.FAMILIES]
    for fam, scale in runs:
        d = S.build(c, fam)
        images = cnet_images(c, d)
        in_scale, out_scale = scale or S.scales(c)[0]
        fed = S.scaled(d, in_scale) if scale else d          # z1 * 16 / in_scale: the window holds the same values at every in_scale
        got, info = run_cnet(c, fed, images, scale=scale)
        again, _ = run_cnet(c, fed, images, scale=scale)
        stored = 16.0 * out_scale            # a stored tensor is the activation at the SH2 scale times out_scale
        inst = (info.kernel, info.hid, info.ms, info.upw, info.pxt, info.ng, info.mode)
        assert inst == c["inst"], (c["name"], inst)
        SEEN_INST.add(inst)
        g = S.add_geometry(N, H, W, info.R, info.NI, info.MS, Cout)
        assert (info.tiles, info.lpxt, info.grid[0], info.scratch_floats) == (g["tiles"], g["lpxt"], g["tiles"], S.scratch_floats_plan(N, H, W, Cout))
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (c["name"], fam, k, "two runs differ")
        # every slot the layout assigns is written, every other one still holds the pre-fill
        sc = got["scratch"]
        used = np.ones(g["floats"], bool)
        _, hup, hdn = S.split_scratch(g, used)
        up, dn = S.unused_halo_mask(g)
        hup[:, up] = False
        hdn[:, dn] = False
        raw = sc.view(np.uint32)
        assert not np.isnan(sc[:g["floats"]][used]).any(), (c["name"], fam, "a partial-sum slot was not written")
        assert (raw[:g["floats"]][~used] == 0xFFFFFFFF).all() and (raw[g["floats"]:] == 0xFFFFFFFF).all(), (c["name"], fam, "a slot outside the layout was written")
        ref = S.reference(d)
        layout = np.where(used, sc[:g["floats"]], f32(0))          # (gather_ref reads the unused halo slots of no element; NaN * 0 stays out)
        out = S.gather_ref(g, layout)[0].reshape(N, Cout, H, W)
        compare(route, c["name"], fam, "h (partial sums gathered)", out, ref["out"][0], ref["out"][1])
        if c["bwd"]:
            for k, name in (("1", "g_u2"), ("2", "g_u0")):
                v, e = S.to_px(ref["h" + k][0]) * stored, S.to_px(ref["h" + k][1]) * stored
                assert not np.isnan(got["tape" + k]).any(), (c["name"], fam, name, "a slot was not written")
                compare(route, c["name"], fam, name + " (fp32)", S.tape_decode(got["tape" + k], hid, P), v, e + 2.0 ** -24 * np.abs(v))
        if c["tape"]:
            for k in ("1", "2"):
                v, e = S.to_px(ref["h" + k][0]) * stored, S.to_px(ref["h" + k][1]) * stored
                tp = S.tape_decode(got["tape" + k], hid, P)
                compare(route, c["name"], fam, "tape h" + k, tp, v.astype(f16).astype(f64) if fam != "random" else v, S.tape_bound(v, e))
                t, tb = S.to_px(ref["t" + k][0]), S.to_px(ref["t" + k][1])
                sure = np.ones(t.shape, bool) if fam != "random" else np.abs(t) > tb
                assert sure.mean() >= 0.999, (c["name"], fam, "more than 0.1 % of the sign bits left out")
                bits = S.mask_decode(got["mask" + k], hid, P)
                wrong = int((bits != (t > 0))[sure].sum())
                assert wrong == 0, (c["name"], fam, "sign words of h" + k, wrong, "bits differ from h > 0")
        if c.get("twin") and fam != "random" and scale is None:
            key = (N, H, W, c["Cin"], Cout, hid, c["tape"], c["bwd"], fam)
            if key in TWIN:
                for k in got:
                    assert twins_agree(g, TWIN[key][k], got[k], k), (c["name"], fam, k, "k_cnet and k_cnet1w differ on an exact set")
            TWIN[key] = got


def gathered(c, got, info):
    g = S.add_geometry(c["N"], c["H"], c["W"], info.R, info.NI, info.MS, c["Cout"])
    used = np.ones(g["floats"], bool)
    _, hup, hdn = S.split_scratch(g, used)
    up, dn = S.unused_halo_mask(g)
    hup[:, up] = False
    hdn[:, dn] = False
    return S.gather_ref(g, np.where(used, got["scratch"][:g["floats"]], f32(0)))[0].reshape(c["N"], c["Cout"], c["H"], c["W"])


NONFINITE = [c for c in CASES if c["inst"] in ((S.K_CNET, 128, 1, 1, 128, 1, 0), (S.K_CNET, 256, 4, 1, 128, 1, 0))]      # 16x16 (NI = 1) and 3x8x8 (NI = 2)


@pytest.mark.parametrize("c", NONFINITE, ids=ids(NONFINITE))
@pytest.mark.parametrize("bad", (float("nan"), 5000.0), ids=("nan", "5000"))
def test_a_non_finite_pixel_stays_in_its_footprint(c, bad):
    """one bad value at one pixel of one channel of z1, every weight non-zero: the partial sums are touched on that pixel's 5x5
    neighbourhood clipped to its own image and nowhere else (the other image sharing the tile included).  NaN: NaN exactly there.
    5000 (above the SH2 activation range 4094: its hi part is inf): non-finite there, or the value the reference gives -- never a
    finite value outside the bound."""
    N, H, W = c["N"], c["H"], c["W"]
    d = S.build(c, "random")
    assert all(d[k].all() for k in ("w0", "w2", "w4"))
    n0, y0, x0 = 0, H - 2, 1
    clean = dict(d, z1=d["z1"].copy())
    clean["z1"][n0, 2, y0, x0] = 0.0 if bad != bad else bad
    ref = S.reference(clean)["out"]
    d["z1"] = d["z1"].copy()
    d["z1"][n0, 2, y0, x0] = bad
    got, info = run_cnet(c, d, cnet_images(c, d))
    assert (info.NI == 2) == (H * W == 64)
    out = gathered(c, got, info)
    foot = np.zeros((N, 1, H, W), bool)
    foot[n0, :, max(y0 - 2, 0):y0 + 3, max(x0 - 2, 0):x0 + 3] = True
    foot = np.broadcast_to(foot, out.shape)
    inside = np.abs(out - ref[0]) <= ref[1]
    assert inside[~foot].all(), (c["name"], "a value outside the footprint left the bound", int((~inside[~foot]).sum()))
    if bad != bad:
        assert np.isnan(out[foot]).all(), (c["name"], "the footprint is not NaN throughout", int((~np.isnan(out[foot])).sum()))
    else:
        assert (~np.isfinite(out[foot]) | inside[foot]).all(), (c["name"], "a finite value outside the bound")
        assert (~np.isfinite(out[foot])).any()


@pytest.mark.parametrize("c", S.REFUSALS, ids=ids(S.REFUSALS))
def test_refusals(c):
    cc = dict(c, tape=bool(c.get("tape_no_masks") or c.get("tape_with_masks")), flags=0, bwd=False)
    r = S.rng_of("refusal", c["name"])
    d = dict(z1=r.standard_normal((c["N"], c["Cin"], c["H"], c["W"])).astype(f32))
    images = tuple(Buf(1 << 20, fill=0) for _ in range(3))          # (never read: the launch is refused before any operand is looked at)
    short = S.scratch_floats_plan(c["N"], c["H"], c["W"], c["Cout"]) - 1 if c.get("short_scratch") else None
    run_cnet(cc, d, images, expect_rc=EINVAL, scratch_floats=short, masks=not c.get("tape_no_masks"))


# ---------------------------------------------------------------------------------------------------------------------
# k_dn_gemm: the deep levels' MIX and F0 -> F2 -> F4
# ---------------------------------------------------------------------------------------------------------------------
SEEN_DN = set()


def dn_probe(op, c, hid, Cout):
    p = L.Sh2Probe()
    p.op, p.N, p.Cin, p.H, p.W, p.hidden, p.Cout = op, c["N"], c["C"], c["H"], c["W"], hid, Cout
    return p


def dn_seen(info, k, epi, M, P):
    inst, grid = S.dn_instance(M, P)
    assert (info.dn_rt[k], info.dn_pt[k], info.dn_npf[k]) == inst and tuple(info.dn_grid[3 * k:3 * k + 2]) == grid, (k, epi, inst, list(info.dn_grid))
    SEEN_DN.add((inst, epi))


@pytest.mark.parametrize("c", S.DN_MIX_CASES, ids=ids(S.DN_MIX_CASES))
def test_dn_mix_equals_fp64(c):
    C, N, H, W = c["C"], c["N"], c["H"], c["W"]
    HW, P, hid = H * W, N * H * W, 32
    lay = S.dn_carve(N, C, H, W, hid, C)
    route = "k_dn_gemm<8,%d,%d,%d> mix%s" % (S.dn_instance(C, P)[0] + (" reverse" if c["reverse"] else "",))
    for fam in S.FAMILIES:
        d = S.build_mix(c, fam)
        img, _ = pack(S.GEMM, d["w"])
        outs = []
        for _ in range(2):
            host = np.full(lay["bytes"], 0xFF, np.uint8)
            host[lay["u"]:lay["u"] + 4 * C * P] = S.sh2_planes(d["v"] * f32(16), P, np.arange(P)).reshape(-1).view(np.uint8)
            scratch = Buf(data=host)
            state = Buf(4 * N * (C * HW + 8))
            ps, pb = (Buf(data=d["ps"]), Buf(data=d["pb"])) if c["reverse"] else (None, None)
            p = dn_probe(L.SH2_DN_MIX, c, hid, C)
            rc, info = call(p)
            assert rc == 0 and (info.part_off, info.scratch_bytes) == (lay["part"], lay["bytes"]), (L.lib().glowhip_last_error(), info.part_off, info.scratch_bytes)
            p.w0, p.state, p.x_bs, p.dn_scratch, p.want_pad = img.ptr, state.ptr, C * HW + 8, scratch.ptr, c["want_pad"]
            p.post_scale, p.post_bias = (ps.ptr, pb.ptr) if ps else (None, None)
            rc, info = call(p)
            assert rc == 0, L.lib().glowhip_last_error()
            assert all(b.intact() for b in (img, scratch, state, ps, pb) if b is not None)
            assert info.dn_launches == 1
            dn_seen(info, 0, "mix", C, P)
            outs.append((state.host(f32).reshape(N, C * HW + 8), scratch.host()))
        (st, sc), (st2, sc2) = outs
        assert st.tobytes() == st2.tobytes() and sc.tobytes() == sc2.tobytes(), (c["name"], fam, "two runs differ")
        assert (st[:, C * HW:].view(np.uint32) == 0xA5A5A5A5).all(), "the gap of the strided state was written"
        got = st[:, :C * HW].reshape(N, C, HW).transpose(1, 0, 2).reshape(C, P)
        ref, e = S.mix_ref(c, d)
        compare(route, c["name"], fam, "state", got, ref, e)
        # the level scratch: u as laid, ypad = the split of 16 x the state the kernel itself stored (first C / 2 channels) inside a zero
        # border when want_pad, all zero otherwise (dnet_level_begin), h2pad zero, everything else untouched
        want = np.full(lay["bytes"], 0xFF, np.uint8)
        want[lay["u"]:lay["u"] + 4 * C * P] = S.sh2_planes(d["v"] * f32(16), P, np.arange(P)).reshape(-1).view(np.uint8)
        ypad = np.zeros((2, (C // 2) * lay["SLN"]), np.uint16)
        if c["want_pad"]:
            ypad = S.sh2_planes(got[:C // 2] * f32(16), lay["SLN"], S.pad_slots(N, H, W))
        want[lay["ypad"]:lay["ypad"] + 4 * (C // 2) * lay["SLN"]] = ypad.reshape(-1).view(np.uint8)
        want[lay["h2pad"]:lay["h2pad"] + 4 * hid * lay["SLN"]] = 0
        assert sc.tobytes() == want.tobytes(), (c["name"], fam, "the level scratch: ypad is not the split of the stored state, or something else was written")


@pytest.mark.parametrize("c", S.DN_NET_CASES, ids=ids(S.DN_NET_CASES))
def test_dn_net_equals_fp64(c):
    C, N, H, W, hid, Cout, Ch = c["C"], c["N"], c["H"], c["W"], c["hid"], c["Cout"], c["Cin"]
    HW, P = H * W, N * H * W
    lay = S.dn_carve(N, C, H, W, hid, Cout)
    ks_want = S.dn_ksplit(Cout, P, S.g0(hid) // 2)
    for fam in S.FAMILIES:
        d = S.build(c, fam)
        w0, _ = pack(S.FIRST, d["w0"], False, d["b0"], d["l0"])
        w2, _ = pack(S.GEMM, d["w2"], False, d["b2"], d["l2"])
        w4, _ = pack(S.FIRST, d["w4"])
        outs = []
        for _ in range(2):
            host = np.full(lay["bytes"], 0xFF, np.uint8)
            host[lay["ypad"]:lay["ypad"] + 4 * Ch * lay["SLN"]] = S.sh2_planes(S.to_px(d["z1"]) * f32(16), lay["SLN"], S.pad_slots(N, H, W)).reshape(-1).view(np.uint8)
            host[lay["h2pad"]:lay["h2pad"] + 4 * hid * lay["SLN"]] = 0
            scratch, state = Buf(data=host), Buf(4 * N * C * HW)
            p = dn_probe(L.SH2_DN_NET, c, hid, Cout)
            p.w0, p.w2, p.w4, p.state, p.x_bs, p.dn_scratch = w0.ptr, w2.ptr, w4.ptr, state.ptr, C * HW, scratch.ptr
            rc, info = call(p)
            assert rc == 0, L.lib().glowhip_last_error()
            assert all(b.intact() for b in (w0, w2, w4, scratch, state)) and (state.host() == 0xA5).all()
            assert (info.ks, info.dn_launches, info.part_off) == (ks_want, 3, lay["part"]) and info.dn_grid[8] == ks_want
            for k, (epi, M) in enumerate((("act", hid), ("act", hid), ("partial", Cout))):
                dn_seen(info, k, epi, M, P)
            outs.append((scratch.host(), host))
        assert outs[0][0].tobytes() == outs[1][0].tobytes(), (c["name"], fam, "two runs differ")
        sc, host = outs[0]
        part = sc[lay["part"]:lay["part"] + 4 * S.DN_KS_MAX * Cout * P].view(f32)
        assert not np.isnan(part[:ks_want * Cout * P]).any() and (part[ks_want * Cout * P:].view(np.uint32) == 0xFFFFFFFF).all(), "the copies beyond ks / a slot not written"
        got = part[:ks_want * Cout * P].astype(f64).reshape(ks_want, N, Cout, H, W).sum(axis=0)
        ref = S.reference(d)
        compare("k_dn_gemm F0 -> F2 -> F4", c["name"], fam, "h (ks parts summed)", got, ref["out"][0], ref["out"][1])
        # nothing but h1, the interior of h2pad and `part` was written
        keep = np.ones(lay["bytes"], bool)
        for a, b in ((lay["h1"], lay["h2pad"]), (lay["h2pad"], lay["part"]), (lay["part"], lay["end"])):
            keep[a:b] = False
        assert (sc[keep] == host[keep]).all(), (c["name"], fam, "u / ypad / the tail of the scratch was written")
        h2 = sc[lay["h2pad"]:lay["h2pad"] + 4 * hid * lay["SLN"]].view(np.uint16).reshape(2, hid // 8, lay["SLN"], 8)
        border = np.ones(lay["SLN"], bool)
        border[S.pad_slots(N, H, W)] = False
        assert not h2[:, :, border].any(), (c["name"], fam, "the zero border of h2pad")


def test_every_instance_and_image_form_was_seen():
    want_dn = {(i, e) for i in S.DN_INSTANCES for e in ("mix", "act", "partial")}
    assert SEEN_DN == want_dn, ("k_dn_gemm instance x epilogue never launched on its own in this process", sorted(want_dn - SEEN_DN))
    missing = sorted(set(S.EXPECTED_INSTANCES) - SEEN_INST)
    assert not missing and SEEN_INST <= set(S.EXPECTED_INSTANCES), ("instances never launched on their own IN THIS PROCESS (the tally is this module's: run the whole file, without -k or xdist)", missing, sorted(SEEN_INST - set(S.EXPECTED_INSTANCES)))
    want = {(S.GEMM, f) for f in S.IMAGE_FORMS} | {(S.FIRST, f) for f in ("plain", "transposed", "folded")} | {(S.TAIL, "kperm"), (S.TAIL, "transposed")}
    assert want <= SEEN_IMAGE, ("image forms never built", sorted(want - SEEN_IMAGE))
    assert len(TWIN) == 6, "k_cnet1w's launches were not compared with k_cnet's"
    for k in sorted(WORST):
        print("  %-70s %.2e" % (k, WORST[k]))
    print("  `exact` sets: %d values compared, %d differing.  Run time of this file: %.1f s" % (EXACT[0], EXACT[1], time.time() - T0))
    assert all(w <= 1.0 for w in WORST.values()) and EXACT[1] == 0
