"""The fp32 code every forward, decode and training step runs between the MFMA launches, each kernel on its own: the finishing kernel
of the coupling network (csrc/cnet_sh.hip k_cfinish<PXB, MSV, HALO>, body in csrc/cnet_fin.h), the channel mixer (csrc/pointwise.hip
launch_chanmix: k_chanmix<16>, k_chanmix<64>, k_chanmix_wide sliced and in place) and the deep levels' k_dn_fin / k_dn_prep
(csrc/dnet_sh.hip), launched through the testing hook glowhip_debug_fin -- which derives the tiling with the producer's own code and
calls the launchers the plan calls -- on operands laid out here, against the fp64 reference of tests/fin_oracle.py on EVERY output
element:

  * `exact` input sets (every sum in every order an fp32 number): the kernel must return the reference value for value;
  * `random` input sets (realistic magnitudes, sigmoid arguments in [-6, 6]): every element within the bound derived in fin_oracle
    from the kernel's roundings, no outliers allowed; the per-sample log-det as the exact integer sum of all 1 + ACC_EXTRA rows;
  * bitwise in every family, from the kernel's own fp32 values: a forward gather / pass-through mixer returns fl(fl(x + b) e); the
    SH2 operand k_dn_fin / k_dn_prep write is hi = fp16(v), lo = fp16(v - hi) of v = 16 ActNorm(state).

tests/test_fin_oracle_host.py shows on the CPU that the promised arithmetic lies inside those bounds and that each of a list of
single faults leaves them.

Every launch: every operand and output sits between 0xA5 guards (and the gaps of the strided tensors hold 0xA5), all intact
afterwards; the partial-sum scratch is sized as the plan sizes it and every slot the gather must not use holds NaN; each case runs
twice into fresh buffers, outputs and accumulator words bitwise equal; k_cfinish also runs in block order, same bits (the
accumulator rows differ, their sum does not); the instance (PXB, MSV, HALO, grid, LDS bytes, XCD-affine order or not) and the
mixer's kernel (grid, LDS bytes, staged matrix) are asserted from what the launchers report (glowhip_fin_info).  The last test
fails if one of the 14 k_cfinish instances or one of the four mixer forms was never seen.  (k_cfinish<256, *, false> cannot be
launched -- 256-pixel workgroups need HW % 256 == 0, maps without halo rows have HW <= 128 -- and was removed with this test.)

Worst multiple of the bound per route, `random` sets, measured on an MI355X (printed by the last test):
  route                                     z / y                       other outputs
  k_cfinish<16>  additive, no mixer         0.624
  k_cfinish<16>  additive, matrix           0.398  (reverse 0.284)
  k_cfinish<16>  additive, gather           0.907  (reverse 0.899)      hout 0.383  z2 write-back 0.484
  k_cfinish<16>  additive, pass-through     0.878
  k_cfinish<16>  affine, no mixer           0.445                       hout 0.484  log-det 0.093
  k_cfinish<16>  affine, matrix             0.469  (reverse 0.389)      hout 0.526  z2 write-back 0.358  log-det 0.071 (reverse 0.033)
  k_cfinish<16>  affine, gather             0.847                       log-det 0.022
  k_cfinish<16>  affine, pass-through       0.930                       log-det 0.061
  k_cfinish<64>  additive, no mixer         0.450
  k_cfinish<64>  additive, matrix           0.484  (reverse 0.324)      hout 0.565  z2 write-back 0.671
  k_cfinish<64>  affine, no mixer           0.742                       log-det 0.110
  k_cfinish<64>  affine, matrix             0.457                       log-det 0.027
  k_cfinish<256> additive, matrix           0.451
  k_cfinish<256> affine, no mixer           0.516                       log-det 0.059
  k_chanmix<16>  matrix 0.203 (reverse 0.119, squeezed view 0.074)   gather 0.941 (reverse 0.902)
  k_chanmix<64>  matrix 0.812 (reverse 0.308, squeezed view 0.303)   gather 0.979 (squeezed view 0.809)   pass-through 0.958
  k_chanmix_wide matrix 0.050 (reverse 0.030)                         gather reverse 0.967
  k_dn_fin       additive state 0.893     affine state 0.579  log-det 0.092
  k_dn_prep      hi + lo against fp64: 0.999 forward and reverse (the fp16 subnormal spacing: half of 2^-24 is the bound's floor)
  `exact` sets: 5 905 377 values compared, none differing.  Run time of this file: 2.9 s (166 tests).
(Outputs that are one or two roundings of an exact value sit just below 1 as they must; a matrix chain's bound grows with C, so the
wide kernel uses little of it; the log-det bound is a sum of worst cases over the sample's elements.)"""
import ctypes
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib  # noqa: E402

import fin_oracle as F  # noqa: E402

DEV = "cuda:0"
GUARD = 4096
EINVAL = -1
WORST = {}          # route + output -> worst multiple of the bound seen (reported by the last test)
EXACT = [0, 0]      # exact values compared, differing
SEEN_CFIN, SEEN_MIX = set(), set()
T0 = time.time()
f32, f64 = np.float32, np.float64
L = _lib


class Buf:
    """`nbytes` of device memory between two 0xA5 guards; the payload starts 0xA5 too unless `data` (numpy) is given."""

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


class Strided:
    """(N, per) fp32 rows at a batch stride of `bs` floats between guards; the gaps hold 0xA5 and must keep it"""

    def __init__(self, N, per, bs, data=None, lead=0):
        self.N, self.per, self.bs, self.lead = N, per, bs, lead
        h = np.full(lead + N * bs, np.frombuffer(b"\xa5" * 4, f32)[0], f32)
        if data is not None:
            for n in range(N):
                h[lead + n * bs:lead + n * bs + per] = np.asarray(data[n], f32).reshape(-1)
        self.buf = Buf(data=h)
        self.ptr = self.buf.ptr + 4 * lead

    def rows(self, shape=None):
        h = self.buf.host(f32)
        r = np.stack([h[self.lead + n * self.bs:self.lead + n * self.bs + self.per] for n in range(self.N)])
        return r if shape is None else r.reshape(shape)

    def intact(self, written=True):
        """guards and gaps; written = False: the rows still hold 0xA5 too"""
        h = self.buf.host(np.uint8).reshape(-1, 4)
        keep = np.ones(h.shape[0], bool)
        if written:
            for n in range(self.N):
                keep[self.lead + n * self.bs:self.lead + n * self.bs + self.per] = False
        return self.buf.intact() and bool((h[keep] == 0xA5).all())


def call(probe):
    info = L.FinInfo()
    rc = L.lib().glowhip_debug_fin(ctypes.byref(probe), ctypes.byref(info), L.stream_ptr(DEV))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this run
        pytest.exit(f"device error after glowhip_debug_fin: {e}", returncode=3)
    return rc, info


def ok(probe):
    rc, info = call(probe)
    assert rc == 0, L.lib().glowhip_last_error()
    return info


def intact(*bufs):
    return all(b.intact() for b in bufs if b is not None)


def compare(route, name, fam, got, ref, key):
    """the assertion of every output: value for value (`exact`) or every element within the bound (`random`); an element whose
    reference is an infinity or NaN (the non-finite sigmoid arguments) must be met exactly"""
    r, b = ref
    got = np.asarray(got).reshape(r.shape)
    if fam == "exact":
        differ = int((got.astype(f64) != r).sum())
        EXACT[0] += got.size
        EXACT[1] += differ
        assert differ == 0, (name, key, route, differ, "of", got.size, "values differ from the fp64 reference")
        return
    fin = np.isfinite(r)
    w = F.worst(got[fin], r[fin], b[fin])
    print(f"{name} [{fam}] {route} {key}: worst multiple of the bound {w:.3f}")
    WORST[route + " " + key] = max(WORST.get(route + " " + key, 0.0), w)
    assert F.inside_nf(got, r, b), (name, key, route, "elements outside the bound; worst multiple", w)


def ids(cases):
    return [c["name"] for c in cases]


def mix_bufs(mix):
    return dict(bias=Buf(data=mix["bias"]) if mix["bias"] is not None else None, scale=Buf(data=mix["scale"]) if mix["scale"] is not None else None,
                matrix=Buf(data=mix["matrix"]) if mix["matrix"] is not None else None, gather=Buf(data=mix["gather"]) if mix["gather"] is not None else None)


def set_mix(p, mb):
    for k in ("bias", "scale", "matrix", "gather"):
        setattr(p, "mix_" + k, mb[k].ptr if mb[k] else None)


def logdet_check(route, name, acc_words, N, ref_ld, fam):
    tot, flagw = F.acc_total(acc_words, N)
    want, b, flags = ref_ld
    assert ((flagw & 7) == flags).all() and ((flagw >> 3) == 0).all(), (name, "flag words", flagw, flags)
    w = float(np.max(np.abs(tot - want) / b))
    print(f"{name} [{fam}] {route} log-det: worst multiple of the bound {w:.3f}")
    WORST[route + " log-det"] = max(WORST.get(route + " log-det", 0.0), w)
    assert (np.abs(tot - want) <= b).all(), (name, "per-sample log-det outside the bound; worst multiple", w)


# ---------------------------------------------------------------------------------------------------------------------
# k_cfinish
# ---------------------------------------------------------------------------------------------------------------------
def run_cfinish(c, d, expect_rc=0):
    N, C, Ch, Cout, HW = c["N"], c["C"], c["Ch"], c["Cout"], c["HW"]
    scratch, bias, scale = Buf(data=d["scratch"]), Buf(data=d["bias"]), Buf(data=d["scale"])
    zin = Strided(N, C * HW, C * HW + 8, data=d["z"])
    zout = zin if c["inplace"] else Strided(N, C * HW, C * HW + 12)
    acc = Buf(data=np.zeros((2 + F.ACC_EXTRA) * N, np.uint64))
    tape = Buf(N * Cout * HW * 4) if c["tape"] else None
    mb = mix_bufs(d["mix"])
    p = L.FinProbe()
    p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden, p.mode, p.MS, p.tile = L.FIN_CFINISH, N, C, c["H"], c["W"], Cout, 128, c["mode"], c["MS"], c["tile"]
    p.scratch, p.scratch_floats, p.bias, p.scale = scratch.ptr, d["scratch"].size, bias.ptr, scale.ptr
    p.z_in, p.z_in_bs, p.z_out, p.z_out_bs, p.acc, p.tape_hout = zin.ptr, zin.bs, zout.ptr, zout.bs, acc.ptr, tape.ptr if tape else None
    if c["mix"] != "none":
        p.mix_C, p.mix_reverse = C, c["reverse"]
        set_mix(p, mb)
    rc, info = call(p)
    assert rc == expect_rc, (rc, L.lib().glowhip_last_error())
    assert intact(scratch, bias, scale, acc, tape, *mb.values()) and zin.intact() and zout.intact(written=rc == 0 or c["inplace"]), c["name"]
    assert scratch.host(f32).tobytes() == d["scratch"].tobytes(), "the partial sums were written"
    if rc:
        assert not acc.host(np.uint64).any() and (tape is None or tape.untouched()) and zin.rows().tobytes() == d["z"].reshape(N, -1).tobytes(), "a refused launch wrote"
        return None, info
    return dict(z_out=zout.rows((N, C, HW)), z_in=zin.rows((N, C, HW)), acc=acc.host(np.uint64), hout=tape.host(f32).reshape(N, Cout, HW) if tape else None), info


@pytest.mark.parametrize("c", F.cfinish_cases(), ids=ids(F.cfinish_cases()))
def test_cfinish_equals_fp64(c):
    N, Ch = c["N"], c["Ch"]
    g = F.cfin_geometry(c)
    for fam in c["families"]:
        d = F.build_cfinish(c, fam)
        got, info = run_cfinish(c, d)
        again, _ = run_cfinish(c, d)
        with L.debug_flags(L.DBG.CFINISH_BLOCK_ORDER):
            block, binfo = run_cfinish(c, d)
        assert (info.kernel, info.pxb, info.msv, info.halo, list(info.grid), info.lds_bytes, info.xcd_affine) == \
            (L.FNI_CFINISH, c["pxb"], c["MS"], c["halo"], [c["grid"], 1, 1], c["lds"], c["affine_order"]), (c["name"], info.pxb, info.msv, info.halo, list(info.grid),
                                                                                                        info.lds_bytes, info.xcd_affine)
        assert (binfo.pxb, binfo.msv, binfo.halo, binfo.xcd_affine) == (c["pxb"], c["MS"], c["halo"], 0), c["name"]
        assert (info.R, info.NI, info.tiles, info.lpxt, info.scratch_floats) == (g["R"], g["NI"], g["tiles"], g["lpxt"], d["scratch"].size), c["name"]
        SEEN_CFIN.add((info.pxb, info.msv, info.halo))
        for k in ("z_out", "z_in", "acc"):
            assert got[k].tobytes() == again[k].tobytes(), (c["name"], fam, k, "two runs differ")
        for k in ("z_out", "z_in"):
            assert got[k].tobytes() == block[k].tobytes(), (c["name"], fam, k, "block order and XCD-affine order differ")
        assert (F.acc_total(got["acc"], N)[0] == F.acc_total(block["acc"], N)[0]).all() and (got["acc"][N:2 * N] == block["acc"][N:2 * N]).all()
        if c["tape"]:
            assert got["hout"].tobytes() == again["hout"].tobytes() == block["hout"].tobytes(), (c["name"], fam, "hout differs between runs")
        ref = F.cfinish_ref(c, d)
        route = "k_cfinish<%d> %s mixer %s%s" % (c["pxb"], "affine" if F.paired(c["mode"]) else "additive", c["mix"], " reverse" if c["reverse"] else "")
        compare(route, c["name"], fam, got["z_out"], ref["z_out"], "z")
        # what must not change: z1 always (read only, or copied along when there is no mixer); z_in altogether unless it is the output
        # or takes the tape's z2 write-back
        z1 = d["z"][:, :Ch]
        zback = None
        if c["inplace"]:
            assert c["mix"] != "none" or got["z_out"][:, :Ch].tobytes() == z1.tobytes(), (c["name"], "z1 changed")
        elif c["tape"]:
            assert got["z_in"][:, :Ch].tobytes() == z1.tobytes(), (c["name"], "z1 changed")
            zback = got["z_in"][:, Ch:]
            compare(route, c["name"], fam, zback, ref["zback"], "z2 write-back")
        else:
            assert got["z_in"].tobytes() == d["z"].tobytes(), (c["name"], "z_in changed")
        if c["mix"] == "none":
            if not c["inplace"]:
                assert got["z_out"][:, :Ch].tobytes() == z1.tobytes(), (c["name"], "z1 did not travel along")
            if c["tape"] and not c["inplace"]:
                assert zback.tobytes() == got["z_out"][:, Ch:].tobytes()
        if c["tape"]:
            compare(route, c["name"], fam, got["hout"], ref["hout"], "hout")
        if "ld" in ref:
            logdet_check(route, c["name"], got["acc"], N, ref["ld"], fam)
            if c["bad"]:
                assert ref["ld"][2][1] != 0 and not ref["ld"][2][[0, 2]].any(), "the case holds its non-finite term in sample 1"
        else:
            assert not got["acc"].any(), (c["name"], "an additive coupling wrote an accumulator")
        # forward gather / pass-through: the stored value is fl(fl(x + b) e) of the selected channel, bit for bit -- for the z2 half
        # from the coupled z2 the kernel itself wrote back, where it did
        if c["mix"] in ("gather", "identity") and not c["reverse"]:
            state = np.concatenate([z1, zback if zback is not None else np.zeros_like(z1)], axis=1)
            want = F.mixer_bitwise(d["mix"], state)
            src = d["mix"]["gather"] if c["mix"] == "gather" else np.arange(c["C"])
            sel = np.ones(c["C"], bool) if zback is not None else src < Ch
            assert got["z_out"][:, sel].tobytes() == want[:, sel].tobytes(), (c["name"], fam, "the gathered value is not fl(fl(x + b) e)")


def test_cfinish_refusals():
    """what launch_cnet_finish or the geometry refuses is refused here, nothing written: a 256-pixel launch with four row copies (no
    instance), 64-pixel tiles on a 128-wide map (no such k_cnet geometry), a mixer of another width, a scratch below the plan's"""
    c = next(x for x in F.cfinish_cases() if x["name"] == "cfin-add-fwd-N2-16x16-t64-MS2-C6-none")
    d = F.build_cfinish(c, "exact")
    d4 = dict(d, scratch=d["scratch"][:-1])
    assert run_cfinish(c, d4, expect_rc=EINVAL)[0] is None
    N, C, HW = 8, 4, 128 * 128
    z, acc, t = Buf(N * C * HW * 4), Buf(data=np.zeros(9 * N, np.uint64)), Buf(data=np.ones(8, f32))
    for MS, tile in ((4, 128), (1, 64)):
        p = L.FinProbe()
        p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden, p.mode, p.MS, p.tile = L.FIN_CFINISH, N, C, 128, 128, 4, 128, F.AFFINE_FWD, MS, tile
        p.scratch, p.scratch_floats, p.bias, p.scale = z.ptr, 1 << 40, t.ptr, t.ptr      # (never read: refused before the launch)
        p.z_in, p.z_in_bs, p.z_out, p.z_out_bs, p.acc = z.ptr, C * HW, z.ptr, C * HW, acc.ptr
        assert call(p)[0] == EINVAL, (MS, tile)
    p.MS, p.tile, p.N, p.H, p.W, p.mix_C, p.mix_bias, p.mix_scale = 1, 64, 2, 16, 16, 6, t.ptr, t.ptr
    assert call(p)[0] == EINVAL
    assert z.untouched() and not acc.host(np.uint64).any() and intact(z, acc, t)


# ---------------------------------------------------------------------------------------------------------------------
# launch_chanmix
# ---------------------------------------------------------------------------------------------------------------------
RNG_SEED, RNG_CALL = 0x5EEDF1A5C0DE, 3


def philox_noise(c, d):
    n = d["sq"].size
    out = Buf(n * 4)
    rc = L.lib().glowhip_dequant_noise(out.ptr, n, RNG_SEED, RNG_CALL, F.SQ_BITS, L.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and out.intact()
    nz = out.host(f32)
    assert (nz >= 0).all() and (nz < 2.0 ** -F.SQ_BITS).all() and len(np.unique(nz)) > n // 2
    return nz.reshape(d["sq"].shape)


def run_chanmix(c, d, draw=False):
    """One launch_chanmix on fresh buffers -> (out (N, C, HW), info).  draw: the Philox draw in the kernel instead of the noise tensor"""
    N, C, HW, Ca = c["N"], c["C"], c["HW"], c["Ca"]
    mb = mix_bufs(d["mix"])
    p = L.FinProbe()
    p.op, p.N, p.C, p.HW, p.Ca, p.mix_reverse = L.FIN_CHANMIX, N, C, HW, Ca, c["reverse"]
    set_mix(p, mb)
    ins, src, noise = [], None, None
    if c["sq"]:
        flat, bs = F.sq_layout(c, d)
        src = Buf(data=flat)
        p.sq_src, p.sq_u8, p.sq_div, p.sq_W, p.sq_bs = src.ptr, int(c["sq"]["src"] == "u8"), F.SQ_DIV, 2 * c["sq"]["Wo"], bs
        if c["sq"]["noise"] != "none" and not draw:
            noise = Buf(data=d["noise"])
            p.sq_noise = noise.ptr
        if draw:
            p.rng_on, p.rng_seed, p.rng_call, p.rng_scale = 1, RNG_SEED, RNG_CALL, 2.0 ** -F.SQ_BITS
        out = Strided(N, C * HW, C * HW + 20)
    elif c["alias"]:
        bs = (C + 1) * HW + 8
        lead = HW if c["alias"] == "shifted" else 0
        # in place: out = the input; shifted: out = in_a + HW, output channel o over input channel o + 1 of the same pixel
        whole = Strided(N, C * HW, bs, data=d["x"].reshape(N, -1), lead=0)
        out = whole
        ins = [whole]
        p.in_a, p.in_a_bs, p.in_b, p.in_b_bs = whole.ptr, bs, whole.ptr + 4 * Ca * HW, bs
        if Ca == C:
            p.in_b = None
        out_ptr = whole.ptr + 4 * lead
    else:
        a = Strided(N, Ca * HW, Ca * HW + 4, data=d["x"][:, :Ca].reshape(N, -1)) if Ca else None
        b = Strided(N, (C - Ca) * HW, (C - Ca) * HW + 12, data=d["x"][:, Ca:].reshape(N, -1)) if Ca < C else None
        ins = [t for t in (a, b) if t]
        p.in_a, p.in_a_bs, p.in_b, p.in_b_bs = a.ptr if a else None, a.bs if a else 0, b.ptr if b else None, b.bs if b else 0
        out = Strided(N, C * HW, C * HW + 20)
    p.out, p.out_bs = (out_ptr, out.bs) if c["alias"] else (out.ptr, out.bs)
    info = ok(p)
    assert intact(src, noise, *mb.values()), c["name"]
    if c["alias"]:
        h = out.buf.host(f32)
        lead = HW if c["alias"] == "shifted" else 0
        res = np.stack([h[lead + n * out.bs:lead + n * out.bs + C * HW] for n in range(N)]).reshape(N, C, HW)
        # the guards, the gaps between the samples, and (shifted) the first plane of every sample, which no output covers
        keep = np.ones(h.size, bool)
        for n in range(N):
            keep[lead + n * out.bs:lead + n * out.bs + C * HW] = False
        want = np.full(h.size, np.frombuffer(b"\xa5" * 4, f32)[0], f32)
        for n in range(N):
            want[n * out.bs:n * out.bs + C * HW] = d["x"][n].reshape(-1)
        assert out.buf.intact() and h[keep].tobytes() == want[keep].tobytes(), (c["name"], "written outside the output")
    else:
        assert out.intact() and all(t.intact() for t in ins), c["name"]
        for t, want in zip(ins, [d["x"][:, :Ca], d["x"][:, Ca:]] if len(ins) == 2 else [d["x"]] if ins else []):
            assert t.rows().tobytes() == want.reshape(N, -1).tobytes(), (c["name"], "an input was written")
        res = out.rows((N, C, HW))
    return res, info


@pytest.mark.parametrize("c", F.chanmix_cases(), ids=ids(F.chanmix_cases()))
def test_chanmix_equals_fp64(c):
    for fam in c["families"]:
        d = F.build_chanmix(c, fam)
        philox = bool(c["sq"]) and c["sq"]["noise"] == "philox"
        if philox:
            d["noise"] = philox_noise(c, d)
        got, info = run_chanmix(c, d, draw=philox)
        again, _ = run_chanmix(c, d, draw=philox)
        want = {"16": L.FNI_CHANMIX16, "64": L.FNI_CHANMIX64, "wide": L.FNI_CHANMIX_WIDE}[c["kernel"]]
        assert (info.kernel, list(info.grid), info.lds_bytes, info.stage_matrix) == (want, c["grid"], c["lds"], c["stage"]), (c["name"], info.kernel, list(info.grid),
                                                                                                                            info.lds_bytes, info.stage_matrix)
        SEEN_MIX.add((c["kernel"], "in place" if c["kernel"] == "wide" and info.grid[1] == 1 else "sliced" if c["kernel"] == "wide" else ""))
        assert got.tobytes() == again.tobytes(), (c["name"], fam, "two runs differ")
        if philox:      # the in-kernel draw is the tensor glowhip_dequant_noise writes
            assert run_chanmix(c, d, draw=False)[0].tobytes() == got.tobytes(), (c["name"], "the draw differs from glowhip_dequant_noise")
        route = "k_chanmix%s %s%s%s" % ({"16": "<16>", "64": "<64>", "wide": "_wide"}[c["kernel"]], c["kind"], " reverse" if c["reverse"] else "",
                                        " squeezed view" if c["sq"] else "")
        compare(route, c["name"], fam, got, F.chanmix_ref(c, d), "y")
        want = F.mixer_bitwise(d["mix"], F.chanmix_input(c, d)[2])
        if want is not None:
            assert got.tobytes() == want.tobytes(), (c["name"], fam, "the gathered value is not fl(fl(x + b) e)")


def test_chanmix_refusals():
    x, y = Buf(data=np.ones(3 * 10 * 16, f32)), Buf(3 * 10 * 16 * 4)
    for kw in (dict(C=513), dict(sq_src=x.ptr, sq_W=8, C=10), dict(sq_src=x.ptr, sq_W=8, C=12, mix_reverse=1), dict(out_bs=100)):
        p = L.FinProbe()
        p.op, p.N, p.C, p.HW, p.Ca, p.in_a, p.in_a_bs, p.out, p.out_bs = L.FIN_CHANMIX, 3, 10, 16, 10, x.ptr, 160, y.ptr, 160
        for k, v in kw.items():
            setattr(p, k, v)
        assert call(p)[0] == EINVAL, kw
    assert y.untouched() and intact(x)


# ---------------------------------------------------------------------------------------------------------------------
# k_dn_fin / k_dn_prep
# ---------------------------------------------------------------------------------------------------------------------
def level_scratch(c):
    lay = F.dn_layout(c)
    return lay, np.full(lay["bytes"], 0xA5, np.uint8)


def dn_probe(op, c, state, scratch):
    p = L.FinProbe()
    p.op, p.N, p.C, p.H, p.W, p.Cout, p.hidden = op, c["N"], c["C"], c["H"], c["W"], c["Cout"], F.DN_HIDDEN
    p.state, p.z_in_bs, p.dn_scratch = state.ptr, state.bs, scratch.ptr
    return p


def check_layout(c, info, lay):
    assert (info.part_off, info.u_off, info.ypad_off, info.u_plane, info.ypad_plane, info.scratch_bytes) == \
        (lay["part_off"], lay["u_off"], lay["ypad_off"], lay["u_plane"], lay["ypad_plane"], lay["bytes"]), c["name"]


def run_dnfin(c, d):
    N, C, HW, Cout, ks = c["N"], c["C"], c["HW"], c["Cout"], c["ks"]
    lay, host = level_scratch(c)
    part = np.full((8, N, Cout, HW), np.nan, f32)      # the copies beyond ks hold NaN: never read
    part[:ks] = d["part"]
    host[lay["part_off"]:lay["part_off"] + part.nbytes] = part.view(np.uint8).reshape(-1)
    scratch = Buf(data=host)
    state = Strided(N, C * HW, C * HW + 8, data=d["z"].reshape(N, -1))
    bias, scale, acc = Buf(data=d["bias"]), Buf(data=d["scale"]), Buf(data=np.zeros((2 + F.ACC_EXTRA) * N, np.uint64))
    mb = mix_bufs(d["mix"])
    p = dn_probe(L.FIN_DN_FIN, c, state, scratch)
    p.ks, p.bias, p.scale, p.mode, p.acc, p.want_u = ks, bias.ptr, scale.ptr, c["mode"], acc.ptr, c["want_u"]
    set_mix(p, mb)
    info = ok(p)
    check_layout(c, info, lay)
    assert intact(scratch, bias, scale, acc, *mb.values()) and state.intact(), c["name"]
    return dict(state=state.rows((N, C, HW)), acc=acc.host(np.uint64), scratch=scratch.host(np.uint8)), info, lay, host


@pytest.mark.parametrize("c", F.dnfin_cases(), ids=ids(F.dnfin_cases()))
def test_dnfin_equals_fp64(c):
    N, C, Ch, HW = c["N"], c["C"], c["Ch"], c["HW"]
    for fam in c["families"]:
        d = F.build_dnfin(c, fam)
        got, info, lay, before = run_dnfin(c, d)
        again, _, _, _ = run_dnfin(c, d)
        assert info.kernel == L.FNI_DN_FIN and list(info.grid) == c["grid"], (c["name"], list(info.grid))
        for k in got:
            assert got[k].tobytes() == again[k].tobytes(), (c["name"], fam, k, "two runs differ")
        ref = F.dnfin_ref(c, d)
        route = "k_dn_fin %s" % ("affine" if F.paired(c["mode"]) else "additive")
        compare(route, c["name"], fam, got["state"], ref["state"], "state")
        assert got["state"][:, :Ch].tobytes() == d["z"][:, :Ch].tobytes(), (c["name"], "z1 changed")
        if "ld" in ref:
            logdet_check(route, c["name"], got["acc"], N, ref["ld"], fam)
        else:
            assert not got["acc"].any()
        # the level scratch: the SH2 operand of the next launch where wanted, bit for bit from the state the kernel stored; nothing else
        want = before.copy()
        if c["want_u"]:
            hi, lo = F.sh2_split(got["state"], d["mix"]["bias"], d["mix"]["scale"])
            P = N * HW
            planes = np.concatenate([F.sh2_plane(hi, P, np.arange(P)), F.sh2_plane(lo, P, np.arange(P))])
            assert planes.size == 2 * lay["u_plane"]
            want[lay["u_off"]:lay["u_off"] + planes.nbytes] = planes.view(np.uint8)
        assert got["scratch"].tobytes() == want.tobytes(), (c["name"], fam, "the level scratch differs from fp16(v), fp16(v - hi) of v = 16 ActNorm(state)")


@pytest.mark.parametrize("c", F.dnprep_cases(), ids=ids(F.dnprep_cases()))
def test_dnprep_writes_the_sh2_operand(c):
    N, C, HW = c["N"], c["C"], c["HW"]
    d = F.build_dnprep(c)
    outs = []
    for _ in range(2):
        lay, host = level_scratch(c)
        scratch = Buf(data=host)
        src = Strided(N, C * HW, C * HW + 8, data=d["src"].reshape(N, -1))
        state = Strided(N, C * HW, C * HW + 4) if c["copy"] else src
        mb = mix_bufs(d["mix"])
        p = dn_probe(L.FIN_DN_PREP, c, state, scratch)
        p.src, p.src_bs, p.mix_reverse = src.ptr, src.bs, c["reverse"]
        set_mix(p, mb)
        info = ok(p)
        check_layout(c, info, lay)
        assert info.kernel == L.FNI_DN_PREP and list(info.grid) == c["grid"], (c["name"], list(info.grid))
        assert intact(scratch, *mb.values()) and src.intact() and state.intact(), c["name"]
        assert src.rows().tobytes() == d["src"].reshape(N, -1).tobytes() and state.rows().tobytes() == d["src"].reshape(N, -1).tobytes(), (c["name"], "source / copy")
        outs.append(scratch.host(np.uint8))
    assert outs[0].tobytes() == outs[1].tobytes(), (c["name"], "two runs differ")
    want = host.copy()
    if not c["reverse"]:      # all channels, with the first step's ActNorm, into u
        hi, lo = F.sh2_split(d["src"], d["mix"]["bias"], d["mix"]["scale"])
        P = N * HW
        planes, off = np.concatenate([F.sh2_plane(hi, P, np.arange(P)), F.sh2_plane(lo, P, np.arange(P))]), lay["u_off"]
        v64 = d["src"].astype(f64) if d["mix"]["bias"] is None else (d["src"].astype(f64) + d["mix"]["bias"].astype(f64)[None, :, None]) * d["mix"]["scale"].astype(f64)[None, :, None]
    else:                     # the first C / 2 channels, plain, into the padded operand of F0; its border is not this kernel's
        hi, lo = F.sh2_split(d["src"][:, :C // 2], None, None)
        slots = F.pad_slots(N, c["H"], c["W"])
        planes, off = np.concatenate([F.sh2_plane(hi, lay["SLN"], slots), F.sh2_plane(lo, lay["SLN"], slots)]), lay["ypad_off"]
        v64 = d["src"][:, :C // 2].astype(f64)
    want[off:off + planes.nbytes] = planes.view(np.uint8)
    assert outs[0].tobytes() == want.tobytes(), (c["name"], "the level scratch differs from fp16(v), fp16(v - hi) of v = 16 ActNorm(src)")
    # against fp64: ActNorm is two roundings, the factor 16 none; the split keeps max(2^-22 |V|, 2^-25) (csrc/sh.h)
    V = 16.0 * v64
    b = F.bnd((2.0 * F.U if d["mix"]["bias"] is not None else 0.0) * np.abs(V) + np.maximum(2.0 ** -22 * np.abs(V), 2.0 ** -25))
    compare("k_dn_prep " + ("reverse" if c["reverse"] else "forward"), c["name"], "random", hi.astype(f64) + lo.astype(f64), (V, b), "hi + lo")


def test_dn_refusals():
    c = F.dnfin_cases()[0]
    d = F.build_dnfin(c, "random")
    lay, host = level_scratch(c)
    scratch, state, t, acc = Buf(data=host), Strided(c["N"], c["C"] * c["HW"], c["C"] * c["HW"] + 8), Buf(data=np.ones(64, f32)), Buf(data=np.zeros(9 * c["N"], np.uint64))
    for kw in (dict(ks=0), dict(ks=9), dict(mode=0), dict(Cout=16), dict(C=48), dict(z_in_bs=10), dict(mix_bias=t.ptr)):
        p = dn_probe(L.FIN_DN_FIN, c, state, scratch)
        p.ks, p.bias, p.scale, p.mode, p.acc = 1, t.ptr, t.ptr, c["mode"], acc.ptr
        for k, v in kw.items():
            setattr(p, k, v)
        assert call(p)[0] == EINVAL, kw
    assert scratch.host(np.uint8).tobytes() == host.tobytes() and state.intact(written=False) and not acc.host(np.uint64).any()


def test_zz_every_instance_and_route_was_seen():
    """Fails if one of the k_cfinish instances or one of the four mixer forms never ran; prints the worst multiple of the bound per
    route, the count of `exact` values compared and the run time of this file (the figures of the module docstring)."""
    for name in sorted(WORST):
        print(f"worst multiple of the bound  {name:70s} {WORST[name]:.3f}")
    print(f"exact values compared: {EXACT[0]}, differing: {EXACT[1]}")
    print(f"run time of this file: {time.time() - T0:.1f} s")
    assert EXACT[1] == 0
    want = {(p, m, h) for p in (16, 64) for m in (1, 2, 4) for h in (0, 1)} | {(256, m, 1) for m in (1, 2)}
    assert SEEN_CFIN == want, ("k_cfinish instances never launched", sorted(want - SEEN_CFIN))
    assert SEEN_MIX == {("16", ""), ("64", ""), ("wide", "sliced"), ("wide", "in place")}, SEEN_MIX
