"""Every weight-gradient kernel instance on its own (csrc/wgrad_mfma.hip: the fourteen instances behind launch_wgrad_mfma, the
one-launch forms k_wgrad_gemm_pair / _trio, k_shift_expand, the split-K reduction; csrc/backward.hip: k_wgrad_direct,
k_half_to_float), launched through the testing hook glowhip_debug_wgrad -- which calls the launchers the backward sweep calls --
on operands laid out here, against the fp64 reference of tests/wgrad_oracle.py on EVERY output element:

  * `exact` input sets (every partial sum in every order an fp32 number): the kernel must return the reference value for value,
    at any loop length;
  * `random` input sets (gradients at 1, 1e-3 and 1e-7 in front of sh_scale, ReLU-like and signed B): every element within the
    bound derived in wgrad_oracle from the kernel's roundings, no outliers allowed.

tests/test_wgrad_host.py shows on the CPU that the promised arithmetic lies inside that bound / is exact on each of these input
sets, and that it leaves both when a product plane, a k-tile or the row-sum rescale is dropped.

Every launch: `partial` is exactly wgrad_mfma_partial_floats long (asked from the hook) with a 0xA5 guard behind it, dW has guards
on both sides, all operands sit between guards; two runs into fresh 0xA5 buffers must give the same dW bytes (row sums: fp64
atomics, order-dependent -- each run within its bound).  The instance, split count and k-tiles per split are asserted from what
the launcher reports (glowhip_wgrad_info)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd import _lib  # noqa: E402

import wgrad_oracle as W  # noqa: E402

DEV = "cuda:0"
GUARD = 4096
EINVAL = -1
WORST = {}          # instance name -> worst multiple of the bound seen (reported by the last test)
EXACT = [0, 0]      # exact values compared, differing


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

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return bool((self.raw == 0xA5).all())

    def host(self, dtype):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype).copy()


def call(probe):
    info = _lib.WgradInfo()
    rc = _lib.lib().glowhip_debug_wgrad(ctypes.byref(probe), ctypes.byref(info), _lib.stream_ptr(DEV))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault: nothing more is started on this GPU by this run
        pytest.exit(f"device error after glowhip_debug_wgrad: {e}", returncode=3)
    return rc, info


def set_taps(slot, taps):
    slot.operand = -1
    if taps is not None:
        slot.operand, slot.C, slot.H, slot.W, slot.sign = taps


def fill_gemm(g, case, d, A, B, partial, dw, rowsum, a_off=0, b_off=0):
    g.A, g.B = A.ptr + a_off, B.ptr + b_off
    g.partial, g.dw, g.rowsum = (partial.ptr if partial else None), dw.ptr, (rowsum.ptr if rowsum else None)
    g.a_bs, g.b_bs = d["a_bs"], d["b_bs"]
    g.Mpad, g.Npad, g.Mreal, g.Nreal, g.mode = case["Mpad"], case["Npad"], case["Mreal"], case["Nreal"], case["mode"]
    g.b_valid, g.b_half, g.tiled = case["b_valid"], int(case["b"] == "half"), case["tiled"]


def rowsum_init(case, d):
    return np.linspace(-3.0, 5.0, case["Mpad"]) / (d["sh_scale"] or 1.0)


def partial_floats(probe, i=0):
    """What the sweep allocates for GEMM i: asked from the hook with a null `partial`."""
    saved = [probe.gemm[k].partial for k in range(3)]
    for k in range(3):
        probe.gemm[k].partial = None
    rc, info = call(probe)
    for k in range(3):
        probe.gemm[k].partial = saved[k]
    assert rc == 0, _lib.lib().glowhip_last_error()
    return [int(info.partial_floats[k]) for k in range(3)]


def run_mfma(case, d, a_dev=None, b_dev=None, a_off=0, b_off=0):
    """One launch_wgrad_mfma on fresh buffers -> (dW float32, row sums or None, info)."""
    A, B = Buf(data=d["A"] if a_dev is None else a_dev), Buf(data=d["B"] if b_dev is None else b_dev)
    p = _lib.WgradProbe()
    p.op, p.N, p.HW, p.sh_scale = _lib.WGRAD_MFMA, case["N"], case["HW"], d["sh_scale"]
    set_taps(p.taps[0], d["taps"])
    dw = Buf(case["Mreal"] * case["Nreal"] * 4)
    rs = Buf(data=rowsum_init(case, d)) if case["rowsum"] else None
    fill_gemm(p.gemm[0], case, d, A, B, None, dw, rs, a_off, b_off)
    pf = partial_floats(p)[0]
    assert dw.untouched()
    part = Buf(pf * 4)
    p.gemm[0].partial = part.ptr
    rc, info = call(p)
    assert rc == 0, _lib.lib().glowhip_last_error()
    assert part.intact() and dw.intact() and A.intact() and B.intact() and (rs is None or rs.intact()), case["name"]
    assert info.splits[0] * case["Mpad"] * case["Npad"] <= pf
    return dw.host(np.float32), (rs.host(np.float64) if rs else None), info


def instance_name(i):
    L = _lib
    if i & L.WGI_SH and i < 0x200:
        f = i & 0xff
        return "k_wgrad_gemm_sh<%d%s%s%s%s>" % (64 if f & L.WGI_BN64 else 128, ",VA" if f & L.WGI_VA else "", ",VB" if f & L.WGI_VB else "",
                                                 ",BV" if f & L.WGI_BV else "", ",BH" if f & L.WGI_BH else "")
    return {L.WGI_F32_128: "k_wgrad_gemm<128>", L.WGI_F32_64: "k_wgrad_gemm<64>", L.WGI_PS128: "k_wgrad_gemm_ps<128>", L.WGI_PS64: "k_wgrad_gemm_ps<64>",
            L.WGI_PS512: "k_wgrad_gemm_ps512", L.WGI_PAIR64: "k_wgrad_gemm_pair<64>", L.WGI_PAIR128: "k_wgrad_gemm_pair<128>",
            L.WGI_TRIO64: "k_wgrad_gemm_trio<64>", L.WGI_TRIO128: "k_wgrad_gemm_trio<128>"}.get(i, hex(i))


def expected_instance(case):
    L = _lib
    total = case["N"] * case["HW"] // 32
    if not case["sh"]:
        return L.WGI_F32_128 if case["Npad"] % 128 == 0 else L.WGI_F32_64
    if case["a"] == "ps" and case["b"] == "half":
        return L.WGI_PS512 if case["Npad"] % 256 == 0 and total >= 512 else L.WGI_PS128 if case["Npad"] % 128 == 0 else L.WGI_PS64
    return L.WGI_SH | (0 if case["Npad"] % 128 == 0 else L.WGI_BN64) | (L.WGI_VA if case["a"] == "taps" else 0) | (L.WGI_VB if case["b"] == "taps" else 0) | \
        (L.WGI_BV if case["b"] == "bvalid" else 0) | (L.WGI_BH if case["b"] == "half" else 0)


def compare(case, fam, d, got, rs, splits, nk, inst):
    """The assertion of every GEMM case: value for value (`exact`) or every element within the bound (`random`); row sums within theirs."""
    name = instance_name(inst)
    if fam == "random":
        bnd = W.bound(d["absd"], splits, nk, d["kind"], d["sh_scale"], d["sum_a"], d["sum_b"], case["mode"], case["Mreal"], case["Nreal"])
        err = np.abs(got.astype(np.float64) - d["ref"])
        ok = np.isnan(d["ref"]) | (err <= bnd)
        assert np.array_equal(np.isnan(got), np.isnan(d["ref"])), (case["name"], "NaN where the reference has none, or the reverse")
        r = float(np.nanmax(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), 0.0)))
        print(f"{case['name']} [{fam}] {name} splits {splits} x {nk} k-tiles: worst multiple of the bound {r:.3f}")
        WORST[name] = max(WORST.get(name, 0.0), r)
        assert ok.all(), (case["name"], name, int((~ok).sum()), "elements outside the bound; worst multiple", r)
    else:
        differ = int((got.astype(np.float64) != d["ref"]).sum())
        EXACT[0] += got.size
        EXACT[1] += differ
        assert differ == 0, (case["name"], fam, name, differ, "of", got.size, "values differ from the fp64 reference",
                             float(np.abs(got - d["ref"]).max()))
    check_rowsum(case, d, rs, splits, nk)


def check_rowsum(case, d, rs, splits, nk):
    """rowsum[m] += the row's sum: the accumulators start at non-zero doubles, and only the first column tile's workgroups add."""
    if rs is None:
        return
    init = rowsum_init(case, d)
    b = W.bound_rowsum(d["rs_abs"], splits, nk, init)
    e = np.abs(rs - (init + d["rs_ref"]))
    assert np.array_equal(np.isnan(rs), np.isnan(d["rs_ref"]))
    r = float(np.nanmax(e / b))
    WORST["row sums"] = max(WORST.get("row sums", 0.0), r)
    assert (np.isnan(e) | (e <= b)).all(), (case["name"], "row sums: worst multiple of the bound", r)


def check_case(case):
    total = case["N"] * case["HW"] // 32
    for fam in case["families"]:
        d = W.build_mfma(case, fam)
        got, rs, info = run_mfma(case, d)
        again, rs2, _ = run_mfma(case, d)
        assert got.tobytes() == again.tobytes(), (case["name"], fam, "two runs differ")
        inst, splits, nk = info.instance[0], info.splits[0], info.ktiles_per_split[0]
        assert inst == expected_instance(case), (case["name"], instance_name(inst), instance_name(expected_instance(case)))
        assert (splits - 1) * nk < total <= splits * nk and info.blocks[0] == info.live[0] > 0
        compare(case, fam, d, got, rs, splits, nk, inst)
        check_rowsum(case, d, rs2, splits, nk)
    return info


def ids(cases):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# launch_wgrad_mfma: the split-half instances
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.shape_cases(), ids=ids(W.shape_cases()))
def test_split_half_instance_equals_fp64(case):
    """k_wgrad_gemm_sh<128 / 64> plain, VA, VB, BV, BH (plain / tiled, with and without VA), k_wgrad_gemm_ps<128 / 64>, and the
    pre-scaled A with a gathered B (f.0's form) on the maps 8x4, 4x8, 2x16, 16x16 at N = 1 and 3."""
    check_case(case)


@pytest.mark.parametrize("case", W.loop_cases(), ids=ids(W.loop_cases()))
def test_k_loop_lengths(case):
    """ktiles_per_split 1 .. 8 at 32 splits on the three-stage loop (k_wgrad_gemm_sh<128,BH>), the two-stage loop (two-plane B at 128
    columns) and k_wgrad_gemm_ps<128>: the prologue, every remainder of the unrolled steady loop and the `last` steps; a shorter last
    split; fewer k-tiles than splits."""
    info = check_case(case)
    name = case["name"]
    if "-per" in name:
        assert (info.splits[0], info.ktiles_per_split[0]) == (32, int(name.split("-per")[1]))
    elif name.endswith("short-last"):
        assert (info.splits[0], info.ktiles_per_split[0]) == (32, 3)
    else:
        assert (info.splits[0], info.ktiles_per_split[0]) == (10, 1)


@pytest.mark.parametrize("case", W.wide_cases(), ids=ids(W.wide_cases()))
def test_wide_instance_at_its_threshold(case):
    """k_wgrad_gemm_ps512 at Npad 256 and 512 with 512 k-tiles; its partial tiles stay inside wgrad_mfma_partial_floats."""
    info = check_case(case)
    assert info.instance[0] == _lib.WGI_PS512


@pytest.mark.parametrize("case", W.reduce_cases(), ids=ids(W.reduce_cases()))
def test_split_k_reduction_layouts_and_split_counts(case):
    """mode 0 / 1, Nreal 54 (two live columns in the last quad) / 108 / 216, splits 1, 7, 8, 9, 17: both loops of wgrad_reduce_body
    and their joint."""
    info = check_case(case)
    assert info.splits[0] == case["N"] and info.ktiles_per_split[0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# gather edges, by name
# ---------------------------------------------------------------------------------------------------------------------
EDGES = {
    "dx-inside-a-chunk-W4-gathered-A": W.mfma_case("edge-w4-va", 3, 8, 4, 108, 100, 128, a="taps", mode=1, families=("exact1", "exact2")),
    "dx-inside-a-chunk-W4-gathered-B": W.mfma_case("edge-w4-vb", 3, 8, 4, 128, 108, 128, b="taps", families=("exact1", "exact2")),
    "both-halo-rows-outside-H2-gathered-A": W.mfma_case("edge-h2-va", 3, 2, 16, 108, 54, 64, a="taps", mode=1, families=("exact1", "exact2")),
    "both-halo-rows-outside-H2-gathered-B": W.mfma_case("edge-h2-vb", 3, 2, 16, 128, 54, 64, b="taps", families=("exact1", "exact2")),
    "zero-rows-behind-9C-in-the-last-row-tile": W.mfma_case("edge-rows-va", 1, 8, 8, 9 * 15, 128, 128, a="taps", b="half", mode=1, tiled=2,
                                                            families=("exact1",)),       # 135 rows: the second row tile holds 7 live rows
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_gather_edge(edge):
    """dx = +-1 inside a 4-pixel chunk at W = 4 (every chunk a whole row, both ends masked), H = 2 (both halo rows outside the
    image), operand rows >= 9 C inside the last row tile (v_off < 0: zero rows) -- value for value on the `exact` sets."""
    check_case(EDGES[edge])


@pytest.mark.parametrize("H,W_", [(8, 4), (2, 16), (16, 16)])
@pytest.mark.parametrize("which", ["A", "B", "A-bvalid"])
def test_gather_never_reads_the_neighbouring_image(which, H, W_):
    """dy = +-1 at the first and last row of an image with other images adjacent in memory: the middle image of a three-image
    tensor is launched as a batch of one, once with clean neighbours and once with the neighbours' values replaced by 3e4 in a
    copy.  Same dW bytes, and the reference of the one image value for value."""
    if which == "A":
        case = W.mfma_case("nb-va", 1, H, W_, 108, 100, 128, a="taps", mode=1)
    elif which == "B":
        case = W.mfma_case("nb-vb", 1, H, W_, 128, 108, 128, b="taps")
    else:
        case = W.mfma_case("nb-bv", 1, H, W_, 108, 6, 64, a="taps", b="bvalid", mode=1, b_valid=6)
    d = W.build_mfma(case, "exact1")
    op = "B" if which == "B" else "A"
    one = d[op]
    outs = []
    for poison in (0.0, 3e4):
        side = np.full_like(one, poison) if poison else W.build_mfma(case, "exact1", seed=7)[op]
        three = np.concatenate([side, one, side])
        kw = dict(a_dev=three, a_off=one.nbytes) if op == "A" else dict(b_dev=three, b_off=one.nbytes)
        got, _, info = run_mfma(case, d, **kw)
        outs.append(got)
    assert outs[0].tobytes() == outs[1].tobytes()
    compare(case, "exact1", d, outs[1], None, info.splits[0], info.ktiles_per_split[0], info.instance[0])


# ---------------------------------------------------------------------------------------------------------------------
# NaN contract
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["live-A", "element-0-of-a-gathered-A", "element-0-of-a-gathered-B", "row-0-of-a-b_valid-B"])
def test_nan_lands_exactly_where_the_reference_has_it(where):
    """One NaN in A at a live position; one at element 0 of a gathered tensor and one in row 0 of a b_valid operand -- the addresses
    the masked lanes load and discard.  dW is NaN exactly where the fp64 reference is, and within the bound elsewhere."""
    if where == "live-A":
        case, op, at = W.mfma_case("nan-a", 3, 16, 16, 100, 100, 128, rowsum=True, families=("random",)), "A", (1, 37, 101)
    elif where == "element-0-of-a-gathered-A":
        case, op, at = W.mfma_case("nan-va", 3, 8, 4, 108, 100, 128, a="taps", mode=1, families=("random",)), "A", (0, 0, 0, 0)
    elif where == "element-0-of-a-gathered-B":
        case, op, at = W.mfma_case("nan-vb", 3, 8, 4, 128, 54, 64, b="taps", families=("random",)), "B", (0, 0, 0, 0)
    else:
        case, op, at = W.mfma_case("nan-bv", 3, 8, 4, 108, 6, 64, a="taps", b="bvalid", mode=1, b_valid=6, families=("random",)), "B", (0, 0, 5)
    d = W.build_mfma(case, "random")
    ref_arr = d[op + "_ref"]
    ref_arr[at] = np.nan
    assert np.isnan(d[op]).sum() == 1, "the device image shares the reference's memory"
    a64, b64 = W.logical(d["A_ref"], d["B_ref"], d["tp"], d["a_div"])
    Mr, Nr = case["Mreal"], case["Nreal"]
    with np.errstate(invalid="ignore"):
        prod = np.einsum("mk,nk->mn", a64[:Mr], b64[:Nr])
        d["ref"] = W.to_layout(prod, case["mode"], Mr, Nr)
        d["absd"] = W.to_layout(np.einsum("mk,nk->mn", np.abs(a64[:Mr]), np.abs(b64[:Nr])), case["mode"], Mr, Nr)
        d["sum_a"], d["sum_b"] = np.nan_to_num(np.abs(a64[:Mr]).sum(1), nan=0.0), np.nan_to_num(np.abs(b64[:Nr]).sum(1), nan=0.0)
        if "rs_ref" in d:
            d["rs_ref"], d["rs_abs"] = a64.sum(1), np.abs(a64).sum(1)
    n_nan = int(np.isnan(d["ref"]).sum())
    assert 0 < n_nan < d["ref"].size
    got, rs, info = run_mfma(case, d)
    compare(case, "random", d, got, rs, info.splits[0], info.ktiles_per_split[0], info.instance[0])


# ---------------------------------------------------------------------------------------------------------------------
# the grouped launches
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = W.group_cases()


@pytest.mark.parametrize("grp", GROUPS, ids=ids(GROUPS))
def test_grouped_launch_equals_fp64(grp):
    """k_wgrad_gemm_pair<64 / 128> / k_wgrad_gemm_trio<64 / 128> + k_wgrad_reduce_batched on the jobs the launcher returned: C = 12, 24,
    48, additive and affine, hidden 128 and 256; live block counts that are no multiple of 8 (dead workgroups in between), shares
    that round both ways.  Each GEMM against its own reference; every scratch exactly as long as the sweep allocates it."""
    L = _lib
    order = ("f4", "f0", "f2") if grp["trio"] else ("f4", "f0")
    for fam in grp["families"]:
        ds = {k: W.build_mfma(grp["sub"][k], fam, seed=i + 1) for i, k in enumerate(order)}
        runs = []
        for _ in range(2):
            p = L.WgradProbe()
            p.op, p.N, p.HW = (L.WGRAD_TRIO if grp["trio"] else L.WGRAD_PAIR), grp["N"], grp["HW"]
            p.sh_scale = ds["f4"]["sh_scale"]
            set_taps(p.taps[0], ds["f4"]["taps"])
            set_taps(p.taps[1], ds["f0"]["taps"])
            bufs = {}
            for i, k in enumerate(order):
                c, d = grp["sub"][k], ds[k]
                bufs[k] = dict(A=Buf(data=d["A"]), B=Buf(data=d["B"]), dw=Buf(c["Mreal"] * c["Nreal"] * 4),
                               rs=Buf(data=rowsum_init(c, d)) if c["rowsum"] else None)
                fill_gemm(p.gemm[i], c, d, bufs[k]["A"], bufs[k]["B"], None, bufs[k]["dw"], bufs[k]["rs"])
            pf = partial_floats(p)
            for i, k in enumerate(order):
                bufs[k]["part"] = Buf(pf[i] * 4)
                p.gemm[i].partial = bufs[k]["part"].ptr
            rc, info = call(p)
            assert rc == 0, L.lib().glowhip_last_error()
            for k in order:
                assert all(b.intact() for b in bufs[k].values() if b is not None), (grp["name"], k, "a guard was written")
            runs.append({k: (bufs[k]["dw"].host(np.float32), bufs[k]["rs"].host(np.float64) if bufs[k]["rs"] else None) for k in order})
        n0 = grp["n0"]
        want = (L.WGI_TRIO64 if n0 == 64 else L.WGI_TRIO128) if grp["trio"] else (L.WGI_PAIR64 if n0 == 64 else L.WGI_PAIR128)
        for i, k in enumerate(order):
            c = grp["sub"][k]
            assert info.instance[i] == want
            assert (info.splits[i], info.ktiles_per_split[i]) == c["splits_per"], (grp["name"], k)
            assert info.live[i] == grp["tiles"][k] * info.splits[i] and info.blocks[i] == (info.live[i] if k == "f0" else (info.live[i] + 7) // 8 * 8)
            assert info.splits[i] * c["Mpad"] * c["Npad"] <= pf[i]
            assert runs[0][k][0].tobytes() == runs[1][k][0].tobytes(), (grp["name"], k, "two runs differ")
            for r in runs:
                compare(c, fam, ds[k], r[k][0], r[k][1], info.splits[i], info.ktiles_per_split[i], info.instance[i])


# ---------------------------------------------------------------------------------------------------------------------
# fp32 pipe on k_shift_expand's output, k_wgrad_direct, k_half_to_float
# ---------------------------------------------------------------------------------------------------------------------
def run_shift_expand(t, sign, rows_pad):
    N, C, H, W_ = t.shape
    src, out = Buf(data=t), Buf(N * rows_pad * H * W_ * 4)
    p = _lib.WgradProbe()
    p.op, p.N, p.HW = _lib.WGRAD_SHIFT_EXPAND, N, H * W_
    set_taps(p.taps[0], (0, C, H, W_, sign))
    p.gemm[0].A, p.gemm[0].dw, p.gemm[0].a_bs, p.gemm[0].Mpad = src.ptr, out.ptr, C * H * W_, rows_pad
    rc, info = call(p)
    assert rc == 0 and info.instance[0] == _lib.WGI_SHIFT_EXPAND and out.intact() and src.intact()
    return out.host(np.float32).reshape(N, rows_pad, H * W_)


@pytest.mark.parametrize("H,W_", [(8, 4), (8, 12), (16, 16)])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("npad", [128, 64])
def test_fp32_instances_on_shift_expanded_operands(npad, N, H, W_):
    """k_shift_expand bit for bit, then k_wgrad_gemm<128 / 64> (sh_scale = 0) on its output, as the per-layer route runs f.4 (expanded
    A, sign -1, mode 1) and f.0 (expanded B, sign +1, mode 0) -- a width that is no power of two included."""
    g4 = W.gen_a("random", (N, 6, H, W_), 1.0, 11)
    col = run_shift_expand(g4, -1, 128)
    assert col.tobytes() == W.expand(g4, -1, 128).tobytes()
    case = W.mfma_case(f"f32-f4-{npad}", N, H, W_, 54, npad, npad, mode=1, sh=False, families=("random",))
    d = W.build_mfma(case, "random")
    d["A"], d["A_ref"] = col.reshape(-1), col
    a64, b64 = W.logical(col, d["B_ref"])
    d["ref"], d["absd"] = W.to_layout(a64[:54] @ b64[:npad].T, 1, 54, npad), W.to_layout(np.abs(a64[:54]) @ np.abs(b64[:npad]).T, 1, 54, npad)
    got, _, info = run_mfma(case, d)
    assert info.instance[0] == expected_instance(case)
    compare(case, "random", d, got, None, info.splits[0], info.ktiles_per_split[0], info.instance[0])

    n0 = npad
    ch = 6 if npad == 64 else 12
    y = W.gen_b("random", (N, ch, H, W_), False, False, 12)
    colb = run_shift_expand(y, +1, n0)
    assert colb.tobytes() == W.expand(y, +1, n0).tobytes()
    case = W.mfma_case(f"f32-f0-{npad}", N, H, W_, 128, 9 * ch, n0, sh=False, families=("random",))
    d = W.build_mfma(case, "random")
    d["B"], d["B_ref"] = colb.reshape(-1), colb
    a64, b64 = W.logical(d["A_ref"], colb)
    d["ref"], d["absd"] = W.to_layout(a64[:128] @ b64[:9 * ch].T, 0, 128, 9 * ch), W.to_layout(np.abs(a64[:128]) @ np.abs(b64[:9 * ch]).T, 0, 128, 9 * ch)
    got, _, info = run_mfma(case, d)
    assert info.instance[0] == expected_instance(case)
    compare(case, "random", d, got, None, info.splits[0], info.ktiles_per_split[0], info.instance[0])


@pytest.mark.parametrize("H,W_", [(3, 5), (6, 10), (8, 4)])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("ksize", [1, 3])
def test_direct_kernel_equals_fp64(ksize, N, H, W_):
    """k_wgrad_direct<1 / 3> with a strided input (x_bs: the first Cin of Cin + 3 channels): 2^-24 absdot + 2^-24 |dW| per element."""
    Cout, Cin = 5, 4
    gy = W.gen_a("random", (N, Cout, H, W_), 1.0, 21)
    xw = W.gen_b("random", (N, Cin + 3, H, W_), False, False, 22)
    x = xw[:, :Cin]
    ref, absd = W.direct_ref(gy, x, ksize)
    G, X, dw = Buf(data=gy), Buf(data=xw), Buf(Cout * Cin * ksize * ksize * 4)
    p = _lib.WgradProbe()
    p.op, p.N, p.HW, p.ksize = _lib.WGRAD_DIRECT, N, H * W_, ksize
    set_taps(p.taps[0], (0, Cin, H, W_, 1))
    g = p.gemm[0]
    g.A, g.B, g.dw, g.b_bs, g.Mreal, g.Nreal = G.ptr, X.ptr, dw.ptr, (Cin + 3) * H * W_, Cout, Cin
    rc, info = call(p)
    assert rc == 0 and info.instance[0] == (_lib.WGI_DIRECT1 if ksize == 1 else _lib.WGI_DIRECT3)
    assert dw.intact() and G.intact() and X.intact()
    got = dw.host(np.float32).astype(np.float64)
    want = ref
    err, bnd = np.abs(got - want), W.bound_direct(absd, want)
    WORST[f"k_wgrad_direct<{ksize}>"] = max(WORST.get(f"k_wgrad_direct<{ksize}>", 0.0), float((err / bnd).max()))
    assert (err <= bnd).all(), float((err / bnd).max())


def test_half_to_float_bit_for_bit():
    N, R, HW = 3, 24, 64
    h = W.gen_b("random", (N, R, HW), True, False, 31)
    src, dst = Buf(data=W.pack_tiled(h)), Buf(N * R * HW * 4)
    p = _lib.WgradProbe()
    p.op, p.N, p.HW = _lib.WGRAD_HALF_TO_FLOAT, N, HW
    p.gemm[0].B, p.gemm[0].dw, p.gemm[0].Npad = src.ptr, dst.ptr, R
    rc, info = call(p)
    assert rc == 0 and info.instance[0] == _lib.WGI_HALF_TO_FLOAT and dst.intact() and src.intact()
    assert dst.host(np.float32).tobytes() == h.astype(np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def refused(p, outputs):
    rc, info = call(p)
    assert rc == EINVAL and _lib.lib().glowhip_last_error(), rc
    assert all(b.untouched() for b in outputs), "a refused call wrote to an output"
    assert list(info.instance) == [0, 0, 0]


def mfma_probe(case, fam="random"):
    d = W.build_mfma(case, fam)
    A, B = Buf(data=d["A"]), Buf(data=d["B"])
    p = _lib.WgradProbe()
    p.op, p.N, p.HW, p.sh_scale = _lib.WGRAD_MFMA, case["N"], case["HW"], d["sh_scale"]
    set_taps(p.taps[0], d["taps"])
    dw, part, rs = Buf(case["Mreal"] * case["Nreal"] * 4), Buf(512 * case["Mpad"] * case["Npad"] * 4 // 8), Buf(case["Mpad"] * 8)
    fill_gemm(p.gemm[0], case, d, A, B, part, dw, None)
    return p, (dw, part, rs), (A, B)


def test_refusals_launch_nothing():
    """Whatever the launchers' own checks refuse comes back as GLOWHIP_EINVAL with the outputs untouched: pixels per image that are
    no whole k-tiles, gathered widths 12 and 2, row sums or an fp16 B on the fp32 pipe, a tiled layout on a gathered operand, and
    grouped shapes outside wgrad_pair_ok."""
    plain = W.mfma_case("ref-plain", 2, 8, 4, 100, 100, 128)
    va = W.mfma_case("ref-va", 2, 8, 4, 108, 100, 128, a="taps", mode=1)
    # HW % 32 != 0
    p, outs, keep = mfma_probe(plain)
    p.HW = 24
    refused(p, outs)
    # gathered widths 12 (no power of two) and 2 (below a 4-pixel chunk)
    for (H, W_) in ((8, 12), (16, 2)):
        p, outs, keep = mfma_probe(W.mfma_case("ref-w", 1, H, W_, 108, 100, 128, a="taps", mode=1))
        refused(p, outs)
    # row sums / an fp16 B without sh_scale
    p, outs, keep = mfma_probe(plain)
    p.sh_scale, p.gemm[0].rowsum = 0.0, outs[2].ptr
    refused(p, outs)
    p, outs, keep = mfma_probe(W.mfma_case("ref-bh", 2, 8, 4, 100, 128, 128, b="half"))
    p.sh_scale = 0.0
    refused(p, outs)
    # the pixel-tile-major layout on a gathered operand
    p, outs, keep = mfma_probe(va)
    p.gemm[0].tiled = 1
    refused(p, outs)
    p, outs, keep = mfma_probe(W.mfma_case("ref-vb", 2, 8, 4, 128, 108, 128, b="taps"))
    p.gemm[0].tiled = 2
    refused(p, outs)
    # grouped shapes outside wgrad_pair_ok: a hidden width of 192, an f.0 operand of 192 columns
    grp = W.group_case("ref-pair", 2, 8, 8, 12, False, 256, False)
    for field, value in (("hid", 192), ("n0", 192)):
        p = _lib.WgradProbe()
        p.op, p.N, p.HW, p.sh_scale = _lib.WGRAD_PAIR, grp["N"], grp["HW"], W.RANDOM_SH_SCALE
        outs, keep = [], []
        for i, k in enumerate(("f4", "f0")):
            c = grp["sub"][k]
            d = W.build_mfma(c, "random", seed=i + 1)
            A, B, dw, part = Buf(data=d["A"]), Buf(data=d["B"]), Buf(c["Mreal"] * c["Nreal"] * 4), Buf(6 * c["Mpad"] * c["Npad"] * 4)
            fill_gemm(p.gemm[i], c, d, A, B, part, dw, None)
            set_taps(p.taps[i], d["taps"])
            outs += [dw, part]
            keep += [A, B]
        if field == "hid":
            p.gemm[0].Npad = p.gemm[1].Mpad = 192
        else:
            p.gemm[1].Npad = 192
        refused(p, outs)


def test_zz_report():
    """Prints the worst multiple of the bound per instance and the count of `exact` values compared (the figures of DESIGN section 6);
    asserts nothing that the tests above have not."""
    for name in sorted(WORST):
        print(f"worst multiple of the bound  {name:45s} {WORST[name]:.3f}")
    print(f"exact values compared: {EXACT[0]}, differing: {EXACT[1]}")
    assert EXACT[1] == 0
