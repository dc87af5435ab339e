"""`-m gpu`: the kernels of the LU-parameterised invertible 1x1 convolution (csrc/invconv_lu.hip) against fp64, stand-alone and as
one FlowStep of a plan.  W = P (tril(l, -1) + I) (triu(u, 1) + diag(sign_s exp(log_s))); the reference names the option and raises
(network/module.py:336-337), so the yardstick is tests/plu_oracle.py: lu_oracle's matrix families factored on the host into fp32
parameters, every truth recomputed in fp64 from THOSE parameters.  The kernels accumulate in fp64 and store fp32, so the bounds
are lu_oracle's (one fp32 ulp of the fp64 value plus its absolute floor; the dot-product bound for products) and are not tuned.

dlog_s = (L^T P^T dW)_ii s_i + logdet_term is held to (C + 2) 2^-24 (|L|^T |P^T dW|)_ii |s_i| for the product, as dl and du are,
plus 2^-24 |logdet_term| for the fp32 store of a sum that contains the term."""
import numpy as np
import pytest
import torch

import pytorch_glow_amd as G
from pytorch_glow_amd._lib import check, lib, ptr, stream_ptr
import lu_oracle as LU
import plu_oracle as PLU
from test_gpu_parity import DEV, dev
from test_gpu_lu import HW, _apply_multiple, _pixels

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24
TERM = 37.625          # logdet_term of the backward checks (exact in fp32)


def _ids(cases):
    return [f"{f}-{C}" for f, C in cases]


def _filled(shape, dtype=torch.float32):
    """A device tensor whose every byte is 0xA5."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV).view(dtype).reshape(shape)


def _dev_params(f, poison=False):
    t = {n: torch.from_numpy(np.array(f[n])).to(DEV) for n in ("l", "u", "log_s", "sign_s", "perm")}
    if poison:          # NaN in every entry the parameterisation masks
        C = f["l"].shape[0]
        t["l"][torch.triu(torch.ones(C, C, dtype=torch.bool, device=DEV))] = float("nan")
        t["u"][torch.tril(torch.ones(C, C, dtype=torch.bool, device=DEV))] = float("nan")
    return t


def _prepare(f, poison=False, want_inverse=True):
    C = f["l"].shape[0]
    t = _dev_params(f, poison)
    w, winv, lad = _filled((C, C)), _filled((C, C)), _filled((1,))
    check(lib().glowhip_invconv_lu_prepare(ptr(t["perm"]), ptr(t["l"]), ptr(t["u"]), ptr(t["log_s"]), ptr(t["sign_s"]), C, ptr(w),
                                           ptr(winv if want_inverse else None), ptr(lad), stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return w.cpu().numpy(), winv.cpu().numpy(), float(lad.cpu().item())


def _backward(f, dW, term, poison=False):
    C = f["l"].shape[0]
    t = _dev_params(f, poison)
    g = torch.from_numpy(np.array(dW, dtype=np.float32)).to(DEV)
    dl, du, ds = _filled((C, C)), _filled((C, C)), _filled((C,))
    check(lib().glowhip_invconv_lu_backward(ptr(t["perm"]), ptr(t["l"]), ptr(t["u"]), ptr(t["log_s"]), ptr(t["sign_s"]), C, ptr(g),
                                            float(term), ptr(dl), ptr(du), ptr(ds), stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return dl.cpu().numpy(), du.cpu().numpy(), ds.cpu().numpy()


def _dw(C):
    return np.random.RandomState(900 + C).randn(C, C).astype(np.float32)


STANDALONE = PLU.standalone_cases()


@pytest.mark.parametrize("family,C", STANDALONE, ids=_ids(STANDALONE))
def test_standalone_prepare_against_fp64(family, C):
    f = PLU.params(family, C)
    W64, ref_ld, ref_inv = PLU.assemble(f), PLU.logdet(f), PLU.inverse_dense(f)
    w, winv, lad = _prepare(f)
    assert np.isfinite(w).all() and np.isfinite(winv).all() and np.isfinite(lad)
    m_w = float((np.abs(w.astype(np.float64) - W64) / (2.0 ** -23 * np.abs(W64) + U24 * 1e-2 * np.abs(W64).max())).max())
    m_ld = abs(lad - ref_ld) / LU.logdet_bound(ref_ld)
    m_inv = float((np.abs(winv.astype(np.float64) - ref_inv) / LU.inverse_bound(ref_inv)).max())
    print(f"PLU-BOUND prepare {family}-{C} w {m_w:.4f} logdet {m_ld:.4f} inverse {m_inv:.4f}")
    assert m_w <= 1.0 and m_ld <= 1.0 and m_inv <= 1.0, (family, C, m_w, m_ld, m_inv)
    # without an inverse buffer: the same W and log-det, the buffer untouched
    w2, winv2, lad2 = _prepare(f, want_inverse=False)
    assert np.array_equal(w2, w) and lad2 == lad and (winv2.view(np.uint8) == 0xA5).all()


@pytest.mark.parametrize("family,C", STANDALONE, ids=_ids(STANDALONE))
def test_standalone_backward_against_fp64(family, C):
    f = PLU.params(family, C)
    dW = _dw(C)
    rdl, rdu, rds, bl, bu, bs = PLU.backward(f, dW, TERM)
    dl, du, ds = _backward(f, dW, TERM)
    k = (C + 2) * U24
    lower, upper = np.tril(np.ones((C, C), bool), -1), np.triu(np.ones((C, C), bool), 1)
    assert not dl[~lower].any() and not du[~upper].any(), "masked gradient entries must be exact zeros"
    m_l = float((np.abs(dl - rdl)[lower] / np.maximum(k * bl[lower], 1e-300)).max()) if lower.any() else 0.0
    m_u = float((np.abs(du - rdu)[upper] / np.maximum(k * bu[upper], 1e-300)).max()) if upper.any() else 0.0
    m_s = float((np.abs(ds - rds) / (k * bs + U24 * abs(TERM))).max())
    print(f"PLU-BOUND backward {family}-{C} dl {m_l:.4f} du {m_u:.4f} dlog_s {m_s:.4f}")
    assert m_l <= 1.0 and m_u <= 1.0 and m_s <= 1.0, (family, C, m_l, m_u, m_s)
    # dW = 0: the log-det term alone reaches log_s, exactly; l and u get nothing
    zl, zu, zs = _backward(f, np.zeros((C, C), np.float32), 0.3)
    assert not zl.any() and not zu.any()
    assert np.array_equal(zs, np.full(C, np.float32(0.3)))


NAN_CASES = [("orth", C) for C in PLU.STANDALONE_C] + [("anti", 66), ("sign", 130)]


@pytest.mark.parametrize("family,C", NAN_CASES, ids=_ids(NAN_CASES))
def test_masked_entries_are_never_read(family, C):
    """NaN in every entry of l on or above and of u on or below the diagonal: every output keeps its bits."""
    f = PLU.params(family, C)
    dW = _dw(C)
    clean = _prepare(f) + _backward(f, dW, TERM)
    dirty = _prepare(f, poison=True) + _backward(f, dW, TERM, poison=True)
    for a, b in zip(clean, dirty):
        assert np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


# ---------------------------------------------------------------- one FlowStep as a plan
_STEPS = {}


def _step(C, lu):
    """The FlowStep of tests/test_gpu_lu.py (hidden 64, additive, zero f.4, identity ActNorm marked inited, 4x4 map) of width C, in
    the LU form or dense; built once per (width, form)."""
    if (C, lu) not in _STEPS:
        np.random.seed(C)
        torch.manual_seed(C)
        st = G.FlowStep(C, 64, permutation="invconv", coupling="additive", lu_decomposition=lu)
        for m in st.modules():
            if isinstance(m, G.ActNorm):
                m.bias_inited = m.logs_inited = True
        st = st.to(DEV).eval()
        _STEPS[(C, lu)] = (st, st._plan(torch.empty(2, C, 4, 4, device=DEV)))
    return _STEPS[(C, lu)]


def _run(C, lu, setter, reverse):
    st, plan = _step(C, lu)
    setter(st)
    x = dev(_pixels(C, 2 if reverse else 1))
    ld0 = torch.zeros(2, device=DEV)
    plan.launch_counts(reset=True)
    if reverse:
        out, ld = plan.decode(x, [], ld0, want_logdet=True, repack=True)
    else:
        out, ld = plan.encode(x, None, ld0, want_logdet=True, repack=True)
    torch.cuda.synchronize()
    return out.cpu(), ld.cpu(), plan.launch_counts(reset=True)


def _dense_pack_keys(C, reverse):
    """The pack counters of a dense FlowStep of width C as tests/lu_oracle.py tables them (what tests/test_gpu_lu.py asserts)."""
    if reverse:
        return {LU.BATCHED, LU.R_GJ_LDS if C <= 64 else LU.R_GJ_GLOBAL}
    if C in LU.WAVE_C:
        return {LU.FUSED}
    # (the route borders lu_oracle.FORWARD_ROUTES straddles: 128 | 130 and 448 | 450)
    return {LU.BATCHED, LU.R_LDS if C <= 128 else (LU.R_BLOCKED if C <= 448 else LU.R_GLOBAL)}


PLAN = PLU.plan_cases()


@pytest.mark.parametrize("family,C", PLAN, ids=_ids(PLAN))
def test_flowstep_plan_forward_and_inverting_pack(family, C):
    f = PLU.params(family, C)
    W64, ref_ld, ref_inv = PLU.assemble(f), PLU.logdet(f), PLU.inverse_dense(f)

    def set_lu(st):
        for n in PLU.NAMES:
            getattr(st.invconv, n).data.copy_(torch.from_numpy(np.array(f[n])).to(DEV))
        for n in ("l", "u", "log_s"):                   # (the version counters the plan watches, as an optimiser step moves them)
            getattr(st.invconv, n).add_(0)
        st.invconv.p.add_(0)

    # forward-only pack + encode
    z, ld, c = _run(C, True, set_lu, reverse=False)
    assert c.get("pack:invconv_lu") == 1 and not [k for k in c if k.startswith("pack:lu:")], c
    assert torch.isfinite(ld).all() and ld[0] == ld[1], ld
    m_ld = abs(ld[0].item() / HW - ref_ld) / LU.logdet_bound(ref_ld)
    m_z, mixer = _apply_multiple(W64, _pixels(C, 1), z, c)
    # inverting pack + decode
    x, ldr, cr = _run(C, True, set_lu, reverse=True)
    assert cr.get("pack:invconv_lu") == 1 and not [k for k in cr if k.startswith("pack:lu:")], cr
    assert torch.isfinite(ldr).all() and ldr[0] == ldr[1], ldr
    m_ldr = abs(-ldr[0].item() / HW - ref_ld) / LU.logdet_bound(ref_ld)
    m_x, mixer_r = _apply_multiple(ref_inv, _pixels(C, 2), x, cr)
    print(f"PLU-BOUND plan {family}-{C} logdet {m_ld:.4f} z({mixer}) {m_z:.4f} logdet(rev) {m_ldr:.4f} x({mixer_r}) {m_x:.4f}")
    assert m_ld <= 1.0 and m_z <= 1.0 and m_ldr <= 1.0 and m_x <= 1.0, (family, C, m_ld, m_z, m_ldr, m_x)
    # the assembled matrix the plan's mixers read is the stand-alone kernel's, bit for bit
    st, _ = _step(C, True)
    assert np.array_equal(st.invconv.weight.cpu().numpy(), _prepare(f, want_inverse=False)[0])

    # the dense twin (same fp32 W): the counters it had before the LU form existed, nothing new; and the LU plan launches what
    # the twin launches outside the pack
    Wf = st.invconv.weight.clone()

    def set_dense(sd):
        sd.invconv.weight.copy_(Wf)

    for reverse, mine, zz in ((False, c, z), (True, cr, x)):
        out, _, cd = _run(C, False, set_dense, reverse)
        assert {k for k in cd if k.startswith("pack:")} == _dense_pack_keys(C, reverse), (C, reverse, cd)
        assert not [k for k in cd if "invconv_lu" in k], cd
        assert {k for k in cd if not k.startswith("pack:")} == {k for k in mine if not k.startswith("pack:")}, (cd, mine)
        if not reverse:
            assert torch.equal(out, zz), "the same kernels read the same fp32 W"
