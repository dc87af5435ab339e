"""GPU tests of the fold kernel (-m gpu): glowhip_eval_reset / glowhip_eval_fold (csrc/evaluate.hip) against the fp64 oracle of
tests/evaluate_oracle.py.

Bounds.  Per-image bits/dim: inputs are fp32 objectives and the output is ONE fp32 rounding of an fp64 value -- 4 * 2^-24 relative
(the fp64 arithmetic on either side differs by parts in 2^-50, which may move the rounding by one ulp).  Counts, histogram, min,
max and the sums of bpd and bpd^2 are integers GIVEN the per-image values the kernel wrote: exact.  The sums of bpd_single and of
the level bits are integer sums of fp64 values that are not output: device and oracle may round an image's value to neighbouring
multiples of 2^-32, so they agree to one unit of 2^-32 per image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_glow_amd.network.evaluate import EvalState, _s128  # noqa: E402

import evaluate_oracle as EO  # noqa: E402

DEV = "cuda:0"
D = 3 * 64 * 64
HIST = (16, 0.0, 8.0)
REL = 4 * 2.0 ** -24


def objectives(K, N, seed, n_levels=0):
    """fp32 objectives near -25 000 nats with spreads of up to +-60 nats between the draws of an image (image 0 -- and every image
    at K = 1 -- has equal draws), and level terms that add up to them (minus the constant offset) in fp64."""
    rs = np.random.RandomState(seed)
    base = -25000.0 + rs.uniform(-3000, 3000, size=N)
    spread = rs.uniform(0, 60, size=N)
    spread[0] = 0.0
    o = (base[None, :] + spread[None, :] * rs.uniform(-1, 1, size=(K, N))).astype(np.float32)
    terms = None
    if n_levels:
        share = rs.dirichlet(np.ones(n_levels), size=(K, N)).transpose(0, 2, 1)      # (K, n_levels, N)
        terms = (share * (o.astype(np.float64)[:, None, :] + 8 * np.log(2.0) * D)).astype(np.float32)
    return o, terms


def run_fold(chunks, n_levels=0, hist=HIST, total=None, only_if_nan=None, state=None, per_image=None):
    """Fold (objective, terms, offset) chunks into one state; returns (host state, per-image array, EvalState)."""
    total = total if total is not None else sum(c[0].shape[1] for c in chunks)
    state = state or EvalState(DEV, n_levels, hist)
    if per_image is None:
        per_image = torch.full((total,), -7.0, dtype=torch.float32, device=DEV)      # (a sentinel no fold writes)
    for o, t, off in chunks:
        od = torch.from_numpy(np.ascontiguousarray(o)).to(DEV)
        td = None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(DEV)
        mask = None if only_if_nan is None else per_image[off:off + o.shape[1]]
        state.fold(od, td, D, per_image, off, only_if_nan=mask)
    return state.read(), per_image.cpu().numpy(), state


def check_state(st, per, o, terms, hist=HIST):
    """Everything the issue asks of one fold against the oracle."""
    ref = EO.fold(o, D, terms=terms, hist=hist)
    keep = ref["keep"]
    assert np.isnan(per[~keep]).all() and np.isfinite(per[keep]).all()
    rel = np.abs(per[keep].astype(np.float64) - ref["bpd"][keep]) / np.abs(ref["bpd"][keep])
    print(f"K={o.shape[0]} N={o.shape[1]}: per-image bpd rel err max {rel.max() if rel.size else 0.0:.3e} (bound {REL:.3e})")
    assert (rel <= REL).all()
    given = EO.fold(o, D, terms=terms, hist=hist, bpd32=per)      # the integer state GIVEN the kernel's per-image values
    assert (st.count, st.flagged) == (given["count"], given["flagged"])
    assert _s128(st.sum_bpd) == given["sum_bpd"] and _s128(st.sum_bpd2) == given["sum_bpd2"]
    if given["count"]:
        assert int(st.min_key) - 2 ** 63 == given["min"] and int(st.max_key) - 2 ** 63 == given["max"]
    if hist is not None:
        assert list(st.hist[:hist[0]]) == given["hist"] and (st.under, st.over) == (given["under"], given["over"])
        assert sum(st.hist) + st.under + st.over == st.count
    units = given["count"]      # one unit of 2^-32 per image (module docstring)
    d = abs(_s128(st.sum_single) - given["sum_single"])
    print(f"   sum_single differs from the oracle by {d} units of 2^-32 (bound {units})")
    assert d <= units
    if terms is not None:
        for l in range(terms.shape[1]):
            dl = abs(_s128(st.sum_level[l]) - given["sum_level"][l])
            assert dl <= units, (l, dl)
        # the levels decompose the draw-averaged figure: n_bits + sum_l level_bits = bpd_single, to the roundings of the fp32 terms
        tot = 8 * 2 ** 32 * given["count"] + sum(_s128(st.sum_level[l]) for l in range(terms.shape[1]))
        assert abs(tot - _s128(st.sum_single)) <= given["count"] * (terms.shape[1] * 2.0 ** -24 * 30000 / (EO.LN2 * D) * 2 ** 32 + terms.shape[1] + 1)
    return ref


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 3, 257])
def test_fold_against_the_fp64_oracle(N, K):
    o, terms = objectives(K, N, seed=10 * N + K, n_levels=3)
    st, per, _ = run_fold([(o, terms, 0)], n_levels=3)
    ref = check_state(st, per, o, terms)
    assert st.flagged == 0 and st.count == N
    single32 = ref["single"]
    assert (per.astype(np.float64) <= single32 * (1 + REL) + 1e-12).all()      # Jensen, per image


def test_fold_without_level_terms_and_without_histogram():
    o, _ = objectives(2, 257, seed=4)
    st, per, _ = run_fold([(o, None, 0)], hist=None)
    check_state(st, per, o, None, hist=None)
    assert st.bins == 0 and sum(st.hist) == 0 and all(_s128(st.sum_level[l]) == 0 for l in range(16))


def test_non_finite_draws_flag_the_image_and_leave_the_sums_alone():
    o, terms = objectives(2, 257, seed=5, n_levels=2)
    bad = [3, 130, 256]
    o2 = o.copy()
    o2[1, 3], o2[0, 130], o2[1, 256] = np.nan, np.inf, -np.inf
    st, per, _ = run_fold([(o2, terms, 0)], n_levels=2)
    assert st.flagged == 3 and st.count == 254 and np.isnan(per[bad]).all()
    check_state(st, per, o2, terms)
    keep = np.setdiff1d(np.arange(257), bad)
    st_ref, per_ref, _ = run_fold([(o[:, keep], terms[:, :, keep], 0)], n_levels=2)
    for name in ("sum_bpd", "sum_bpd2", "sum_single"):
        assert _s128(getattr(st, name)) == _s128(getattr(st_ref, name)), name
    assert [_s128(st.sum_level[l]) for l in range(2)] == [_s128(st_ref.sum_level[l]) for l in range(2)]
    assert (st.min_key, st.max_key, list(st.hist)) == (st_ref.min_key, st_ref.max_key, list(st_ref.hist))
    assert np.array_equal(per[keep], per_ref)
    # NaN level terms of an image with finite objectives flag it too: a part is never summed when it is not a number
    t3 = terms.copy()
    t3[0, 1, 7] = np.nan
    st3, per3, _ = run_fold([(o, t3, 0)], n_levels=2)
    assert st3.flagged == 1 and np.isnan(per3[7])


def test_histogram_edges_land_where_the_header_says():
    """bins = 16 over [0, 8): bin i holds [i / 2, (i + 1) / 2).  A value exactly at lo belongs to bin 0, one exactly at hi to the
    overflow counter, one on an inner edge to the upper bin -- and the neighbours one fp32 step below to the lower one."""
    want = np.array([0.0, 8.0, 2.5, np.nextafter(np.float32(2.5), np.float32(0)), np.nextafter(np.float32(8.0), np.float32(0)),
                     -0.001, 7.5], dtype=np.float32)
    # K = 1 and dims = 1 / ln2: bpd = -objective exactly (ln2 * dims rounds to 1.0 in fp64)
    dims = 1.0 / EO.LN2
    assert 1.0 / (EO.LN2 * dims) == 1.0
    state = EvalState(DEV, 0, HIST)
    per = torch.zeros(len(want), dtype=torch.float32, device=DEV)
    state.fold(torch.from_numpy(-want[None, :].copy()).to(DEV), None, dims, per, 0)
    st = state.read()
    assert np.array_equal(per.cpu().numpy(), want)
    hist = list(st.hist[:16])
    assert hist[0] == 1 and hist[5] == 1 and hist[4] == 1 and hist[15] == 2 and sum(hist) == 5
    assert st.over == 1 and st.under == 1 and st.count == 7
    for v in want:
        assert EO.hist_slot(float(v), *HIST) in ("under", "over") or hist[EO.hist_slot(float(v), *HIST)] >= 1


def test_state_is_byte_identical_for_any_partition_and_order():
    o, terms = objectives(3, 257, seed=6, n_levels=3)
    st1, per1, _ = run_fold([(o, terms, 0)], n_levels=3)
    cuts = [(200, 257), (0, 64), (64, 200)]
    chunks = [(o[:, a:b], terms[:, :, a:b], a) for a, b in cuts]
    st2, per2, _ = run_fold(chunks, n_levels=3, total=257)
    assert bytes(st1) == bytes(st2)
    assert np.array_equal(per1, per2)


def test_only_if_nan_folds_the_marked_images_alone():
    o, terms = objectives(2, 67, seed=7, n_levels=2)
    first = o.copy()
    marked = [0, 5, 66]
    first[0, marked] = np.nan
    st1, per1, state = run_fold([(first, terms, 0)], n_levels=2)
    assert st1.flagged == 3 and st1.count == 64
    # the re-run: the repaired objectives for everybody, but image 5 is still not a number
    again = o.copy()
    again[1, 5] = np.inf
    per_dev = torch.from_numpy(per1).to(DEV)
    st2, per2, _ = run_fold([(again, terms, 0)], n_levels=2, only_if_nan=True, state=state, per_image=per_dev)
    assert st2.count == 66 and st2.flagged == 1 and np.isnan(per2[5])
    others = np.setdiff1d(np.arange(67), marked)
    assert np.array_equal(per2[others], per1[others])      # untouched
    keep = np.setdiff1d(np.arange(67), [5])
    st_ref, per_ref, _ = run_fold([(o[:, keep], terms[:, :, keep], 0)], n_levels=2)
    assert np.array_equal(per2[keep], per_ref)
    st2.flagged = 0
    assert bytes(st2) == bytes(st_ref)      # every image counted exactly once: the state of the 66 good images
