"""glowhip_grad_accumulate (csrc/accumulate.hip) through the C ABI, bit for bit against tests/accumulate_oracle.py (-m gpu).

Every segment is a view into one allocation per side, at a chosen offset (in floats) from a 16-byte boundary, with guard words
either side of it.  The alignment pairs cover every route of the kernel: both aligned (16-byte accesses from the first element),
a common offset (peeled head), and offsets that differ (element by element).  Lengths: around the 16-byte access, the 256-thread
block and the 4 096-element tile, one of 3 M elements (733 workgroups), and -- in a test of their own -- sizes either side of the
grid cap of 2 048 workgroups (8.4 M elements), from which the stride loop runs."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytorch_glow_amd as G  # noqa: E402
from pytorch_glow_amd import _lib  # noqa: E402

import accumulate_oracle as AO  # noqa: E402

DEV = "cuda:0"
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 65537, 3_000_001]
# (offset of grad, offset of acc) from a 16-byte boundary, in floats
ALIGNMENTS = {"both_aligned": (0, 0), "grad_off_by_one": (1, 0), "acc_off_by_one": (0, 1), "both_off_by_one": (1, 1),
              "off_by_different_amounts": (1, 2), "common_peel_of_one": (3, 3)}
SCALES = [0.5, float(np.float32(1.0 / 3.0)), 1.0]
GUARD = 8                     # guard words either side of every segment
GUARD_BITS = 0x7bcdef12       # a finite pattern no arithmetic here produces


def values(rng, n):
    """Normal-range randoms over magnitudes 1e-6 .. 1e3 with planted +-0, +-inf and NaN; no subnormals."""
    v = (10.0 ** rng.uniform(-6, 3, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    k = min(n, max(1, n // 50))
    v[rng.choice(n, size=k, replace=False)] = special[rng.integers(0, len(special), size=k)]
    return v


class Case:
    """Segments of the given lengths laid out in one `grad` and one `acc` allocation; numpy mirrors of both."""

    def __init__(self, lengths, offsets, seed):
        rng = np.random.default_rng(seed)
        self.lengths = list(lengths)
        self.slots = []       # (start in grad buffer, start in acc buffer, n)
        pos = [0, 0]
        for n, (og, oa) in zip(self.lengths, offsets):
            start = []
            for side, off in ((0, og), (1, oa)):
                base = (pos[side] + GUARD + 3) // 4 * 4 + off          # a 16-byte boundary behind the guard, plus the offset
                start.append(base)
                pos[side] = base + n + GUARD
            self.slots.append((start[0], start[1], n))
        guard = np.array([GUARD_BITS], dtype=np.int32).view(np.float32)[0]
        self.g_host = np.full(pos[0] + 4, guard, dtype=np.float32)
        self.a_host = np.full(pos[1] + 4, guard, dtype=np.float32)
        for sg, sa, n in self.slots:
            self.g_host[sg:sg + n] = values(rng, n)
            self.a_host[sa:sa + n] = values(rng, n)
            if n >= 8:          # both sides special at the same place: inf + -inf, NaN + NaN, -0 + -0, 0 + -0
                self.g_host[sg:sg + 4] = np.array([np.inf, np.nan, -0.0, 0.0], dtype=np.float32)
                self.a_host[sa:sa + 4] = np.array([-np.inf, np.nan, -0.0, -0.0], dtype=np.float32)
        self.g_dev = torch.from_numpy(self.g_host.copy()).to(DEV)
        self.a_dev = torch.from_numpy(self.a_host.copy()).to(DEV)
        assert self.g_dev.data_ptr() % 16 == 0 and self.a_dev.data_ptr() % 16 == 0
        entries = [_lib.GradSeg(self.g_dev.data_ptr() + 4 * sg if n else 0, self.a_dev.data_ptr() + 4 * sa if n else 0, n)
                   for sg, sa, n in self.slots]
        self.table = (_lib.GradSeg * len(entries))(*entries)

    def refresh_grad(self, seed):
        """New gradient contents in place (same addresses), host mirror alike."""
        rng = np.random.default_rng(seed)
        for sg, _, n in self.slots:
            self.g_host[sg:sg + n] = values(rng, n)
        self.g_dev.copy_(torch.from_numpy(self.g_host))

    def launch(self, mode, scale=1.0):
        _lib.check(G.lib().glowhip_grad_accumulate(self.table, len(self.table), mode, scale, _lib.stream_ptr(torch.device(DEV))))

    def expect(self, mode, scale=1.0):
        """Apply the oracle to the host mirrors."""
        for sg, sa, n in self.slots:
            g, a = AO.apply(mode, self.g_host[sg:sg + n], self.a_host[sa:sa + n], scale)
            self.g_host[sg:sg + n], self.a_host[sa:sa + n] = g, a

    def check(self, what):
        """The whole of both allocations -- segments, guard words, gaps -- equals the host mirrors."""
        g, a = self.g_dev.cpu().numpy(), self.a_dev.cpu().numpy()
        for name, got, want in (("grad", g, self.g_host), ("acc", a, self.a_host)):
            if not AO.same_bits(got, want):
                bad = np.nonzero(AO.bits(got) != AO.bits(want))[0]
                raise AssertionError(f"{what}: {name} differs at {len(bad)} of {len(want)} words, first {bad[:5]}: "
                                     f"{got[bad[:5]]} vs {want[bad[:5]]} (slots {self.slots})")

    def step(self, mode, scale, what):
        before_g, before_a = self.g_host.copy(), self.a_host.copy()
        self.launch(mode, scale)
        self.expect(mode, scale)
        if mode in (AO.FIRST, AO.ADD):
            assert AO.same_bits(self.g_host, before_g)       # (the oracle's own contract: grad untouched)
        else:
            assert AO.same_bits(self.a_host, before_a)       # acc untouched
        self.check(what)


@pytest.mark.parametrize("align", list(ALIGNMENTS))
def test_each_mode_equals_the_oracle_to_the_bit(align):
    """One segment per call, every length, every mode: FIRST leaves grad and writes acc = g; ADD leaves grad; FINISH leaves acc and
    writes (acc + g) * scale for scale = 1/2, 1/3, 1 -- every word of both allocations compared, guard words included."""
    og, oa = ALIGNMENTS[align]
    for i, n in enumerate(LENGTHS):
        case = Case([n], [(og, oa)], seed=1000 + i)
        case.step(AO.FIRST, 7.0, f"{align} n={n} FIRST")                  # (scale is ignored by FIRST and ADD)
        case.refresh_grad(2000 + i)
        case.step(AO.ADD, float("nan"), f"{align} n={n} ADD")
        for j, scale in enumerate(SCALES):
            case.refresh_grad(3000 + 10 * i + j)
            case.step(AO.FINISH, scale, f"{align} n={n} FINISH x{scale}")


@pytest.mark.parametrize("count", [2, 16])
def test_several_segments_in_one_launch(count):
    """2 and 16 segments per call, an empty one among them, alignments mixed from segment to segment (so the routes differ
    inside one launch), the 3 M segment among the sixteen."""
    if count == 2:
        lengths, offsets = [1025, 5], [(1, 1), (0, 0)]
        cases = [Case(lengths, offsets, seed=41), Case([0, 257], [(0, 0), (2, 1)], seed=42), Case([4, 0], [(0, 0), (0, 0)], seed=43)]
    else:
        lengths = [1, 3, 4, 5, 255, 256, 257, 0, 1023, 1024, 1025, 65537, 4096, 4097, 8191, 3_000_001]
        pairs = list(ALIGNMENTS.values())
        cases = [Case(lengths, [pairs[(i + shift) % len(pairs)] for i in range(16)], seed=50 + shift) for shift in (0, 1)]
    for c, case in enumerate(cases):
        case.step(AO.FIRST, 1.0, f"{count} segments, case {c}, FIRST")
        case.refresh_grad(60 + c)
        case.step(AO.ADD, 1.0, f"{count} segments, case {c}, ADD")
        case.refresh_grad(70 + c)
        case.step(AO.FINISH, SCALES[1], f"{count} segments, case {c}, FINISH")


GRID_CAP = 2048 * 4096        # elements of as many tiles (4 096 elements) as the grid has workgroups at its cap (csrc/accumulate.hip)


@pytest.mark.parametrize("lengths,offsets", [
    ([GRID_CAP - 4096], [(0, 0)]),                   # one tile short of the cap: one tile per workgroup
    ([GRID_CAP + 1], [(0, 0)]),                      # one tile beyond it, of one element: workgroup 0 strides once
    ([9_000_003], [(3, 3)]),                         # the stride loop behind a peeled head, a ragged last tile and a scalar tail
    ([9_000_003], [(1, 2)]),                         # the stride loop, element by element
    ([5, 8_400_000, 0, 4097], [(0, 0), (1, 1), (0, 0), (2, 1)]),      # a workgroup's tiles lie in different segments
])
def test_launches_beyond_the_grid_cap(lengths, offsets):
    """From 2 048 tiles on the grid is at its cap and a workgroup strides over several tiles -- of different segments, where the
    launch has several.  Same checks, same oracle."""
    case = Case(lengths, offsets, seed=700 + len(lengths))
    case.step(AO.FIRST, 1.0, f"{lengths} FIRST")
    case.refresh_grad(710)
    case.step(AO.ADD, 1.0, f"{lengths} ADD")
    case.refresh_grad(720)
    case.step(AO.FINISH, SCALES[1], f"{lengths} FINISH")


def _round(case, seeds):
    """FIRST, ADD, ADD, FINISH over four gradient contents; returns the four host gradients per slot for the oracle."""
    grads = []
    for mode, seed in zip(AO.modes(4), seeds):
        case.refresh_grad(seed)
        grads.append([case.g_host[sg:sg + n].copy() for sg, _, n in case.slots])
        case.launch(mode, float(AO.scale_for(4)))
    return grads


def test_four_micro_steps_equal_the_oracle_composition():
    lengths = [5, 1025, 65537, 300_001]
    case = Case(lengths, [(0, 0), (1, 1), (1, 2), (0, 0)], seed=80)
    grads = _round(case, [81, 82, 83, 84])
    got = case.g_dev.cpu().numpy()
    for s, (sg, _, n) in enumerate(case.slots):
        want = AO.compose([grads[i][s] for i in range(4)])
        assert AO.same_bits(got[sg:sg + n], want), (s, n)
        mean = np.stack([grads[i][s] for i in range(4)]).astype(np.float64)
        finite = np.isfinite(mean).all(0)
        with np.errstate(all="ignore"):
            err = np.abs(got[sg:sg + n].astype(np.float64) - mean.sum(0) / 4)[finite]
        assert (err <= 4 * 2.0 ** -24 * np.abs(mean).sum(0)[finite]).all()      # and that is the mean, to fp32 rounding


def test_captured_round_replays_to_the_eager_bits():
    """FIRST, ADD, ADD, FINISH captured in one graph between device-side copies of four staged gradients into the segment buffer;
    two replays on refreshed staging contents equal the eager launches on the same contents."""
    lengths = [257, 4099, 70_001]
    offsets = [(0, 0), (3, 3), (2, 1)]
    case = Case(lengths, offsets, seed=90)
    stage = [torch.empty_like(case.g_dev) for _ in range(4)]
    scale = float(AO.scale_for(4))
    dev = torch.device(DEV)

    def body():
        for mode, st in zip(AO.modes(4), stage):
            case.g_dev.copy_(st)
            case.launch(mode, scale)

    def fill(seeds):
        for st, seed in zip(stage, seeds):
            case.refresh_grad(seed)
            st.copy_(case.g_dev)

    side = torch.cuda.Stream(device=dev)
    fill([91, 92, 93, 94])
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()                                   # warm-up on the capture stream
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        body()
    for seeds in ([101, 102, 103, 104], [111, 112, 113, 114]):
        fill(seeds)
        body()
        torch.cuda.synchronize(dev)
        eager_g, eager_a = case.g_dev.cpu().numpy().copy(), case.a_dev.cpu().numpy().copy()
        scrambled = eager_a.copy()               # (FIRST overwrites: nothing of the eager round may be needed)
        for _, sa, n in case.slots:
            scrambled[sa:sa + n] = np.nan
        case.a_dev.copy_(torch.from_numpy(scrambled))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert AO.same_bits(case.g_dev.cpu().numpy(), eager_g) and AO.same_bits(case.a_dev.cpu().numpy(), eager_a)
        # ... and the eager bits are the oracle's
        for s, (sg, _, n) in enumerate(case.slots):
            grads = []
            for seed in seeds:
                rng = np.random.default_rng(seed)
                per_slot = [values(rng, m) for _, _, m in case.slots]
                grads.append(per_slot[s])
            assert AO.same_bits(eager_g[sg:sg + n], AO.compose(grads)), (s, n)
