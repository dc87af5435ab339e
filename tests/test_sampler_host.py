"""Host checks of the sampler's random stream (no GPU): the numpy restatement tests/sampler_oracle.py against the Random123 known
answers of Philox4x32-10, the statistics of the draws it defines, and the disjointness of its counters from the dequantisation
stream's.  The GPU tests (test_gpu_sampler.py) hold the kernels to this oracle."""
import ctypes

import numpy as np
import pytest

import pytorch_glow_amd as G
from pytorch_glow_amd import _lib

import sampler_oracle as SO


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, out):
    assert _hex(philox := SO.philox4x32_10(counter, key)) == out, _hex(philox)


def test_known_answers_through_the_vector_path():
    """Counters as arrays (the form every other check uses): one key per call, so the three vectors take three calls."""
    c = [np.array([0, 0xffffffff, v], dtype=np.uint64) for v in (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    for row, key, out in ((0, (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                          (1, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                          (2, (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert _hex(v[row] for v in SO.philox4x32_10(c, key)) == out


def test_uniforms_are_exact_in_fp32_and_open():
    u1, u2 = SO.uniforms(1 << 16, 1234, 0, 0)
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    assert u1.min() > 0.0 and u1.max() < 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    # the extreme words: u1 of 0 and of 0xffffffff
    lo, hi = (0 + 0.5) * 2.0 ** -23, ((0xffffffff >> 9) + 0.5) * 2.0 ** -23
    assert 0.0 < lo and hi < 1.0 and np.float32(hi) < 1.0
    assert np.sqrt(-2.0 * np.log(lo)) <= SO.MAX_ABS < 5.77


def test_moments_of_the_defined_stream():
    worst = SO.check_moments(lambda n, seed, call, stream: SO.normal(n, seed, call, stream))
    print(f"worst: {worst:.2f} standard errors")


def test_std_is_one_fp32_product():
    e = SO.normal(4099, 99, 7, 3)
    assert np.array_equal(SO.normal(4099, 99, 7, 3, std=0.7), e * float(np.float32(0.7)))
    assert SO.normal(5, 99, 7, 3).shape == (5,) and np.array_equal(SO.normal(5, 99, 7, 3), e[:5])


def test_positions_and_streams_differ():
    a = SO.words(64, 1234, 0, 0)
    for other in ((1234, 1, 0), (1234, 0, 1), (1235, 0, 0), (1234, 1 << 32, 0)):
        assert not np.array_equal(a, SO.words(64, *other)), other


def test_counters_disjoint_from_the_dequantisation_stream():
    """The sampler's c3 has a non-zero top byte for every stream 0..254 and every call; the dequantisation stream's c3 is
    call >> 32 < 2^24 for every call < 2^56: no counter of one is a counter of the other."""
    calls = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 56) - 1]
    idx = np.array([0, 1, 3, 4, (1 << 34) - 1, 1 << 34, (1 << 40) + 5], dtype=np.uint64)
    deq = set()
    for c in calls:
        c0, c1, c2, c3 = SO.dequant_counter(idx, c)
        assert int(c3) >> 24 == 0
        deq |= {(int(a), int(b), int(c2), int(c3)) for a, b in zip(c0, c1)}
    for s in (0, 1, 2, 127, 253, 254):
        for c in calls:
            c0, c1, c2, c3 = SO.sampler_counter(idx, c, s)
            assert 1 <= int(c3) >> 24 <= 255 and int(c3) < (1 << 32)
            assert int(c3) & 0xffffff == (c >> 32) & 0xffffff and int(c2) == c & 0xffffffff
            assert not deq & {(int(a), int(b), int(c2), int(c3)) for a, b in zip(c0, c1)}
    # distinct (call, stream) pairs give distinct (c2, c3)
    seen = {(int(SO.sampler_counter(0, c, s)[2]), int(SO.sampler_counter(0, c, s)[3])) for c in calls for s in (0, 1, 254)}
    assert len(seen) == len(calls) * 3


def test_eps_std_mapping():
    """`level_eps_stds` as the numbers the kernels multiply by: (std of the top draw, [std per Split2d in decode order])."""
    import torch
    from pytorch_glow_amd.network.model import level_eps_stds, sampler_stds
    assert sampler_stds(None, 3) == (1.0, [1.0, 1.0])                      # the reference's `eps_std or 1.`
    assert sampler_stds(0.7, 3) == (0.7, [0.7, 0.7]) and sampler_stds(0.7, 1) == (0.7, [])
    assert sampler_stds(0, 2) == (1.0, [1.0])
    assert sampler_stds([0.9, 0.7, 0.5], 3) == (0.9, [0.7, 0.5])
    assert sampler_stds([0.5, 0.0, 0.25], 3) == (0.5, [1.0, 0.25])
    top, splits = sampler_stds(torch.tensor(0.5), 2)
    assert (top, splits) == (0.5, [0.5]) and isinstance(top, float) and isinstance(splits[0], float)
    assert sampler_stds(np.float32(0.25), 2) == (0.25, [0.25])
    for arg in (None, 0.7, [0.9, 0.7, 0.5]):                               # the same levels as the torch-drawn route
        top, splits = level_eps_stds(arg, 3)
        assert sampler_stds(arg, 3) == (float(top or 1.), [float(v or 1.) for v in splits])
    with pytest.raises(ValueError, match="L = 3"):
        sampler_stds([0.5, 0.5], 3)


def test_sampler_position_is_per_process_and_keyed_by_torchs_seed():
    import torch
    from pytorch_glow_amd.network import model as gmodel
    torch.manual_seed(4321)
    gmodel.reset_sampler_stream()
    assert gmodel.sampler_position() == (4321, 0) and gmodel.sampler_position() == (4321, 0)
    assert gmodel.sampler_position(advance=True) == (4321, 0) and gmodel.sampler_position() == (4321, 1)
    assert gmodel.dequant_position()[1] == gmodel.dequant_position()[1]   # (the dequantisation stream counts on its own)
    torch.manual_seed(99)                                                  # a new seed restarts the count
    assert gmodel.sampler_position() == (99, 0)
    gmodel.reset_sampler_stream()


def test_host_side_argument_checks():
    """The entry points refuse what the stream layout cannot number -- before any launch, so this runs without a GPU."""
    lib = G.lib()
    buf = ctypes.c_void_p(256)      # never dereferenced: the calls below fail their argument checks
    assert lib.glowhip_normal_noise(buf, 16, 1, 0, 255, 1.0, None) == -1 and b"stream" in lib.glowhip_last_error()
    assert lib.glowhip_normal_noise(buf, 16, 1, 0, -1, 1.0, None) == -1
    assert lib.glowhip_normal_noise(buf, 16, 1, 1 << 56, 0, 1.0, None) == -1 and b"2^56" in lib.glowhip_last_error()
    assert lib.glowhip_normal_noise(None, 16, 1, 0, 0, 1.0, None) == -1
    assert lib.glowhip_normal_noise(buf, 0, 1, 0, 0, 1.0, None) == 0      # nothing to write: no launch
    d = (_lib.LayerDesc * 2)()
    d[0].kind, d[0].C, d[0].H, d[0].W = _lib.LAYER_SQUEEZE, 3, 8, 8
    d[1].kind, d[1].C, d[1].H, d[1].W = _lib.LAYER_SQUEEZE, 12, 4, 4
    h = lib.glowhip_plan_create(d, 2)
    assert h
    std = (ctypes.c_float * 1)(1.0)
    assert lib.glowhip_plan_bind_sampler(h, buf, std, 1, 0) == -1 and b"Split2d" in lib.glowhip_last_error()
    assert lib.glowhip_plan_bind_sampler(h, ctypes.c_void_p(257), None, 0, 0) == -1 and b"aligned" in lib.glowhip_last_error()
    assert lib.glowhip_plan_bind_sampler(h, buf, None, 0, 1) == 0
    assert lib.glowhip_plan_bind_sampler(h, None, None, 0, 0) == 0
    lib.glowhip_plan_destroy(h)
