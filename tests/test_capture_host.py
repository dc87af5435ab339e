"""The capture protocol, everything that needs no GPU: the pure part of the signature rule (`_capture.moved`) and the optimiser's
side of a captured step (`_HipOptimizer.capturing`) on CPU tensors -- no kernel is called.  The five captured sites are held to
their eager routes bit for bit by the GPU tests of each."""
import pytest
import torch

from pytorch_glow_amd import _capture, training


def test_a_signature_reports_the_one_item_that_moved():
    then = {"parameters": (16, 32), "pack_epoch": 0, "_ws": 4096, "packed": 8192, "family": 0}
    assert _capture.moved(then, dict(then)) == []
    for name, value in (("parameters", (16, 48)), ("pack_epoch", 1), ("_ws", 12288), ("packed", 0), ("family", 1)):
        assert _capture.moved(then, dict(then, **{name: value})) == [name]
    assert _capture.moved(then, dict(then, _ws=1, family=1)) == ["_ws", "family"]      # in the order the site named them
    gone = dict(then)
    del gone["packed"]
    assert _capture.moved(then, gone) == ["packed"]                                   # an item that vanished has moved


def test_an_item_absent_at_capture_is_not_compared():
    then = {"parameters": (16,), "_ws": None, "pack_epoch": 0}
    assert _capture.moved(then, dict(then, _ws=4096)) == []                            # allocated later: no captured launch reaches it
    assert _capture.moved(then, dict(then, _ws=4096, pack_epoch=1)) == ["pack_epoch"]
    assert _capture.moved(then, dict(then, extra=1)) == []                            # nor an item the capture never named
    t = torch.zeros(3)
    assert _capture.address(None) is None and _capture.address(t) == t.data_ptr()      # how a buffer becomes an item


def cpu_optimizer(**kw):
    opt = training.HipAdam([torch.zeros(4, requires_grad=True)], lr=1e-3, **kw)
    opt._steps, opt._ema_t = 7, 5
    opt._table_token = token = object()
    return opt, token


def test_the_capture_context_puts_both_counters_back():
    opt, token = cpu_optimizer(ema_decay=0.9)
    with opt.capturing():
        opt._steps += 1              # what the recorded fused_step counts on the host
        opt._ema_t += 1
    assert (opt._steps, opt._ema_t, opt.ema_updates) == (7, 5, 5)
    assert opt._table_token is token, "a recording that succeeded keeps the chunk table's token"


def test_a_recording_that_raises_restores_the_counters_and_drops_the_table_token():
    opt, token = cpu_optimizer(ema_decay=0.9)
    with pytest.raises(RuntimeError, match="half-way"):
        with opt.capturing():
            opt._steps += 1
            opt._ema_t += 1
            raise RuntimeError("the recording failed half-way")
    assert (opt._steps, opt._ema_t) == (7, 5)
    assert opt._table_token is None
