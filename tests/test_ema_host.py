"""Host checks of the Polyak average (no GPU): the oracle's warm-up rule against hand values, the optimiser's policy against the
oracle, `util.averaged_state_dict` on a hand-made snapshot, and what `build_optimizer` does with and without ``hps.optim.ema_decay``.
The GPU tests (test_gpu_ema.py, test_gpu_ema_model.py) hold the kernels to tests/ema_oracle.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_glow_amd import training
from pytorch_glow_amd.misc import util

import ema_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warmup_rule_against_hand_values():
    assert EO.decay_at(0, 0.999, True) == 0.1                      # (1 + 0) / (10 + 0)
    assert EO.decay_at(1, 0.999, True) == 2.0 / 11.0
    assert EO.decay_at(90, 0.999, True) == 0.91
    assert EO.decay_at(8990, 0.999, True) == 8991.0 / 9000.0       # 0.99900 exactly: the last count the ramp decides
    assert EO.decay_at(8991, 0.999, True) == 0.999 and EO.decay_at(10 ** 6, 0.999, True) == 0.999
    assert EO.decay_at(0, 0.999, False) == 0.999 and EO.decay_at(0, 0.5, True) == 0.1 and EO.decay_at(4, 0.5, True) == 5.0 / 14.0
    assert EO.decay_at(5, 0.5, True) == 0.4 and EO.decay_at(8, 0.5, True) == 0.5 and EO.decay_at(9, 0.5, True) == 0.5
    # w: the subtraction in doubles, then one rounding to float32
    assert EO.weight_at(0, 0.999, True) == float(np.float32(0.9))
    assert EO.weight_at(0, 0.999, False) == float(np.float32(1.0 - 0.999)) != 1.0 - 0.999
    assert EO.weight_at(3, 0.5, False) == 0.5
    # the recurrence and its bound
    assert np.array_equal(EO.advance([1.0, -2.0], [3.0, -2.0], 0.25), [1.5, -2.0])
    assert EO.bound(5, 2.0) == 50.0 * 2.0 ** -24


@pytest.mark.parametrize("cls", [training.HipAdam, training.HipAdamax])
def test_optimiser_policy_is_the_oracles_rule(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    for decay, warmup in ((0.5, False), (0.9, True), (0.999, True), (0.9999, False)):
        opt = cls(p, ema_decay=decay, ema_warmup=warmup)
        for t in (0, 1, 2, 9, 90, 8990, 8991, 10 ** 5):
            assert opt.ema_weight(t) == EO.weight_at(t, decay, warmup), (decay, warmup, t)
        assert len(opt.hyper_values(1e-3, 4)) == 3
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            cls(p, ema_decay=bad)
    off = cls(p)
    assert off.ema_decay == 0.0 and "ema_decay" not in off.defaults and set(off.state_dict()["param_groups"][0]) == \
        {"lr", "betas", "eps", "weight_decay", "params"}


class _Graph(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.b = torch.nn.Parameter(torch.full((2,), 2.0))           # registration order IS parameters() order: b before a
        self.inner = torch.nn.Linear(2, 1)
        self.a = torch.nn.Parameter(torch.full((3,), 1.0))
        self.register_buffer("inited", torch.tensor(1.0))


def test_averaged_state_dict_maps_positions_to_names():
    graph = _Graph()
    names = [n for n, _ in graph.named_parameters()]
    assert names == ["b", "a", "inner.weight", "inner.bias"]
    ema = {0: torch.full((2,), 20.0), 1: torch.full((3,), 10.0), 2: torch.full((1, 2), 30.0)}        # position 3: no average kept
    state = dict(step=5, graph=graph.state_dict(), seconds=0.0, criterion={},
                 optimizer=dict(state={i: dict(step=torch.tensor(5.0), exp_avg=torch.zeros_like(e), exp_avg_sq=torch.zeros_like(e), ema=e)
                                       for i, e in ema.items()},
                                param_groups=[dict(lr=1e-3, params=[0, 1, 2, 3])]))
    state["optimizer"]["state"][3] = dict(step=torch.tensor(5.0))
    out = util.averaged_state_dict(state, graph)
    assert list(out) == list(state["graph"])
    assert torch.equal(out["b"], ema[0]) and torch.equal(out["a"], ema[1]) and torch.equal(out["inner.weight"], ema[2])
    assert torch.equal(out["inner.bias"], state["graph"]["inner.bias"]) and torch.equal(out["inited"], torch.tensor(1.0))
    assert torch.equal(state["graph"]["b"], torch.full((2,), 2.0))        # the snapshot itself is not written to
    out["b"].add_(1.0)
    assert torch.equal(ema[0], torch.full((2,), 20.0))
    graph.load_state_dict(out)

    for st in state["optimizer"]["state"].values():
        st.pop("ema", None)
    with pytest.raises(KeyError, match="no averaged weights"):
        util.averaged_state_dict(state, graph)
    with pytest.raises(KeyError, match="no averaged weights"):
        util.averaged_state_dict(dict(graph=graph.state_dict(), optimizer=None), graph)
    state["optimizer"]["state"][1]["ema"] = torch.zeros(4)
    with pytest.raises(ValueError, match="shape"):
        util.averaged_state_dict(state, graph)


@pytest.mark.parametrize("name", ["celeba", "test"])
def test_reference_profiles_keep_no_average(name):
    hps = util.load_profile(name)
    assert "ema_decay" not in hps.optim and "ema_eval" not in hps.optim and "use_ema" not in hps.general
    opt = training.build_optimizer(hps, [torch.nn.Parameter(torch.zeros(3))])
    assert isinstance(opt, (training.HipAdam, training.HipAdamax)) and opt.ema_decay == 0.0
    hps.optim.ema_decay = 0.0
    assert training.build_optimizer(hps, [torch.nn.Parameter(torch.zeros(3))]).ema_decay == 0.0
    hps.optim.ema_decay, hps.optim.ema_warmup = 0.999, True
    opt = training.build_optimizer(hps, [torch.nn.Parameter(torch.zeros(3))])
    assert opt.ema_decay == 0.999 and opt.ema_warmup is True


def test_torch_optimisers_refuse_an_average():
    """GLOWHIP_TORCH_OPTIM=1 is read when the package is imported: a fresh child process."""
    code = (
        "import torch\n"
        "from pytorch_glow_amd import training\n"
        "from pytorch_glow_amd.misc import util\n"
        "hps = util.load_profile('celeba')\n"
        "p = [torch.nn.Parameter(torch.zeros(3))]\n"
        "assert type(training.build_optimizer(hps, p)) is torch.optim.Adam\n"
        "hps.optim.ema_decay = 0.999\n"
        "try:\n"
        "    training.build_optimizer(hps, p)\n"
        "except ValueError as e:\n"
        "    assert 'ema_decay' in str(e) and 'GLOWHIP_TORCH_OPTIM' in str(e), e\n"
        "    print('REFUSED')\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                         env=dict(os.environ, GLOWHIP_TORCH_OPTIM="1"))
    assert out.returncode == 0 and "REFUSED" in out.stdout, out.stdout + out.stderr
