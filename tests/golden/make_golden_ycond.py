#!/usr/bin/env python3
"""Generate g10_glow_tiny_ycond.npz by running the REAL reference's class-conditional Glow (ablation.y_condition,
network/model.py:345-348, 362-379, 440-445, 508-538; trainer.py:100-131).

Runs only where the reference is available (see make_golden.py, whose stubs and helpers this imports):

    python -B tests/golden/make_golden_ycond.py

Tiny Glow 16x16x3, L 2, K 2, hidden 32, affine + invconv, batch 4, num_classes 5, weight_y 0.5, randomised parameters.
Cases {learn_top off, on} x {ce: CrossEntropy with integer y, bce: BCEWithLogits with a multi-hot y_onehot}; ONE flow state
dict, input and dequantisation draw shared by the four (so z is shared too).  Per case: nll, y_logits, both loss terms, every
parameter gradient and dx of loss = generative + weight_y * classification (split_channel clone shim as g7_grads), and a
conditional sample + a reconstruction with every eps draw recorded.  learn_top.weight multiplies h_top == 0; it is filled
with a constant so that it costs no fixture bytes, and its (exactly zero) gradient is recorded as a flag only.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (installs the stubs, puts the reference on sys.path)

rmodel, rops = MG.rmodel, MG.rops
NUM_CLASSES, WEIGHT_Y = 5, 0.5


def hps_for(learn_top):
    hps = MG.tiny_hps("affine", "invconv")
    hps.ablation.y_condition = True
    hps.ablation.learn_top = learn_top
    hps.dataset.num_classes = NUM_CLASSES
    hps.model.weight_y = WEIGHT_Y
    return hps


def keys_with_shapes(sd):
    return np.array(sorted("{}|{}".format(k, ",".join(str(d) for d in v.shape)) for k, v in sd.items()))


def main():
    orig_split = rops.split_channel
    rops.split_channel = lambda t, s="simple": tuple(a.clone() for a in orig_split(t, s))
    out = {}
    try:
        g = torch.Generator().manual_seed(9876)
        np.random.seed(11)
        full = rmodel.Glow(hps_for(True))
        MG.randomize_(full, g, std=0.1)
        with torch.no_grad():
            full.h_top.zero_()
            full.learn_top.weight.fill_(0.01)
            full.learn_top.bias.copy_(torch.randn(full.learn_top.bias.shape, generator=g) * 0.3)
        sd_full = {k: v.clone() for k, v in full.state_dict().items()}
        out.update({f"sd.{k}": v for k, v in sd_full.items()})
        x0 = torch.rand(4, 3, 16, 16, generator=g)
        y = torch.tensor([1, 4, 0, 2])
        labels = {"ce": torch.nn.functional.one_hot(y, NUM_CLASSES).float(),
                  "bce": torch.tensor([[1, 0, 1, 0, 0], [0, 1, 1, 0, 1], [0, 0, 0, 0, 0], [1, 1, 0, 1, 0]], dtype=torch.float32)}
        out.update(x=x0, y=y, y_onehot_ce=labels["ce"], y_onehot_bce=labels["bce"], weight_y=np.float32(WEIGHT_Y),
                   num_classes=np.int64(NUM_CLASSES))
        for lt in (0, 1):
            np.random.seed(11)
            glow = rmodel.Glow(hps_for(bool(lt)))
            sd = {k: v for k, v in sd_full.items() if lt or not k.startswith("learn_top.")}
            glow.load_state_dict(sd)          # strict: the key set of this case
            out[f"keys_lt{lt}"] = keys_with_shapes(glow.state_dict())
            glow.set_actnorm_inited()
            glow.eval()
            for crit in ("ce", "bce"):
                tag = f"lt{lt}_{crit}"
                yo = labels[crit]
                glow.zero_grad()
                x = x0.clone().requires_grad_(True)
                torch.manual_seed(41)
                z, nll, y_logits = glow(x=x, y_onehot=yo, reverse=False)
                torch.manual_seed(41)
                noise = torch.nn.init.uniform_(torch.empty(*x.shape), 0, 1. / 2 ** glow.hps.model.n_bits_x)
                assert tuple(y_logits.shape) == (4, NUM_CLASSES)
                loss_gen = rmodel.Glow.generative_loss(nll)
                loss_cls = (rmodel.Glow.single_class_loss(y_logits, y) if crit == "ce"
                            else rmodel.Glow.multi_class_loss(y_logits, yo))
                loss = loss_gen + WEIGHT_Y * loss_cls
                loss.backward()
                if "noise" in out:
                    assert torch.equal(out["noise"], noise) and torch.equal(out["z"], z.detach())
                out.update(noise=noise, z=z.detach())
                out.update({f"{tag}.nll": nll.detach(), f"{tag}.y_logits": y_logits.detach(), f"{tag}.loss_generative": loss_gen.detach(),
                            f"{tag}.loss_classes": loss_cls.detach(), f"{tag}.loss": loss.detach(), f"{tag}.dx": x.grad.detach()})
                none = []
                for name, p_ in glow.named_parameters():
                    if p_.grad is None:
                        none.append(name)
                    elif name == "learn_top.weight":
                        assert float(p_.grad.abs().max()) == 0.0
                        out[f"{tag}.learn_top_weight_grad_is_zero"] = np.bool_(True)
                    else:
                        out[f"{tag}.grad.{name}"] = p_.grad.detach()
                assert none == ["h_top"], none
                with torch.no_grad():
                    with MG.EpsTap() as tap:          # conditional sample: top draw first, then one per Split2d
                        torch.manual_seed(43)
                        xs = glow(z=None, y_onehot=yo, eps_std=0.6, reverse=True)
                    out[f"{tag}.sample_x"] = xs
                    for j, e in enumerate(tap.draws):
                        out[f"{tag}.sample_eps{j}"] = e
                    with MG.EpsTap() as tap:          # reconstruction from z
                        torch.manual_seed(44)
                        xr = glow(z=z.detach().clone(), y_onehot=yo, eps_std=0.6, reverse=True)
                    out[f"{tag}.recon_x"] = xr
                    for j, e in enumerate(tap.draws):
                        out[f"{tag}.recon_eps{j}"] = e
    finally:
        rops.split_channel = orig_split
    path = os.path.join(HERE, "g10_glow_tiny_ycond.npz")
    np.savez_compressed(path, **MG.npd(out))
    print(f"g10_glow_tiny_ycond.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
