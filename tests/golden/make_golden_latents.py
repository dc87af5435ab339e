#!/usr/bin/env python3
"""Generate g11_glow_latents.npz: what the REAL reference's Split2d layers score and drop (network/module.py:526-530), recorded so
that the full-latent encode of the HIP path has reference numbers to stand against.

Runs only where the reference is available (see make_golden.py, whose stubs and helpers this imports):

    python -B tests/golden/make_golden_latents.py

Glow 32x32x3, L 3 (two Split2d), K 2, hidden 32, affine + invconv, batch 4, every parameter randomised (std 0.1), so the priors'
mean / logs are not zero.  The reference's `flow.layers` are walked as its `FlowModel.encode` walks them (network/model.py:274-276);
at each Split2d the dropped half z2, the prior (mean, logs) of the kept half and eps = (z2 - mean) * exp(-logs) are recorded.  The
walk must end on the z of the reference's own forward.  Then the reference decodes (z, eps) itself: its `GaussianDiag.eps`
(network/module.py:408-421) is replaced for that call by one that hands out the recorded draws, deepest split first.

Arrays: x, noise, z, nll, sd.<key>; per Split2d k in DECODE order (0 = the deepest): z2_k, mean_k, logs_k, eps_k; recon_x.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (installs the stubs, puts the reference on sys.path)

rmod, rmodel, rops = MG.rmod, MG.rmodel, MG.rops


def hps():
    h = MG.tiny_hps("affine", "invconv")
    h.model.image_shape = [32, 32, 3]
    h.model.L = 3
    return h


class EpsFeed:
    """Replace GaussianDiag.eps by one that returns recorded draws in the order the decode asks for them."""

    def __init__(self, draws):
        self.draws = list(draws)
        self.orig = rmod.GaussianDiag.eps

    def __enter__(self):
        feed = self

        def eps(shape_tensor, eps_std=None):
            e = feed.draws.pop(0)
            assert e.shape == shape_tensor.shape, (e.shape, shape_tensor.shape)
            return e.clone()

        rmod.GaussianDiag.eps = staticmethod(eps)
        return self

    def __exit__(self, *a):
        rmod.GaussianDiag.eps = staticmethod(self.orig)


def main():
    g = torch.Generator().manual_seed(2468)
    np.random.seed(17)
    glow = rmodel.Glow(hps())
    MG.randomize_(glow, g, std=0.1)
    with torch.no_grad():
        glow.h_top.zero_()
    glow.eval()
    x = torch.rand(4, 3, 32, 32, generator=g)
    out = {"x": x}
    out.update({f"sd.{k}": v.clone() for k, v in glow.state_dict().items()})
    with torch.no_grad():
        z, nll, noise = MG.run_glow(glow, x, 21)
        out.update(noise=noise, z=z, nll=nll)
        # the reference's encode loop, with a look inside every Split2d
        h, logdet, splits = x + noise, torch.zeros(4), []
        for layer in glow.flow.layers:
            if isinstance(layer, rmod.Split2d):
                z1, z2 = rops.split_channel(h, 'simple')
                mean, logs = layer.prior(z1)
                splits.append(dict(z2=z2.clone(), mean=mean.clone(), logs=logs.clone(), eps=(z2 - mean) * torch.exp(-logs)))
            h, logdet = layer(h, logdet, reverse=False)
        assert torch.equal(h, z), "the walk is not the reference's encode"
        splits = splits[::-1]      # decode order: deepest first
        assert len(splits) == 2
        for k, s in enumerate(splits):
            out.update({f"{name}_{k}": v for name, v in s.items()})
        with EpsFeed([s["eps"] for s in splits]) as feed:
            recon = glow(z=z.clone(), eps_std=None, reverse=True)
        assert not feed.draws, "the reference's decode did not ask for every draw"
        out["recon_x"] = recon
        err = (recon - (x + noise)).abs().max().item()
        print(f"reference round trip: max |decode(z, eps) - (x + noise)| = {err:.2e}; min logs "
              f"{min(s['logs'].min().item() for s in splits):.3f}, max |eps| {max(s['eps'].abs().max().item() for s in splits):.2f}")
    path = os.path.join(HERE, "g11_glow_latents.npz")
    np.savez_compressed(path, **MG.npd(out))
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "g11_glow_latents.npz")
    print(f"g11_glow_latents.npz: {size / 1024:.1f} KiB, {len(out)} arrays (largest other fixture {largest / 1024:.1f} KiB)")
    assert size <= largest, "fixture larger than the largest one already there"


if __name__ == "__main__":
    main()
