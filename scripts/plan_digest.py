#!/usr/bin/env python3
"""Behaviour table of a libglowhip build, for executor refactors: per (model, debug switch, operation) the plan's launch counts
and a sha256 of every output tensor, from seeded weights and inputs.  Two builds that run the same kernels on the same arguments
print the same table.  Operations: encode, decode, init (the data-dependent ActNorm pass of a fresh model: z, nll and every ActNorm
bias / logs), decode_vjp and train; the switches of PACK_ONLY change the pack alone and run the first three.

    python scripts/plan_digest.py LIB [LIB ...]

Each library runs in a fresh child process (GLOWHIP_LIB_PATH).  The tables go to stdout, one after the other, each followed by its
row count and digest; with several libraries the rows that differ from the FIRST one's are listed at the end (exit status 1 if
any).  Give the parent's library twice first: a row that differs between its own two runs is not deterministic there (fp64 atomics
over more pixel blocks than accumulator copies) and is no evidence either way."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(hw=(16, 16), L=2, K=2, hidden=32, batch=3)
L3 = dict(hw=(64, 64), L=3, K=2, hidden=512, batch=4)
DEEP = dict(hw=(128, 128), L=6, K=1, hidden=64, batch=3)
MODELS = {      # affine + invconv unless said otherwise
    "tiny-affine": TINY, "tiny-additive-reverse": dict(TINY, coup="additive", perm="reverse"),
    "64x64-h512-b4": L3, "64x64-h512-b28": dict(L3, batch=28),      # backward k_cnet: pair GEMMs / the one-wave instances, trio
    "64x64-h256-additive-shuffle": dict(hw=(64, 64), L=3, K=1, hidden=256, batch=4, coup="additive", perm="shuffle"),
    "48x80-h128": dict(hw=(48, 80), L=2, K=2, hidden=128, batch=2), "8x64-h128-shuffle": dict(hw=(8, 64), L=2, K=2, hidden=128, batch=3, perm="shuffle"),
    "256x256-L4-h512": dict(hw=(256, 256), L=4, K=1, hidden=512, batch=2),      # four levels, C = 12 .. 96
    "128x128-L6": DEEP, "128x128-L6-additive-shuffle": dict(DEEP, coup="additive", perm="shuffle"),      # wide mixer at C = 384
    "tiny-lu": dict(TINY, lu=True), "tiny-ycond": dict(TINY, batch=4, ycond=True),
}
SWITCHES = {"none": [], "per_layer_bwd": ["TRAIN_PER_LAYER_BWD"], "per_layer_fwd": ["TRAIN_PER_LAYER_FWD"],
            "per_layer_both": ["TRAIN_PER_LAYER_FWD", "TRAIN_PER_LAYER_BWD"], "exact_fp32": ["EXACT_FP32"],
            "no_cnet1w_bwd": ["NO_CNET1W_BWD"], "wgrad_narrow": ["WGRAD_NARROW"], "no_mixer_fusion": ["NO_MIXER_FUSION"],
            "pack_unfused": ["PACK_UNFUSED"], "lu_workgroup": ["LU_WORKGROUP"], "pack_one_stream": ["PACK_ONE_STREAM"]}
PACK_ONLY = ("pack_unfused", "lu_workgroup", "pack_one_stream")      # these change the pack alone: encode, decode and init rows


def worker():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import pytorch_glow_amd as G
    from pytorch_glow_amd import _lib
    from pytorch_glow_amd.misc import util
    from pytorch_glow_amd.network import Latents

    dev = "cuda:0"
    sha = lambda t: hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()[:12]

    def hps(m, lu):
        return util.AttrDict(dict(
            model=dict(image_shape=[m["hw"][0], m["hw"][1], 3], hidden_channels=m["hidden"], K=m["K"], L=m["L"], actnorm_scale=1.0,
                       n_bits_x=8, weight_y=0.5 if m.get("ycond") else 0.0),
            ablation=dict(learn_top=bool(m.get("ycond")), y_condition=bool(m.get("ycond")), y_criterion="single_class", lu_decomposition=lu,
                          flow_permutation=m.get("perm", "invconv"), flow_coupling=m.get("coup", "affine")),
            optim=dict(num_batch_train=m["batch"]), dataset=dict(num_classes=5 if m.get("ycond") else 1), device=dict(graph=[dev])))

    def state(m):      # seeded parameters away from every special value; the LU form is the dense weights factored
        np.random.seed(1)
        g = torch.Generator().manual_seed(5)
        sd = {k: v.detach().clone() for k, v in G.Glow(hps(m, False)).state_dict().items()}
        for k, v in sd.items():
            if k.endswith("invconv.weight"):
                sd[k] = torch.from_numpy(np.linalg.qr(np.random.randn(*v.shape))[0].astype("float32")) + 0.05 * torch.randn(v.shape, generator=g)
            elif v.is_floating_point() and k != "h_top":
                sd[k] = torch.randn(v.shape, generator=g) * (0.1 if k.endswith(("logs", "bias")) else 0.02 if (".f.4." in k or "zeros" in k) else 0.05)
        return util.lu_state_dict_from_dense(sd) if m.get("lu") else sd

    for name, m in MODELS.items():
        sd, g = state(m), torch.Generator().manual_seed(7)
        n, shape = m["batch"], (m["batch"], 3) + m["hw"]
        x, noise, gx = torch.rand(shape, generator=g).to(dev), (torch.rand(shape, generator=g) / 256).to(dev), torch.randn(shape, generator=g).to(dev)
        y = torch.nn.functional.one_hot(torch.arange(n) % 5, 5).float().to(dev) if m.get("ycond") else None
        for sw, bits in SWITCHES.items():
            with _lib.debug_flags(sum(int(_lib.DBG[b]) for b in bits)):
                def model():
                    np.random.seed(2)      # (the fixed permutations are drawn at construction)
                    glow = G.Glow(hps(m, bool(m.get("lu"))))
                    glow.load_state_dict({k: v.clone() for k, v in sd.items()})
                    return glow.to(dev)

                glow = model().eval()
                glow.set_actnorm_inited()
                plan = glow.flow.plan_for(x)
                z0 = torch.randn((n,) + tuple(plan.out_chw), generator=g).to(dev) * 0.7
                eps = [(torch.randn((n,) + tuple(s), generator=g) * 0.7).to(dev) for s in plan.split_chw]

                def row(op, outs, plan=plan):
                    torch.cuda.synchronize()
                    counts = " ".join(f"{k}={v}" for k, v in sorted(plan.launch_counts(reset=True).items()))
                    print(f"{name} | {sw} | {op} | {counts} | " + " ".join(f"{k}:{sha(t)}" for k, t in outs), flush=True)

                plan.launch_counts(reset=True)
                with torch.no_grad():
                    z, nll, _ = glow.normal_flow(x, y, noise=noise)
                    row("encode", [("z", z), ("nll", nll)])
                    row("decode", [("x", glow.reverse_flow(z0, y, eps=eps))])
                    fresh = model().train()      # data-dependent ActNorm init: the first training-mode forward of an un-initialised model
                    z, nll, _ = fresh.normal_flow(x, y, noise=noise)
                    row("init", [("z", z), ("nll", nll)] + [(k, p) for k, p in fresh.named_parameters() if k.endswith(("bias", "logs")) and "actnorm" in k],
                        fresh.flow.plan_for(x))
                if sw in PACK_ONLY:
                    continue
                with torch.enable_grad():
                    lat = Latents(z0.clone(), [e.clone() for e in eps]).requires_grad_()
                    grads = torch.autograd.grad(glow.decode_latents(lat, safe=False), lat.tensors(), gx)
                    row("decode_vjp", [("grad_z", grads[0])] + [(f"grad_eps{i}", t) for i, t in enumerate(grads[1:])])
                    glow.train()
                    xd = x.clone().requires_grad_(True)
                    z, nll, _ = glow.normal_flow(xd, y, noise=noise)
                    nll.mean().backward()
                    row("train", [("z", z), ("nll", nll), ("grad_x", xd.grad)] + [(k, p.grad) for k, p in glow.named_parameters() if p.grad is not None])


def main(libs):
    tables = []
    for lib in libs:
        env = dict(os.environ, GLOWHIP_LIB_PATH=os.path.abspath(lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
        rows = out.splitlines()
        print(out, end="")
        print(f"# {lib}: {len(rows)} rows, sha256 {hashlib.sha256(out.encode()).hexdigest()[:16]}", flush=True)
        tables.append(rows)
    bad = 0
    for lib, rows in zip(libs[1:], tables[1:]):
        diff = [a.split(" | ")[:3] for a, b in zip(tables[0], rows) if a != b]
        print(f"# {lib} against {libs[0]}: {len(diff)} rows differ" + (" (and the row counts)" if len(rows) != len(tables[0]) else ""), *diff, sep="\n#   ")
        bad += len(diff) + (len(rows) != len(tables[0]))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--worker"]:
        worker()
    elif len(sys.argv) < 2:
        sys.exit(__doc__)
    else:
        sys.exit(main(sys.argv[1:]))
