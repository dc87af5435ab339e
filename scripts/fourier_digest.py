#!/usr/bin/env python3
"""Behaviour table of the Fourier-domain entry points of a libglowhip build, in the manner of scripts/plan_digest.py: per (shape,
batch, weights) a sha256 of every output of glowhip_restore_objective_fourier (loss, grad_x, resid) and of glowhip_fourier2d both
ways, from seeded inputs.  Two builds whose kernels give the same bits print the same table.

    python scripts/fourier_digest.py LIB [LIB ...]

Each library runs in a fresh child process (GLOWHIP_LIB_PATH), one after the other; with several libraries the rows that differ from
the FIRST one's are listed at the end (exit status 1 if any, or if a child fails)."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 2, 2), (3, 4, 8), (3, 8, 4), (2, 16, 64), (3, 64, 64), (1, 256, 2), (1, 2, 256), (1, 256, 256), (3, 128, 128))
BATCHES = (1, 5, 64)
WEIGHTS = ("mask", "real", "ones")


def worker():
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    from pytorch_glow_amd import _lib
    from pytorch_glow_amd.network import fourier2d, fourier2d_adjoint, restore_objective

    # an older build of the same ABI lacks the entry points added since: bind what it has (none of the missing ones is called here)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(handle, n)]:
        print(f"# {os.path.basename(_lib.LIB_PATH)} has no {name}", file=sys.stderr)
        del _lib.SIGNATURES[name]

    dev = "cuda:0"
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().view(torch.int32).numpy().tobytes()).hexdigest()[:16]
    for shape in SHAPES:
        for n in BATCHES:
            if n == 64 and shape[1] * shape[2] > 64 * 64:
                continue
            for weights in WEIGHTS:
                g = torch.Generator().manual_seed(100 * n + shape[1] + shape[2])
                full = (n,) + shape
                x = (torch.rand(full, generator=g) - 0.25).to(dev)
                t = torch.randn(full + (2,), generator=g).to(dev)
                w = inv = None
                if weights != "ones":
                    w = torch.rand(full, generator=g)
                    w = ((w < 1.0 / 3.0).float() if weights == "mask" else w).to(dev)
                    inv = 1.0 / w.sum(dim=(1, 2, 3)).clamp(min=1.0)
                resid = torch.full(full + (2,), float("nan"), device=dev)
                loss, grad = restore_objective(x, t, w, inv, 1, resid_out=resid, fourier=True)
                row = [sha(loss), sha(grad), sha(resid)]
                if weights == "ones":
                    row += [sha(torch.view_as_real(fourier2d(x))), sha(fourier2d_adjoint(t))]
                print("x".join(map(str, shape)), n, weights, *row, flush=True)


def main():
    if len(sys.argv) < 2:
        print(__doc__, file=sys.stderr)
        return 2
    if sys.argv[1] == "--worker":
        worker()
        return 0
    tables = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, GLOWHIP_LIB_PATH=os.path.abspath(lib))
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            print(f"{lib}: the worker failed with status {run.returncode}\n{run.stderr[-2000:]}", file=sys.stderr)
            return 1
        rows = run.stdout.strip().splitlines()
        tables.append(rows)
        print(f"== {lib}: {len(rows)} rows, digest {hashlib.sha256(run.stdout.encode()).hexdigest()[:16]}")
    differ = [(k, a, b) for k, rows in enumerate(tables[1:], 1) for a, b in zip(tables[0], rows) if a != b]
    differ += [(k, "row count", str(len(rows))) for k, rows in enumerate(tables[1:], 1) if len(rows) != len(tables[0])]
    for k, a, b in differ:
        print(f"DIFFERS in {sys.argv[1 + k]}:\n  {a}\n  {b}")
    if len(tables) > 1 and not differ:
        print(f"every row of {len(tables) - 1} further librar{'y' if len(tables) == 2 else 'ies'} equals the first one's")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
