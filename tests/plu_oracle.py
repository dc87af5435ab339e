"""Host side of the LU-parameterised invconv tests (tests/test_lu_param_host.py, tests/test_gpu_lu_param*.py), in fp64.

The parameterisation is W = P (tril(l, -1) + I) (triu(u, 1) + diag(sign_s exp(log_s))) with fp32 parameters (csrc/invconv_lu.hip).
The test matrices are tests/lu_oracle.py's families, factored here on the host into fp32 parameters; the fp64 TRUTH of every check
is recomputed from those fp32 parameters (widened exactly), never taken from the matrix that was factored: the rounding of the
factors is the caller's business, not the kernels'.

  assemble / logdet        W and sum(log_s)
  inverse_dense / _solve   W^-1 by two independent routes: numpy's inverse of the assembled matrix, and U_f^-1 (L^-1 P^T) by two
                           solves on the factors -- their difference, against lu_oracle.inverse_bound, says how far the yardstick
                           itself can be trusted (conditioning_ratios; held to 1e-2 on the host)
  backward                 dl, du, dlog_s of the stand-alone gradient call as fp64 products, with the operand-magnitude products
                           |A||B| the dot-product bound of lu_oracle.apply_bound needs
  glow_grads               gradients of mean(nll) of a whole model: W built from l, u, log_s as torch fp64 leaves and fed to
                           oracle.glow_oracle under the dense key
"""
import numpy as np
import torch

import lu_oracle as LU

NAMES = ("p", "l", "u", "log_s", "sign_s")
STANDALONE_C = (1, 2, 12, 48, 64, 66, 130, 200, 384, 512)     # the stand-alone kernels: below / at / above the 16-, 32- and 64-wide tiles
PLAN_C = (12, 48, 66, 200, 384)                              # one FlowStep as a plan


def standalone_cases():
    return [(f, C) for C in STANDALONE_C for f in LU.families_for(C)]


def plan_cases():
    return [(f, C) for C in PLAN_C for f in LU.families_for(C)]

_cache = {}


def factor(W):
    """fp32 LU parameters (numpy dict p, l, u, log_s, sign_s + the int32 row table perm) of a dense matrix: partial pivoting in
    fp64 (torch.linalg.lu), rounded to fp32."""
    P, L, U = torch.linalg.lu(torch.from_numpy(np.array(W, dtype=np.float64)))
    d = torch.diagonal(U)
    out = dict(p=P.numpy().astype(np.float32), l=torch.tril(L, -1).numpy().astype(np.float32),
               u=torch.triu(U, 1).numpy().astype(np.float32), log_s=d.abs().log().numpy().astype(np.float32),
               sign_s=torch.sign(d).numpy().astype(np.float32))
    out["perm"] = out["p"].argmax(axis=1).astype(np.int32)
    return out


def params(family, C, seed=LU.SEED):
    """factor(lu_oracle.matrix(family, C)), cached and read-only."""
    key = (family, C, seed)
    if key not in _cache:
        f = factor(LU.matrix(family, C, seed))
        for v in f.values():
            v.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def factors64(f):
    """(P, L, U_f) in fp64 from the fp32 parameters; masked entries of l / u are ignored whatever they hold."""
    C = f["l"].shape[0]
    L = np.tril(np.nan_to_num(f["l"].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0), -1) + np.eye(C)
    s = f["sign_s"].astype(np.float64) * np.exp(f["log_s"].astype(np.float64))
    U = np.triu(np.nan_to_num(f["u"].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0), 1) + np.diag(s)
    return f["p"].astype(np.float64), L, U


def assemble(f):
    P, L, U = factors64(f)
    return P @ (L @ U)


def abs_product(f):
    """|L| |U_f| with the rows permuted as W's: the magnitude the rounding of the factors scales with."""
    P, L, U = factors64(f)
    return P @ (np.abs(L) @ np.abs(U))


def logdet(f):
    return float(f["log_s"].astype(np.float64).sum())


def inverse_dense(f):
    return np.linalg.inv(assemble(f))


def inverse_solve(f):
    P, L, U = factors64(f)
    return np.linalg.solve(U, np.linalg.solve(L, P.T))


def conditioning_ratios(f):
    """(inverse, logdet): the two inverse routes' difference over lu_oracle.inverse_bound (elementwise maximum), and
    |sum(log_s) - slogdet(W)| over lu_oracle.logdet_bound."""
    a, b = inverse_dense(f), inverse_solve(f)
    r_inv = float((np.abs(a - b) / LU.inverse_bound(a)).max())
    ld = logdet(f)
    r_ld = abs(ld - float(np.linalg.slogdet(assemble(f))[1])) / LU.logdet_bound(ld)
    return r_inv, r_ld


def backward(f, dW, logdet_term):
    """(dl, du, dlog_s, bound_l, bound_u, bound_s): the fp64 gradients of the factors for dW (the gradient w.r.t. W without a
    log-det part) and logdet_term, and the products of operand magnitudes |A||B| behind each (bound_s: for the product alone)."""
    P, L, U = factors64(f)
    G = np.asarray(dW, dtype=np.float64)
    A = P.T @ G
    s = np.diag(U)
    full_l, full_u = A @ U.T, L.T @ A
    mag_l, mag_u = np.abs(A) @ np.abs(U).T, np.abs(L).T @ np.abs(A)
    dl, du = np.tril(full_l, -1), np.triu(full_u, 1)
    dlog_s = np.diag(full_u) * s + float(logdet_term)
    return dl, du, dlog_s, np.tril(mag_l, -1), np.triu(mag_u, 1), np.diag(mag_u) * np.abs(s)


# ---------------------------------------------------------------- whole models
def dense_state_dict(sd, dtype=torch.float64):
    """State dict of an lu_decomposition=True model -> the dense-key state dict oracle.glow_oracle reads, W assembled in `dtype`
    with torch from the (fp32) factors.  Differentiable w.r.t. tensors of `sd` that require grad."""
    out = {}
    done = set()
    for k, v in sd.items():
        if ".invconv." in k:
            prefix = k[:k.index(".invconv.") + len(".invconv.")]
            if prefix in done:
                continue
            done.add(prefix)
            p, l, u, log_s, sign_s = (sd[prefix + n].to(dtype) for n in NAMES)
            eye = torch.eye(l.shape[0], dtype=dtype)
            out[prefix + "weight"] = p @ (torch.tril(l, -1) + eye) @ (torch.triu(u, 1) + torch.diag(sign_s * torch.exp(log_s)))
        else:
            out[k] = v.to(dtype) if v.is_floating_point() else v
    return out


def glow_grads(cfg, sd, x, noise):
    """mean(nll) of the fp64 oracle and its gradient for every floating-point entry of `sd` but h_top and the LU buffers:
    ({name: grad}, loss, nll, z)."""
    from oracle import glow_oracle as O
    fixed = ("h_top",)
    with torch.enable_grad():
        leaf = {k: v.detach().double().clone().requires_grad_(not (k in fixed or k.endswith(".invconv.p") or k.endswith(".invconv.sign_s")))
                for k, v in sd.items()}
        z, nll, _ = O.glow_forward(x.double(), noise.double(), dense_state_dict(leaf), cfg)
        loss = nll.mean()
        loss.backward()
    return {k: v.grad for k, v in leaf.items() if v.grad is not None}, float(loss), nll.detach(), z.detach()
