"""`Latents`: everything a full-latent encode keeps of a batch -- the top latent ``z`` and, per Split2d, the draw ``eps`` that
its dropped half implies under the prior predicted from the kept half (reference network/module.py:526-536 scores that half and
discards it).  ``decode(z, eps)`` is then the exact inverse of the encode; the container is plain tensors, device-agnostic."""
import torch


class Latents:
    """``z`` (N, C, H, W); ``eps``: list of (N, c, h, w), one per Split2d in DECODE order (deepest split first -- the order
    `FlowModel.decode(eps=)` reads); ``nll`` (N,) bits/dim of the encoded batch, or None."""

    __slots__ = ("z", "eps", "nll")

    def __init__(self, z, eps, nll=None):
        eps = list(eps)
        for e in eps:
            assert e.shape[0] == z.shape[0], f"eps batch {e.shape[0]} != z batch {z.shape[0]}"
        assert nll is None or nll.shape[0] == z.shape[0]
        self.z, self.eps, self.nll = z, eps, nll

    def __len__(self):
        return self.z.shape[0]

    def tensors(self):
        """z and every eps: what `lerp` blends and `decode_latents` reads."""
        return [self.z] + self.eps

    def _map(self, fn):
        return Latents(fn(self.z), [fn(e) for e in self.eps], None if self.nll is None else fn(self.nll))

    def __getitem__(self, idx):
        """Batch indexing: an int keeps the batch axis (length 1); slices, index lists and masks as on a tensor."""
        if isinstance(idx, int):
            n = len(self)
            if not -n <= idx < n:
                raise IndexError(f"index {idx} out of range for {n} latents")
            idx = slice(idx % n, idx % n + 1)
        return self._map(lambda t: t[idx])

    def to(self, *args, **kwargs):
        return self._map(lambda t: t.to(*args, **kwargs))

    def requires_grad_(self, requires_grad=True):
        """Mark z and every eps as leaves that `Glow.decode_latents` differentiates with respect to (detached first where they
        are results of other operations); the nll is carried along unchanged."""
        def leaf(t):
            return (t if t.is_leaf else t.detach()).requires_grad_(requires_grad)
        return Latents(leaf(self.z), [leaf(e) for e in self.eps], self.nll)

    def detach(self):
        """The same latents cut out of any autograd graph (shared storage)."""
        return self._map(lambda t: t.detach())

    def lerp(self, other, t):
        """(1 - t) * self + t * other on every latent tensor.  ``t``: a number, or a (steps,) sequence / tensor -- then both
        sides must hold ONE latent and the result holds ``steps`` of them.  The endpoints are exact (t = 0: self, t = 1: other).
        The result carries no nll."""
        assert len(self.eps) == len(other.eps), "latents of different models"
        if not isinstance(t, (int, float)):
            assert len(self) == 1 and len(other) == 1, "a sequence of weights blends ONE pair of latents"
            t = torch.as_tensor(t, dtype=torch.float32, device=self.z.device).view(-1, 1, 1, 1)

        def blend(a, b):
            assert a.shape == b.shape, (a.shape, b.shape)
            return a * (1.0 - t) + b * t            # (not a + t * (b - a): t = 1 must give b itself)
        return Latents(blend(self.z, other.z), [blend(a, b) for a, b in zip(self.eps, other.eps)])

    def state_dict(self):
        """Plain dict of tensors (torch.save-able): 'z', 'eps.0' .. 'eps.{k-1}' and, when there is one, 'nll'."""
        sd = {"z": self.z}
        sd.update({f"eps.{k}": e for k, e in enumerate(self.eps)})
        if self.nll is not None:
            sd["nll"] = self.nll
        return sd

    @classmethod
    def from_state_dict(cls, sd):
        n_eps = sum(1 for k in sd if k.startswith("eps."))
        unknown = set(sd) - {"z", "nll"} - {f"eps.{k}" for k in range(n_eps)}
        if "z" not in sd or unknown:
            raise KeyError(f"not a Latents state_dict: missing 'z' or unexpected keys {sorted(unknown)}")
        return cls(sd["z"], [sd[f"eps.{k}"] for k in range(n_eps)], sd.get("nll"))

    def __repr__(self):
        return f"Latents(n={len(self)}, z={tuple(self.z.shape[1:])}, eps={[tuple(e.shape[1:]) for e in self.eps]})"
