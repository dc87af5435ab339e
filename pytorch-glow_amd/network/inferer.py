"""`Inferer` of the reference (network/inferer.py:10-188): the inverse-path application -- sampling, encode / decode of a
single image, and attribute manipulation in latent space -- on the HIP flow path.

Differences, all deliberate:
* `compute_attribute_delta` accumulates on the device (two matrix products per batch instead of a Python loop over
  samples x classes and a device->host copy per image) and, in a multi-process run, ends with ONE all-reduce of the
  (classes, C, H, W) sums and the counts -- images are independent, so ranks just see different batches.
* The reference's accumulation loop runs `for i in range(len(batch))` where `batch` is the DICT of the data loader
  (inferer.py:131): it visits len({'x', 'y_onehot'}) = 2 samples of every batch, not the batch.  `samples_per_batch=None`
  (default) uses every sample -- what the method documents; `samples_per_batch="reference"` reproduces the loop as written
  (the parity tests check both against the oracle).
* `sample` returns the batch; building an image grid is torchvision's job (`make_grid`), outside the flow path.
* Beyond the reference: the full-latent calls `encode_full` / `decode_full` / `reconstruct` / `interpolate` and
  `apply_attribute_delta(keep_details=True)`.  The reference's encode keeps the top latent only -- every Split2d's other half
  is scored and dropped (network/module.py:526-536) -- so its decode re-draws all finer detail; these keep the per-level eps
  (`Glow.encode_latents`), take batches as they are (no `make_batch` replication) and round-trip an image to rounding."""
import numpy as np
import torch
import torch.distributed as dist

from ..misc import util
from .latents import Latents


class Inferer:
    def __init__(self, hps, graph, devices, data_device):
        self.hps = hps
        self.graph = graph
        self.graph.eval()
        self.devices = devices
        self.data_device = data_device
        self.batch_size = self.graph.h_top.shape[0]
        self.num_classes = self.hps.dataset.num_classes
        self.y_condition = self.hps.ablation.y_condition
        self.device = self.graph.h_top.device

    def sample(self, z, y_onehot, eps_std=0.5, *, in_kernel=False, uint8=False, seed=None, call=None):
        """Images drawn from the model (z=None: the top latent is sampled too), inferer.py:41-62.  ``eps_std``: one temperature,
        or one per level in decode order (the top prior's first, then every Split2d's from the deepest).
        ``in_kernel=True`` (or a ``seed`` / ``call`` / ``uint8``; only with ``z=None``): the sampler route, `Glow.sample` --
        every draw is made inside the kernel that consumes it and the batch is named by its ``(seed, call)``.  The images are
        distributed the same; the bits differ from the default route, whose draws are torch's."""
        with torch.no_grad():
            if in_kernel or uint8 or seed is not None or call is not None:
                assert z is None, "the sampler route draws the top latent itself"
                return self.graph.sample(y_onehot=y_onehot, eps_std=eps_std, uint8=uint8, seed=seed, call=call)
            return self.graph(z=z, y_onehot=y_onehot, eps_std=eps_std, reverse=True)

    def resample_details(self, img, levels, eps_std=None, seed=None, call=None):
        """Variations of an image that keep its layout: the image's full latents (`encode_full`) are decoded with the top latent
        and the deepest Split2d draws as they are, while the finest ``levels`` Split2d layers draw afresh inside their kernels
        (the sampler's stream at ``(seed, call)``, or the process's position).  ``levels=0`` is `reconstruct`.  ``eps_std``: the
        std of the fresh draws (a number, or one per level as for `sample`)."""
        from .model import sampler_position, sampler_stds
        with torch.no_grad():
            lat = self.encode_full(img)
            flow = self.graph.flow
            plan = flow.plan_for(flow.in_chw, self.device)
            n_split = plan.n_split
            assert 0 <= levels <= n_split, f"levels = {levels}: the model has {n_split} Split2d layers"
            if levels == 0:
                out = self.decode_full(lat)
                return out[0] if img.dim() == 3 else out
            eps = list(lat.eps[:n_split - levels]) + [None] * levels      # decode order: the finest splits come last
            key, c = sampler_position(advance=seed is None and call is None)
            key = key if seed is None else int(seed) & (2 ** 64 - 1)
            c = c if call is None else int(call)
            plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
            plan.bind_sampler(plan.sampler_position(key, c), sampler_stds(eps_std, flow.L)[1], advance=False)
            try:
                out, _, _ = plan.sample(len(lat), z=lat.z, eps=eps)      # (z is given: the prior is not evaluated)
            finally:
                plan.bind_sampler(None)
            return out[0] if img.dim() == 3 else out

    def encode(self, img):
        """Latent of ONE image (C,H,W tensor; a batch is accepted and its first latent returned), inferer.py:64-85."""
        with torch.no_grad():
            if not torch.is_tensor(img):
                raise TypeError("encode takes a tensor; image decoding (cv2 / PIL) is outside this package")
            if len(img.shape) == 3:
                img = util.make_batch(img, self.batch_size)
            z, _, _ = self.graph(img.to(self.device))
            return z[0, :, :, :]

    def decode(self, z):
        """Image of ONE latent, inferer.py:87-102."""
        with torch.no_grad():
            if len(z.shape) == 3:
                z = util.make_batch(z, self.batch_size)
            return self.graph(z=z.to(self.device), y_onehot=None, reverse=True)[0, :, :, :]

    # ---- full latents (beyond the reference): nothing dropped, so decode_full(encode_full(img)) is img
    def _batch(self, img):
        if not torch.is_tensor(img):
            raise TypeError("takes a tensor; image decoding (cv2 / PIL) is outside this package")
        return (img[None] if img.dim() == 3 else img).to(self.device)

    def encode_full(self, img, y_onehot=None, dequantize=False):
        """`Latents` of an image (C,H,W) or a batch (N,C,H,W), fp32 in [0, 1] or uint8.  No dequantisation noise by default:
        the latents then decode to the image itself."""
        return self.graph.encode_latents(self._batch(img), y_onehot, dequantize=dequantize)

    def decode_full(self, latents):
        """Images (N,C,H,W) of `Latents`, each Split2d fed the latents' own eps."""
        return self.graph.decode_latents(latents.to(self.device))

    def reconstruct(self, img):
        """decode_full(encode_full(img)): the image back, to fp32 rounding; a (C,H,W) input gives a (C,H,W) output."""
        out = self.decode_full(self.encode_full(img))
        return out[0] if img.dim() == 3 else out

    def interpolate(self, img_a, img_b, steps):
        """``steps`` images on the straight line between two images in latent space -- every latent tensor blended, top
        latent and per-level eps alike -- from ONE decode of a batch of ``steps``; the first is img_a, the last img_b."""
        assert steps >= 2, "an interpolation has two endpoints"
        a, b = self._batch(img_a), self._batch(img_b)
        assert a.shape[0] == 1 and b.shape[0] == 1 and a.shape == b.shape, "interpolate takes two single images of one shape"
        both = self.encode_full(torch.cat([a, b]))
        t = torch.linspace(0.0, 1.0, steps, device=self.device)
        t[-1] = 1.0
        return self.decode_full(both[0].lerp(both[1], t))

    def fit_latents(self, target, mask=None, steps=100, lr=0.05, init=None):
        """Latents whose decode matches ``target`` (C,H,W or N,C,H,W) where ``mask`` (broadcastable to it; None = everywhere) is
        set: in-painting / projection by gradient descent on the latent tensors.  Starts from ``encode_full(target)`` (or
        ``init``), minimises the masked squared error of `Glow.decode_latents` with torch.optim.Adam, the gradient coming from the
        differentiable decode.  Returns ``(Latents, [loss per step])``; the model's parameters get no gradient."""
        target = self._batch(target).float()
        m = torch.ones_like(target) if mask is None else torch.as_tensor(mask, dtype=torch.float32, device=self.device).expand_as(target)
        lat = (self.encode_full(target) if init is None else init.to(self.device)).detach()
        lat = Latents(lat.z.clone(), [e.clone() for e in lat.eps]).requires_grad_()
        opt = torch.optim.Adam(lat.tensors(), lr=lr)
        history = []
        with torch.enable_grad():
            for _ in range(steps):
                opt.zero_grad(set_to_none=True)
                loss = ((self.graph.decode_latents(lat, safe=False) - target) ** 2 * m).sum() / m.sum().clamp(min=1.0)
                loss.backward()
                opt.step()
                history.append(loss.detach())
        return lat.detach(), [float(v) for v in torch.stack(history).cpu()] if history else []

    def _linear_problem(self, measurement, weight, pool, init, chains, psf, operator):
        """`_problem` with a dense ``operator`` (M,C,H,W): the measurement is (N, M) -- (M,) for one problem -- and so is the weight;
        ``init`` None = all-zero latents, the prior's mode (there is no image to encode); ``chains`` > 1 repeats a single measurement
        and shares the one operator.  Every refusal is a ValueError raised before any device work."""
        from .restore import check_operator_shape
        if psf is not None or int(pool) != 1:
            raise ValueError("operator: a dense operator excludes psf, and pool must be 1")
        if not torch.is_tensor(operator) or not torch.is_tensor(measurement):
            raise TypeError("operator and measurement are tensors (network.restore.gaussian_operator makes an operator on the device)")
        m, _ = check_operator_shape(operator.shape, self.graph.flow.in_chw)
        if measurement.dim() not in (1, 2) or measurement.shape[-1] != m:
            raise ValueError(f"measurement of shape {tuple(measurement.shape)}: expected (N, {m}) or ({m},) with this operator")
        n = 1 if measurement.dim() == 1 else measurement.shape[0]
        if weight is not None:
            wshape = tuple(weight.shape) if torch.is_tensor(weight) else tuple(torch.as_tensor(weight).shape)
            if len(wshape) not in (1, 2) or wshape[-1] != m or (len(wshape) == 2 and wshape[0] not in (1, n)):
                raise ValueError(f"weight of shape {wshape}: expected ({n}, {m}) or ({m},) with this operator")
        if chains < 1 or (chains > 1 and n != 1):
            raise ValueError(f"chains = {chains}: several chains run on ONE measurement (a batch of {n} runs one chain each)")
        if operator.dtype != torch.float32 or not operator.is_contiguous() or not operator.is_cuda:
            raise ValueError("operator must be a contiguous fp32 tensor on the device (it is held by reference, never copied)")
        meas = measurement.reshape(n, m).to(self.device).float().contiguous()
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32, device=self.device).expand(n, m).contiguous()
        if chains > 1:
            meas = meas.expand(chains, m).contiguous()
            weight = None if weight is None else weight.expand(chains, m).contiguous()
            n = chains
        if init is None:
            plan = self.graph.flow.plan_for(tuple(operator.shape[1:]), self.device)
            zeros = lambda chw: torch.zeros((n,) + tuple(chw), dtype=torch.float32, device=self.device)
            init = Latents(zeros(plan.out_chw), [zeros(chw) for chw in plan.split_chw])
        elif chains > 1 and len(init) == 1:
            rep = lambda t: t.expand(chains, *t.shape[1:]).contiguous()
            init = Latents(rep(init.z), [rep(e) for e in init.eps])
        return meas, weight, 1, init, None

    def _coils_problem(self, measurement, weight, pool, init, chains, psf, operator, estimate_psf, coils):
        """`_problem` with ``fourier=True, coils=maps``: the measurement is complex64 (N,C,Q,H,W) -- (C,Q,H,W) for one problem -- or
        fp32 with a trailing 2, and comes back as the latter; ``maps`` are the Q complex sensitivity maps, (Q,H,W) or (N,Q,H,W); the
        weight is the real k-space mask, shared by the coils, broadcast to (N,C,H,W); ``init`` None =
        ``encode_full(clamp(coils2d_adjoint(w t, maps), 0, 1))``, with normalised maps the coil-combined zero-filled image;
        ``chains`` > 1 repeats a single measurement (and per-sample maps of one sample).  Returns the maps as the sixth value.  Every
        refusal is a ValueError raised before any device work."""
        from .restore import as_kspace, check_coil_maps, check_fourier_shape, coils2d_adjoint
        if psf is not None or operator is not None or estimate_psf is not None or int(pool) != 1:
            raise ValueError("coils: multi-coil measurements exclude psf, operator and estimate_psf, and pool must be 1")
        real = as_kspace(measurement)
        if real.dim() not in (5, 6):
            raise ValueError(f"measurement of shape {tuple(measurement.shape)}: expected complex (C, Q, H, W) or (N, C, Q, H, W), or fp32 with a trailing 2")
        c, q, h, w = (int(v) for v in real.shape[-5:-1])
        check_fourier_shape((h, w), "measurement")
        chw = (c, h, w)
        if chw != tuple(int(v) for v in self.graph.flow.in_chw):
            raise ValueError(f"measurement of shape {tuple(measurement.shape)} is not the coil spectra of this model's images {tuple(self.graph.flow.in_chw)}")
        n = 1 if real.dim() == 5 else int(real.shape[0])
        maps, qs, per_sample = check_coil_maps(coils, n, (h, w))
        if qs != q:
            raise ValueError(f"measurement of shape {tuple(measurement.shape)} holds {q} coils, the maps {qs}")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32)
            try:
                torch.broadcast_shapes(tuple(weight.shape), (n,) + chw)
                ok = weight.dim() <= 4
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError(f"weight of shape {tuple(weight.shape)} does not broadcast to the k-space of {(n,) + chw}")
            if bool((weight < 0).any()):
                raise ValueError("weight: a k-space weight must be >= 0")
        if chains < 1 or (chains > 1 and n != 1):
            raise ValueError(f"chains = {chains}: several chains run on ONE measurement (a batch of {n} runs one chain each)")
        meas = real.reshape((n, c, q, h, w, 2)).to(self.device).contiguous()
        maps = maps.to(self.device).contiguous()
        if weight is not None:
            weight = weight.to(self.device).expand((n,) + chw).contiguous()
        if init is None:
            start = meas if weight is None else meas * weight.view(n, c, 1, h, w, 1)
            init = self.encode_full(coils2d_adjoint(start.contiguous(), maps).clamp_(0.0, 1.0))
        if chains > 1:
            rep = lambda t: t.expand(chains, *t.shape[1:]).contiguous()
            meas, weight = rep(meas), None if weight is None else rep(weight)
            if per_sample:
                maps = rep(maps)
            if len(init) == 1:
                init = Latents(rep(init.z), [rep(e) for e in init.eps])
        return meas, weight, 1, init, None, maps

    def _fourier_problem(self, measurement, weight, pool, init, chains, psf, operator, estimate_psf):
        """`_problem` with ``fourier=True``: the measurement is complex64 (N,C,H,W) -- (C,H,W) for one problem -- or fp32 with a
        trailing 2, and comes back as the latter; the weight is the real k-space mask, broadcast to (N,C,H,W); ``init`` None =
        ``encode_full(clamp(fourier2d_adjoint(w t), 0, 1))``, the zero-filled reconstruction; ``chains`` > 1 repeats a single
        measurement.  Every refusal is a ValueError raised before any device work."""
        from .restore import as_kspace, check_fourier_shape, fourier2d_adjoint
        if psf is not None or operator is not None or estimate_psf is not None or int(pool) != 1:
            raise ValueError("fourier: Fourier-domain measurements exclude psf, operator and estimate_psf, and pool must be 1")
        real = as_kspace(measurement)
        if real.dim() not in (4, 5):
            raise ValueError(f"measurement of shape {tuple(measurement.shape)}: expected complex (C, H, W) or (N, C, H, W), or fp32 with a trailing 2")
        chw = tuple(int(v) for v in real.shape[-4:-1])
        check_fourier_shape(chw[1:], "measurement")
        if chw != tuple(int(v) for v in self.graph.flow.in_chw):
            raise ValueError(f"measurement of shape {tuple(measurement.shape)} is not the spectrum of this model's images {tuple(self.graph.flow.in_chw)}")
        n = 1 if real.dim() == 4 else int(real.shape[0])
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32)
            try:
                torch.broadcast_shapes(tuple(weight.shape), (n,) + chw)
                ok = weight.dim() <= 4
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError(f"weight of shape {tuple(weight.shape)} does not broadcast to the k-space of {(n,) + chw}")
            if bool((weight < 0).any()):      # (a host weight -- `fourier_mask` makes one -- is checked without the device)
                raise ValueError("weight: a k-space weight must be >= 0")
        if chains < 1 or (chains > 1 and n != 1):
            raise ValueError(f"chains = {chains}: several chains run on ONE measurement (a batch of {n} runs one chain each)")
        meas = real.reshape((n,) + chw + (2,)).to(self.device).contiguous()
        if weight is not None:
            weight = weight.to(self.device).expand((n,) + chw).contiguous()
        if init is None:
            start = meas if weight is None else meas * weight.unsqueeze(-1)
            init = self.encode_full(fourier2d_adjoint(start.contiguous()).clamp_(0.0, 1.0))
        if chains > 1:
            rep = lambda t: t.expand(chains, *t.shape[1:]).contiguous()
            meas, weight = rep(meas), None if weight is None else rep(weight)
            if len(init) == 1:
                init = Latents(rep(init.z), [rep(e) for e in init.eps])
        return meas, weight, 1, init, None

    def _problem(self, measurement, weight, pool, init, chains=1, psf=None, border="valid", operator=None, estimate_psf=None,
                 fourier=False):
        """``(measurement batch, weight broadcast to it, pool, start latents, psf)`` of `restore` / `posterior`: ``init`` None =
        ``encode_full`` of the measurement (``pool>1``: of its pixel-repeated upsampling); ``chains`` > 1 repeats a single measurement
        (and a single PSF).  With a ``psf``, ``border="valid"`` multiplies the weight (None = ones) by
        `network.restore.psf_valid_weight`; every refusal of a PSF is raised before any device work.  ``estimate_psf``: ``psf`` is
        the start of a blind fit -- a pair of ints (kh, kw) is the uniform PSF of that support -- checked and normalised by
        `network.restore.blind_start`, here, on the host."""
        from .restore import blind_start, check_psf_shape, psf_valid_weight
        if fourier:
            return self._fourier_problem(measurement, weight, pool, init, chains, psf, operator, estimate_psf)
        if estimate_psf is not None:
            if not torch.is_tensor(measurement):
                raise TypeError("takes a tensor; image decoding (cv2 / PIL) is outside this package")
            psf = blind_start(psf, estimate_psf, 1 if measurement.dim() == 3 else len(measurement), operator)
        if operator is not None:
            return self._linear_problem(measurement, weight, pool, init, chains, psf, operator)
        if psf is not None:
            psf = torch.as_tensor(psf, dtype=torch.float32)
            if border not in ("valid", "zero"):
                raise ValueError(f"border = {border!r}: 'valid' or 'zero'")
            if not torch.is_tensor(measurement):
                raise TypeError("takes a tensor; image decoding (cv2 / PIL) is outside this package")
            kh, kw = check_psf_shape(psf.shape, 1 if measurement.dim() == 3 else len(measurement))
            band = None
            if border == "valid":
                band = psf_valid_weight(tuple(measurement.shape)[-2:], kh, kw, int(pool))
                if not bool(band.any()):
                    raise ValueError(f"border='valid': a psf of {kh} x {kw} taps leaves no cell of the "
                                     f"{tuple(measurement.shape)[-2:]} measurement (pool {int(pool)}) whose footprint is inside the image")
        meas = self._batch(measurement).float().contiguous()
        pool = int(pool)
        if chains < 1 or (chains > 1 and meas.shape[0] != 1):
            raise ValueError(f"chains = {chains}: several chains run on ONE measurement (a batch of {meas.shape[0]} runs one chain each)")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32, device=self.device).expand_as(meas).contiguous()
        if psf is not None:
            psf = psf.to(self.device).contiguous()
            if band is not None:
                band = band.to(self.device)
                weight = band.expand_as(meas).contiguous() if weight is None else weight * band
        if init is None:
            start = meas if pool <= 1 else meas.repeat_interleave(pool, dim=-2).repeat_interleave(pool, dim=-1)
            init = self.encode_full(start)
        if chains > 1:
            rep = lambda t: t.expand(chains, *t.shape[1:]).contiguous()
            meas, weight = rep(meas), None if weight is None else rep(weight)
            if len(init) == 1:
                init = Latents(rep(init.z), [rep(e) for e in init.eps])
            if psf is not None and psf.dim() == 3:
                psf = rep(psf)
        return meas, weight, pool, init, psf

    def restore(self, measurement, weight=None, pool=1, steps=100, lr=0.05, prior_weight=0.0, init=None, max_grad_norm=0.0,
                graph=True, exact=False, psf=None, border="valid", operator=None, estimate_psf=None, psf_lr=0.2, fourier=False,
                coils=None):
        """Latents whose decode explains ``measurement`` -- in-painting, denoising, projection (``pool=1``: ``measurement`` is an
        image (C,H,W) or a batch, ``weight`` its mask or per-pixel confidence, broadcast to it; None = everywhere) and
        super-resolution (``pool>1``: ``measurement`` is the LOW-resolution image, the decode is compared after a pool x pool average
        pool) -- as a maximum-a-posteriori fit under the flow prior, on the device (`network.restore.LatentFit`):

            minimise  sum_n  inv_wsum[n] * sum w (P decode(latents)_n - measurement_n)^2  +  prior_weight * 1/2 ||latents||^2

        by ``steps`` Adam iterations at ``lr``.  Returns ``(Latents, RestoreInfo)``: the per-sample loss history (steps, N), the
        gradient-norm history (steps,), ``finite``, ``captured``, ``fallback``.

        The data term is normalised PER SAMPLE, ``inv_wsum[n] = 1 / max(sum w[n], 1)``: every image of a batch is its own
        problem, its loss and its gradient independent of the others'.  Two couplings across the batch remain: the norm clip
        (``max_grad_norm`` > 0 clips the total gradient norm of all samples) and the skip of an iteration whose total norm is not
        finite (it is skipped for every sample).
        ``prior_weight``: the weight of 1/2 ||latents||^2 -- the negative log-density of the latents when the top prior is standard
        normal; it rides on the optimiser's weight decay and costs nothing.  A model with a learned or class-conditional top prior
        (``learn_top`` / ``y_condition``) raises ValueError for ``prior_weight > 0``: its top latent is not standard normal.
        ``init``: start `Latents`; None = ``encode_full`` of the measurement (``pool>1``: of its pixel-repeated upsampling).
        ``graph``: iterations after the first run as ONE hipGraph launch each (a failed capture falls back to the eager loop;
        the reason is in ``RestoreInfo.graph_error``).  ``exact``: the whole fit on the exact-fp32 kernel family.  With ``exact``
        off and ``glow.range_check`` on, a fit whose norm history holds a non-finite value is run once more from the same start on
        the exact family (``fallback=1``); non-finite there too: ``finite=False``.  Nothing raises; one host sync, at the end.

        ``psf``: deblurring (and, with ``pool>1``, super-resolution as blur then decimate) -- the decode is observed through the
        point-spread function before the pool, ``A = P B`` with ``B`` the zero-padded convolution by ``psf`` (include/glowhip.h,
        glowhip_restore_objective_psf).  Anything ``torch.as_tensor`` takes, of shape (kh,kw) -- one PSF for the batch -- or
        (N,kh,kw), sides odd and at most 15, the same for every channel, not normalised.  ``border="valid"`` (the default) gives
        weight 0 to the measurement cells whose footprint leaves the image (`network.restore.psf_valid_weight`: ceil(ah / pool)
        rows and ceil(aw / pool) columns at each edge), before ``inv_wsum`` is formed; ``border="zero"`` leaves the weight alone
        and takes the kernel's zero padding as the truth.  An even side, a side above 15, a wrong leading dimension or a band that
        leaves no cell raise ValueError before any device work.  ``init=None`` stays ``encode_full`` of the measurement.

        ``operator``: compressed sensing -- the decode, flattened in (C,H,W) order, is observed through a dense matrix,
        ``measurement = A x + noise`` (include/glowhip.h, glowhip_restore_objective_linear).  A contiguous fp32 DEVICE tensor of
        shape (M, C, H, W) with (C, H, W) the model's image shape, shared by the batch, not normalised and held by reference: do
        not write to it during the fit (`network.restore.gaussian_operator` makes the standard N(0, 1/M) matrix on the device).
        ``measurement`` and ``weight`` are then (N, M), or (M,) for one problem.  ``operator`` together with ``psf`` or
        ``pool != 1``, a measurement or weight whose last dimension is not M, and an operator that is not 4-D or not of the model's
        image shape raise ValueError before any device work.  ``init=None`` starts from all-zero latents, the prior's mode: there
        is no image to encode.

        ``estimate_psf`` = ``"shared"`` / ``"per_sample"``: BLIND deblurring -- the PSF is not known, and is fitted with the latents
        (one for the batch, or one per image) in the same captured loop, as ``softmax(theta)`` by Adam at ``psf_lr``
        (`network.restore.LatentFit`; include/glowhip.h, glowhip_restore_psf_grad).  ``psf`` is then the START: a pair of ints
        ``(kh, kw)`` for the uniform PSF of that support, or taps that are all > 0 (normalised to sum 1).  ``border="valid"`` works
        as it stands: the band depends on the support only.  The estimate comes back as ``RestoreInfo.psf`` -- on the device,
        ready for ``posterior(measurement, psf=info.psf)`` -- with ``psf_grad_norm``.  The softmax fixes the scale of the PSF; a
        shift of the PSF against the image is NOT determined by the measurement: the centred start and the valid band select the
        solution.  A tap <= 0 in the start, (N,kh,kw) with ``"shared"``, an ``operator`` beside it, an unknown value and no start
        at all raise ValueError before any device work.  ``estimate_psf=None`` is every call above, unchanged.

        ``fourier=True``: Fourier-domain measurements (MRI k-space undersampling, interferometry, partial-Fourier compressed
        sensing) -- ``measurement`` is the unitary 2-D DFT of each channel's plane, `torch.fft.fft2(x, norm="ortho")`: complex64
        (C,H,W) or (N,C,H,W), or fp32 with a trailing 2; unshifted, index (0,0) the DC term (include/glowhip.h,
        glowhip_restore_objective_fourier).  ``weight`` is the real k-space mask or weight, broadcast to (N,C,H,W)
        (`network.restore.fourier_mask` makes the usual undersampling masks); ``inv_wsum[n] = 1 / max(sum w[n], 1)`` as always.
        H and W must each be a power of two up to 256.  ``init=None`` starts from
        ``encode_full(clamp(fourier2d_adjoint(w * measurement), 0, 1))``, the zero-filled reconstruction.  ``fourier`` together with
        ``psf``, ``operator``, ``estimate_psf`` or ``pool != 1``, a side that is not a power of two or is above 256, a measurement
        that is not the spectrum of the model's image shape, and a negative weight raise ValueError before any device work.
        ``fourier=False`` is every call above, unchanged.

        ``coils=maps`` (with ``fourier=True``): multi-coil k-space, parallel imaging as SENSE states it -- Q receive coils each see
        the image through a complex sensitivity map, Y[c,q] = F (S_q x_c) (include/glowhip.h, glowhip_restore_objective_coils).
        ``measurement`` is complex64 (C,Q,H,W) or (N,C,Q,H,W), or fp32 with a trailing 2; ``maps`` complex64 (Q,H,W), shared by the
        batch, or (N,Q,H,W), 1 <= Q <= 32, the same for every channel and not normalised here
        (`network.restore.coil_maps` makes smooth synthetic ones with sum_q |S_q|^2 = 1); ``weight`` stays the real (N,C,H,W) mask,
        shared by the coils, and ``inv_wsum[n] = 1 / max(Q sum w[n], 1)``.  ``init=None`` starts from
        ``encode_full(clamp(coils2d_adjoint(w * measurement, maps), 0, 1))``, with normalised maps the usual coil-combined
        zero-filled image.  ``coils`` without ``fourier=True``, with ``psf``, ``operator``, ``estimate_psf`` or ``pool != 1``, maps of
        another plane, batch or coil count than the measurement's, and Q outside 1..32 raise ValueError before any device work.
        ``coils=None`` is every call above, unchanged."""
        from .restore import LatentFit, check_prior_weight
        check_prior_weight(self.graph, prior_weight)
        if coils is not None:
            if not fourier:
                raise ValueError("coils needs fourier=True (the maps multiply the image in front of the transform)")
            meas, weight, pool, init, psf, coils = self._coils_problem(measurement, weight, pool, init, 1, psf, operator, estimate_psf, coils)
            fit = LatentFit(self.graph, meas, weight=weight, pool=pool, init=init, steps=steps, lr=lr, prior_weight=prior_weight,
                            max_grad_norm=max_grad_norm, graph=graph, fourier=True, coils=coils)
            info = fit.run(exact=exact)
            return fit.latents(), info
        meas, weight, pool, init, psf = self._problem(measurement, weight, pool, init, psf=psf, border=border, operator=operator,
                                                      estimate_psf=estimate_psf, fourier=fourier)
        fit = LatentFit(self.graph, meas, weight=weight, pool=pool, init=init, steps=steps, lr=lr, prior_weight=prior_weight,
                        max_grad_norm=max_grad_norm, graph=graph, psf=psf, operator=operator, estimate_psf=estimate_psf, psf_lr=psf_lr,
                        fourier=fourier)
        info = fit.run(exact=exact)
        return fit.latents(), info

    def estimate_psf(self, sharp, blurred, psf=(5, 5), per_sample=False, weight=None, pool=1, border="valid", steps=100, psf_lr=0.2):
        """Calibration: the point-spread function that turns ``sharp`` (C,H,W or N,C,H,W) into ``blurred`` (the same at
        H/pool x W/pool) -- the iteration of blind `restore` without the flow (`network.restore.PsfFit`: softmax of the logits,
        the objective through the PSF, its gradient with respect to the taps, Adam at ``psf_lr``), on the same kernels.  ``psf``: the
        start, a pair of ints (kh, kw) for the uniform PSF of that support or taps that are all > 0; ``per_sample``: one PSF per
        image pair instead of one for the batch; ``weight`` / ``border`` as for `restore`.  Returns ``(psf, RestoreInfo)``: the
        estimate (kh,kw) or (N,kh,kw) on the device, the loss history (steps, N) and the logits' gradient norms.  Eager only: the
        capture protocol is tied to a flow plan and this loop has none (``captured`` is False).  Every refusal is a ValueError
        raised before any device work."""
        from .restore import PsfFit, blind_start, psf_valid_weight
        if not torch.is_tensor(sharp) or not torch.is_tensor(blurred):
            raise TypeError("takes tensors; image decoding (cv2 / PIL) is outside this package")
        if sharp.dim() not in (3, 4) or blurred.dim() != sharp.dim():
            raise ValueError(f"sharp {tuple(sharp.shape)} and blurred {tuple(blurred.shape)}: two images (C,H,W) or two batches (N,C,H,W)")
        n, pool = 1 if sharp.dim() == 3 else len(sharp), int(pool)
        start = blind_start(psf, "per_sample" if per_sample else "shared", n)
        kh, kw = start.shape[-2:]
        if border not in ("valid", "zero"):
            raise ValueError(f"border = {border!r}: 'valid' or 'zero'")
        want = tuple(sharp.shape[:-2]) + (sharp.shape[-2] // max(pool, 1), sharp.shape[-1] // max(pool, 1))
        if pool < 1 or sharp.shape[-2] % pool or sharp.shape[-1] % pool or tuple(blurred.shape) != want:
            raise ValueError(f"blurred of shape {tuple(blurred.shape)}: expected {want} for sharp {tuple(sharp.shape)} at pool {pool}")
        band = None
        if border == "valid":
            band = psf_valid_weight(tuple(blurred.shape)[-2:], kh, kw, pool)
            if not bool(band.any()):
                raise ValueError(f"border='valid': a psf of {kh} x {kw} taps leaves no cell of the {tuple(blurred.shape)[-2:]} "
                                 f"measurement (pool {pool}) whose footprint is inside the image")
        x, meas = self._batch(sharp).float().contiguous(), self._batch(blurred).float().contiguous()
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32, device=self.device).expand_as(meas).contiguous()
        if band is not None:
            band = band.to(self.device)
            weight = band.expand_as(meas).contiguous() if weight is None else weight * band
        fit = PsfFit(x, meas, start, weight=weight, pool=pool, steps=steps, psf_lr=psf_lr)
        info = fit.run()
        return info.psf, info

    def posterior(self, measurement, weight=None, pool=1, noise_std=0.1, chains=1, steps=200, burn_in=None, thin=1, step_size=1e-3,
                  seed=None, init=None, graph=True, adapt_rate=0.5, psf=None, border="valid", operator=None, fourier=False, coils=None):
        """Draws from the posterior of the latents given ``measurement`` -- what else is consistent with it, and how sure the model
        is of each pixel -- by a Metropolis-adjusted Langevin chain on the device (`network.posterior.LatentMALA`):

            p(latents | measurement)  ~  exp(-(sum w (P decode(latents) - measurement)^2 / (2 noise_std^2) + 1/2 ||latents||^2))

        with ``measurement`` / ``weight`` / ``pool`` as for `restore` and ``noise_std`` the standard deviation of the measurement
        noise.  A single measurement (C,H,W, or a batch of one) with ``chains=K`` runs K independent chains on it; a batch of
        measurements runs one chain each.  ``steps`` iterations, the first ``burn_in`` (None: half) adapting each chain's step from
        ``step_size`` towards an acceptance rate of 0.574 (``adapt_rate``) and the rest at a frozen step; every ``thin``-th image
        from ``burn_in`` on enters the per-pixel moments.  Returns ``(Latents, PosteriorInfo)``: the final states, and ``mean`` /
        ``std`` per chain, ``pooled_mean`` / ``pooled_std`` over the chains, ``count``, ``accept_rate``, ``step_size``,
        ``nonfinite_rejections``, the ``energy`` history, ``finite``, ``captured``, ``graph_error``.

        ``seed``: the chain is a function of it (two calls with one seed give the same bits); None takes the process's sampler
        position and advances it, as `resample_details` does.  ``init``: start `Latents`; None = ``encode_full`` of the measurement
        (``pool>1``: of its pixel-repeated upsampling).  A model with a learned or class-conditional top prior raises ValueError:
        the prior term assumes a standard-normal top latent.  A proposal whose decode is not finite (outside the fp16 pairs' range
        of the product kernels) is rejected on the device and counted; a start whose own decode is not finite gives
        ``finite=False`` and runs no iteration.  Nothing else raises; one host sync at the start state, one read at the end.

        ``psf`` / ``border``: the measurement is a blurred image, as for `restore`; with ``chains=K`` a single PSF is repeated as
        the measurement is.  ``operator``: the measurement (N, M) or (M,) is the decode seen through a dense matrix (M,C,H,W), as for
        `restore`; ``chains=K`` repeats the measurement and shares the one operator, and ``init=None`` starts every chain from the
        all-zero latents.  ``fourier=True``: the measurement is the decode's unitary 2-D DFT and ``weight`` the k-space mask, as for
        `restore`; ``noise_std`` is then the standard deviation of EACH of the real and imaginary parts, the energy
        sum w |F x - measurement|^2 / (2 noise_std^2); ``chains=K`` repeats the one measurement and ``init=None`` starts every chain
        from the zero-filled reconstruction.  ``coils=maps`` (with ``fourier=True``): multi-coil k-space as for `restore`, the
        measurement (C,Q,H,W) or (N,C,Q,H,W); ``noise_std`` is the standard deviation of each of the real and imaginary parts of each
        coil's coefficient, the energy sum_{c,q,k} w |F (S_q x) - measurement|^2 / (2 noise_std^2); ``chains=K`` repeats the one
        measurement and ``init=None`` starts every chain from the coil-combined zero-filled image."""
        from .model import sampler_position
        from .posterior import LatentMALA
        from .restore import check_prior_weight
        check_prior_weight(self.graph, 1.0)
        if coils is not None:
            if not fourier:
                raise ValueError("coils needs fourier=True (the maps multiply the image in front of the transform)")
            meas, weight, pool, init, psf, coils = self._coils_problem(measurement, weight, pool, init, int(chains), psf, operator, None, coils)
        else:
            meas, weight, pool, init, psf = self._problem(measurement, weight, pool, init, chains=int(chains), psf=psf, border=border,
                                                          operator=operator, fourier=fourier)
        if seed is None:
            seed, call = sampler_position(advance=True)
            call = call << 32      # (the chain's call is call + iteration: runs at successive positions share no counter)
        else:
            seed, call = int(seed) & (2 ** 64 - 1), 0
        chain = LatentMALA(self.graph, meas, weight=weight, pool=pool, noise_std=noise_std, init=init, steps=steps, burn_in=burn_in,
                           thin=thin, step_size=step_size, adapt_rate=adapt_rate, seed=seed, graph=graph, call=call, psf=psf,
                           operator=operator, fourier=fourier, coils=coils)
        info = chain.run()
        return chain.latents(), info

    def compute_attribute_delta(self, dataset, samples_per_batch=None, shuffle=True, num_workers=None, world=1, _exact=False):
        """deltaz[c] = mean latent of the images with attribute c - mean latent of those without (inferer.py:104-153).
        `dataset` yields dicts with 'x' (C,H,W) and 'y_onehot' (classes,).

        Range check without a host sync per batch: the encodes run unchecked on the product kernels, a device flag collects
        "some nll was not finite", and it is read once with the sums at the end -- only then (an input beyond the fp16 pairs'
        range) the pass is repeated with the plans on the exact-fp32 family."""
        from torch.utils.data import DataLoader
        shape = tuple(self.graph.flow.output_shapes[-1][1:])
        dim = int(np.prod(shape))
        pos = torch.zeros(self.num_classes, dim, dtype=torch.float64, device=self.device)
        neg = torch.zeros_like(pos)
        n_pos = torch.zeros(self.num_classes, dtype=torch.float64, device=self.device)
        n_neg = torch.zeros_like(n_pos)
        bad = torch.zeros((), dtype=torch.bool, device=self.device)
        loader = DataLoader(dataset, batch_size=self.batch_size, shuffle=shuffle, drop_last=True,
                            num_workers=self.hps.dataset.num_workers if num_workers is None else num_workers)
        with torch.no_grad():
            for batch in loader:
                assert 'y_onehot' in batch.keys(), 'Compute attribute deltaz needs "y_onehot" in batch data'
                x = batch['x'].to(self.device)
                y = batch['y_onehot'].to(self.device)
                if hasattr(self.graph.flow, "plan_for"):
                    plan = self.graph.flow.plan_for(x)
                    fam = plan.family
                    if _exact:
                        plan.set_family(plan.FAMILY_EXACT_FP32)
                    try:
                        z, nll, _ = self.graph.normal_flow(x, None, safe=False)
                    finally:
                        plan.set_family(fam)
                    bad |= ~torch.isfinite(nll).all()
                else:                                               # (a graph without flow plans: the bookkeeping tests' stand-in)
                    z, _, _ = self.graph(x)
                take = len(batch) if samples_per_batch == "reference" else (samples_per_batch or x.shape[0])
                zf = z[:take].reshape(take, dim).double()
                has = (y[:take] > 0).double()                       # (take, classes)
                pos += has.t() @ zf
                neg += (1.0 - has).t() @ zf
                n_pos += has.sum(0)
                n_neg += (1.0 - has).sum(0)
        if world > 1:                                               # ranks saw different batches: one exchange at the end
            flat = torch.cat([pos.reshape(-1), neg.reshape(-1), n_pos, n_neg, bad.double().reshape(1)])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)
            k = self.num_classes * dim
            pos, neg = flat[:k].view(self.num_classes, dim), flat[k:2 * k].view(self.num_classes, dim)
            n_pos, n_neg = flat[2 * k:2 * k + self.num_classes], flat[2 * k + self.num_classes:2 * k + 2 * self.num_classes]
            bad = flat[-1] > 0
        if getattr(self.graph, "range_check", True) and not _exact and bool(bad):
            return self.compute_attribute_delta(dataset, samples_per_batch, shuffle, num_workers, world, _exact=True)
        delta = pos / n_pos.clamp(min=1.0)[:, None] - neg / n_neg.clamp(min=1.0)[:, None]
        return delta.view(self.num_classes, *shape).cpu().numpy()

    def apply_attribute_delta(self, img, deltaz, interpolation, keep_details=False):
        """decode(encode(img) + sum_c interpolation[c] * deltaz[c]), inferer.py:155-188.  As in the reference, that decode draws
        every Split2d's half afresh: the result keeps the top-level content of ``img`` and new fine detail.
        ``keep_details=True``: the shift is applied to the top latent of the image's full latents and the decode reads the image's
        own eps -- an all-zero ``interpolation`` returns the image; a batch is taken as it is."""
        if isinstance(deltaz, np.ndarray):
            deltaz = torch.as_tensor(deltaz, dtype=torch.float32)
        assert len(interpolation) == self.num_classes
        assert deltaz.shape == torch.Size([self.num_classes, *self.graph.flow.output_shapes[-1][1:]])
        coef = torch.as_tensor(np.asarray(interpolation, dtype=np.float32), device=self.device)
        shift = (deltaz.to(self.device) * coef.view(-1, 1, 1, 1)).sum(0)
        if keep_details:
            lat = self.encode_full(img)
            out = self.decode_full(Latents(lat.z + shift, lat.eps))
            return out[0] if img.dim() == 3 else out
        z = self.encode(img)
        z_interpolated = z + shift
        return self.decode(z_interpolated)
