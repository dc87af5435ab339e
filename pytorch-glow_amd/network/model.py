"""FlowStep / FlowModel / Glow with the reference's surface (corenel/pytorch-glow network/model.py),
executed as flow plans on libglowhip: one C call per encode / decode / Glow forward.

state_dict keys and shapes equal the reference's, so its snapshots load unchanged.
"""
from __future__ import annotations

import ctypes
from functools import partial

import torch
import torch.nn as nn

from .. import _lib
from .._capture import Capture
from .._lib import require_device_tensor
from .._plan import PlanCache
from ..misc import util
from ..parallel import micro_slices
from . import module
from .latents import Latents
from .module import _deepcopy_without_plans, _logdet_arg


def _uninited_actnorms(mod):
    return [m for m in mod.modules() if isinstance(m, module.ActNorm) and not (m.bias_inited and m.logs_inited)]


def _all_actnorms(mod):
    return [m for m in mod.modules() if isinstance(m, module.ActNorm)]


def _maybe_data_dependent_init(owner, plan, x, noise, actnorm_scale):
    """First training-mode forward: set every ActNorm of the plan from this batch
    (reference network/module.py:45-46,66-67; trainer.py:112-115)."""
    if not owner.training or getattr(owner, "_actnorms_all_inited", None) == module.ActNorm.RESET_EPOCH[0]:
        return
    pending = _uninited_actnorms(owner)
    if not pending:
        # (the walk over ~6 400 sub-modules costs 1.5 ms: remembered until any ActNorm flag anywhere is cleared again)
        owner._actnorms_all_inited = module.ActNorm.RESET_EPOCH[0]
        return
    if len(pending) != len(_all_actnorms(owner)):
        raise _lib.GlowHipError("partially initialised ActNorm layers: call set_actnorm_inited() or reset all flags")
    plan.actnorm_init(x, noise, actnorm_scale)
    for m in pending:
        m.bias_inited = True
        m.logs_inited = True
    owner._actnorms_all_inited = module.ActNorm.RESET_EPOCH[0]


def level_eps_stds(eps_std, L):
    """Per-level temperature: (std of the top prior's draw, [std per Split2d, decode order]).  ``eps_std`` is a number / None --
    one temperature everywhere, passed through untouched -- or a sequence of L numbers in decode order: the top prior first, then
    the deepest Split2d, and so on.  Every entry follows the reference's ``eps_std or 1.`` (network/module.py:419)."""
    if eps_std is None or isinstance(eps_std, (int, float)) or getattr(eps_std, "ndim", 1) == 0:      # (numpy / 0-dim tensor scalars too)
        return eps_std, [eps_std] * (L - 1)
    stds = [float(v) for v in eps_std]
    if len(stds) != L:
        raise ValueError(f"eps_std: {len(stds)} entries for a model of L = {L} levels (one per level in decode order: "
                         "the top prior, then every Split2d from the deepest)")
    return stds[0] or 1., [v or 1. for v in stds[1:]]


class FlowStep(nn.Module):
    """One step of flow: ActNorm -> permutation (invconv | reverse | shuffle) -> coupling (additive | affine).
    Reference network/model.py:10-173."""

    flow_permutation_list = ['invconv', 'reverse', 'shuffle']
    flow_coupling_list = ['additive', 'affine']
    glowhip_kind = _lib.LAYER_FLOWSTEP

    def __init__(self, in_channels, hidden_channels, permutation='invconv', coupling='additive',
                 actnorm_scale=1., lu_decomposition=False):
        super().__init__()
        assert permutation in self.flow_permutation_list, 'Unsupported flow permutation: {}'.format(permutation)
        assert coupling in self.flow_coupling_list, 'Unsupported flow coupling: {}'.format(coupling)
        self.permutation = permutation
        self.coupling = coupling
        self.in_channels = in_channels
        self.hidden_channels = hidden_channels
        self.actnorm_scale = actnorm_scale
        self.actnorm = module.ActNorm(num_channels=in_channels, scale=actnorm_scale)
        if permutation == 'invconv':
            # (lu_decomposition: W kept as P L U factors -- its own class; the dense class keeps the reference's contract and raises)
            self.invconv = (module.Invertible1x1ConvLU(num_channels=in_channels) if lu_decomposition
                            else module.Invertible1x1Conv(num_channels=in_channels))
        elif permutation == 'reverse':
            self.reverse = module.Permutation2d(num_channels=in_channels, shuffle=False)
        else:
            self.shuffle = module.Permutation2d(num_channels=in_channels, shuffle=True)
        if coupling == 'additive':
            self.f = module.f(in_channels // 2, hidden_channels, in_channels // 2)
        else:
            self.f = module.f(in_channels // 2, hidden_channels, in_channels)
        self._plans = PlanCache()

    def _plan(self, x):
        return self._plans.get([self], tuple(x.shape[1:]), x.device)

    def normal_flow(self, x, logdet=None):
        x = require_device_tensor(x, "FlowStep input")
        plan = self._plan(x)
        _maybe_data_dependent_init(self, plan, x, None, self.actnorm_scale)
        ld = _logdet_arg(logdet, x.shape[0], x.device)
        return plan.encode(x, None, ld, want_logdet=ld is not None)

    def reverse_flow(self, x, logdet=None):
        x = require_device_tensor(x, "FlowStep input")
        ld = _logdet_arg(logdet, x.shape[0], x.device)
        return self._plan(x).decode(x, [], ld, want_logdet=ld is not None)

    def forward(self, x, logdet=None, reverse=False):
        assert x.shape[1] % 2 == 0
        return self.reverse_flow(x, logdet) if reverse else self.normal_flow(x, logdet)

    def __deepcopy__(self, memo):
        return _deepcopy_without_plans(self, memo)


class FlowModel(nn.Module):
    """Multi-scale flow: [Squeeze2d, FlowStep x K, Split2d] x (L-1) + [Squeeze2d, FlowStep x K].
    Reference network/model.py:176-314.  ``in_shape`` is (H, W, C)."""

    def __init__(self, in_shape, hidden_channels, K, L, permutation='invconv', coupling='additive',
                 actnorm_scale=1., lu_decomposition=False):
        super().__init__()
        self.K = K
        self.L = L
        self.actnorm_scale = actnorm_scale
        assert len(in_shape) == 3
        assert in_shape[2] == 1 or in_shape[2] == 3
        nh, nw, nc = in_shape
        self.in_chw = (nc, nh, nw)
        self.layers = nn.ModuleList()
        self.output_shapes = []
        for i in range(L):
            self.layers.append(module.Squeeze2d(factor=2))
            nc, nh, nw = nc * 4, nh // 2, nw // 2
            self.output_shapes.append([-1, nc, nh, nw])
            for _ in range(K):
                self.layers.append(FlowStep(in_channels=nc, hidden_channels=hidden_channels, permutation=permutation,
                                            coupling=coupling, actnorm_scale=actnorm_scale,
                                            lu_decomposition=lu_decomposition))
                self.output_shapes.append([-1, nc, nh, nw])
            if i < L - 1:
                self.layers.append(module.Split2d(num_channels=nc))
                nc = nc // 2
                self.output_shapes.append([-1, nc, nh, nw])
        self._plans = PlanCache()

    def plan_for(self, x_or_chw, device=None):
        if isinstance(x_or_chw, torch.Tensor):
            return self._plans.get(list(self.layers), tuple(x_or_chw.shape[1:]), x_or_chw.device)
        return self._plans.get(list(self.layers), tuple(x_or_chw), device)

    def pop_grad_buckets(self):
        """[(flat gradient bucket, ready event)] of the backward that just ran (FlowPlan.glow_backward), in the order the buckets
        become final -- for `parallel.allreduce_buckets`; None when no HIP backward ran since the last call."""
        for plan in self._plans._plans.values():
            b = getattr(plan, "last_grad_buckets", None)
            if b is not None:
                plan.last_grad_buckets = None
                return b
        return None

    def invalidate_packed(self):
        """Call after writing parameters through ``.data`` (which torch's version counters do not see)."""
        self._plans.invalidate()

    def encode(self, z, logdet=0., *, return_eps=False):
        """``return_eps``: also return the list of draws the Split2d layers' dropped halves imply, in decode order -- what
        ``decode(eps=)`` takes to give the input back."""
        z = require_device_tensor(z, "FlowModel input")
        plan = self.plan_for(z)
        _maybe_data_dependent_init(self, plan, z, None, self.actnorm_scale)
        ld = _logdet_arg(logdet, z.shape[0], z.device)
        if return_eps:
            eps_out = plan.latent_buffers(z.shape[0])
            out, ld_out = plan.encode(z, None, ld, want_logdet=ld is not None, eps_out=eps_out)
            return out, ld_out, eps_out
        return plan.encode(z, None, ld, want_logdet=ld is not None)

    _RANGE_FALLBACKS = 0

    def decode(self, z, eps_std=None, eps=None, safe=False):
        """``eps``: optional list of injected draws, one per Split2d in decode order (deepest first).  ``eps_std``: a number, or
        one per level (`level_eps_stds`; the first entry belongs to the top prior and is not used here).  ``safe``: see
        Glow.reverse_flow."""
        z = require_device_tensor(z, "FlowModel latent")
        n = z.shape[0]
        c, h, w = z.shape[1:]
        # input CHW of the plan from the latent shape: invert the squeeze/split bookkeeping
        plan = self._plans.get(list(self.layers), self._input_chw_for_latent((c, h, w)), z.device)
        if eps is None:
            eps = self.draw_eps(n, plan, eps_std, z.device)
        eps = [require_device_tensor(e, "eps") for e in eps]
        if torch.is_grad_enabled() and (z.requires_grad or any(e.requires_grad for e in eps)):
            return _GlowDecodeFn.apply(plan, bool(safe), z, *eps[:plan.n_split])
        return self._decode_plain(plan, z, eps, safe)

    @staticmethod
    def _decode_plain(plan, z, eps, safe):
        n = z.shape[0]
        x, _ = plan.decode(z, eps, None, want_logdet=False)
        if safe and bool(plan.status(n, x).any()):       # out of the fp16 pairs' range somewhere: the exact-fp32 kernels, same draws
            FlowModel._RANGE_FALLBACKS += 1
            prev = plan.family
            plan.set_family(plan.FAMILY_EXACT_FP32)
            try:
                x, _ = plan.decode(z, eps, None, want_logdet=False)
            finally:
                plan.set_family(prev)
        return x

    def _input_chw_for_latent(self, chw):
        c, h, w = chw
        for i in range(self.L):
            if i > 0:
                c = c * 2
            c, h, w = c // 4, h * 2, w * 2
        return (c, h, w)

    def split_shapes(self, in_chw):
        """(C,H,W) of the z2 half dropped at each Split2d, in DECODE order (deepest first)."""
        c, h, w = in_chw
        shapes = []
        for i in range(self.L):
            c, h, w = c * 4, h // 2, w // 2
            if i < self.L - 1:
                c = c // 2
                shapes.append((c, h, w))
        return shapes[::-1]

    def draw_eps(self, n, plan, eps_std, device):
        stds = [v or 1. for v in level_eps_stds(eps_std, self.L)[1]]  # reference network/module.py:419
        return [torch.randn((n,) + s, dtype=torch.float32, device=device) * std
                for s, std in zip(self.split_shapes(plan.in_chw), stds)]

    def forward(self, z, logdet=0., eps_std=None, reverse=False):
        if not reverse:
            return self.encode(z, logdet)
        return self.decode(z, eps_std)

    def __deepcopy__(self, memo):
        return _deepcopy_without_plans(self, memo)


class _GlowDecodeFn(torch.autograd.Function):
    """`FlowModel.decode` as one autograd node with respect to the LATENTS: forward is the plain decode (``safe`` keeps its
    meaning), backward is `FlowPlan.decode_vjp` on the returned image -- one taping re-encode of it plus the HIP reverse-flow
    sweep -- on the kernel family that produced the image.  Nothing is kept between forward and backward but the image, so the
    node can be differentiated any number of times.  Gradients of the model's PARAMETERS do not flow through the decode; a
    parameter changed between forward and backward raises."""

    @staticmethod
    def forward(ctx, plan, safe, z, *eps):
        before = FlowModel._RANGE_FALLBACKS
        x = FlowModel._decode_plain(plan, z, list(eps), safe)
        ctx.plan = plan
        ctx.family = plan.FAMILY_EXACT_FP32 if FlowModel._RANGE_FALLBACKS != before else plan.family
        ctx.version = plan._version_signature()
        ctx.save_for_backward(x)
        return x

    @staticmethod
    def backward(ctx, gx):
        plan = ctx.plan
        x, = ctx.saved_tensors
        if plan._version_signature() != ctx.version:
            raise _lib.GlowHipError("decode backward: a parameter changed between the decode and its backward -- the gradient "
                                    "would belong to another model than the image")
        need = ctx.needs_input_grad[2:]
        prev = plan.family
        plan.set_family(ctx.family)
        try:
            gz, geps = plan.decode_vjp(x, gx.contiguous().float(), want_z=need[0], want_eps=need[1:])
        finally:
            plan.set_family(prev)
        return (None, None, gz) + tuple(geps)


class _GlowTrainFn(torch.autograd.Function):
    """Glow.normal_flow as one autograd node: forward records the HIP activation tape, backward runs the HIP reverse
    sweep (glowhip_glow_backward) and hands the parameter gradients to autograd.  With a top head on the plan (learned /
    class-conditional prior, classifier: csrc/tophead.hip) ``y_logits`` is a third, differentiable output: the caller's own
    classification loss hands d loss / d y_logits back to the head's backward kernel."""

    @staticmethod
    def forward(ctx, plan, x, noise, n_bits, head, *params):
        z, nll, tape = plan.glow_forward_train(x, noise, None, None, 0, n_bits, head=head)
        ctx.plan, ctx.tape, ctx.x_in, ctx.head = plan, tape, x, head
        ctx.want_gx = x.requires_grad
        if head is not None and head.y_logits is not None:
            return z, nll, head.y_logits
        return z, nll

    @staticmethod
    def backward(ctx, gz, gnll, glogit=None):
        plan = ctx.plan
        n = ctx.x_in.shape[0]
        gnll = torch.zeros(n, device=ctx.x_in.device) if gnll is None else gnll.contiguous().float()
        gz = None if gz is None else gz.contiguous().float()
        glogit = None if glogit is None else glogit.contiguous().float()
        grads, gx = plan.glow_backward(ctx.x_in, ctx.tape, gnll, gz, None, None, 0, want_grad_x=ctx.want_gx, head=ctx.head,
                                       g_logit=glogit)
        ctx.tape = None
        return (None, gx, None, None, None) + tuple(grads)


# ---- the dequantisation stream of the inference path (network/model.py:421: z = x + U(0, 1/2^n_bits), drawn inside the leading
# squeeze kernel by Philox4x32-10).  ONE stream per process: key = torch's seed with the data-parallel rank folded in (ranks
# seeded alike still draw different noise), position = a process-wide count of such forwards (plans of different batch shapes
# do not repeat one another's draws).  A new torch.manual_seed value restarts it at 0; re-seeding with the SAME value cannot
# be seen from here -- call reset_dequant_stream() to replay.  (The reference consumes torch's CPU generator instead; the
# draws differ, their distribution does not.  Training mode and explicit `noise=` are unaffected.)
_DEQUANT_STREAM = {"seed": None, "calls": 0}


def reset_dequant_stream():
    _DEQUANT_STREAM["seed"], _DEQUANT_STREAM["calls"] = None, 0


def dequant_position(advance=False):
    """(key, call) the next in-kernel draw uses; advance=True consumes it."""
    import torch.distributed as dist
    seed = torch.initial_seed()
    st = _DEQUANT_STREAM
    if st["seed"] != seed:
        st["seed"], st["calls"] = seed, 0
    call = st["calls"]
    if advance:
        st["calls"] += 1
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    return (seed + 0x9E3779B97F4A7C15 * rank) & (2 ** 64 - 1), call


# The sampler's position (csrc/sampler_rng.h): ONE per process beside the dequantisation stream -- the key is torch's seed with the
# rank folded in, the call number counts the implicit `Glow.sample` calls.  The kernels read the position from a device word (one
# per device, created lazily): "holds" is what that word contains once everything enqueued has run, so it is uploaded only when a
# call needs another position than the device reached by counting itself.
_SAMPLER_STREAM = {"seed": None, "calls": 0, "words": {}}


def reset_sampler_stream():
    _SAMPLER_STREAM["seed"], _SAMPLER_STREAM["calls"] = None, 0


def sampler_position(advance=False):
    """(key, call) the next implicit `Glow.sample` draws with; advance=True consumes it."""
    import torch.distributed as dist
    seed = torch.initial_seed()
    st = _SAMPLER_STREAM
    if st["seed"] != seed:
        st["seed"], st["calls"] = seed, 0
    call = st["calls"]
    if advance:
        st["calls"] += 1
    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    return (seed + 0x9E3779B97F4A7C15 * rank) & (2 ** 64 - 1), call


def _sampler_word(plan, key, call):
    """The process's device word on the plan's device, holding (key, call): [tensor, (key, call) it holds]."""
    words = _SAMPLER_STREAM["words"]
    ent = words.get(str(plan.device))
    if ent is None:
        ent = words[str(plan.device)] = [plan.sampler_position(key, call), (key, call)]
    elif ent[1] != (key, call):
        ent[0].copy_(plan.sampler_position(key, call))
        ent[1] = (key, call)
    return ent


def sampler_stds(eps_std, L):
    """`level_eps_stds` as the numbers the sampler kernels multiply by: (std of the top draw, [std per Split2d, decode order]),
    every entry following the reference's ``eps_std or 1.`` (network/module.py:419)."""
    top, splits = level_eps_stds(eps_std, L)
    return float(top or 1.), [float(v or 1.) for v in splits]


class GraphedSampler:
    """`Glow.sample` for one batch size, captured in a hipGraph: ONE graph launch per batch of images.

    Static buffers: ``y_onehot`` (class-conditional models: write the labels in, or pass them to __call__), ``x`` (fp32 pixels)
    or ``x_u8`` (8-bit pixels, ``uint8=True``), ``z`` (the top latent of the last replay).  The captured body is
    `FlowPlan.sample` alone -- the top draw, the decode, the store and the one-thread launch that moves the device position --
    a single linear chain of kernels: no pack (the plan is packed and synchronised before the capture), no side stream.  Every
    replay draws at the position the previous one left: replay r after a capture at ``(seed, call)`` is
    ``Glow.sample(seed=seed, call=call + r)`` bit for bit.  A changed parameter, a re-allocated one, a pack for the other
    kernel family or an eager call with a larger batch on this plan (it re-allocates the workspace) needs a new capture: the replay
    raises.  No range fall-back inside a graph."""

    def __init__(self, glow, n, y_onehot=None, eps_std=None, uint8=False, seed=None, call=0):
        assert not glow.training, "capture_sampler is the inference path: call glow.eval() first"
        dev = glow.h_top.device
        self.glow, self.uint8 = glow, bool(uint8)
        self.plan = plan = glow.flow.plan_for(glow.flow.in_chw, dev)
        self.n, y_onehot = glow._sampler_batch(n, y_onehot)
        self.y_onehot = None if y_onehot is None else y_onehot.clone()
        self.std_top, self.std_split = sampler_stds(eps_std, glow.flow.L)
        if seed is None:
            seed = sampler_position()[0]
        self.seed, self._first, self._replays = int(seed) & (2 ** 64 - 1), int(call), 0
        self.pos = plan.sampler_position(self.seed, self._first)
        n = self.n
        self.x = None if uint8 else torch.empty((n,) + plan.in_chw, dtype=torch.float32, device=dev)
        self.x_u8 = torch.empty((n,) + plan.in_chw, dtype=torch.uint8, device=dev) if uint8 else None
        self.z = torch.empty((n,) + plan.out_chw, dtype=torch.float32, device=dev)
        self._head = plan.head_call(n, self.y_onehot) if glow._attach_head(plan) else None
        with torch.no_grad():
            plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
        # (no pack inside: the parameters' versions, the family and the pack count are watched, and the workspace every batch size of
        # this image shape shares -- an eager call with a larger batch re-allocates it)
        self._capture = Capture(plan, self._body, partial(plan.capture_signature, versions=True, family=True, buffers=("_ws",)), warmup=2)
        self.pos.copy_(plan.sampler_position(self.seed, self._first))      # (the warm-up moved it; the recording ran nothing)

    def _body(self):
        plan = self.plan
        plan.bind_sampler(self.pos, self.std_split, advance=True)
        try:
            plan.sample(self.n, self.std_top, head=self._head, out=(self.x, self.x_u8, self.z))
        finally:
            plan.bind_sampler(None)

    @property
    def last_position(self):
        """``(seed, call)`` the last replay drew with (kept on the host by counting); None before the first."""
        return None if self._replays == 0 else (self.seed, self._first + self._replays - 1)

    def __call__(self, y_onehot=None):
        """Replay; returns the static ``x`` (or ``x_u8``), valid until the next replay."""
        self._capture.check("capture_sampler")
        if y_onehot is not None and y_onehot is not self.y_onehot:
            self.y_onehot.copy_(y_onehot)
        self._capture.replay()
        self._replays += 1
        return self.x_u8 if self.uint8 else self.x


class GraphedForward:
    """`Glow.normal_flow` (eval, no grad; network/model.py:409-452) for one batch shape, captured in a hipGraph.

    Static buffers: ``x`` (copy the batch in, or pass one to __call__), ``noise``, ``z``, ``nll``.  What a replay runs: the
    dequantisation draw U(0, 2^-n_bits) with torch's Philox generator (registered with the graph, so every replay advances the
    stream like an eager draw), optionally `glowhip_plan_pack`, then the plan's launch list.  Parameters are read through their
    live addresses, so updates between replays are seen (with ``repack=True``); re-allocating a parameter, changing the
    kernel family or an eager call with a larger batch on this plan (it re-allocates the workspace) needs a new capture: the replay
    raises.  No range fall-back inside a graph: look at ``nll`` (non-finite = flagged)."""

    def __init__(self, glow, x, repack=True):
        assert not glow.training, "capture_forward is the inference path: call glow.eval() first"
        x = require_device_tensor(x, "Glow input")
        self.glow, self.repack = glow, repack
        self.n_bits = glow.hps.model.n_bits_x
        self.plan = plan = glow.flow.plan_for(x)
        assert not glow._attach_head(plan), "capture_forward: a learned / class-conditional top prior is not captured"
        self.x = x.clone()
        self.noise = torch.empty_like(self.x)
        n = x.shape[0]
        self.z = torch.empty((n,) + plan.out_chw, dtype=torch.float32, device=x.device)
        self.nll = torch.empty(n, dtype=torch.float32, device=x.device)
        self._obj = torch.empty(n, dtype=torch.float32, device=x.device)
        plan.set_dequant_rng(0, False)
        # repack=True: the captured pack reads the live parameters, so their versions are NOT watched (updates between replays are
        # the point) but the pack count is; repack=False: the versions instead.  Either way the shared inference workspace.
        self._capture = Capture(plan, self._body, partial(plan.capture_signature, versions=not repack, pack=repack, buffers=("_ws",)),
                                warmup=2)

    def _body(self):
        self.noise.uniform_(0, 1. / 2 ** self.n_bits)
        self.plan.glow_forward(self.x, self.noise, None, None, 0, self.n_bits, repack=self.repack, out=(self.z, self.nll, self._obj))

    def __call__(self, x=None):
        """Replay; returns the static (z, nll) (valid until the next replay)."""
        if x is not None and x is not self.x:
            self.x.copy_(x)
        self._capture.check("capture_forward")
        self._capture.replay()
        return self.z, self.nll


class _GradBinding:
    """Token for "the parameters' .grad are this plan's persistent gradient views" (`Glow.loss_and_grads`): the optimiser keeps its
    chunk table while it is shown the same token object."""
    __slots__ = ("grads",)

    def __init__(self, grads):
        self.grads = grads


class Glow(nn.Module):
    """Glow (reference network/model.py:317-550): dequantisation noise, flow encode, top prior, nll in bits/dim."""

    bce_criterion = nn.BCEWithLogitsLoss()
    ce_criterion = nn.CrossEntropyLoss()

    def __init__(self, hps):
        super().__init__()
        self.hps = hps
        self.flow = FlowModel(in_shape=hps.model.image_shape, hidden_channels=hps.model.hidden_channels,
                              K=hps.model.K, L=hps.model.L, permutation=hps.ablation.flow_permutation,
                              coupling=hps.ablation.flow_coupling, actnorm_scale=hps.model.actnorm_scale,
                              lu_decomposition=hps.ablation.lu_decomposition)
        if hps.ablation.learn_top:
            nc = self.flow.output_shapes[-1][1]
            self.learn_top = module.Conv2dZeros(in_channels=2 * nc, out_channels=2 * nc)
        if hps.ablation.y_condition:       # reference network/model.py:345-348
            nc = self.flow.output_shapes[-1][1]
            self.y_emb = module.LinearZeros(hps.dataset.num_classes, nc * 2)
            self.classifier = module.LinearZeros(nc, hps.dataset.num_classes)
        num_device = len(util.get_devices(self.hps.device.graph, verbose=False))
        assert hps.optim.num_batch_train % num_device == 0
        self.register_parameter('h_top', nn.Parameter(torch.zeros([hps.optim.num_batch_train // num_device,
                                                                   self.flow.output_shapes[-1][1] * 2,
                                                                   self.flow.output_shapes[-1][2],
                                                                   self.flow.output_shapes[-1][3]])))

    @property
    def batch_h_top(self):
        return self.h_top.shape[0]

    CRITERIA = {None: _lib.CRIT_NONE, "single_class": _lib.CRIT_CE, "multi_class": _lib.CRIT_BCE}

    def _head_parts(self):
        """{glowhip_head_desc field: live parameter} of the top head (csrc/tophead.hip): learn_top's bias / logs (its weight
        multiplies h_top == 0), y_emb under y_condition, the classifier when its logits are asked for (network/model.py:441)."""
        parts = {}
        ab = self.hps.ablation
        if ab.learn_top:
            parts.update(lt_bias=self.learn_top.bias, lt_logs=self.learn_top.logs)
        if ab.y_condition:
            parts.update(ye_w=self.y_emb.weight, ye_b=self.y_emb.bias, ye_logs=self.y_emb.logs)
            if self.hps.model.weight_y > 0:
                parts.update(cl_w=self.classifier.weight, cl_b=self.classifier.bias, cl_logs=self.classifier.logs)
        return parts

    def _attach_head(self, plan, criterion=None):
        """Make `plan` carry this model's head (host bookkeeping; no C call when nothing changed).  ``criterion``: None (logits
        only), 'single_class' or 'multi_class' -- the head kernel then also writes the loss term and its gradient."""
        assert criterion in self.CRITERIA, 'Unsupported criterion: {}'.format(criterion)
        parts = self._head_parts()
        if not parts:
            plan.set_head({})
            return False
        K = self.hps.dataset.num_classes if self.hps.ablation.y_condition else 0
        plan.set_head(parts, K, self.CRITERIA[criterion] if "cl_w" in parts else _lib.CRIT_NONE, float(self.hps.model.weight_y))
        return True

    def prior(self, y_onehot=None):
        """Top prior parameters (mean, logs), reference network/model.py:362-379, as dense tensors from one `k_top_prior`
        launch.  The reference asserts h_top == 0 with a host sync on every call (:373); the sync is not reproduced.  Returns
        (None, None) for the all-zero prior.  The forward / training paths do not call this: the head kernels compute the prior
        themselves."""
        ab = self.hps.ablation
        if not (ab.learn_top or ab.y_condition):
            return None, None
        n = self.batch_h_top
        if ab.y_condition:
            assert y_onehot is not None
            y_onehot = require_device_tensor(y_onehot.float(), "y_onehot")
            n = y_onehot.shape[0]
        else:
            y_onehot = None
        parts = {k: v for k, v in self._head_parts().items() if not k.startswith("cl_")}
        d = _lib.HeadDesc()
        d.K = self.hps.dataset.num_classes if ab.y_condition else 0
        for k, v in parts.items():
            setattr(d, k, require_device_tensor(v.detach(), k).data_ptr())
        dev = self.h_top.device
        c2, h, w = self.h_top.shape[1:]
        mean = torch.empty((n, c2 // 2, h, w), dtype=torch.float32, device=dev)
        logs = torch.empty_like(mean)
        _lib.check(_lib.lib().glowhip_top_prior(d, _lib.ptr(y_onehot), n, c2 // 2, h * w, _lib.ptr(mean), _lib.ptr(logs),
                                                _lib.stream_ptr(dev)))
        return mean, logs

    def normal_flow(self, x, y_onehot=None, noise=None, repack=False, safe=False, *, eps_out=None, dequantize=True):
        """z = x + U(0, 1/2^n_bits); objective = -ln(n_bins)*CHW + logdet + logp(z); nll = -objective/(ln2*CHW).
        ``noise`` (optional, beyond the reference signature) injects the dequantisation draw.

        Range: the product kernels carry the coupling networks' activations as fp16 pairs (csrc/sh.h): a hidden activation
        beyond 4094 becomes inf there where the fp32 reference stays finite.  That never yields a finite wrong answer -- a
        sticky per-sample flag makes the nll NaN -- and ``safe=True`` (inference path; costs one host sync) re-runs such a batch
        on the exact-fp32 MFMA kernels, so the result is the reference's up to fp32 rounding for any input the reference
        handles.

        ``eps_out`` / ``dequantize`` (inference path only) serve `encode_latents`: buffers that receive the Split2d draws
        (FlowPlan.latent_buffers), and ``dequantize=False`` = no noise at all."""
        x = require_device_tensor(x, "Glow input", allow_uint8=True)   # uint8 = pixels as loaded, scaled by 1/255 in-kernel
        if x.dtype == torch.uint8 and (self.training or torch.is_grad_enabled()):
            x = x.float() / 255.0   # the ActNorm init pass and the training step take fp32; inference reads the bytes itself
        n_bits = self.hps.model.n_bits_x
        plan = self.flow.plan_for(x)
        in_kernel_rng = False
        if not dequantize:
            assert noise is None, "dequantize=False: no noise is added, so none can be given"
        elif noise is None:
            if self.training or torch.is_grad_enabled():
                noise = torch.empty(x.shape, dtype=torch.float32, device=x.device).uniform_(0, 1. / 2 ** n_bits)
            else:     # inference: the leading squeeze draws it (Philox keyed by torch's seed; no noise tensor, no RNG launch)
                in_kernel_rng = True
                rng_key, rng_call = dequant_position(advance=True)      # (key, call number) this forward draws with
                plan.set_dequant_stream(rng_key, rng_call)
        else:
            noise = require_device_tensor(noise, "noise")
            assert noise.shape == x.shape
        if not in_kernel_rng:
            plan.set_dequant_rng(0, False)
        _maybe_data_dependent_init(self.flow, plan, x, noise, self.flow.actnorm_scale)
        n = x.shape[0]
        head = plan.head_call(n, y_onehot) if self._attach_head(plan) else None
        params = plan.trainable_parameters() if torch.is_grad_enabled() else ()     # (a walk over ~1 060 tensors: skipped on the inference path)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            assert eps_out is None and dequantize, "the training forward keeps no latents (use encode_latents)"
            # training step: one autograd node over the whole flow (HIP forward with tape + HIP backward)
            out = _GlowTrainFn.apply(plan, x, noise, n_bits, head, *params)
            return out[0], out[1], (out[2] if len(out) > 2 else None)
        z, nll, _ = plan.glow_forward(x, noise, None, None, 0, n_bits, repack=repack, head=head, eps_out=eps_out)
        if safe and not bool(torch.isfinite(nll).all()):
            if in_kernel_rng:     # the re-run sees the same dequantisation draw as the flagged run
                noise = plan.dequant_noise(x.shape, rng_key, rng_call, n_bits)
            z, nll = self._forward_exact_fp32(plan, x.float() / 255.0 if x.dtype == torch.uint8 else x, noise, n_bits, head,
                                              eps_out=eps_out)      # (the latents of a flagged batch come from the re-run)
        return z, nll, (None if head is None else head.y_logits)

    def loss_and_grads(self, x, noise=None, y_onehot=None, y=None, force_pack=False, criterion=None, accumulate=1):
        """mean(nll) of the batch (`generative_loss`) and its gradient for every trainable parameter, WITHOUT an autograd graph:
        the HIP forward with tape and the HIP reverse sweep are called directly, and the gradients land in the plan's persistent
        flat buckets, whose views are the parameters' ``.grad`` (assigned once).  This is `Trainer`'s step (network/trainer.py:123-133:
        forward, `loss.backward()`) minus ~10 ms of per-step host work in autograd's bookkeeping for ~1 060 parameter tensors --
        eight data-parallel ranks share one host.  Same kernels, same bits as ``normal_flow(x)`` + ``loss.backward()``
        (tests/test_gpu_grad.py).  Returns the loss (a device scalar); gradient buckets: ``flow.pop_grad_buckets()``.

        Class-conditional model (network/trainer.py:100-131): ``y_onehot`` feeds the prior; with ``weight_y > 0`` and a
        ``criterion`` ('single_class': integer targets ``y``; 'multi_class': multi-hot ``y_onehot``) the head kernel computes the
        classification term and its gradient itself, and the returned loss is generative + weight_y * classification
        (``self.last_losses`` holds the two terms).

        ``accumulate`` = k > 1: gradient accumulation -- the batch is cut into k contiguous micro-batches (`parallel.micro_slices`;
        views, labels and a given ``noise`` alike; ``noise=None`` draws one micro-batch-shaped ``uniform_`` per micro-step, in order),
        each runs as a plain call on its slice (same plan, tape and workspace of batch n / k, same bits in the buckets), and one
        launch per micro-step (csrc/accumulate.hip) carries the gradients: afterwards the ``.grad`` views hold
        (g_0 + ... + g_{k-1}) * float32(1 / k), the effective batch's gradient, and the returned loss and ``last_losses`` are the
        means over the micro-steps.  Needs n % k == 0 (ValueError) and an initialised ActNorm (the data-dependent init belongs
        to the full batch: `training.TrainLoop.step`).  ``force_pack`` goes to the first micro-step only.  ``pop_grad_buckets()``
        then returns every bucket with the ONE event recorded behind the last combine.  k = 1: the plain call, nothing added."""
        assert self.training, "loss_and_grads is the training step: call glow.train() first"
        if accumulate is not None and int(accumulate) != 1:
            return self._loss_and_grads_accumulated(x, noise, y_onehot, y, force_pack, criterion, int(accumulate))
        x = require_device_tensor(x, "Glow input", allow_uint8=True)
        if x.dtype == torch.uint8:
            x = x.float() / 255.0
        n_bits = self.hps.model.n_bits_x
        plan = self.flow.plan_for(x)
        if noise is None:
            noise = torch.empty(x.shape, dtype=torch.float32, device=x.device).uniform_(0, 1. / 2 ** n_bits)
        else:
            noise = require_device_tensor(noise, "noise")
        plan.set_dequant_rng(0, False)
        _maybe_data_dependent_init(self.flow, plan, x, noise, self.flow.actnorm_scale)
        n = x.shape[0]
        head = plan.head_call(n, y_onehot, y) if self._attach_head(plan, criterion) else None
        with torch.no_grad():
            z, nll, tape = plan.glow_forward_train(x, noise, None, None, 0, n_bits, force_pack=force_pack, head=head)
            loss = loss_generative = self.generative_loss(nll)
            loss_classes = None
            if head is not None and head.cls_loss is not None:
                loss_classes = torch.mean(head.cls_loss)
                loss = loss_generative + float(self.hps.model.weight_y) * loss_classes
            self.last_losses = (loss_generative, loss_classes)
            gn = getattr(plan, "_mean_grad", None)
            if gn is None or gn.numel() != n:
                gn = plan._mean_grad = torch.full((n,), 1.0 / n, dtype=torch.float32, device=x.device)      # d mean(nll) / d nll
            grads, _ = plan.glow_backward(x, tape, gn, None, None, None, 0, want_grad_x=False, persistent=True, head=head)
        # the views ARE the parameters' gradients: bound once per plan -- and again whenever somebody took them away in between
        # (optimizer.zero_grad() sets .grad to None, an autograd backward assigns its own tensors): ~1 060 identity tests, 60 us.  A
        # re-bind hands out a NEW token, so the optimiser rebuilds its chunk table from the gradients that are there now
        params = plan.trainable_parameters()
        bound = getattr(plan, "_pgrad_bound", None)
        if bound is None or bound.grads is not grads or any(p.grad is not g for p, g in zip(params, grads)):
            for p, g in zip(params, grads):
                p.grad = g
            plan._pgrad_bound = _GradBinding(grads)
        self._train_plan = plan        # (parallel.train_step: the optimiser's table stays valid while this plan's buckets are the gradients)
        return loss

    def _loss_and_grads_accumulated(self, x, noise, y_onehot, y, force_pack, criterion, k):
        """`loss_and_grads(accumulate=k)`, k > 1."""
        x = require_device_tensor(x, "Glow input", allow_uint8=True)
        cuts = micro_slices(x.shape[0], k)
        if x.dtype == torch.uint8:
            x = x.float() / 255.0
        if noise is not None:
            noise = require_device_tensor(noise, "noise")
            assert noise.shape == x.shape
        if getattr(self.flow, "_actnorms_all_inited", None) != module.ActNorm.RESET_EPOCH[0] and _uninited_actnorms(self.flow):
            raise _lib.GlowHipError("loss_and_grads(accumulate > 1): the ActNorm layers are not initialised -- the data-dependent init "
                                    "takes the full batch, forward only (TrainLoop.step / parallel.data_dependent_init), not a micro-batch")
        losses, terms = [], []
        for i, (lo, hi) in enumerate(cuts):
            losses.append(self.loss_and_grads(x[lo:hi], None if noise is None else noise[lo:hi],
                                              None if y_onehot is None else y_onehot[lo:hi], None if y is None else y[lo:hi],
                                              force_pack=force_pack and i == 0, criterion=criterion))
            terms.append(self.last_losses)
            plan = self._train_plan
            if i == 0:
                plan.accumulate_grads(_lib.ACC_FIRST)
            elif i < k - 1:
                plan.accumulate_grads(_lib.ACC_ADD)
            else:
                plan.accumulate_grads(_lib.ACC_FINISH, ctypes.c_float(1.0 / k).value)
        done = torch.cuda.Event()
        done.record()
        # the per-level marks of the last sweep are not final gradients any more: every bucket is final behind the last combine
        plan.last_grad_buckets = [(flat, done) for flat, _ in plan.last_grad_buckets]
        with torch.no_grad():
            loss = torch.stack(losses).mean()
            self.last_losses = (torch.stack([t[0] for t in terms]).mean(),
                                None if terms[0][1] is None else torch.stack([t[1] for t in terms]).mean())
        return loss

    def capture_forward(self, x, repack=True):
        """The inference forward of this batch shape as ONE hipGraph launch (`GraphedForward`): the flow plan's launch list is
        static (~220 kernels for celeba64), so it is captured once and replayed -- host cost per step ~10 us instead of ~1 ms of
        launches from Python / C.  ``repack=True`` keeps `glowhip_plan_pack` inside the graph: every replay re-derives the
        weight images from the LIVE parameters, as a forward after an optimiser step must."""
        return GraphedForward(self, x, repack=repack)

    _RANGE_FALLBACKS = 0   # how often safe=True had to re-run on the exact-fp32 kernels (diagnostics / tests)

    def _forward_exact_fp32(self, plan, x, noise, n_bits, head=None, eps_out=None):
        """The same forward on the exact-fp32 MFMA kernels (v_mfma_f32_32x32x2_f32): no fp16 range limit.  The kernel family is
        a property of the plan (glowhip_plan_set_family), set for this one call: nothing process-wide is touched, the product
        kernels' weight images stay valid for the next call."""
        Glow._RANGE_FALLBACKS += 1
        prev = plan.family
        plan.set_family(plan.FAMILY_EXACT_FP32)
        try:
            z, nll, _ = plan.glow_forward(x, noise, None, None, 0, n_bits, head=head, eps_out=eps_out)      # (same labels, same head tensors)
        finally:
            plan.set_family(prev)
        return z, nll

    def reverse_flow(self, z, y_onehot=None, eps_std=None, eps=None, safe=False, eps_top=None):
        """``safe=True``: the decode's range status (glowhip_plan_status: sticky log-det flags | a non-finite pixel) is read back
        -- one host sync -- and a flagged batch is decoded again on the exact-fp32 kernels with the same eps draws.
        ``z=None``: the top latent is sampled from the (class-conditional) prior, mean + exp(logs) * eps (network/model.py:466-468);
        ``eps_top`` (beyond the reference signature) injects that draw, already multiplied by its std.
        ``eps_std``: a number, or one per level in decode order (`level_eps_stds`: the top prior's first)."""
        # Differentiable with respect to the latents (`_GlowDecodeFn`) when grad mode is on and z, an eps or eps_top requires grad;
        # otherwise -- and always for the parameters -- the call runs without autograd, bit for bit as it always did.
        want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in [z, eps_top] + list(eps or []))
        with torch.no_grad():
            std_top = level_eps_stds(eps_std, self.flow.L)[0]
            if z is None:
                mean, logs = self.prior(y_onehot)
                if mean is None:
                    c2, h, w = self.h_top.shape[1:]
                    mean = logs = torch.zeros((self.batch_h_top, c2 // 2, h, w), device=self.h_top.device)
                if eps_top is None:
                    z = module.GaussianDiag.sample(mean, logs, std_top)
                elif not want_grad:
                    z = mean + torch.exp(logs) * require_device_tensor(eps_top, "eps_top")
            if not want_grad:
                return self.flow.decode(z, eps_std=eps_std, eps=eps, safe=safe)
        if z is None:      # (plain torch: eps_top gets its gradient through autograd by itself)
            z = mean + torch.exp(logs) * require_device_tensor(eps_top, "eps_top")
        return self.flow.decode(z, eps_std=eps_std, eps=eps, safe=safe)

    # ---- the sampler: draws made inside the kernels, every sample a (seed, call, index) triple
    def _sampler_batch(self, n, y_onehot):
        """(batch size, labels on the device) of a sampler call: the labels' batch under y_condition, else ``n`` or h_top's."""
        if self.hps.ablation.y_condition:
            assert y_onehot is not None, "y_condition: y_onehot is required"
            y_onehot = require_device_tensor(y_onehot.float(), "y_onehot")
            assert n is None or int(n) == y_onehot.shape[0], f"n = {n} but y_onehot holds {y_onehot.shape[0]} rows"
            return y_onehot.shape[0], y_onehot
        return (self.batch_h_top if n is None else int(n)), None

    def sample(self, n=None, y_onehot=None, eps_std=None, uint8=False, return_latents=False, safe=None, seed=None, call=None):
        """``n`` images drawn from the model -- `reverse_flow(z=None)` with every Gaussian draw made inside the kernel that
        consumes it (csrc/sampler_rng.h: no noise tensor exists), the top prior computed where the top latent is written, and
        optionally 8-bit pixels stored by the final un-squeeze (``uint8=True``: (N,C,H,W) uint8, the reference's
        ``tensor_to_ndarray`` rule, saturating).  Sample i of the call is named by ``(seed, call, i)``: the same triple gives the
        same bits again.  ``seed`` / ``call`` name the position for this one call; left out, the process's sampler position is
        used (torch's seed with the rank folded in) and advances by one.  Same distribution as `reverse_flow`, other bits: the
        generator is another one.
        ``eps_std``: a number or one per level (`level_eps_stds`).  ``safe`` (None: `range_check` in eval mode): a flagged batch
        is sampled again on the exact-fp32 kernels at the same position.  ``return_latents``: also the `Latents` whose
        `decode_latents` is the returned image, rebuilt from the stream (`FlowPlan.normal_noise`) -- nothing extra is stored
        during the decode."""
        if safe is None:
            safe = bool(self.range_check) and not self.training
        with torch.no_grad():
            dev = self.h_top.device
            n, y_onehot = self._sampler_batch(n, y_onehot)
            plan = self.flow.plan_for(self.flow.in_chw, dev)
            std_top, std_split = sampler_stds(eps_std, self.flow.L)
            head = plan.head_call(n, y_onehot) if self._attach_head(plan) else None
            plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
            implicit = seed is None and call is None
            if implicit:
                key, c = sampler_position(advance=True)
                word = _sampler_word(plan, key, c)
                pos = word[0]
            else:
                key = sampler_position()[0] if seed is None else int(seed) & (2 ** 64 - 1)
                c = 0 if call is None else int(call)
                pos = plan.sampler_position(key, c)
            want_x = not uint8 or safe      # (the range status scans the fp32 pixels)

            def run():
                plan.bind_sampler(pos, std_split, advance=implicit)
                try:
                    return plan.sample(n, std_top, head=head, want_x=want_x, want_u8=uint8)
                finally:
                    plan.bind_sampler(None)
            x, x8, z = run()
            if implicit:
                word[1] = (key, c + 1)
            if safe and bool(plan.status(n, x).any()):      # out of the fp16 pairs' range: the exact-fp32 kernels, same position
                FlowModel._RANGE_FALLBACKS += 1
                if implicit:
                    word = _sampler_word(plan, key, c)      # (back to where the flagged run drew)
                prev = plan.family
                plan.set_family(plan.FAMILY_EXACT_FP32)
                try:
                    plan.ensure_packed(use=plan.PACK_INFERENCE | plan.PACK_INVERSE)
                    x, x8, z = run()
                finally:
                    plan.set_family(prev)
                if implicit:
                    word[1] = (key, c + 1)
            out = x8 if uint8 else x
            if not return_latents:
                return out
            eps = [plan.normal_noise((n,) + s, key, c, 1 + k, std) for k, (s, std) in enumerate(zip(plan.split_chw, std_split))]
            return out, Latents(z, eps)

    def capture_sampler(self, n=None, y_onehot=None, eps_std=None, uint8=False, seed=None, call=0):
        """`sample` for one batch size as ONE hipGraph launch (`GraphedSampler`), a class-conditional prior included: the first
        replay draws at ``(seed, call)`` (seed None: the process's key), every later one at the next call number."""
        return GraphedSampler(self, n, y_onehot, eps_std=eps_std, uint8=uint8, seed=seed, call=call)

    # ---- held-out evaluation (network/evaluate.py)
    def evaluate(self, batches, **kw):
        """Bits per dimension of a data set, importance-weighted over ``draws`` dequantisation draws, with the per-level breakdown:
        ``Evaluator(self, **kw).run(batches)`` (draws=1, levels=True, seed=0, hist=None, safe=True) -> `EvalResult`."""
        from .evaluate import Evaluator
        return Evaluator(self, **kw).run(batches)

    # ---- full-latent encode: the bijection with nothing dropped
    def encode_latents(self, x, y_onehot=None, noise=None, dequantize=True, safe=None):
        """`Latents` of a batch (fp32 in [0, 1] or uint8 pixels): the top latent ``z``, the draw ``eps`` every Split2d's dropped
        half implies under its prior (the reference scores that half and discards it, network/module.py:526-536), and the nll.
        ``decode_latents`` of the result is the dequantised input, x + noise, to rounding.  ``noise`` injects the dequantisation
        draw; ``dequantize=False`` adds none, so the reconstruction is x itself (the nll then is that of the discrete pixels).
        Runs without autograd.  ``safe`` (None: `range_check` in eval mode, the policy of ``forward``): a batch flagged by a
        non-finite nll is encoded again on the exact-fp32 kernels, and the returned latents are that run's."""
        if safe is None:
            safe = bool(self.range_check) and not self.training
        with torch.no_grad():
            x = require_device_tensor(x, "Glow input", allow_uint8=True)
            eps_out = self.flow.plan_for(x).latent_buffers(x.shape[0])
            z, nll, _ = self.normal_flow(x, y_onehot, noise=noise, safe=safe, eps_out=eps_out, dequantize=dequantize)
        return Latents(z, eps_out, nll)

    def decode_latents(self, latents, safe=None):
        """Images of `Latents`: the decode with every Split2d fed the latents' own eps instead of a fresh draw.  Differentiable
        with respect to the latents: with grad mode on and ``latents.requires_grad_()``, a loss on the result back-propagates
        to ``z.grad`` and every ``eps.grad`` through the HIP reverse-flow sweep.  Parameter gradients do NOT flow through it."""
        if safe is None:
            safe = bool(self.range_check) and not self.training
        return self.reverse_flow(latents.z, eps=latents.eps, safe=safe)

    # Range policy of ``forward`` -- the call the reference's Trainer / Inferer make (network/trainer.py:113,123,163,171,
    # inferer.py:55,81,98,133).  Under torch.no_grad() in eval mode (validation, sampling, Inferer) the checked path is the default:
    # the result is the reference's for every input the reference handles, at the price of one host sync per call -- which those
    # callers pay anyway when they take the result to the host.  ``Glow.range_check = False`` (class or instance) switches it off;
    # benchmarks call normal_flow / reverse_flow directly (safe=False).  Training steps are checked by training.TrainLoop.
    range_check = True

    def forward(self, x=None, y_onehot=None, z=None, eps_std=None, reverse=False):
        safe = bool(self.range_check) and not self.training and not torch.is_grad_enabled()
        if not reverse:
            return self.normal_flow(x, y_onehot, safe=safe)
        return self.reverse_flow(z, y_onehot, eps_std, safe=safe)

    @staticmethod
    def generative_loss(nll):
        return torch.mean(nll)

    @staticmethod
    def single_class_loss(y_logits, y):
        if y_logits is None:
            return 0
        return Glow.ce_criterion(y_logits, y.long())

    @staticmethod
    def multi_class_loss(y_logits, y_onehot):
        if y_logits is None:
            return 0
        return Glow.bce_criterion(y_logits, y_onehot.float())

    def actnorm_inited(self):
        """True when every ActNorm already holds its data-dependent statistics (nothing left for a first batch to do)."""
        return not _uninited_actnorms(self)

    def set_actnorm_inited(self, inited=True):
        for name, m in self.named_modules():
            if m.__class__.__name__.find("ActNorm") >= 0:
                m.bias_inited = inited
                m.logs_inited = inited

