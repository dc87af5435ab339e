"""FlowPlan: Python handle of a `glowhip_plan` (include/glowhip.h) built from live nn.Modules.

A plan is the MI355X-native replacement of the reference's Python loop over ``FlowModel.layers``
(network/model.py:263-294): the layer list is static, so the whole stack (Squeeze2d / FlowStep / Split2d)
becomes ONE C call that issues a fixed kernel sequence on torch's current HIP stream.  torch only owns
the memory (parameters, workspace, packed-parameter buffer).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from . import _capture, _lib
from ._lib import LayerDesc, check, lib, ptr, stream_ptr


def _param_tensors(layer) -> List[torch.Tensor]:
    return [p for p in layer.parameters()]


class FlowPlan:
    """One executable stack of flow layers for a fixed input (C, H, W) on one device."""

    def __init__(self, layers: Sequence[torch.nn.Module], in_chw, device: torch.device):
        self.layers = list(layers)
        self.in_chw = tuple(int(v) for v in in_chw)
        self.device = torch.device(device)
        self._keep = []  # tensors whose addresses the C plan holds
        self._lu = []    # (layer index, Invertible1x1ConvLU, its assembled-W buffer): bound once the plan exists
        descs = (LayerDesc * len(self.layers))()
        c, h, w = self.in_chw
        split_chw = []   # shape of the z2 half each Split2d drops, in encode order
        for i, layer in enumerate(self.layers):
            d = descs[i]
            d.C, d.H, d.W = c, h, w
            kind = layer.glowhip_kind
            d.kind = kind
            if kind == _lib.LAYER_SQUEEZE:
                if layer.factor != 2:
                    raise _lib.GlowHipError("flow plans support Squeeze2d(factor=2) only")
                c, h, w = c * 4, h // 2, w // 2
            elif kind == _lib.LAYER_FLOWSTEP:
                self._fill_flowstep(d, layer, i)
            else:
                self._fill_split(d, layer)
                c = c // 2
                split_chw.append((c, h, w))
        self.out_chw = (c, h, w)
        self.split_chw = split_chw[::-1]      # DECODE order (deepest first): the order of decode's eps and of bound latents
        self._params = [p for layer in self.layers for p in _param_tensors(layer)]
        # (the LU modules' buffers decide W like parameters do: a load_state_dict or broadcast into them must re-pack as well)
        self._params += [b for _, m, _ in self._lu for b in (m.p, m.sign_s)]
        for p in self._params:
            if p.device != self.device:
                raise _lib.GlowHipError(f"parameter on {p.device}, plan on {self.device}")
        self._ptr_sig = self._pointer_signature()
        handle = lib().glowhip_plan_create(descs, len(self.layers))
        if not handle:
            raise _lib.GlowHipError("glowhip_plan_create: " + lib().glowhip_last_error().decode())
        self._h = ctypes.c_void_p(handle)
        self._descs = descs
        for i, m, wbuf in self._lu:
            b = _lib.InvconvLU()
            b.perm, b.l, b.u, b.log_s, b.sign_s = (self._dev_any(m.perm_table()), self._dev(m.l), self._dev(m.u), self._dev(m.log_s),
                                                   self._dev(m.sign_s))
            b.w = wbuf.data_ptr()
            check(lib().glowhip_plan_bind_invconv_lu(self._h, i, ctypes.byref(b)))
        self.packed_bytes = int(lib().glowhip_plan_packed_bytes(self._h))
        self.packed = torch.empty(max(self.packed_bytes, 256), dtype=torch.uint8, device=self.device)
        self._packed_version = None
        self._ws: Optional[torch.Tensor] = None
        self.n_split = sum(1 for l in self.layers if l.glowhip_kind == _lib.LAYER_SPLIT2D)

    # ------------------------------------------------------------------ construction helpers
    def _dev(self, t: torch.Tensor) -> int:
        if not t.is_cuda:
            raise _lib.GlowHipError("flow plans need parameters on a HIP device (module.cuda() first)")
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise _lib.GlowHipError("parameters must be contiguous fp32")
        self._keep.append(t)
        return t.data_ptr()

    def _fill_flowstep(self, d: LayerDesc, step, index: int) -> None:
        d.hidden = step.hidden_channels
        d.coupling = _lib.COUPLING_AFFINE if step.coupling == 'affine' else _lib.COUPLING_ADDITIVE
        d.an_bias, d.an_logs = self._dev(step.actnorm.bias), self._dev(step.actnorm.logs)
        if step.permutation == 'invconv':
            d.permutation = _lib.PERM_INVCONV
            if getattr(step.invconv, "lu_decomposition", False):
                # LU form: the plan owns the buffer every pack assembles W = P L U_f into (csrc/invconv_lu.hip); the layer is bound
                # to its factors below, once the C plan exists
                wbuf = torch.empty((d.C, d.C), dtype=torch.float32, device=self.device)
                d.invconv_w = self._dev(wbuf)
                self._lu.append((index, step.invconv, wbuf))
            else:
                d.invconv_w = self._dev(step.invconv.weight)
        else:
            d.permutation = _lib.PERM_GATHER
            perm = getattr(step, step.permutation)
            idx, inv = perm.device_tables(self.device)
            self._keep += [idx, inv]
            d.perm_idx, d.perm_idx_inv = idx.data_ptr(), inv.data_ptr()
        f0, f2, f4 = step.f[0], step.f[2], step.f[4]
        d.f0_w, d.f0_an_bias, d.f0_an_logs = self._dev(f0.weight), self._dev(f0.actnorm.bias), self._dev(f0.actnorm.logs)
        d.f2_w, d.f2_an_bias, d.f2_an_logs = self._dev(f2.weight), self._dev(f2.actnorm.bias), self._dev(f2.actnorm.logs)
        d.f4_w, d.f4_bias, d.f4_logs = self._dev(f4.weight), self._dev(f4.bias), self._dev(f4.logs)

    def _dev_any(self, t: torch.Tensor) -> int:
        if t.device != self.device or not t.is_contiguous():
            raise _lib.GlowHipError(f"tensor on {t.device}, plan on {self.device}")
        self._keep.append(t)
        return t.data_ptr()

    def _fill_split(self, d: LayerDesc, split) -> None:
        cz = split.conv2d_zeros
        d.f4_w, d.f4_bias, d.f4_logs = self._dev(cz.weight), self._dev(cz.bias), self._dev(cz.logs)

    def _pointer_signature(self):
        return tuple(p.data_ptr() for p in self._params)

    def _version_signature(self):
        return tuple(p._version for p in self._params)

    def still_valid(self) -> bool:
        """False when a parameter was re-allocated (module moved / parameter replaced): rebuild the plan."""
        return self._pointer_signature() == self._ptr_sig

    def capture_signature(self, versions=False, family=False, pack=True, buffers=(), grads=False, accumulators=False):
        """This plan's part of a captured graph's signature (`_capture.Capture`).  Always the parameter addresses; ``versions``: the
        parameters' version counters (a graph without a pack inside); ``family``: the kernel family; ``pack``: the count of packs
        that changed family (`pack`); ``buffers``: names of this plan's lazily (re-)allocated buffers the captured launches reach
        (None while absent); ``grads``: the persistent gradient buckets and the count of eager backwards with NON-persistent
        gradients, which rewrite the gradient job tables with pointers to their own temporaries; ``accumulators``: the buffers of a
        step with gradient accumulation."""
        sig = {"parameters": self._pointer_signature()}
        if versions:
            sig["versions"] = self._version_signature()
        if family:
            sig["family"] = self.family
        if pack:
            sig["pack_epoch"] = getattr(self, "_pack_epoch", 0)
        for name in buffers:
            sig[name] = _capture.address(getattr(self, name, None))
        if grads:
            pg = getattr(self, "_pgrad", None)
            sig["grad_buckets"] = tuple(f.data_ptr() for f in pg[0]) if pg else ()
            sig["grad_table_epoch"] = getattr(self, "_grad_table_epoch", 0)
        if accumulators:
            sig["accumulators"] = tuple(a.data_ptr() for a in self.grad_accumulators() or ())
        return sig

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().glowhip_plan_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------ top head (csrc/tophead.hip)
    def set_head(self, parts, K=0, criterion=_lib.CRIT_NONE, weight_y=0.0) -> None:
        """Attach the top head (glowhip_plan_set_head): ``parts`` maps the names of `_lib.HEAD_PARAMS` to the live parameters
        (learn_top.{bias,logs}, y_emb.{weight,bias,logs}, classifier.{weight,bias,logs}); an empty mapping detaches it.  Cheap when
        nothing changed: the C call is made only for a new parameter address, criterion or weight."""
        key = (tuple((n, t.data_ptr()) for n, t in parts.items()), int(K), int(criterion), float(weight_y))
        if key == getattr(self, "_head_key", ((), 0, 0, 0.0)):
            return
        names = tuple(parts)
        if names != tuple(n for n, _ in getattr(self, "_head_parts", ())):
            # another set of parameters gets gradients: the cached field list, bucket layout and persistent buckets go
            self._fields = self._bucket_lay = self._pgrad = self._pgrad_bound = None
        if not parts:
            check(lib().glowhip_plan_set_head(self._h, None))
        else:
            d = _lib.HeadDesc()
            d.K, d.criterion, d.weight_y = int(K), int(criterion), float(weight_y)
            for n, t in parts.items():
                if t.device != self.device or not t.is_contiguous() or t.dtype != torch.float32:
                    raise _lib.GlowHipError(f"top head parameter {n}: needs contiguous fp32 on {self.device}")
                setattr(d, n, t.data_ptr())
            check(lib().glowhip_plan_set_head(self._h, ctypes.byref(d)))
        self._head_parts = tuple(parts.items())
        self._head_key = key

    @property
    def has_head(self) -> bool:
        return bool(getattr(self, "_head_parts", ()))

    def head_call(self, n, y_onehot=None, y=None):
        """Per-batch tensors of the head for ONE forward (+ its backward): `HeadCall`."""
        return HeadCall(self, n, y_onehot, y)

    def _bind_head(self, head, g_logit=None):
        if not self.has_head:
            if head is not None:
                raise _lib.GlowHipError("a head call was given but the plan has no head attached")
            return
        if head is None:
            raise _lib.GlowHipError("the plan has a top head attached: pass head=plan.head_call(...)")
        io = _lib.HeadIO()
        io.y_onehot, io.y, io.state = _p(head.y_onehot), _p(head.y), _p(head.state)
        io.y_logits, io.cls_loss = _p(head.y_logits), _p(head.cls_loss)
        io.g_logit = _p(head.g_logit if g_logit is None else g_logit)
        check(lib().glowhip_plan_bind_head(self._h, ctypes.byref(io)))

    # ------------------------------------------------------------------ full-latent encode (glowhip_plan_bind_latents)
    def latent_buffers(self, n: int) -> List[torch.Tensor]:
        """Fresh eps buffers for a batch of ``n``: one per Split2d, decode order -- what ``eps_out=`` takes and decode reads."""
        return [torch.empty((n,) + s, dtype=torch.float32, device=self.device) for s in self.split_chw]

    def _bind_latents(self, eps_out, n: int) -> None:
        eps_out = list(eps_out)
        if len(eps_out) != self.n_split:
            raise _lib.GlowHipError(f"eps_out: {len(eps_out)} buffers given, the plan has {self.n_split} Split2d layers")
        for k, (e, s) in enumerate(zip(eps_out, self.split_chw)):
            if e.device != self.device or e.dtype != torch.float32 or not e.is_contiguous() or tuple(e.shape) != (n,) + s:
                raise _lib.GlowHipError(f"eps_out[{k}]: needs a contiguous fp32 tensor of shape {(n,) + s} on {self.device}")
        arr = (ctypes.c_void_p * max(len(eps_out), 1))(*[e.data_ptr() for e in eps_out])
        check(lib().glowhip_plan_bind_latents(self._h, arr, len(eps_out)))

    def _unbind_latents(self) -> None:
        check(lib().glowhip_plan_bind_latents(self._h, None, 0))

    # ------------------------------------------------------------------ per-level terms (glowhip_plan_bind_level_terms)
    @property
    def n_levels(self) -> int:
        """Levels of the objective's split: Split2d count + 1 (glowhip_plan_level_count)."""
        return int(lib().glowhip_plan_level_count(self._h))

    def level_terms_buffer(self, n: int) -> torch.Tensor:
        """A fresh (n_levels, n) buffer for ``level_terms=`` of `glow_forward`."""
        return torch.empty((self.n_levels, n), dtype=torch.float32, device=self.device)

    def _bind_level_terms(self, terms, n: int) -> None:
        if terms.device != self.device or terms.dtype != torch.float32 or not terms.is_contiguous() or tuple(terms.shape) != (self.n_levels, n):
            raise _lib.GlowHipError(f"level_terms: needs a contiguous fp32 tensor of shape {(self.n_levels, n)} on {self.device}")
        scratch = self._cached_bytes("_level_scratch", int(lib().glowhip_plan_level_scratch_bytes(self._h, n)))
        check(lib().glowhip_plan_bind_level_terms(self._h, ptr(terms), ptr(scratch), scratch.numel()))

    def _unbind_level_terms(self) -> None:
        check(lib().glowhip_plan_bind_level_terms(self._h, None, None, 0))

    # ------------------------------------------------------------------ execution
    def _workspace(self, n: int) -> torch.Tensor:
        need = int(lib().glowhip_plan_workspace_bytes(self._h, n))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    PACK_INFERENCE, PACK_TRAINING, PACK_INVERSE = 1, 2, 4   # glowhip.h GLOWHIP_PACK_*
    FAMILY_AUTO, FAMILY_EXACT_FP32 = 0, 1                   # glowhip.h GLOWHIP_FAMILY_*

    @property
    def family(self) -> int:
        return int(lib().glowhip_plan_get_family(self._h))

    def set_family(self, family: int) -> None:
        """Kernel family of this plan's coupling networks (glowhip_plan_set_family): per plan, no process-wide state.  The
        exact-fp32 family reads the fp32 MFMA weight images; they are packed on demand by the next call (ensure_packed)."""
        check(lib().glowhip_plan_set_family(self._h, int(family)))

    def _family_use(self, use: int) -> int:
        return use | (self.PACK_TRAINING if self.family == self.FAMILY_EXACT_FP32 else 0)

    def status(self, n: int, result: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(n,) int32 device tensor: sticky non-finite flags of the call that last used this plan's workspace (bits 0-2) |
        8 where `result` (that call's output tensor) holds a non-finite element.  Asynchronous: no host sync."""
        st = torch.empty(n, dtype=torch.int32, device=self.device)
        if n:
            ws = self._workspace(n)
            elems = 0 if result is None else result[0].numel()
            check(lib().glowhip_plan_status(self._h, ptr(ws), ws.numel(), n, ptr(result), elems, ptr(st), stream_ptr(self.device)))
        return st

    def pack(self, use: int = 7, merge: bool = True) -> None:
        """Refresh what is derived from the parameters (exp(3 logs), LU, and the weight images `use` asks for: the inference
        kernels' and/or the training kernels')."""
        version = self._version_signature()
        if merge and version == self._packed_version:
            use |= getattr(self, "_packed_use", 0)       # same parameters: the images packed earlier stay valid, add to them
        elif self._lu:
            for _, m, _ in self._lu:                     # the row tables of p follow a rewritten p (in place: same addresses)
                m.perm_table()
        check(lib().glowhip_plan_pack_for(self._h, ptr(self.packed), self.packed.numel(), use, stream_ptr(self.device)))
        self._packed_version = version
        self._packed_use = use
        # (a pack for the OTHER kernel family rebuilds the plan's host-side job tables with other contents and sizes -- and the copy
        # nodes of a CAPTURED pack read them through the addresses of capture time: a replay of the training step's graph after a
        # re-run on the exact-fp32 family faulted on a host address.  A graph with this plan's pack inside watches this count
        # (`capture_signature`).  Packs of the same family, whatever their image set, keep their tables in place:
        # tests/test_gpu_fused.py test_captured_forward_survives_packs_of_other_use_masks.)
        key = self.family
        if key != getattr(self, "_pack_key", None):
            self._pack_key = key
            self._pack_epoch = getattr(self, "_pack_epoch", 0) + 1

    def ensure_packed(self, force: bool = False, use: int = 1) -> None:
        """Re-derive the packed data when the parameters changed since the last pack (or `force`), or when images `use` asks
        for have not been packed for the current parameter version."""
        use = self._family_use(use)
        have = getattr(self, "_packed_use", 0)
        stale = self._packed_version != self._version_signature()
        if force or stale or (use & ~have):
            # forced = the caller declares the parameters changed (behind the version counters' back): nothing packed earlier counts
            self.pack(use if (force or stale) else (use & ~have), merge=not force)

    def pack_sync(self) -> None:
        """Host-wait for the side-stream part of the last pack (glowhip_plan_pack_sync): before capturing pack-free calls."""
        check(lib().glowhip_plan_pack_sync(self._h))

    def invalidate(self) -> None:
        self._packed_version = None

    def timing(self, enable: bool) -> None:
        """Record HIP events around every coupling-path kernel launch of subsequent encode/decode calls."""
        check(lib().glowhip_plan_timing_enable(self._h, int(enable)))

    def timing_read(self, max_records: int = 1 << 16):
        """[(kind, layer, mfma, ms)] in launch order since the last read (synchronises with the events)."""
        buf = (_lib.TimingRecord * max_records)()
        n = ctypes.c_int(0)
        check(lib().glowhip_plan_timing_read(self._h, buf, max_records, ctypes.byref(n)))
        return [(buf[i].kind, buf[i].layer, buf[i].mfma, buf[i].ms) for i in range(n.value)]

    def set_dequant_rng(self, seed, enable: bool = True) -> int:
        """In-kernel dequantisation noise for glow_forward calls without a noise tensor; returns the next call number."""
        nxt = ctypes.c_ulonglong(0)
        check(lib().glowhip_plan_set_dequant_rng(self._h, int(seed) & (2 ** 64 - 1), -1 if enable is None else int(bool(enable)), ctypes.byref(nxt)))
        return int(nxt.value)

    def set_dequant_stream(self, seed, call) -> None:
        """In-kernel dequantisation noise on, the next forward without a noise tensor draws with (seed, call)."""
        check(lib().glowhip_plan_set_dequant_stream(self._h, int(seed) & (2 ** 64 - 1), int(call)))

    def dequant_noise(self, shape, seed, call, n_bits) -> torch.Tensor:
        """The draw the kernel makes for call number `call` under `seed`, as a tensor shaped like x."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        check(lib().glowhip_dequant_noise(ptr(out), out.numel(), int(seed) & (2 ** 64 - 1), int(call), int(n_bits), stream_ptr(self.device)))
        return out

    # ------------------------------------------------------------------ the sampler's stream (csrc/sampler_rng.h)
    def normal_noise(self, shape, seed, call, stream, std=1.0) -> torch.Tensor:
        """Stream ``stream`` (0 = the top latent, 1 + k = the k-th Split2d in decode order) at position ``(seed, call)`` as a
        tensor, times ``std``: the draw the kernels make in place (glowhip_normal_noise)."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        check(lib().glowhip_normal_noise(ptr(out), out.numel(), int(seed) & _U64, int(call), int(stream), float(std),
                                         stream_ptr(self.device)))
        return out

    def sampler_position(self, seed, call) -> torch.Tensor:
        """A device word ``{seed, call}`` for `bind_sampler` (two uint64 kept in an int64 tensor)."""
        return torch.tensor([_i64(int(seed) & _U64), _i64(int(call))], dtype=torch.int64, device=self.device)

    @staticmethod
    def read_position(pos: torch.Tensor):
        """``(seed, call)`` held by a device word (synchronises)."""
        seed, call = (int(v) & _U64 for v in pos.cpu().tolist())
        return seed, call

    def bind_sampler(self, pos: Optional[torch.Tensor], std_split: Sequence[float] = (), advance: bool = False) -> None:
        """Bind the stream at the device word ``pos`` (glowhip_plan_bind_sampler; ``None`` unbinds): while bound, `decode` draws
        the eps of every Split2d it is given ``None`` for inside that split's prior kernel, with ``std_split[k]`` (decode order).
        ``advance``: a call that drew ends with ``call += 1`` on the device word."""
        if pos is None:
            check(lib().glowhip_plan_bind_sampler(self._h, None, None, 0, 0))
            self._sampler_pos = None
            return
        if pos.device != self.device or pos.dtype != torch.int64 or pos.numel() != 2 or not pos.is_contiguous():
            raise _lib.GlowHipError(f"bind_sampler: the position is two int64 words on {self.device} (sampler_position)")
        stds = [float(v) for v in std_split]
        if len(stds) != self.n_split:
            raise _lib.GlowHipError(f"bind_sampler: {len(stds)} stds given, the plan has {self.n_split} Split2d layers")
        arr = (ctypes.c_float * max(len(stds), 1))(*stds)
        check(lib().glowhip_plan_bind_sampler(self._h, ptr(pos), arr, len(stds), int(bool(advance))))
        self._sampler_pos = pos      # (the C plan holds its address)

    def sample(self, n, std_top=1.0, z=None, eps=None, head=None, want_x=True, want_u8=False, out=None, prior=None):
        """glowhip_plan_sample: the top draw (``z=None``; from the attached head's prior, labels through ``head``), the decode
        and the store in one C call, with the sampler bound by `bind_sampler` supplying every draw not injected through ``z`` /
        ``eps[k]``.  Returns ``(x, x_u8, z_used)`` -- fp32 pixels (``want_x``), 8-bit pixels (``want_u8``; stored by the final
        un-squeeze) and the top latent that was decoded.  ``out``: the three buffers to write instead of fresh ones (None
        entries for outputs not wanted).  ``prior``: a dense ``(mean, logs)`` base of shape (n,) + out_chw added to the head's.  No packing here: `ensure_packed(use=PACK_INFERENCE | PACK_INVERSE)` first."""
        dev = self.device
        if out is None:
            x = torch.empty((n,) + self.in_chw, dtype=torch.float32, device=dev) if want_x else None
            x8 = torch.empty((n,) + self.in_chw, dtype=torch.uint8, device=dev) if want_u8 else None
            z_used = torch.empty((n,) + self.out_chw, dtype=torch.float32, device=dev)
        else:
            x, x8, z_used = out
        if n == 0:
            return x, x8, z_used
        if z is not None:
            assert tuple(z.shape) == (n,) + self.out_chw, (z.shape, self.out_chw)
        eps = [None] * self.n_split if eps is None else list(eps)
        assert len(eps) >= self.n_split
        if getattr(self, "_sampler_pos", None) is None and (z is None or any(e is None for e in eps[:self.n_split])):
            raise _lib.GlowHipError("sample: a draw is needed and no sampler is bound (bind_sampler)")
        if z is None or head is not None:      # (a given top latent needs no prior: no labels, no head call)
            self._bind_head(head)
        ws = self._workspace(n)
        arr = (ctypes.c_void_p * max(len(eps), 1))(*[_p(e) for e in eps])
        pm, pl = (None, None) if prior is None else prior
        for t in (pm, pl):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (n,) + self.out_chw)
        per = self.out_chw[0] * self.out_chw[1] * self.out_chw[2]
        check(lib().glowhip_plan_sample(self._h, ptr(self.packed), ptr(z), ptr(pm), ptr(pl), per, float(std_top), arr, len(eps), ptr(x),
                                        ptr(x8), ptr(z_used), n, ptr(ws), ws.numel(), stream_ptr(dev)))
        return x, x8, z_used

    def describe(self, n: int = 0) -> str:
        """Kernel selection per layer; with a batch size ``n`` the choices that depend on the grid size are resolved as a
        call with that batch resolves them (n = 0: what the shapes support)."""
        buf = ctypes.create_string_buffer(1 << 16)
        check(lib().glowhip_plan_describe_for(self._h, int(n), buf, len(buf)))
        return buf.value.decode()

    def launch_counts(self, reset: bool = False) -> dict:
        """{kernel family: launches} recorded by the C executor as it launched them (run-time evidence, not a prediction)."""
        buf = ctypes.create_string_buffer(1 << 14)
        check(lib().glowhip_plan_launch_counts(self._h, buf, len(buf), int(reset)))
        return {k: int(v) for k, v in (line.split("=") for line in buf.value.decode().splitlines() if line)}

    def encode(self, x, noise=None, logdet=None, want_logdet=True, repack=False, *, eps_out=None):
        """``eps_out``: optional list of buffers (`latent_buffers`) that receive, per Split2d in decode order, the draw its
        dropped half implies; bound for this call only."""
        n = x.shape[0]
        assert tuple(x.shape[1:]) == self.in_chw, (x.shape, self.in_chw)
        self.ensure_packed(repack)
        z = torch.empty((n,) + self.out_chw, dtype=torch.float32, device=self.device)
        ld_out = torch.empty(n, dtype=torch.float32, device=self.device) if want_logdet else None
        if n == 0:
            return z, ld_out
        ws = self._workspace(n)
        if eps_out is not None:
            self._bind_latents(eps_out, n)
        try:
            check(lib().glowhip_plan_encode(self._h, ptr(self.packed), ptr(x), ptr(noise), ptr(logdet), ptr(z), ptr(ld_out), n,
                                            ptr(ws), ws.numel(), stream_ptr(self.device)))
        finally:
            if eps_out is not None:
                self._unbind_latents()
        return z, ld_out

    def _out_buffer(self, out, shape, what):
        """A caller's persistent output buffer (``out=``), checked; None: a fresh one, as ever."""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != tuple(shape):
            raise _lib.GlowHipError(f"{what}: out= needs a contiguous fp32 tensor of shape {tuple(shape)} on {self.device}")
        return out

    def decode(self, z, eps: Sequence[Optional[torch.Tensor]], logdet=None, want_logdet=False, repack=False, *, out=None):
        """``eps[k]`` may be ``None`` while a sampler is bound (`bind_sampler`): that Split2d draws its own.
        ``out``: the image buffer to write (a loop that decodes into one static image); None: a fresh tensor."""
        n = z.shape[0]
        assert tuple(z.shape[1:]) == self.out_chw, (z.shape, self.out_chw)
        assert len(eps) >= self.n_split
        if getattr(self, "_sampler_pos", None) is None and any(e is None for e in eps[:self.n_split]):
            raise _lib.GlowHipError("decode: an eps entry is None and no sampler is bound (bind_sampler)")
        self.ensure_packed(repack, use=self.PACK_INFERENCE | self.PACK_INVERSE)
        x = self._out_buffer(out, (n,) + self.in_chw, "decode")
        ld_out = torch.empty(n, dtype=torch.float32, device=self.device) if want_logdet else None
        if n == 0:
            return x, ld_out
        ws = self._workspace(n)
        arr = (ctypes.c_void_p * max(len(eps), 1))(*[_p(e) for e in eps])
        check(lib().glowhip_plan_decode(self._h, ptr(self.packed), ptr(z), arr, len(eps), ptr(logdet), ptr(x), ptr(ld_out),
                                        n, ptr(ws), ws.numel(), stream_ptr(self.device)))
        return x, ld_out

    def decode_vjp(self, x, grad_x, want_z=True, want_eps=None, *, out=None):
        """Vector-Jacobian product of `decode` (glowhip_plan_decode_vjp) at the latents whose decode is ``x``: returns
        ``(g_z, [g_eps])`` = J^T ``grad_x``, the eps gradients in decode order.  ``want_z`` / ``want_eps`` (one flag per Split2d)
        skip outputs nobody asked for (None in their place).  One taping re-encode of ``x`` plus the sweep; the tape and the
        workspace are cached per plan and live only for the call.  Gradients of the PARAMETERS do not flow through the decode.
        ``out``: ``(g_z, [g_eps])`` buffers to write instead of fresh ones (persistent gradients of a loop; an entry for an output
        not wanted is ignored)."""
        n = x.shape[0]
        assert tuple(x.shape[1:]) == self.in_chw and grad_x.shape == x.shape, (x.shape, grad_x.shape, self.in_chw)
        want_eps = [True] * self.n_split if want_eps is None else list(want_eps)
        assert len(want_eps) == self.n_split
        self.ensure_packed(use=self.PACK_TRAINING | self.PACK_INVERSE)
        out_z, out_eps = (None, [None] * self.n_split) if out is None else (out[0], list(out[1]))
        assert len(out_eps) == self.n_split
        gz = self._out_buffer(out_z, (n,) + self.out_chw, "decode_vjp g_z") if want_z else None
        geps = [self._out_buffer(o, (n,) + s, "decode_vjp g_eps") if w else None for s, w, o in zip(self.split_chw, want_eps, out_eps)]
        if n == 0:
            return gz, geps
        tape = self._cached_bytes("_vjp_tape", int(lib().glowhip_plan_tape_bytes(self._h, n)))
        ws = self._cached_bytes("_vjp_ws", int(lib().glowhip_plan_decode_vjp_workspace_bytes(self._h, n)))
        arr = (ctypes.c_void_p * max(len(geps), 1))(*[_p(e) for e in geps])
        check(lib().glowhip_plan_decode_vjp(self._h, ptr(self.packed), ptr(x), ptr(grad_x), ptr(gz), arr, len(geps), n, ptr(tape),
                                            tape.numel(), ptr(ws), ws.numel(), stream_ptr(self.device)))
        return gz, geps

    def _cached_bytes(self, name, need):
        buf = getattr(self, name, None)
        if buf is None or buf.numel() < need:
            setattr(self, name, None)
            buf = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            setattr(self, name, buf)
        return buf

    def glow_forward(self, x, noise, prior_mean, prior_logs, prior_stride, n_bits, repack=False, out=None, head=None, *,
                     eps_out=None, level_terms=None):
        """``eps_out``: as in `encode`.  ``level_terms``: a (n_levels, n) buffer (`level_terms_buffer`) that receives the per-level
        terms of the objective, in nats (glowhip_plan_bind_level_terms); bound for this call only."""
        n = x.shape[0]
        self.ensure_packed(repack)
        if n:
            self._bind_head(head)
        if out is None:
            z = torch.empty((n,) + self.out_chw, dtype=torch.float32, device=self.device)
            nll = torch.empty(n, dtype=torch.float32, device=self.device)
            obj = torch.empty(n, dtype=torch.float32, device=self.device)
        else:
            z, nll, obj = out
        if n == 0:
            return z, nll, obj
        ws = self._workspace(n)
        if eps_out is not None:
            self._bind_latents(eps_out, n)
        if level_terms is not None:
            self._bind_level_terms(level_terms, n)
        try:
            if x.dtype == torch.uint8:   # 8-bit pixels straight from the data loader: converted inside the leading squeeze
                check(lib().glowhip_glow_forward_u8(self._h, ptr(self.packed), ptr(x), 255.0, ptr(noise), ptr(prior_mean),
                                                    ptr(prior_logs), prior_stride, n_bits, ptr(z), ptr(nll), ptr(obj), n, ptr(ws),
                                                    ws.numel(), stream_ptr(self.device)))
            else:
                check(lib().glowhip_glow_forward(self._h, ptr(self.packed), ptr(x), ptr(noise), ptr(prior_mean), ptr(prior_logs),
                                                 prior_stride, n_bits, ptr(z), ptr(nll), ptr(obj), n, ptr(ws), ws.numel(),
                                                 stream_ptr(self.device)))
        finally:
            if eps_out is not None:
                self._unbind_latents()
            if level_terms is not None:
                self._unbind_level_terms()
        return z, nll, obj

    # ------------------------------------------------------------------ training step
    def _grad_fields(self):
        """[(layer index, LayerGrads field, parameter)] for every parameter the C backward produces a gradient for (cached: the
        plan is rebuilt when a parameter is replaced, PlanCache.get / still_valid)."""
        cached = getattr(self, "_fields", None)
        if cached is not None:
            return cached
        out = []
        for i, layer in enumerate(self.layers):
            kind = layer.glowhip_kind
            if kind == _lib.LAYER_FLOWSTEP:
                out += [(i, "an_bias", layer.actnorm.bias), (i, "an_logs", layer.actnorm.logs)]
                if layer.permutation == 'invconv' and getattr(layer.invconv, "lu_decomposition", False):
                    # (glowhip_invconv_lu_grads of the layer, not a glowhip_layer_grads field; all three in the small bucket)
                    out += [(i, "lu_dl", layer.invconv.l), (i, "lu_du", layer.invconv.u), (i, "lu_dlog_s", layer.invconv.log_s)]
                elif layer.permutation == 'invconv':
                    out.append((i, "invconv_w", layer.invconv.weight))
                f0, f2, f4 = layer.f[0], layer.f[2], layer.f[4]
                out += [(i, "f0_w", f0.weight), (i, "f0_an_bias", f0.actnorm.bias), (i, "f0_an_logs", f0.actnorm.logs),
                        (i, "f2_w", f2.weight), (i, "f2_an_bias", f2.actnorm.bias), (i, "f2_an_logs", f2.actnorm.logs),
                        (i, "f4_w", f4.weight), (i, "f4_bias", f4.bias), (i, "f4_logs", f4.logs)]
            elif kind == _lib.LAYER_SPLIT2D:
                cz = layer.conv2d_zeros
                out += [(i, "f4_w", cz.weight), (i, "f4_bias", cz.bias), (i, "f4_logs", cz.logs)]
        # the top head's parameters (layer index -1: they go to the glowhip_head_grads struct and the small bucket)
        out += [(-1, name, p) for name, p in getattr(self, "_head_parts", ())]
        self._fields = out
        self._trainable = [p for _, _, p in out]
        return out

    def trainable_parameters(self):
        self._grad_fields()
        return self._trainable

    def glow_forward_train(self, x, noise, prior_mean, prior_logs, prior_stride, n_bits, force_pack=False, head=None):
        """Forward that records the activation tape; returns (z, nll, tape).  ``force_pack``: re-derive the weight images whatever the
        version counters say (a captured training step: every replay follows an update the counters of capture time know nothing of)."""
        n = x.shape[0]
        self.ensure_packed(force_pack, use=self.PACK_TRAINING)   # re-packs when the weights changed since the last pack (optimizer step)
        z = torch.empty((n,) + self.out_chw, dtype=torch.float32, device=self.device)
        nll = torch.empty(n, dtype=torch.float32, device=self.device)
        tape = torch.empty(int(lib().glowhip_plan_tape_bytes(self._h, n)), dtype=torch.uint8, device=self.device)
        ws = self._train_workspace(n)
        self._bind_head(head)
        check(lib().glowhip_glow_forward_train(self._h, ptr(self.packed), ptr(x), ptr(noise), ptr(prior_mean),
                                               ptr(prior_logs), prior_stride, n_bits, ptr(z), ptr(nll), None, n, ptr(tape),
                                               tape.numel(), ptr(ws), ws.numel(), stream_ptr(self.device)))
        self._tape_version = self._packed_version           # glow_backward must see the same weights (and their images)
        return z, nll, tape

    def _train_workspace(self, n):
        need = int(lib().glowhip_plan_train_workspace_bytes(self._h, n))
        ws = getattr(self, "_tws", None)
        if ws is None or ws.numel() < need:
            self._tws = None
            self._tws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def glow_backward(self, x, tape, nll_grad, z_grad, prior_mean, prior_logs, prior_stride, want_grad_x=False, persistent=False,
                      head=None, g_logit=None):
        """Parameter gradients (list aligned with trainable_parameters()) and optionally dL/dx.
        ``persistent``: the flat gradient buckets, the views into them, the pointer table handed to the C sweep and the
        gradient-ready events are created ONCE per plan and reused by every call (the sweep writes every gradient in full) -- the
        per-step host cost of ~1 000 tensor views and ~1 000 ctypes assignments disappears; the caller must have consumed the
        previous call's gradients (training.TrainLoop: the optimiser step of step N is enqueued before the sweep of step N + 1).
        ``head``: the `HeadCall` of the matching forward; ``g_logit``: d loss / d y_logits from the caller's own loss (autograd route;
        None = what the forward's criterion wrote, or zero without one)."""
        n = x.shape[0]
        if (self._version_signature() != getattr(self, "_tape_version", None) or self._packed_version != self._tape_version
                or not (getattr(self, "_packed_use", 0) & self.PACK_TRAINING)):
            raise _lib.GlowHipError("glow_backward: the parameters (or their packed images) changed between the training forward "
                                    "and its backward -- an in-place update or optimizer step in between would mix weight versions")
        fields = self._grad_fields()
        layout = self._bucket_layout()
        # Gradients live in one flat buffer per bucket (the convolution weights of one LEVEL; everything small in a last one):
        # a data-parallel run all-reduces each bucket in place -- no concatenation, no copy back -- and starts with a level's
        # bucket as soon as the sweep has left that level (gradient-ready marks), while the lower levels are still being swept.
        cached = getattr(self, "_pgrad", None) if persistent else None
        if cached is None:
            flats = [torch.empty(nel, dtype=torch.float32, device=self.device) for nel in layout["sizes"]]
            grads = [flats[b][off:off + p.numel()].view_as(p) for (_, _, p), (b, off) in zip(fields, layout["slots"])]
            arr = (_lib.LayerGrads * len(self.layers))()
            hg = _lib.HeadGrads()
            lug = {i: _lib.InvconvLUGrads() for i, _, _ in self._lu}
            for (i, name, _), gt in zip(fields, grads):
                if name.startswith("lu_"):
                    setattr(lug[i], name[3:], gt.data_ptr())
                else:
                    setattr(hg if i < 0 else arr[i], name, gt.data_ptr())
            events = [torch.cuda.Event() for _ in layout["marks"]]
            for ev in events:
                ev.record()                  # (creates the handle; the C sweep records it again where it belongs)
            marks = (ctypes.c_int32 * max(len(events), 1))(*layout["marks"])
            handles = (ctypes.c_void_p * max(len(events), 1))(*[ev.cuda_event for ev in events])
            if persistent:
                self._pgrad = (flats, grads, arr, events, marks, handles, hg, lug)
        else:
            flats, grads, arr, events, marks, handles, hg, lug = cached
        if lug and getattr(self, "_lu_bound", None) is not lug:      # (the persistent set is bound once, not per step)
            for i, g in lug.items():
                check(lib().glowhip_plan_bind_invconv_lu_grads(self._h, i, ctypes.byref(g)))
            self._lu_bound = lug
        if not persistent:
            # the sweep rewrites the plan's host-side gradient job tables with THIS call's temporary buffers, and the copy nodes of a
            # captured training step read those tables at replay time: training.GraphedTrainStep sees this epoch move and captures
            # again after an eager step.  (A captured inference forward reads none of them: it keeps to _pack_epoch.)
            self._grad_table_epoch = getattr(self, "_grad_table_epoch", 0) + 1
        gx = torch.empty_like(x) if want_grad_x else None
        ws = self._train_workspace(n)
        self._bind_head(head, g_logit)
        if self.has_head:
            check(lib().glowhip_plan_bind_head_grads(self._h, ctypes.byref(hg)))
        check(lib().glowhip_plan_backward_marks(self._h, marks, handles, len(events)))
        try:
            check(lib().glowhip_glow_backward(self._h, ptr(self.packed), ptr(x), ptr(tape), tape.numel(), ptr(nll_grad),
                                              ptr(z_grad), ptr(prior_mean), ptr(prior_logs), prior_stride, arr, ptr(gx), n,
                                              ptr(ws), ws.numel(), stream_ptr(self.device)))
        finally:
            check(lib().glowhip_plan_backward_marks(self._h, None, None, 0))
        done = torch.cuda.Event()
        done.record()
        # in sweep order: (flat bucket, event after which it is final); the small bucket is final at the end of the call
        self.last_grad_buckets = [(flats[b], events[k]) for k, b in enumerate(layout["mark_bucket"])] + [(flats[-1], done)]
        return grads, gx

    # ------------------------------------------------------------------ gradient accumulation (csrc/accumulate.hip)
    def grad_accumulators(self):
        """The accumulators parallel to the persistent flat gradient buckets (same sizes; allocated at the first accumulation,
        again when the buckets were): None before."""
        held = getattr(self, "_gacc", None)
        pg = getattr(self, "_pgrad", None)
        return held[1] if held is not None and pg is not None and held[0] is pg[0] else None

    def accumulate_grads(self, mode: int, scale: float = 1.0) -> None:
        """One launch of glowhip_grad_accumulate over (persistent flat buckets, accumulators) on the current stream: `mode` =
        _lib.ACC_FIRST (acc = g), ACC_ADD (acc += g) or ACC_FINISH (g = (acc + g) * scale).  The buckets are those of the last
        ``glow_backward(persistent=True)``; the segment table is built once per set of buckets."""
        pg = getattr(self, "_pgrad", None)
        if pg is None:
            raise _lib.GlowHipError("accumulate_grads: no persistent gradient buckets yet (glow_backward(persistent=True) first)")
        flats = pg[0]
        held = getattr(self, "_gacc", None)
        if held is None or held[0] is not flats:
            accs = [torch.empty_like(f) for f in flats]
            tables = []
            for i in range(0, len(flats), _lib.ACC_MAX_SEGS):      # (L + 1 buckets: one table for every model the reference trains)
                part = list(zip(flats, accs))[i:i + _lib.ACC_MAX_SEGS]
                tables.append((_lib.GradSeg * len(part))(*[_lib.GradSeg(f.data_ptr(), a.data_ptr(), f.numel()) for f, a in part]))
            held = self._gacc = (flats, accs, tables)
        for table in held[2]:
            check(lib().glowhip_grad_accumulate(table, len(table), int(mode), float(scale), stream_ptr(self.device)))

    def _bucket_layout(self):
        lay = getattr(self, "_bucket_lay", None)
        if lay is not None:
            return lay
        fields = self._grad_fields()
        level_of, starts, cur = [], [], -1
        for i, layer in enumerate(self.layers):
            if layer.glowhip_kind == _lib.LAYER_SQUEEZE or cur < 0:
                cur += 1
                starts.append(i)
            level_of.append(cur)
        nlev = cur + 1
        sizes = [0] * (nlev + 1)                                   # one bucket per level + the small one (last)
        slots = []
        for i, name, p in fields:
            b = level_of[i] if name in ("f0_w", "f2_w", "f4_w") else nlev
            slots.append((b, sizes[b]))
            sizes[b] += (p.numel() + 63) // 64 * 64                # 256-byte aligned slots
        order = [l for l in range(nlev - 1, -1, -1) if sizes[l] > 0]   # sweep order: deepest level first
        lay = dict(sizes=[max(v, 64) for v in sizes], slots=slots, marks=[starts[l] for l in order], mark_bucket=order)
        self._bucket_lay = lay
        return lay

    def actnorm_init(self, x, noise, actnorm_scale: float) -> None:
        """Data-dependent init of every ActNorm in the plan from batch x (writes the parameters in place)."""
        n = x.shape[0]
        ws = self._workspace(n)
        for _, m, _ in self._lu:      # (the init pass packs from C: the row tables of p must be current before it)
            m.perm_table()
        check(lib().glowhip_plan_actnorm_init(self._h, ptr(self.packed), self.packed.numel(), ptr(x), ptr(noise),
                                              float(actnorm_scale), n, ptr(ws), ws.numel(), stream_ptr(self.device)))
        self._packed_version = self._version_signature()   # the init pass ends with a pack of the inference kernels' data
        self._packed_use = self.PACK_INFERENCE


def _p(t):
    return None if t is None else t.data_ptr()


_U64 = 2 ** 64 - 1


def _i64(v: int) -> int:
    """The int64 with the bit pattern of the uint64 ``v``."""
    return v - 2 ** 64 if v >= 2 ** 63 else v


class HeadCall:
    """What the top head reads and writes for one batch (glowhip_head_io): labels in, ``y_logits`` (N, K), ``cls_loss`` (N: the
    per-sample term whose mean is the classification loss) and ``g_logit`` out, ``state`` kept for the backward."""
    __slots__ = ("y_onehot", "y", "y_logits", "cls_loss", "g_logit", "state")

    def __init__(self, plan, n, y_onehot=None, y=None):
        parts = dict(plan._head_parts)
        _, K, criterion, _ = plan._head_key
        dev = plan.device
        if "ye_w" in parts:
            assert y_onehot is not None, "y_condition: y_onehot is required"      # reference network/model.py:377
        if y_onehot is not None:
            y_onehot = _lib.require_device_tensor(y_onehot.float() if y_onehot.dtype != torch.float32 else y_onehot, "y_onehot")
            assert tuple(y_onehot.shape) == (n, K), f"y_onehot {tuple(y_onehot.shape)}: expected {(n, K)}"
        if y is not None:
            y = y.long().contiguous()
            assert y.is_cuda and tuple(y.shape) == (n,), f"y {tuple(y.shape)} on {y.device}: expected {(n,)} on the GPU"
        self.y_onehot, self.y = y_onehot, y
        self.state = torch.empty(int(lib().glowhip_plan_head_state_bytes(plan._h, n)) // 4 or 1, dtype=torch.float32, device=dev)
        self.y_logits = self.cls_loss = self.g_logit = None
        if "cl_w" in parts:
            self.y_logits = torch.empty((n, K), dtype=torch.float32, device=dev)
            if criterion != _lib.CRIT_NONE:
                if criterion == _lib.CRIT_CE:
                    assert y is not None, "single_class criterion: integer targets y are required"
                self.cls_loss = torch.empty(n, dtype=torch.float32, device=dev)
                self.g_logit = torch.empty((n, K), dtype=torch.float32, device=dev)


class PlanCache:
    """Per-module cache of FlowPlans keyed by (input CHW, device); rebuilt when parameters move."""

    def __init__(self):
        self._plans = {}

    def get(self, layers, in_chw, device) -> FlowPlan:
        key = (tuple(in_chw), str(device))
        plan = self._plans.get(key)
        if plan is None or not plan.still_valid():
            plan = FlowPlan(layers, in_chw, device)
            self._plans[key] = plan
        return plan

    def clear(self):
        self._plans.clear()

    def invalidate(self):
        for p in self._plans.values():
            p.invalidate()
