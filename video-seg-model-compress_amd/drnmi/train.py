"""Fine-tune path: train-mode DRNSeg forward/backward, CrossEntropyLoss, SGD — on HIP kernels.

Reference training step (semantic_seg.py:166-230):

    model.train()
    output = model(input)[0]                      # DRNSeg.forward, BN on batch statistics
    loss = criterion(output, target)              # CrossEntropyLoss(ignore_index=255), :817
    optimizer.zero_grad(); loss.backward()        # autograd through ~70 ATen ops
    optimizer.step()                              # SGD(momentum, weight_decay), :963-966
    if pruner: pruner.apply_masks(model)          # :213-214

Here the same step keeps that exact user-facing shape: `DRNSeg.forward` in train mode is one
autograd.Function whose forward runs the fp32 HIP plan (conv -> batch-stat BN -> ReLU/residual
per node, then up x8 + LogSoftmax) and whose backward runs the HIP backward kernels in reverse
node order (include/drnmi.h "Fine-tune path"), writing every parameter's .grad directly.  A
gradient-ready callback per node lets the data-parallel wrapper (drnmi.parallel) launch the
bucketed RCCL all-reduce of finished buckets while earlier layers are still in backward.
`CrossEntropyLoss` and `SGD` below are the HIP drop-ins for the criterion and optimizer (the
optimizer can fuse the pruner's mask into the update: `SGD(..., pruner=p)`).
`DistillationLoss` is the criterion with a teacher: that CE plus the KL divergence to the
log-probs of a frozen dense model (`teacher_logprobs`), the reference's --mc-kd.

Precision: fp32 (the reference trains in fp32; model.set_precision("fp32"), the default) or
"fp32x": the forward and data-gradient convs with >= 32 input channels run on the fp32-accurate
split-bf16 kernel (csrc/conv_x6.hip: exact 3-way bf16 split of weights and activations, the six
products above 2^-24, fp32 accumulation, 2.5 PF / 6 peak) instead of the exact-f32 MFMA
(157 TF), and so do their weight gradients (drnmi_conv_wgrad_f32x3, the same split on dy and x);
BN, the head and the small-channel convs stay exact fp32.
Quantisation-aware fine-tuning (model.set_qat("int8")), in either precision: the convs
precision "int8" launches W8A8 read their weights and activations on the int8 grids (csrc/qat.hip,
fake quantisation in fp32), straight-through in the backward.  Off by default; with it off no launch,
buffer or record of the step differs.
Activations NHWC with a power-of-two channel stride, like the inference engine.  There is no
CPU or ATen fallback.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from .engine import COUT_ALIGN, K_ALIGN, X6_PATCH_SHAPES, _conv_out, _pow2_at_least, _round_up, int8_layout

F32 = _lib.DRNMI_F32
# TrainRunner default (tests switch it off to compare against the per-layer packs)
BATCHED_PACK = True
# BN batch statistics from the conv_x6 epilogue where the launch can write them (tests switch it
# off to compare against the separate statistics pass over y)
FUSED_BN_STATS = True
# fp32x data gradient of a stride-2 conv as four parity-class convs of dy (tests switch it off to
# compare against the zero-inserted conv, which it reproduces bit for bit when neither splits K)
S2_CLASS_DGRAD = True
# conv_x6 training launches may split K where their tiles leave CUs idle (tests switch it off for
# bit-for-bit comparisons of launch forms: a split sums the same products in another association)
X6_SPLIT_K = True


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _NodeState:
    """Per-node packed weights (forward / dgrad layouts) cached across steps."""

    __slots__ = ("wf", "wd", "wfx", "wdx", "k", "k_pad", "cout_pad", "kd", "kd_pad", "rows_d", "shift", "patch",
                 "dpatch", "dys", "s2_step", "s2_cls", "s2_planes", "wq", "wq_scale", "wsrc")

    def __init__(self):
        self.wf = self.wd = self.wfx = self.wdx = self.shift = None
        self.patch = self.dpatch = False
        self.dys = None
        self.s2_step = self.s2_cls = self.s2_planes = None   # stride-2 dgrad parity classes (per step)
        # QAT: the fake-quantised OIHW shadow of the weight and its per-row scales; wsrc is what this
        # step's packs read in place of conv.weight (the shadow, or None)
        self.wq = self.wq_scale = self.wsrc = None


class TrainRunner:
    """Executes one DRNSeg's train-mode forward and backward on the HIP kernels."""

    def __init__(self, model):
        self.model = model
        self.graph = model._graph
        self.cstride = {"input": 8}
        for v, c in self.graph.channels.items():
            if v != "input":
                self.cstride[v] = _pow2_at_least(c)
        self.nodes = self.graph.nodes
        self.state = [_NodeState() for _ in self.nodes]
        self._red_ws = None
        self._wg_ws = None
        self._cv_ws = None
        self._st_ws = None
        self._step_id = 0               # backward passes run (keys the per-step stride-2 class planes)
        self._zeros = None
        self.grad_ready = None          # callback(list[Parameter]) after each node's grads land
        self.grad_scale = 1.0           # multiplies dL/dlogprobs (DDP averaging: 1 / world_size)
        self._flat = None               # flat gradient buffer (views = param.grad)
        self._flat_params = None
        # diagnostics: record(kind, node name, dict) after every launch of forward / backward, with
        # what the launch read and wrote (tensors the step overwrites or frees are cloned on the
        # stream first).  None: no clone, no query, no synchronisation -- the step is unchanged.
        self.record = None
        self._last_conv = None
        # batched re-pack (drnmi_pack_conv_weights_batched): after the first step has allocated every
        # packed buffer, each forward re-packs all forward and dgrad weights (+ fp32x planes) in one
        # launch instead of ~4 launches per layer; the table is rebuilt when a buffer moves
        self.batched_pack = BATCHED_PACK
        self._pack_key = None
        self._pack_prec = None
        self._pack_tab = None
        self._pack_total = 0
        self._packed_now = False
        # quantisation-aware fine-tuning (model.set_qat): the node indices whose weights and inputs are
        # on the int8 grids this step (None: off) and {value: (scale, 1 / scale)} of the fake-quantised
        # values; the device table of the one weight launch, rebuilt when a buffer moves
        self._qat_layout = None
        self._qat_E = None
        self._qat_sc = {}
        self._qat_key = None
        self._qat_tab = None
        self._qat_rows = 0

    # ------------------------------------------------------------------ helpers
    def _ws(self, attr, nbytes, device):
        buf = getattr(self, attr)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            setattr(self, attr, buf)
        return buf

    def _zeros_f32(self, n, device):
        if self._zeros is None or self._zeros.numel() < n:
            self._zeros = torch.zeros(max(n, 4096), dtype=torch.float32, device=device)
        return self._zeros

    def _rec(self, kind, name, **items):
        self.record(kind, name, items)

    @staticmethod
    def _snap(t):
        return None if t is None else t.detach().clone()

    def ordered_params(self):
        """Parameters in the order backward finishes them (seg first, then nodes reversed)."""
        out = []
        for nd in reversed(self.nodes):
            ps = [nd.conv.weight] + ([nd.conv.bias] if nd.conv.bias is not None else [])
            if nd.bn is not None:
                ps += [nd.bn.weight, nd.bn.bias]
            out += [p for p in ps if p is not None]
        return out

    def _ensure_flat_grads(self, device):
        """param.grad of every trainable parameter is a view of one flat fp32 buffer laid out
        in backward order (contiguous all-reduce buckets).  Returns {param: accumulate?}."""
        params = [p for p in self.ordered_params() if p.requires_grad]
        if self._flat_params is None or [id(p) for p in self._flat_params] != [id(p) for p in params]:
            total = sum(p.numel() for p in params)
            self._flat = torch.zeros(total, dtype=torch.float32, device=device)
            self._flat_params = params
            self._views = {}
            off = 0
            for p in params:
                self._views[id(p)] = self._flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        acc = {}
        for p in params:
            if p.grad is None:
                p.grad = self._views[id(p)]
                acc[id(p)] = False
            else:
                if not (p.grad.is_contiguous() and p.grad.dtype == torch.float32 and p.grad.device == p.device):
                    raise RuntimeError("drnmi train: existing .grad must be contiguous fp32 on the device")
                acc[id(p)] = True
        return acc

    @staticmethod
    def _weight(nd, st):
        """The OIHW fp32 weight this step's packs read: the QAT shadow where there is one."""
        return st.wsrc if st.wsrc is not None else nd.conv.weight.detach()

    def _qat_begin(self, device, stream):
        """QAT on: fake-quantise the weights of the int8 engine's W8A8 convs into their shadows in one
        launch (drnmi_fake_quant_rows_batched_f32), before any pack reads them, and fix this step's
        activation scales.  QAT off: nothing is launched or allocated."""
        if getattr(self.model, "_qat", None) is None:
            if self._qat_E is not None:
                for st in self.state:
                    st.wsrc = None
                self._qat_E, self._qat_sc = None, {}
            return
        scales = self.model._qat_scales()         # raises the engine's error without calibrated scales
        if self._qat_layout is None:
            self._qat_layout = int8_layout(self.graph, self.cstride)
        elig = sorted(self._qat_layout[0])
        self._qat_E = self._qat_layout[0]
        self._qat_sc = {v: (s, 1.0 / s) for v, s in scales.items()}
        key = []
        for i in elig:
            nd, st = self.nodes[i], self.state[i]
            w = nd.conv.weight.detach()
            if not (w.is_contiguous() and w.dtype == torch.float32):
                raise RuntimeError(f"{nd.name}: expected a contiguous fp32 weight")
            if st.wq is None or st.wq.shape != w.shape or st.wq.device != w.device:
                st.wq = torch.empty_like(w)
                st.wq_scale = torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
            st.wsrc = st.wq
            key.append((w.data_ptr(), st.wq.data_ptr(), st.wq_scale.data_ptr()))
        key = tuple(key)
        lib = _lib.load()
        if key != self._qat_key:
            rows, total = [], 0
            for i, (pw, pq, ps) in zip(elig, key):
                w = self.nodes[i].conv.weight
                rows.append([pw, pq, ps, w.shape[0], w[0].numel(), total])
                total += w.shape[0]
            tab = torch.tensor(rows, dtype=torch.int64)
            tot = ctypes.c_int64(0)
            _lib.check(lib.drnmi_fake_quant_rows_table_check(ctypes.c_void_p(tab.data_ptr()), len(rows),
                                                             ctypes.byref(tot)), "fake-quant weight table")
            self._qat_tab, self._qat_rows, self._qat_key = tab.to(device), int(tot.value), key
        _lib.check(lib.drnmi_fake_quant_rows_batched_f32(_vp(self._qat_tab), self._qat_tab.shape[0], self._qat_rows,
                                                         stream), "fake-quant weights")
        if self.record is not None:
            for i in elig:
                nd, st = self.nodes[i], self.state[i]
                self._rec("fq_rows", nd.name, w=self._snap(nd.conv.weight), wq=self._snap(st.wq),
                          scale=self._snap(st.wq_scale))

    def _fake_quant(self, v, z, stream):
        """fq(v) of this step (drnmi_fake_quant_f32), computed once, right after v's producer."""
        s, inv = self._qat_sc[v]
        zq = torch.empty_like(z)
        _lib.check(_lib.load().drnmi_fake_quant_f32(_vp(z), z.numel(), s, inv, _vp(zq), stream), f"fake_quant {v}")
        if self.record is not None:
            self._rec("fq", v, x=z, y=zq, scale=s, inv_scale=inv)
        return zq

    def _pack(self, nd, st, device, stream):
        lib = _lib.load()
        conv = nd.conv
        cout, cin, ks, _ = conv.weight.shape
        cs = self.cstride[nd.src]
        if st.wf is None:
            st.k = ks * ks * cs
            st.k_pad = _round_up(st.k, K_ALIGN)
            st.cout_pad = _round_up(cout, COUT_ALIGN)
            st.wf = torch.empty(st.cout_pad, st.k_pad, dtype=torch.float32, device=device)
            st.shift = torch.zeros(st.cout_pad, dtype=torch.float32, device=device)
        w = self._weight(nd, st)
        if not (w.is_contiguous() and w.dtype == torch.float32):
            raise RuntimeError(f"{nd.name}: expected a contiguous fp32 weight")
        if not self._packed_now:
            _lib.check(lib.drnmi_pack_conv_weight(_vp(w), cout, cin, ks, cs, st.cout_pad, st.k_pad, 0, None, F32,
                                                  _vp(st.wf), stream), f"pack {nd.name}")
            # fp32x: the full-resolution small-channel convs (stem, layer1, layer2 shapes) run on
            # the split-bf16 patch kernels, as in the inference engine (engine.X6_PATCH_SHAPES)
            st.patch = self.model.precision == "fp32x" and not nd.out_fp32_nchw and \
                (cs, cout, ks, conv.stride[0], conv.dilation[0]) in X6_PATCH_SHAPES
            st.wfx = self._split(st.wf, cs, st.k, st.k_pad, patch=st.patch, out=st.wfx)
        if conv.bias is not None:
            st.shift[:cout].copy_(conv.bias.detach())

    def _pack_dgrad(self, nd, st, device, stream):
        lib = _lib.load()
        cout, cin, ks, _ = nd.conv.weight.shape
        dys = self.cstride[nd.dst] if not nd.out_fp32_nchw else _pow2_at_least(cout)
        if st.wd is None:
            st.kd = ks * ks * dys
            st.kd_pad = _round_up(st.kd, K_ALIGN)
            st.rows_d = _round_up(cin, COUT_ALIGN)
            st.wd = torch.empty(st.rows_d, st.kd_pad, dtype=torch.float32, device=device)
        st.dys = dys
        if self._packed_now:                      # packed with the forward weights (batched launch)
            return dys
        _lib.check(lib.drnmi_pack_conv_weight(_vp(self._weight(nd, st)), cout, cin, ks, dys, st.rows_d,
                                              st.kd_pad, 1, None, F32, _vp(st.wd), stream), f"pack dgrad {nd.name}")
        # fp32x: a data gradient whose (stride-1) conv is a patch-kernel shape (layer1's 16 -> 16
        # at full resolution) runs split-bf16 on the patch kernel, not on the f32 igemm
        st.dpatch = self.model.precision == "fp32x" and \
            (dys, cin, ks, 1, nd.conv.dilation[0]) in X6_PATCH_SHAPES
        st.wdx = self._split(st.wd, dys, st.kd, st.kd_pad, patch=st.dpatch, out=st.wdx)
        return dys

    def _s2_classes(self, nd, st, device, stream):
        """The parity classes of a stride-2 conv's data gradient in fp32x (drnmi_dgrad_s2_class_planes):
        [(a, b, ksc, planes)] for the classes some tap reaches, their weight planes gathered from this
        step's packed dgrad planes; None when the layer keeps the zero-insert path (not conv_x6, a
        dilated conv, or a class whose taps would start above its pixel).  Cached per step."""
        if st.s2_step == self._step_id:
            return st.s2_cls
        st.s2_step, st.s2_cls = self._step_id, None
        cout, cin, ks, _ = nd.conv.weight.shape
        p, d = nd.conv.padding[0], nd.conv.dilation[0]
        dys = self._pack_dgrad(nd, st, device, stream)
        if st.wdx is None or st.dpatch or d != 1 or dys % 8 != 0 or st.kd != st.kd_pad:
            return None
        pad_d = d * (ks - 1) - p
        parts = []
        for a_ in (0, 1):
            k0 = (pad_d - a_) % 2
            nh = (ks - k0 + 1) // 2 if k0 < ks else 0
            if nh and (a_ - pad_d + k0) // 2 != 0:       # the class conv would need a nonzero pad
                return None
            parts.append((k0, nh))
        lib = _lib.load()
        cls = []
        cache = st.s2_planes or {}
        for a_ in (0, 1):
            for b_ in (0, 1):
                nh, nw = parts[a_][1], parts[b_][1]
                if nh == 0 or nw == 0:
                    continue
                ksc = max(nh, nw)
                kpc = ksc * ksc * dys
                buf = cache.get((a_, b_))
                if buf is None or buf.shape != (3, st.rows_d, kpc):
                    buf = torch.empty(3, st.rows_d, kpc, dtype=torch.bfloat16, device=device)
                    cache[(a_, b_)] = buf
                _lib.check(lib.drnmi_dgrad_s2_class_planes(_vp(st.wdx), st.rows_d, st.kd_pad, dys, ks, pad_d, a_, b_,
                                                           ksc, _vp(buf), kpc, stream), f"dgrad classes {nd.name}")
                cls.append((a_, b_, ksc, buf))
        st.s2_planes = cache
        st.s2_cls = cls
        return cls

    def _batched_pack(self, device, stream) -> bool:
        """Re-pack every forward and dgrad weight (and fp32x planes) of the network in one launch
        (drnmi_pack_conv_weights_batched), bit-identical to the per-layer calls.  Needs the buffers
        of a previous step (False on the first step, or when disabled)."""
        if not self.batched_pack:
            return False
        if self._pack_prec != self.model.precision:   # a per-layer step sets the new mode's buffers
            self._pack_prec = self.model.precision
            self._pack_key = None
            return False
        key = [self.model.precision]
        for nd, st in zip(self.nodes, self.state):
            if st.wf is None or (nd.src != "input" and st.wd is None):
                return False
            key.append((self._weight(nd, st).data_ptr(), st.wf.data_ptr(), st.wfx.data_ptr() if st.wfx is not None else 0,
                        st.wd.data_ptr() if st.wd is not None else 0,
                        st.wdx.data_ptr() if st.wdx is not None else 0))
        key = tuple(key)
        if key != self._pack_key:
            rows = []
            total = 0
            for nd, st in zip(self.nodes, self.state):
                cout, cin, ks, _ = nd.conv.weight.shape
                w = self._weight(nd, st)
                if not (w.is_contiguous() and w.dtype == torch.float32):
                    return False
                ents = [(st.wf, st.wfx, self.cstride[nd.src], st.cout_pad, st.k_pad, 0)]
                if st.wd is not None:
                    ents.append((st.wd, st.wdx, st.dys, st.rows_d, st.kd_pad, 1))
                for out, planes, kst, rows_pad, k_pad, mode in ents:
                    rows.append([w.data_ptr(), out.data_ptr(), planes.data_ptr() if planes is not None else 0,
                                 cout, cin, ks, kst, rows_pad, k_pad, mode, total, 0])
                    total += rows_pad * k_pad
            tab = torch.tensor(rows, dtype=torch.int64)
            tot = ctypes.c_int64(0)
            _lib.check(_lib.load().drnmi_pack_table_check(ctypes.c_void_p(tab.data_ptr()), len(rows),
                                                          ctypes.byref(tot)), "pack table")
            self._pack_tab = tab.to(device)
            self._pack_total = int(tot.value)
            self._pack_key = key
        _lib.check(_lib.load().drnmi_pack_conv_weights_batched(_vp(self._pack_tab), self._pack_tab.shape[0],
                                                               self._pack_total, ctypes.c_void_p(stream)),
                   "batched weight pack")
        return True

    def _split(self, wpk, cin_stride, k, k_pad, patch=False, out=None):
        """fp32x: the three bf16 planes of a packed fp32 weight, for the convs conv_x6 takes
        (>= 32 input channels, k == k_pad) or the split-bf16 patch kernels take (`patch`); None
        keeps the launch on the exact-f32 kernel.  `out`: the previous step's planes (reused)."""
        if self.model.precision != "fp32x" or (not patch and (cin_stride < 32 or k != k_pad)):
            return None
        # one HIP pass (drnmi_split3_bf16), bit-identical to engine.split3_bf16
        if out is None or out.shape != (3,) + tuple(wpk.shape):
            out = torch.empty((3,) + tuple(wpk.shape), dtype=torch.bfloat16, device=wpk.device)
        _lib.check(_lib.load().drnmi_split3_bf16(_vp(wpk), wpk.numel(), _vp(out), _lib.stream_ptr(wpk.device)),
                   "split3_bf16")
        return out

    def _conv(self, x, cin_stride, h, w, wpk, k, k_pad, cout_pad, cout, ks, stride, pad, dil, y, y_strides,
              shift, res, n, ho, wo, stream, what, wx=None, algo=_lib.ALGO_IGEMM, want_stats=False, y_sr=0,
              split=True):
        """One drnmi_conv2d_bn_act launch.  want_stats: let a conv_x6 launch write the BN statistics
        partials of its output (self._st_ws); returns their row count, 0 when it cannot."""
        a = _lib.ConvArgs()
        a.x, a.wgt, a.scale, a.shift = x.data_ptr(), (wx if wx is not None else wpk).data_ptr(), None, shift.data_ptr()
        a.res = res.data_ptr() if res is not None else None
        a.y = y.data_ptr()
        a.y_sn, a.y_sp, a.y_sc = y_strides
        a.y_sr = y_sr
        a.n, a.h, a.w, a.cin = n, h, w, cin_stride
        a.ho, a.wo, a.cout, a.cout_pad = ho, wo, cout, cout_pad
        a.ks, a.stride, a.pad, a.dil = ks, stride, pad, dil
        a.k, a.k_pad = k, k_pad
        a.relu = 0
        a.dtype = a.out_dtype = F32
        if wx is not None:
            a.dtype = _lib.DRNMI_F32X3           # fp32x: conv_x6 (fp32 in/out, bf16 weight planes)
        a.tile, a.algo = -1, algo
        lib = _lib.load()
        nb = 0
        if wx is not None and algo == _lib.ALGO_IGEMM and split and X6_SPLIT_K:
            # split-K scratch for the launches whose tiles would leave CUs idle (the 1/8-res layers)
            nb = lib.drnmi_conv_workspace_bytes(ctypes.byref(a))
            if nb > 0:
                ws = self._ws("_cv_ws", nb, y.device)
                a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        if wx is None and algo == _lib.ALGO_IGEMM:
            # exact fp32: a workspace marks the training plan (long K summed in folded chains); unused
            ws = self._ws("_cv_ws", 256, y.device)
            a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
        rows = 0
        if want_stats and wx is not None and algo == _lib.ALGO_IGEMM:
            rows = lib.drnmi_conv_stats_rows(ctypes.byref(a))
            if rows > 0:
                a.stats = self._ws("_st_ws", 2 * rows * cout * 8, y.device).data_ptr()
        _lib.check(lib.drnmi_conv2d_bn_act(ctypes.byref(a), ctypes.c_void_p(stream)), what)
        if self.record is not None:
            kn = lib.drnmi_conv_kernel_name(ctypes.byref(a))
            self._last_conv = {"kernel": kn.decode() if kn else None, "x3": wx is not None,
                               "split_k": max(1, nb // (4 * n * ho * wo * cout)) if nb > 0 else 1}
        return max(rows, 0)

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, save: bool):
        """Train-mode forward; returns (logprobs, logits, saved) — saved is None if not save."""
        lib = _lib.load()
        dev = x.device
        stream = _lib.stream_ptr(dev)
        n, _, h, w = x.shape
        vals = {}
        shapes = {"input": (h, w)}
        xin = torch.empty(n, h, w, 8, dtype=torch.float32, device=dev)
        _lib.check(lib.drnmi_nchw_to_nhwc(x.data_ptr(), xin.data_ptr(), n, 3, h, w, 8, F32, ctypes.c_void_p(stream)),
                   "nchw_to_nhwc")
        vals["input"] = xin
        self._packed_now = False
        self._qat_begin(dev, ctypes.c_void_p(stream))
        self._packed_now = self._batched_pack(dev, stream)
        per_node = []
        logits = None
        qvals = {}                       # QAT: value -> fq(value), what the W8A8 convs read
        for idx, (nd, st) in enumerate(zip(self.nodes, self.state)):
            c = nd.conv
            # a conv the int8 engine runs W8A8 reads fq(src) / fq(res); every other conv the values
            rd = qvals if self._qat_E is not None and idx in self._qat_E else vals
            ih, iw = shapes[nd.src]
            ks, s, p, d = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]
            oh, ow = _conv_out(ih, ks, s, p, d), _conv_out(iw, ks, s, p, d)
            shapes[nd.dst] = (oh, ow)
            self._pack(nd, st, dev, ctypes.c_void_p(stream))
            cout = c.out_channels
            cs_in = self.cstride[nd.src]
            if nd.out_fp32_nchw:        # seg 1x1 + bias -> fp32 NCHW logits
                logits = torch.empty(n, cout, oh, ow, dtype=torch.float32, device=dev)
                self._conv(rd[nd.src], cs_in, ih, iw, st.wf, st.k, st.k_pad, st.cout_pad, cout, ks, s, p, d,
                           logits, (cout * oh * ow, 1, oh * ow), st.shift, None, n, oh, ow, stream, nd.name, st.wfx)
                vals[nd.dst] = logits
                per_node.append(None)
                if self.record is not None:
                    self._rec("conv", nd.name, x=rd[nd.src], y=logits, **self._last_conv)
                continue
            cs = self.cstride[nd.dst]
            if cs != cout:
                raise NotImplementedError("train path: channel count must be a power of two")
            rows = n * oh * ow
            y = torch.empty(rows, cs, dtype=torch.float32, device=dev)
            bn = nd.bn
            if bn.momentum is None or not bn.track_running_stats:
                raise NotImplementedError("BatchNorm2d with momentum=None / no running stats")
            # conv_x6 launches write the BN statistics partials in their epilogue (no pass over y)
            g_rows = self._conv(rd[nd.src], cs_in, ih, iw, st.wf, st.k, st.k_pad, st.cout_pad, cout, ks, s, p,
                                d, y, (oh * ow * cs, cs, 1), st.shift, None, n, oh, ow, stream, nd.name, st.wfx,
                                _lib.ALGO_PATCH if st.patch else _lib.ALGO_IGEMM, want_stats=FUSED_BN_STATS)
            mean = torch.empty(cs, dtype=torch.float32, device=dev)
            invstd = torch.empty(cs, dtype=torch.float32, device=dev)
            if self.record is not None:
                self._rec("conv", nd.name, x=rd[nd.src], y=y, **self._last_conv)
                run0 = [self._snap(b) for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
            if g_rows > 0:
                # the epilogue wrote [2][g_rows][cout] partials (row stride = cout); cs == cout here
                # (checked above), so the finalize reads them with the same channel count
                _lib.check(lib.drnmi_bn_stats_partials_f32(
                    _vp(self._st_ws), g_rows, rows, cs, float(bn.eps), float(bn.momentum), _vp(mean), _vp(invstd),
                    _vp(bn.running_mean), _vp(bn.running_var), _vp(bn.num_batches_tracked), ctypes.c_void_p(stream)),
                    f"bn_stats {nd.name}")
            else:
                ws = self._ws("_red_ws", lib.drnmi_reduce_workspace_bytes(rows, cs), dev)
                _lib.check(lib.drnmi_bn_stats_f32(_vp(y), rows, cs, float(bn.eps), float(bn.momentum), _vp(mean),
                                                  _vp(invstd), _vp(bn.running_mean), _vp(bn.running_var),
                                                  _vp(bn.num_batches_tracked), _vp(ws), ctypes.c_void_p(stream)),
                           f"bn_stats {nd.name}")
            for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
                torch.autograd.graph.increment_version(b)
            z = torch.empty(rows, cs, dtype=torch.float32, device=dev)
            res = rd[nd.res] if nd.res else None
            _lib.check(lib.drnmi_bn_act_f32(_vp(y), _vp(mean), _vp(invstd), _vp(bn.weight.detach()),
                                            _vp(bn.bias.detach()), _vp(res), 1 if nd.relu else 0, rows, cs, _vp(z),
                                            ctypes.c_void_p(stream)), f"bn_act {nd.name}")
            vals[nd.dst] = z
            per_node.append((y, mean, invstd) if save else None)
            if self.record is not None:
                run1 = [self._snap(b) for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
                self._rec("bn_stats", nd.name, y=y, mean=mean, invstd=invstd, fused=g_rows > 0, before=run0,
                          after=run1)
                self._rec("bn_act", nd.name, y=y, mean=mean, invstd=invstd, res=res, z=z)
            if nd.dst in self._qat_sc:
                qvals[nd.dst] = self._fake_quant(nd.dst, z, ctypes.c_void_p(stream))
        lh, lw = shapes["logits"]
        logprobs = torch.empty(n, logits.shape[1], 8 * lh, 8 * lw, dtype=torch.float32, device=dev)
        if self.model.use_torch_up:      # UpsamplingBilinear2d(8) head (lmodels/drnseg.py:285-287)
            up = None
            _lib.check(lib.drnmi_up8_bilinear_logsoftmax_argmax(logits.data_ptr(), logprobs.data_ptr(), None,
                                                                _lib.DRNMI_U8, n, logits.shape[1], lh, lw,
                                                                ctypes.c_void_p(stream)), "up8_bilinear_logsoftmax")
        else:
            up = self.model._up_plane(dev)
            _lib.check(lib.drnmi_up8_logsoftmax_argmax(logits.data_ptr(), up.data_ptr(), logprobs.data_ptr(), None,
                                                       _lib.DRNMI_U8, n, logits.shape[1], lh, lw,
                                                       ctypes.c_void_p(stream)), "up8_logsoftmax")
        if self.record is not None:
            self._rec("head", None, logits=logits, logprobs=logprobs, up=up)
        saved = None
        if save:
            saved = {"vals": vals, "shapes": shapes, "nodes": per_node, "n": n, "up": up,
                     "qat": (self._qat_E, qvals, dict(self._qat_sc))}
        return logprobs, logits, saved

    # ------------------------------------------------------------------ backward
    def backward(self, saved, logprobs, logits, g_lp, g_logits):
        lib = _lib.load()
        self._step_id += 1
        dev = logprobs.device
        stream = _lib.stream_ptr(dev)
        sp = ctypes.c_void_p(stream)
        vals, shapes, n = saved["vals"], saved["shapes"], saved["n"]
        acc = self._ensure_flat_grads(dev)
        ncls, lh, lw = logits.shape[1], logits.shape[2], logits.shape[3]
        # head: LogSoftmax backward + transpose of the bilinear up-conv
        dlog = torch.empty_like(logits)
        du = torch.empty_like(logprobs) if g_lp is not None else None
        glp = g_lp.contiguous() if g_lp is not None else None
        glg = g_logits.contiguous() if g_logits is not None else None
        if saved["up"] is None:          # use_torch_up: transpose of the bilinear x8
            _lib.check(lib.drnmi_up8_bilinear_lsm_bwd_f32(_vp(glp), _vp(logprobs) if glp is not None else None,
                                                          _vp(glg), float(self.grad_scale), n, ncls, lh, lw, _vp(du),
                                                          _vp(dlog), sp), "up8_bilinear_lsm_bwd")
        else:
            _lib.check(lib.drnmi_up8_lsm_bwd_f32(_vp(glp), _vp(logprobs) if glp is not None else None, _vp(glg),
                                                 _vp(saved["up"]), float(self.grad_scale), n, ncls, lh, lw, _vp(du),
                                                 _vp(dlog), sp), "up8_lsm_bwd")
        del du
        if self.record is not None:
            self._rec("head_bwd", None, g_lp=glp, g_logits=glg, logprobs=logprobs, up=saved["up"],
                      grad_scale=float(self.grad_scale), dlog=self._snap(dlog))
        grads = {}          # value -> NHWC fp32 gradient buffer
        # QAT (the forward's layout and scales): the W8A8 convs read fq(v), so their data and residual
        # gradients collect in qgrads[v] = d fq(v), folded into grads[v] straight-through (where the
        # level was not clamped) before v's producer consumes it
        q_e, qvals, q_sc = saved["qat"]
        qgrads = {}
        for idx in range(len(self.nodes) - 1, -1, -1):
            nd, st = self.nodes[idx], self.state[idx]
            c = nd.conv
            is_q = q_e is not None and idx in q_e
            rd, gd = (qvals, qgrads) if is_q else (vals, grads)
            cout, cin, ks, _ = c.weight.shape
            s, p, d = c.stride[0], c.padding[0], c.dilation[0]
            ih, iw = shapes[nd.src]
            oh, ow = shapes[nd.dst]
            rows = n * oh * ow
            done = []
            if nd.out_fp32_nchw:
                dys = _pow2_at_least(cout)
                dy = torch.empty(rows, dys, dtype=torch.float32, device=dev)
                _lib.check(lib.drnmi_nchw_to_nhwc(dlog.data_ptr(), dy.data_ptr(), n, cout, oh, ow, dys, F32, sp),
                           "seg grad nhwc")
                if self.record is not None:
                    dy_rec = self._snap(dy)
                    self._rec("seg_nhwc", nd.name, dlog=self._snap(dlog), dy=dy_rec)
                if c.bias is not None and c.bias.requires_grad:
                    ws = self._ws("_red_ws", lib.drnmi_reduce_workspace_bytes(rows, dys), dev)
                    before = self._snap(c.bias.grad) if self.record is not None and acc[id(c.bias)] else None
                    _lib.check(lib.drnmi_channel_sum_f32(_vp(dy), rows, dys, cout, _vp(c.bias.grad),
                                                         1 if acc[id(c.bias)] else 0, _vp(ws), sp), "seg bias grad")
                    done.append(c.bias)
                    if self.record is not None:
                        self._rec("bias_grad", nd.name, dy=dy_rec, before=before, after=self._snap(c.bias.grad))
            else:
                dys = self.cstride[nd.dst]
                dq = qgrads.pop(nd.dst, None)
                if dq is not None:
                    prev = grads.get(nd.dst)
                    dx = prev if prev is not None else torch.empty_like(dq)
                    before = self._snap(prev) if self.record is not None else None
                    _lib.check(lib.drnmi_fake_quant_bwd_f32(_vp(dq), _vp(vals[nd.dst]), dq.numel(), q_sc[nd.dst][1],
                                                            _vp(dx), 1 if prev is not None else 0, sp),
                               f"fake_quant_bwd {nd.dst}")
                    grads[nd.dst] = dx
                    if self.record is not None:
                        self._rec("fq_bwd", nd.dst, dq=dq, x=vals[nd.dst], inv_scale=q_sc[nd.dst][1], before=before,
                                  after=self._snap(dx))
                    del dq
                dz = grads.pop(nd.dst, None)
                if dz is None:
                    raise RuntimeError(f"no gradient reached {nd.name}")
                y, mean, invstd = saved["nodes"][idx]
                z = vals[nd.dst]
                bn = nd.bn
                dres = None
                dres_acc = 0
                if nd.res:
                    dres = gd.get(nd.res)
                    if dres is None:
                        dres = torch.empty_like(vals[nd.res])
                        gd[nd.res] = dres
                    else:
                        dres_acc = 1
                gw, gb = bn.weight, bn.bias
                ws = self._ws("_red_ws", lib.drnmi_reduce_workspace_bytes(rows, dys), dev)
                gacc = 1 if (gw.requires_grad and acc[id(gw)]) else 0
                if self.record is not None:
                    bn0 = dict(dz=self._snap(dz), dres_before=self._snap(dres) if dres_acc else None,
                               dgamma_before=self._snap(gw.grad) if gacc else None,
                               dbeta_before=self._snap(gb.grad) if gacc and gb.requires_grad else None)
                if nd.relu and not nd.res:
                    # residual-free BN + ReLU: the mask is recomputed from y (z is not read)
                    _lib.check(lib.drnmi_bn_relu_bwd_y_f32(
                        _vp(dz), _vp(y), _vp(mean), _vp(invstd), _vp(gw.detach()), _vp(gb.detach()), rows, dys,
                        _vp(dz), _vp(gw.grad) if gw.requires_grad else None,
                        _vp(gb.grad) if gb.requires_grad else None, gacc, _vp(ws), sp), f"bn_bwd {nd.name}")
                else:
                    _lib.check(lib.drnmi_bn_act_bwd_f32(
                        _vp(dz), _vp(z), _vp(y), _vp(mean), _vp(invstd), _vp(gw.detach()), 1 if nd.relu else 0,
                        rows, dys, _vp(dz), _vp(dres), dres_acc,
                        _vp(gw.grad) if gw.requires_grad else None, _vp(gb.grad) if gb.requires_grad else None,
                        gacc, _vp(ws), sp), f"bn_bwd {nd.name}")
                if gw.requires_grad and gb.requires_grad and acc[id(gw)] != acc[id(gb)]:
                    raise RuntimeError("BN weight/bias grads must be both set or both None")
                done += [q for q in (gw, gb) if q.requires_grad]
                dy = dz
                if self.record is not None:
                    dy_rec = self._snap(dy)
                    self._rec("bn_bwd", nd.name, z=z, y=y, mean=mean, invstd=invstd, dy=dy_rec, dres=self._snap(dres),
                              dgamma=self._snap(gw.grad) if gw.requires_grad else None,
                              dbeta=self._snap(gb.grad) if gb.requires_grad else None,
                              from_y=bool(nd.relu and not nd.res), **bn0)
            # weight gradient
            if c.weight.requires_grad:
                wa = _lib.WgradArgs()
                wa.dy, wa.x, wa.dw = dy.data_ptr(), rd[nd.src].data_ptr(), c.weight.grad.data_ptr()
                wa.n, wa.h, wa.w, wa.cin, wa.cin_stride = n, ih, iw, cin, self.cstride[nd.src]
                wa.ho, wa.wo, wa.cout, wa.dy_stride = oh, ow, cout, dys
                wa.ks, wa.stride, wa.pad, wa.dil = ks, s, p, d
                wa.accumulate = 1 if acc[id(c.weight)] else 0
                # fp32x: every weight gradient is split-bf16 (the forward's small-channel layers
                # run split on the patch kernels as well); fp32 sizes only its own partials
                x3 = self.model.precision == "fp32x"
                nb = (lib.drnmi_conv_wgrad_workspace_bytes if x3 else lib.drnmi_conv_wgrad_f32_workspace_bytes)(
                    ctypes.byref(wa))
                if nb < 0:
                    raise RuntimeError(f"wgrad {nd.name}: bad geometry")
                ws = self._ws("_wg_ws", nb, dev)
                wa.ws, wa.ws_bytes = ws.data_ptr(), ws.numel()
                wg = lib.drnmi_conv_wgrad_f32x3 if x3 else lib.drnmi_conv_wgrad_f32
                before = self._snap(c.weight.grad) if self.record is not None and wa.accumulate else None
                _lib.check(wg(ctypes.byref(wa), sp), f"wgrad {nd.name}")
                done.append(c.weight)
                if self.record is not None:
                    self._rec("wgrad", nd.name, dy=dy_rec, x=rd[nd.src], before=before,
                              after=self._snap(c.weight.grad), x3=x3, plan=_lib.wgrad_plan(wa, x3))
            if self.grad_ready is not None and done:
                self.grad_ready(done)
            # data gradient (not needed for the network input)
            classes = (self._s2_classes(nd, st, dev, sp) if nd.src != "input" and s == 2 and S2_CLASS_DGRAD
                       else None)
            if classes is not None:
                # stride 2: four parity-class convs of dy itself, no zero-inserted copy
                cs_src = self.cstride[nd.src]
                prev = gd.get(nd.src)
                if prev is not None:
                    out = prev
                elif len(classes) < 4:          # pixels no tap reaches keep a zero gradient
                    out = torch.zeros(n * ih * iw, cs_src, dtype=torch.float32, device=dev)
                else:
                    out = torch.empty(n * ih * iw, cs_src, dtype=torch.float32, device=dev)
                flat = out.view(-1)
                fill = "prev" if prev is not None else "zeros" if len(classes) < 4 else "empty"
                for (a_, b_, ksc, planes) in classes:
                    ho_c, wo_c = (ih - a_ + 1) // 2, (iw - b_ + 1) // 2
                    if ho_c <= 0 or wo_c <= 0:
                        continue
                    base = (a_ * iw + b_) * cs_src
                    view = flat[base:]
                    before = self._snap(out) if self.record is not None else None
                    self._conv(dy, dys, oh, ow, None, ksc * ksc * dys, ksc * ksc * dys, st.rows_d, cin, ksc, 1, 0,
                               1, view, (ih * iw * cs_src, 2 * cs_src, 1), self._zeros_f32(st.rows_d, dev),
                               view if prev is not None else None, n, ho_c, wo_c, stream,
                               f"dgrad {nd.name} class {a_}{b_}", planes, y_sr=2 * iw * cs_src, split=False)
                    if self.record is not None:
                        self._rec("dgrad", nd.name, form="class", cls=(a_, b_), fill=fill, dy=dy_rec, before=before,
                                  after=self._snap(out), **self._last_conv)
                gd[nd.src] = out
            elif nd.src != "input":
                dys_d = self._pack_dgrad(nd, st, dev, sp)
                assert dys_d == dys
                cs_src = self.cstride[nd.src]
                src = dy
                hu, wu = oh, ow
                pad_d = d * (ks - 1) - p
                if s > 1:
                    hu, wu = ih + 2 * p - d * (ks - 1), iw + 2 * p - d * (ks - 1)
                    src = torch.empty(n * hu * wu, dys, dtype=torch.float32, device=dev)
                    _lib.check(lib.drnmi_zero_insert_f32(_vp(dy), n, oh, ow, dys, s, hu, wu, _vp(src), sp),
                               f"zero_insert {nd.name}")
                prev = gd.get(nd.src)
                out = prev if prev is not None else torch.empty(n * ih * iw, cs_src, dtype=torch.float32, device=dev)
                patch = st.dpatch and prev is None       # the patch kernels take no residual
                before = self._snap(prev) if self.record is not None else None
                self._conv(src, dys, hu, wu, st.wd, st.kd, st.kd_pad, st.rows_d, cin, ks, 1, pad_d, d, out,
                           (ih * iw * cs_src, cs_src, 1), self._zeros_f32(st.rows_d, dev), prev, n, ih, iw,
                           stream, f"dgrad {nd.name}", st.wdx if (patch or not st.dpatch) else None,
                           _lib.ALGO_PATCH if patch else _lib.ALGO_IGEMM)
                if self.record is not None:
                    self._rec("dgrad", nd.name, form="zero_insert" if s > 1 else "s1", cls=None,
                              fill="prev" if prev is not None else "empty", dy=dy_rec, before=before,
                              after=self._snap(out), **self._last_conv)
                gd[nd.src] = out
            del dy


class _TrainFn(torch.autograd.Function):
    """DRNSeg train-mode forward as one autograd node; backward = the HIP backward kernels."""

    @staticmethod
    def forward(ctx, runner, x, *params):
        ctx.set_materialize_grads(False)
        lp, logits, saved = runner.forward(x, save=True)
        ctx.runner = runner
        ctx.saved = saved
        ctx.outs = (lp, logits)
        return lp, logits

    @staticmethod
    def backward(ctx, g_lp, g_logits):
        lp, logits = ctx.outs
        if g_lp is not None or g_logits is not None:
            ctx.runner.backward(ctx.saved, lp, logits, g_lp, g_logits)
        ctx.saved = None
        # parameter grads were written straight into .grad (flat buffer views)
        return (None,) * len(ctx.needs_input_grad)


def train_forward(model, x: torch.Tensor):
    """DRNSeg.forward in train mode (batch-stat BN, autograd through the HIP backward)."""
    runner = getattr(model, "_train_runner", None)
    if runner is None:
        runner = TrainRunner(model)
        model._train_runner = runner
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("DRNSeg.forward expects fp32 [B,3,H,W]")
    x = x.contiguous()
    params = [p for p in runner.ordered_params() if p.requires_grad]
    if torch.is_grad_enabled() and params:
        return _TrainFn.apply(runner, x, *params)
    lp, logits, _ = runner.forward(x, save=False)
    return lp, logits


# ====================================================================== criterion
class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, target, ignore_index):
        lib = _lib.load()
        n, c = lp.shape[0], lp.shape[1]
        hw = lp[0, 0].numel()
        dev = lp.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.drnmi_ce_workspace_bytes(), dtype=torch.uint8, device=dev)
        sp = ctypes.c_void_p(_lib.stream_ptr(dev))
        _lib.check(lib.drnmi_ce_loss_f32(_vp(lp), _vp(target), n, c, hw, int(ignore_index), _vp(loss), _vp(count),
                                         _vp(ws), sp), "ce_loss")
        ctx.save_for_backward(lp, target, count)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, g):
        lp, target, count = ctx.saved_tensors
        lib = _lib.load()
        n, c = lp.shape[0], lp.shape[1]
        hw = lp[0, 0].numel()
        glp = torch.empty_like(lp)
        g = g.contiguous().to(torch.float32)
        _lib.check(lib.drnmi_ce_loss_bwd_f32(_vp(lp), _vp(target), n, c, hw, int(ctx.ignore_index), _vp(g),
                                             _vp(count), _vp(glp), ctypes.c_void_p(_lib.stream_ptr(lp.device))),
                   "ce_loss_bwd")
        return glp, None, None


class CrossEntropyLoss(torch.nn.Module):
    """nn.CrossEntropyLoss(ignore_index=255) drop-in (semantic_seg.py:817) on the HIP kernels.

    Like the reference it is applied to DRNSeg's log-probs (model(x)[0]), i.e. it computes
    mean over target != ignore_index of logsumexp(lp) - lp[target] (a second log-softmax,
    semantic_seg.py:197-198).  Only mean reduction and no class weights (the reference's use)."""

    def __init__(self, weight=None, ignore_index: int = -100, reduction: str = "mean"):
        super().__init__()
        if weight is not None or reduction != "mean":
            raise NotImplementedError("class weights / reduction != 'mean' are not used by the reference")
        self.ignore_index = ignore_index

    def forward(self, logprobs: torch.Tensor, target: torch.Tensor):
        if not logprobs.is_cuda:
            raise RuntimeError("drnmi CrossEntropyLoss runs on the HIP kernels (no CPU fallback)")
        if logprobs.dtype != torch.float32:
            raise ValueError("expected fp32 log-probs")
        if target.dtype != torch.int64:
            raise ValueError("expected int64 targets (semantic_seg.py:195 target.long())")
        if target.shape != (logprobs.shape[0],) + tuple(logprobs.shape[2:]):
            raise ValueError(f"target shape {tuple(target.shape)} does not match {tuple(logprobs.shape)}")
        return _CEFn.apply(logprobs.contiguous(), target.contiguous(), self.ignore_index)


class _DistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, tlp, target, ignore_index, student_wt, distill_wt, temperature, batchmean):
        lib = _lib.load()
        n, c = lp.shape[0], lp.shape[1]
        hw = lp[0, 0].numel()
        dev = lp.device
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.drnmi_distill_workspace_bytes(), dtype=torch.uint8, device=dev)
        _lib.check(lib.drnmi_distill_loss_f32(_vp(lp), _vp(tlp), _vp(target), n, c, hw, int(ignore_index), student_wt,
                                              distill_wt, temperature, batchmean, _vp(out3), _vp(count), _vp(ws),
                                              ctypes.c_void_p(_lib.stream_ptr(dev))), "distill_loss")
        ctx.save_for_backward(lp, tlp, target, count)
        ctx.args = (int(ignore_index), student_wt, distill_wt, temperature, batchmean)
        loss, ce, kd = out3.unbind(0)
        ctx.mark_non_differentiable(ce, kd)
        return loss, ce, kd

    @staticmethod
    def backward(ctx, g, _g_ce, _g_kd):
        lp, tlp, target, count = ctx.saved_tensors
        n, c = lp.shape[0], lp.shape[1]
        hw = lp[0, 0].numel()
        glp = torch.empty_like(lp)
        g = g.contiguous().to(torch.float32)
        _lib.check(_lib.load().drnmi_distill_loss_bwd_f32(_vp(lp), _vp(tlp), _vp(target), n, c, hw, *ctx.args, _vp(g),
                                                          _vp(count), _vp(glp),
                                                          ctypes.c_void_p(_lib.stream_ptr(lp.device))),
                   "distill_loss_bwd")
        return (glp,) + (None,) * 7


class DistillationLoss(torch.nn.Module):
    """Knowledge distillation from a dense teacher into the pruned student (the reference's
    --mc-kd, rmbsnn_main.py:192-243, for the segmentation loop) as one HIP pass forward and one
    backward over the two log-prob tensors:

        loss = student_wt * CE + distill_wt * KD
        CE   = CrossEntropyLoss(ignore_index) of the student's log-probs (the criterion above)
        KD   = sum over pixels of KL(softmax(teacher / T) || softmax(student / T)) / D

    Every pixel counts for KD, labelled or not (the teacher supervises the pixels ignore_index
    hides from CE); only labelled pixels count for CE.  kd_reduction="mean" divides by the number
    of pixels n * h * w; "batchmean" by n, which is the reference's
    F.kl_div(size_average=False) / shape[0].  There is NO T^2 factor on the KD term: the reference
    has none, so at T > 1 the KD gradient is 1 / T of the T = 1 one — fold T^2 into distill_wt if
    Hinton's scaling is wanted.  The teacher gets no gradient.  A batch with no labelled pixel
    gives a NaN CE (0 / 0, as CrossEntropyLoss) and so a NaN loss, whatever student_wt is.

    After a forward, `.ce` and `.kd` hold the two terms as detached device scalars (no host
    synchronisation).  No CPU or ATen fallback."""

    def __init__(self, student_wt: float = 0.5, distill_wt: float = 0.5, temperature: float = 1.0,
                 ignore_index: int = -100, kd_reduction: str = "mean"):
        super().__init__()
        student_wt, distill_wt, temperature = float(student_wt), float(distill_wt), float(temperature)
        if not (temperature > 0 and temperature != float("inf")):
            raise ValueError("temperature must be finite and > 0")
        for w in (student_wt, distill_wt):
            if not (0 <= w < float("inf")):
                raise ValueError("student_wt and distill_wt must be finite and >= 0")
        if kd_reduction not in ("mean", "batchmean"):
            raise ValueError("kd_reduction must be 'mean' (per pixel) or 'batchmean' (per image, the reference's)")
        self.student_wt, self.distill_wt, self.temperature = student_wt, distill_wt, temperature
        self.ignore_index = ignore_index
        self.kd_reduction = kd_reduction
        self.ce = self.kd = None

    def forward(self, logprobs: torch.Tensor, teacher_logprobs: torch.Tensor, target: torch.Tensor):
        if logprobs.dtype != torch.float32 or teacher_logprobs.dtype != torch.float32:
            raise ValueError("expected fp32 log-probs (student and teacher)")
        if target.dtype != torch.int64:
            raise ValueError("expected int64 targets (semantic_seg.py:195 target.long())")
        if logprobs.dim() < 2 or teacher_logprobs.shape != logprobs.shape:
            raise ValueError(f"teacher log-probs {tuple(teacher_logprobs.shape)} do not match the student's "
                             f"{tuple(logprobs.shape)}")
        if target.shape != (logprobs.shape[0],) + tuple(logprobs.shape[2:]):
            raise ValueError(f"target shape {tuple(target.shape)} does not match {tuple(logprobs.shape)}")
        if teacher_logprobs.requires_grad:
            raise ValueError("the teacher gets no gradient: compute its log-probs under torch.no_grad() "
                             "(teacher_logprobs()) or detach them")
        if not logprobs.is_cuda:
            raise RuntimeError("drnmi DistillationLoss runs on the HIP kernels (no CPU fallback)")
        if teacher_logprobs.device != logprobs.device or target.device != logprobs.device:
            raise ValueError("student log-probs, teacher log-probs and target must be on one device")
        loss, ce, kd = _DistillFn.apply(logprobs.contiguous(), teacher_logprobs.contiguous(), target.contiguous(),
                                        self.ignore_index, self.student_wt, self.distill_wt, self.temperature,
                                        1 if self.kd_reduction == "batchmean" else 0)
        self.ce, self.kd = ce, kd
        return loss


def teacher_logprobs(teacher, x: torch.Tensor) -> torch.Tensor:
    """The frozen teacher's log-probs for DistillationLoss: teacher(x)[0] under torch.no_grad(), at
    whichever inference precision the teacher is set to (bf16 is the fast engine).  The teacher must
    be in eval mode: its BatchNorm has to use the running statistics and must not update them."""
    if teacher.training:
        raise RuntimeError("the distillation teacher must be in eval mode (teacher.eval()): train-mode "
                           "BatchNorm would use batch statistics and update the running ones")
    with torch.no_grad():
        return teacher(x)[0]


# ====================================================================== eval score
def accuracy(output: torch.Tensor, target: torch.Tensor, ignore_index: int = 255) -> torch.Tensor:
    """utils.accuracy drop-in for `eval_score=accuracy` (utils.py:267-277; semantic_seg.py:1072,
    :1004): the percentage of pixels with target != ignore_index whose argmax over the class planes
    equals the target, as a 0-dim fp32 device tensor float32(correct) * float32(100.0 / count).
    One pass (drnmi_pixel_accuracy_f32) instead of the reference's argmax plus boolean-index
    gather, and no host synchronisation.  count == 0 gives NaN (the reference raises
    ZeroDivisionError there)."""
    if not output.is_cuda:
        raise RuntimeError("drnmi accuracy runs on the HIP kernel (no CPU fallback)")
    if output.dtype != torch.float32 or output.dim() < 2:
        raise ValueError("expected fp32 [n, c, ...] scores")
    if target.dtype != torch.int64:
        raise ValueError("expected int64 targets (semantic_seg.py:195 target.long())")
    n, c = output.shape[0], output.shape[1]
    hw = output[0, 0].numel()
    if target.numel() != n * hw or target.device != output.device:
        raise ValueError(f"target shape {tuple(target.shape)} does not match {tuple(output.shape)}")
    output, target = output.detach().contiguous(), target.contiguous()
    counts = torch.zeros(2, dtype=torch.int64, device=output.device)
    _lib.check(_lib.load().drnmi_pixel_accuracy_f32(_vp(output), _vp(target), n, c, hw, int(ignore_index), _vp(counts),
                                                    ctypes.c_void_p(_lib.stream_ptr(output.device))), "pixel_accuracy")
    return counts[1].float() * (100.0 / counts[0].double()).float()


# ====================================================================== optimizer
class SGD(torch.optim.Optimizer):
    """torch.optim.SGD drop-in (semantic_seg.py:963-966) whose step is one multi-tensor HIP
    launch per 48 parameters.  With `pruner=` the pruner's masks are applied inside the same
    pass (replacing the separate Pruner.apply_masks after optimizer.step(), :213-214);
    state['momentum_buffer'] matches torch's, so state_dict()/load_state_dict() interoperate."""

    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, pruner=None,
                 model=None):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))
        self.pruner = pruner
        self._mask_of = {}
        if pruner is not None:
            if model is None:
                raise ValueError("SGD(pruner=...) needs model= to resolve mask keys to parameters")
            self.attach_pruner(pruner, model)

    def attach_pruner(self, pruner, model):
        self.pruner = pruner
        named = dict(model.named_parameters())
        self._mask_of = {}
        for key in pruner.mask_dict:
            for cand in (key, "module." + key, key[len("module."):] if key.startswith("module.") else None):
                if cand is not None and cand in named:
                    self._mask_of[id(named[cand])] = key
                    break
            else:
                raise KeyError(key)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for group in self.param_groups:
            ps, gs, bs, ns, ms, fs = [], [], [], [], [], []
            mom = group["momentum"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("drnmi SGD: parameters/grads must be contiguous fp32 on the ROCm device")
                st = self.state[p]
                first = 0
                if mom != 0:
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = torch.empty_like(p)
                        st["momentum_buffer"] = buf
                        first = 1
                    bs.append(buf)
                ps.append(p)
                gs.append(p.grad)
                ns.append(p.numel())
                fs.append(first)
                key = self._mask_of.get(id(p))
                ms.append(self.pruner._mask_bits(key, p.device) if key is not None else None)
            if not ps:
                continue
            k = len(ps)
            arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() if t is not None else None for t in ts])
            mask_arr = arr(ms) if any(m is not None for m in ms) else None
            _lib.check(lib.drnmi_sgd_step_f32(
                k, arr(ps), arr(gs), arr(bs) if mom != 0 else None, (ctypes.c_int64 * k)(*ns), mask_arr,
                (ctypes.c_int32 * k)(*fs), float(group["lr"]), float(mom), float(group["dampening"]),
                float(group["weight_decay"]), 1 if group["nesterov"] else 0,
                ctypes.c_void_p(_lib.stream_ptr(ps[0].device))), "sgd_step")
            for p in ps:
                torch.autograd.graph.increment_version(p)
        return loss
