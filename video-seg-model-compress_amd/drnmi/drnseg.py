"""DRNSeg — drop-in for the reference segmentation module, run on HIP kernels.

Reference API (kept): semantic_seg.py:126-164 / lmodels/drnseg.py:268-305
  DRNSeg(model_name, classes, pretrained_model=None, pretrained=True, use_torch_up=False)
  forward(x: fp32 [B,3,H,W]) -> (log_probs fp32 [B,C,8h,8w], logits fp32 [B,C,h,w])
  optim_parameters()  -> layer + seg params (up excluded)
  state_dict keys     layer.{0..8}.*, seg.weight, seg.bias, up.weight  (DRN-C, drn_c_26 / 42 / 58:
                      layer.0.weight, layer.1.*, layer.{3..10}.*: the stem is three bare children)
                      (load_state_dict also accepts the seg_video "base." prefix,
                       log.txt:18-170, and a DataParallel/DDP "module." prefix)

Differences by design:
  * forward runs the fused HIP plan (drnmi.engine) on a ROCm device, as the registered
    custom op torch.ops.drnmi.forward (drnmi.torch_ops; also .predict / .segment).  It never
    falls back to ATen; on CPU it raises.  In train mode it runs the fine-tune path
    (drnmi.train: batch-stat BN, autograd through the HIP backward kernels, fp32).
  * use_torch_up=True keeps the reference's nn.UpsamplingBilinear2d(scale_factor=8) head
    (lmodels/drnseg.py:285-287: bilinear, align_corners=True, output 8h x 8w) on its own
    fused HIP kernel (drnmi_up8_bilinear_logsoftmax_argmax).
  * precision: "fp32" (default; the reference's arithmetic, parity mode, exact-fp32
    MFMA), "fp32x" (fp32-accurate arithmetic on the bf16 MFMA pipe: exact 3-way bf16 splits,
    6 products, for every conv with cin >= 32; parity gates as fp32, ~3x faster), "bf16"
    (perf mode, fp32 accumulation), "fp8" (OCP e4m3 weights and activations on the same convs
    as int8, fp32 accumulation, the int8 calibration's scales; inference only) or "int8" (W8A8 for the cin >= 64 convs,
    config C5; needs calibrate_int8() or load_int8_state() first — the reference has no
    quantisation, so this mode is ours; DRN-D only) via set_precision().
  * segment(frames_u8) is the fused seg_video path (seg_video_old_no_plot.py:157-169:
    normalise -> model(img)[0] -> torch.max(final, 1)) producing uint8 labels without
    materialising the 19-plane log-prob tensor.  segment(render="color" | "overlay") also returns
    the picture that loop ends in (CITYSCAPE_PALETTE[pred], :170, alone or drawn over the frame),
    made on the GPU by drnmi_render_labels with an integer blend (not matplotlib's compositing).
  * model_name is honoured (lmodels/drnseg.py:272 always builds D-22; semantic_seg.py
    :130-131 builds model_name — we follow the driver copy).
"""
from __future__ import annotations

import json
import math
import os

import torch
import torch.nn as nn

from . import _lib, drn, torch_ops
from .engine import PackedNet, Plan, lower_drnseg
from .weights import bilinear_up_kernel

# info.json:1 (Cityscapes normalisation used by every reference driver)
INFO_MEAN = (0.29010095242892997, 0.32808144844279574, 0.28696394422942517)
INFO_STD = (0.1829540508368939, 0.18656561047509476, 0.18447508988480435)


def fill_up_weights(up: nn.ConvTranspose2d) -> None:
    """Bilinear kernel into every depthwise plane (lmodels/drnseg.py:257-266)."""
    k = up.weight.shape[2]
    w = torch.from_numpy(bilinear_up_kernel(k))
    with torch.no_grad():
        up.weight.copy_(w.expand_as(up.weight))


class DRNSeg(nn.Module):
    def __init__(self, model_name, classes, pretrained_model=None, pretrained=True,
                 use_torch_up=False):
        super().__init__()
        factory = getattr(drn, model_name, None)
        if factory is None:
            raise KeyError(f"unknown model {model_name!r}; known: {drn.ARCHS}")
        model = factory(pretrained=pretrained, num_classes=1000)
        if pretrained_model is not None:
            model.load_state_dict(pretrained_model)
        self.layer = nn.Sequential(*list(model.children())[:-2])
        self.seg = nn.Conv2d(model.out_dim, classes, kernel_size=1, bias=True)
        self.softmax = nn.LogSoftmax(dim=1)
        n = self.seg.kernel_size[0] * self.seg.kernel_size[1] * self.seg.out_channels
        self.seg.weight.data.normal_(0, math.sqrt(2.0 / n))
        self.seg.bias.data.zero_()
        if use_torch_up:
            self.up = nn.UpsamplingBilinear2d(scale_factor=8)
        else:
            up = nn.ConvTranspose2d(classes, classes, 16, stride=8, padding=4, output_padding=0,
                                    groups=classes, bias=False)
            fill_up_weights(up)
            up.weight.requires_grad = False
            self.up = up
        self.use_torch_up = bool(use_torch_up)
        self.model_name = model_name
        self.arch = model.arch       # "D" or "C" (lmodels/drn.py:119)
        self.classes = classes
        self.precision = "fp32"
        self.block_sparse = False    # opt-in: measured slower than dense below ~60 % zero units
        self.sparse24 = False        # opt-in: 2:4-pruned bf16 layers on the sparse MFMA (set_sparse24)
        self._graph = lower_drnseg(self.layer, self.seg)
        self._act_scales = None      # int8: per-value activation scales (calibrate_int8)
        self._int8_hists = None      # value -> |x| histogram of the last histogram calibration
        self._int8_method = None     # how _act_scales were derived (int8_state)
        self._int8_percentile = None
        self._qat = None             # "int8": quantisation-aware fine-tuning (set_qat)
        self._packed = {}
        self._plans = {}
        self._pack_key = None
        self._key_tensors = None     # cached parameter/buffer list of the repack key
        self._key_ids = None         # ids of the parameter/buffer/submodule objects it was built from
        self._key_dicts = []         # the modules' _parameters/_buffers/_modules dicts behind them
        self.timing_hook = None      # optional per-launch callback (bench.py's HIP events)
        self._handle = torch_ops.register_model(self)   # torch.ops.drnmi.* state handle

    # copies and unpickled modules register a handle of their own: the handle keys the
    # torch.ops.drnmi.* state, and a copied integer would dispatch to the ORIGINAL model's
    # weights.  Packed weights and launch plans hold device pointers of this instance: not copied.
    # The int8 activation scales travel with the copy; the calibration histograms behind them
    # (256 KiB per activation) do not.
    def __getstate__(self):
        st = self.__dict__.copy()
        st.pop("_handle", None)
        st.update(_packed={}, _plans={}, _pack_key=None, _key_tensors=None, _key_ids=None, _key_dicts=[],
                  timing_hook=None, _int8_hists=None)
        st.pop("_train_runner", None)
        st.pop("_qat", None)         # like the runner: a copy fine-tunes without QAT until set_qat
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        self._handle = torch_ops.register_model(self)

    # ----------------------------------------------------------------- reference API
    def optim_parameters(self, memo=None):
        for param in self.layer.parameters():
            yield param
        for param in self.seg.parameters():
            yield param

    def forward(self, x: torch.Tensor):
        if self.training:
            # fine-tune path: batch-stat BN + autograd through the HIP backward kernels
            if x.device.type != "cuda":
                raise RuntimeError("drnmi.DRNSeg runs on the HIP engine only (no CPU fallback by design)")
            if self.precision not in ("fp32", "fp32x"):
                raise NotImplementedError("the fine-tune path runs in fp32 (the reference's arithmetic) or fp32x "
                                          "(fp32-accurate split-bf16 forward/dgrad convs)")
            from .train import train_forward
            return train_forward(self, x)
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("DRNSeg.forward expects fp32 [B,3,H,W]")
        self._check_device(x)
        return torch.ops.drnmi.forward(x, self._handle)

    # ----------------------------------------------------------------- fused paths
    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """torch.max(model(x)[0], 1)[1] (semantic_seg.py:444-445) as one fused pass: int64 labels."""
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("DRNSeg.predict expects fp32 [B,3,H,W]")
        self._check_device(x)
        return torch.ops.drnmi.predict(x, self._handle)

    def segment(self, frames_u8: torch.Tensor, mean=INFO_MEAN, std=INFO_STD, bgr: bool = False,
                labels: torch.Tensor | None = None, size=None, render: str | None = None, alpha: float = 0.6,
                palette=None):
        """Video path: uint8 HWC frames [B,H,W,3] on the GPU -> uint8 label maps [B,8h,8w].

        Fuses ToTensorVideoImage + Normalize (data_transforms.py:256-281, :109-125) into the
        ingest kernel and model(img)[0] + torch.max(final,1) into the head kernel.  Runs as
        torch.ops.drnmi.segment (graph-capturable); `labels=` writes into a caller buffer.
        size=(oh, ow): first resize the frames on the GPU exactly as seg_video's
        T.Resize((300, 300)) does on each PIL frame (seg_video_old_no_plot.py:126-127;
        Pillow BILINEAR arithmetic, drnmi_resize_bilinear_u8).
        render="color" / "overlay": returns (labels, image), image uint8 [B,H,W,3] at the size of
        the frames the network saw (with size= the resized frames, what the reference overlays
        onto: raw_images[i] is the resized PIL image): palette[label] (None = CITYSCAPE_PALETTE,
        seg_video_old_no_plot.py:170; a model with more than 20 classes: generic_palette), for "overlay" drawn over the frame with `alpha` by the
        integer blend of drnmi_render_labels, in the frames' channel order (bgr).  As
        torch.ops.drnmi.segment_render it is graph-capturable too."""
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
            raise ValueError("segment expects uint8 [B,H,W,3] frames")
        if render not in (None, "color", "overlay"):
            raise ValueError("render must be None, 'color' or 'overlay'")
        self._check_device(frames_u8)
        if size is not None and tuple(size) != tuple(frames_u8.shape[1:3]):
            from .ops import resize_bilinear_u8
            frames_u8 = resize_bilinear_u8(frames_u8, size)
        if render is not None:
            from .ops import render_labels
            from .palette import CITYSCAPE_PALETTE, as_device_palette, generic_palette
            if not 0.0 <= float(alpha) <= 1.0:
                raise ValueError("alpha must be in [0, 1]")
            if palette is None:
                palette = CITYSCAPE_PALETTE if self.classes <= 20 else generic_palette(self.classes)
            pal = as_device_palette(palette, frames_u8.device)
            if labels is None:
                return torch.ops.drnmi.segment_render(frames_u8, self._handle, [float(v) for v in mean],
                                                      [float(v) for v in std], bool(bgr), pal,
                                                      int(round(float(alpha) * 256)), render == "overlay")
            labels = self._segment_impl(frames_u8, mean, std, bgr, labels)
            return labels, render_labels(labels, pal, frames_u8 if render == "overlay" else None, alpha, bgr,
                                         frames_u8.shape[1:3])
        if labels is not None:
            return self._segment_impl(frames_u8, mean, std, bgr, labels)
        return torch.ops.drnmi.segment(frames_u8, self._handle, [float(v) for v in mean],
                                       [float(v) for v in std], bool(bgr))

    # bodies of the torch.ops.drnmi ops (drnmi/torch_ops.py)
    def _forward_impl(self, x: torch.Tensor):
        plan, stream = self._prepare(x.shape[0], x.shape[2], x.shape[3], x.device)
        x = x.contiguous()
        plan.ingest_nchw(x, stream)
        plan.run_backbone(stream, self.timing_hook)
        oh, ow = plan.out_hw
        logprobs = torch.empty(x.shape[0], self.classes, oh, ow, dtype=torch.float32, device=x.device)
        self._head(plan, stream, logprobs, None)
        logits = plan.bufs["logits"].clone()
        return logprobs, logits

    def _predict_impl(self, x: torch.Tensor) -> torch.Tensor:
        plan, stream = self._prepare(x.shape[0], x.shape[2], x.shape[3], x.device)
        plan.ingest_nchw(x.contiguous(), stream)
        plan.run_backbone(stream, self.timing_hook)
        oh, ow = plan.out_hw
        labels = torch.empty(x.shape[0], oh, ow, dtype=torch.int64, device=x.device)
        self._head(plan, stream, None, labels)
        return labels

    def _segment_impl(self, frames_u8, mean, std, bgr, labels):
        plan, stream = self._prepare(frames_u8.shape[0], frames_u8.shape[1], frames_u8.shape[2],
                                     frames_u8.device)
        plan.ingest_u8(frames_u8.contiguous(), mean, std, bgr, stream)
        path = plan.labels_path(self.use_torch_up)
        plan.run_backbone(stream, self.timing_hook, labels_only=path != "nchw")
        oh, ow = plan.out_hw
        if labels is None:
            labels = torch.empty(frames_u8.shape[0], oh, ow, dtype=torch.uint8, device=frames_u8.device)
        elif labels.shape != (frames_u8.shape[0], oh, ow) or labels.dtype not in (torch.uint8, torch.int64) \
                or not labels.is_contiguous() or labels.device != frames_u8.device:
            raise ValueError(f"labels must be a contiguous uint8/int64 [{frames_u8.shape[0]}, {oh}, {ow}] tensor "
                             f"on {frames_u8.device}")
        hook, head_idx = self.timing_hook, len(plan.packed.graph.nodes)   # (the head's launch index)
        if hook is not None:
            hook(head_idx, None, True)
        if path == "seg2":
            plan.head_labels_seg2(self._up_plane(plan.packed.device), stream, labels)
        elif path == "nhwc":
            plan.head_labels_nhwc(self._up_plane(plan.packed.device), stream, labels)
        else:
            self._head(plan, stream, None, labels)
        if hook is not None:
            hook(head_idx, None, False)
        return labels

    def _head(self, plan, stream, logprobs, labels):
        if self.use_torch_up:
            plan.head_bilinear(stream, logprobs, labels)
        else:
            plan.head(self._up_plane(plan.packed.device), stream, logprobs, labels)

    @staticmethod
    def _check_device(t: torch.Tensor):
        if t.device.type != "cuda":
            raise RuntimeError("drnmi.DRNSeg runs on the HIP engine only: move the model and input "
                               "to a ROCm device (no CPU fallback by design)")

    # ----------------------------------------------------------------- configuration
    def set_precision(self, precision: str) -> "DRNSeg":
        if precision not in ("fp32", "fp32x", "bf16", "int8", "fp8"):
            raise ValueError("precision must be 'fp32', 'fp32x', 'bf16', 'int8' or 'fp8'")
        if precision in ("int8", "fp8") and self.arch != "D":
            # the int8 launches are pinned bit for bit by an oracle that restates DRN-D only, and fp8
            # follows int8's layout
            raise NotImplementedError(f"precision '{precision}' covers the DRN-D family only; {self.model_name} "
                                      "runs in 'fp32', 'fp32x' or 'bf16'")
        self.precision = precision
        return self

    @torch.no_grad()
    def calibrate_int8(self, frames_u8, mean=INFO_MEAN, std=INFO_STD, bgr: bool = False,
                       method: str = "absmax", percentile: float = 99.99):
        """Per-tensor activation scales for precision "int8": the bf16 engine runs the
        calibration frames (uint8 [B,H,W,3] on the GPU) and every activation's scale is
        absmax / 127 (drnmi_absmax on the HBM buffer).  Re-packs the int8 weights.

        frames_u8 may also be an iterable of such batches (one shape; a DataLoader, a list), and
        method "percentile" or "mse" (drnmi.calibrate.scale_from_histogram) picks a clip below
        the maximum.  Anything but one tensor with method "absmax" accumulates an exact |x|
        histogram per activation over all batches (drnmi_abs_histogram, 256 KiB each) and derives
        the scales from it; the histograms stay available (int8_histograms, rescale_int8)."""
        from .calibrate import METHODS
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        if not (isinstance(frames_u8, torch.Tensor) and method == "absmax"):
            batches = [frames_u8] if isinstance(frames_u8, torch.Tensor) else frames_u8
            return self._calibrate_int8_hist(batches, mean, std, bgr, method, percentile)
        import ctypes
        prev = self.precision
        self.precision = "bf16"
        try:
            plan, stream = self._prepare(frames_u8.shape[0], frames_u8.shape[1], frames_u8.shape[2],
                                         frames_u8.device, keep_all=True)
            plan.ingest_u8(frames_u8.contiguous(), mean, std, bgr, stream)
            plan.run_backbone(stream)
            lib = _lib.load()
            amax = torch.empty(1, dtype=torch.float32, device=frames_u8.device)
            scales = {}
            values = set(plan.packed.graph.channels)             # graph values only (not the
            for v, buf in plan.bufs.items():                      # head's logits_nhwc / seg_part buffers)
                if v in ("input", "logits") or v not in values:
                    continue
                _lib.check(lib.drnmi_absmax(buf.data_ptr(), _lib.DRNMI_BF16, buf.numel(), amax.data_ptr(),
                                            ctypes.c_void_p(stream)), "absmax")
                a = float(amax.item())
                scales[v] = a / 127.0 if a > 0 else 1.0
        finally:
            self.precision = prev
            self._plans = {k: p for k, p in self._plans.items() if not k[-1]}   # drop the keep_all plan
        self._int8_hists = None
        return self._install_act_scales(scales, "absmax", None)

    def _install_act_scales(self, scales, method, percentile):
        """New activation scales: the int8 / fp8 packs and plans built on the old ones go."""
        self._act_scales = scales
        self._int8_method, self._int8_percentile = method, percentile
        for q8 in ("int8", "fp8"):
            self._packed.pop(q8, None)
        self._plans = {k: p for k, p in self._plans.items() if k[0] not in ("int8", "fp8")}
        self._pack_key = None
        return scales

    def _int8_values(self):
        """The graph values that carry an activation scale (all but the input and the logits)."""
        return [v for v in self._graph.channels if v not in ("input", "logits")]

    def _calibrate_int8_hist(self, batches, mean, std, bgr, method, percentile):
        from .ops import abs_histogram
        prev = self.precision
        self.precision = "bf16"
        hists, shape = {}, None
        try:
            for frames in batches:
                if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 \
                        or frames.shape[3] != 3:
                    raise ValueError("calibrate_int8 expects uint8 [B,H,W,3] batches")
                if shape is None:
                    shape = tuple(frames.shape)
                elif tuple(frames.shape) != shape:
                    raise ValueError(f"calibrate_int8: batches must share one shape, got {shape} and "
                                     f"{tuple(frames.shape)}")
                plan, stream = self._prepare(shape[0], shape[1], shape[2], frames.device, keep_all=True)
                plan.ingest_u8(frames.contiguous(), mean, std, bgr, stream)
                plan.run_backbone(stream)
                for v in self._int8_values():
                    hists[v] = abs_histogram(plan.bufs[v], hists.get(v))
            if shape is None:
                raise ValueError("calibrate_int8: no calibration batches")
            hists = {v: h.cpu().numpy() for v, h in hists.items()}
        finally:
            self.precision = prev
            self._plans = {k: p for k, p in self._plans.items() if not k[-1]}   # drop the keep_all plan
        self._int8_hists = hists
        return self.rescale_int8(method, percentile)

    def int8_histograms(self):
        """{value: int64 numpy [32768]} |x| histograms of the last histogram calibration
        (drnmi.calibrate.bin_values() gives the bins' magnitudes), or None if there was none."""
        return self._int8_hists

    def rescale_int8(self, method: str, percentile: float = 99.99):
        """Re-derive the activation scales from the stored histograms with another method, without
        running frames again."""
        from .calibrate import scale_from_histogram
        if self._int8_hists is None:
            raise RuntimeError("rescale_int8 needs the histograms of calibrate_int8(batches, method=...)")
        scales = {v: scale_from_histogram(h, method, percentile) for v, h in self._int8_hists.items()}
        return self._install_act_scales(scales, method, float(percentile) if method == "percentile" else None)

    def int8_state(self) -> dict:
        """The calibrated activation scales as plain data (JSON-safe: a Python float's repr
        round-trips exactly), to store next to the weights; see load_int8_state."""
        if self._act_scales is None:
            raise RuntimeError("no int8 activation scales: call calibrate_int8 or load_int8_state first")
        return {"version": 1, "method": self._int8_method, "percentile": self._int8_percentile,
                "scales": {v: float(s) for v, s in self._act_scales.items()}}

    def load_int8_state(self, state: dict) -> "DRNSeg":
        """Install activation scales saved by int8_state(): no calibration frames needed."""
        if not isinstance(state, dict) or state.get("version") != 1 or not isinstance(state.get("scales"), dict):
            raise ValueError("not an int8 state of version 1")
        scales, want = state["scales"], set(self._int8_values())
        if set(scales) != want:
            raise ValueError(f"int8 state does not match this model's activations: missing "
                             f"{sorted(want - set(scales))}, unknown {sorted(set(scales) - want)}")
        for v, s in scales.items():
            if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or not s > 0:
                raise ValueError(f"int8 state: scale of {v!r} is {s!r}, not a finite positive number")
        self._int8_hists = None
        self._install_act_scales({v: float(scales[v]) for v in self._int8_values()}, state.get("method"),
                                 state.get("percentile"))
        return self

    def set_qat(self, mode: str | None) -> "DRNSeg":
        """Quantisation-aware fine-tuning: with "int8" the train-mode forward (precision "fp32" or
        "fp32x") reads the int8 engine's grids wherever precision "int8" would launch W8A8 for this
        model: those convs (qat_layers()[0]) see their weights on the per-output-channel int8 grid and,
        as input and residual, the activations (qat_layers()[1]) on their calibrated per-tensor grid;
        the backward is straight-through.  The scales are the installed ones
        (calibrate_int8 / rescale_int8 / load_int8_state), read at every forward and fixed during a
        step; without them this call raises the engine's "no calibrated activation scale"
        RuntimeError.  Eval-mode paths are untouched: after the fine-tune, re-calibrate and
        set_precision("int8").  None switches it off (the default): the step is then launch for launch
        what it was.  The DRN-D family only, like precision "int8"."""
        if mode not in ("int8", None):
            raise ValueError("set_qat takes 'int8' or None")
        if mode is not None:
            if self.arch != "D":
                raise NotImplementedError(f"quantisation-aware fine-tuning covers the DRN-D family only, as precision "
                                          f"'int8' does; {self.model_name} fine-tunes in 'fp32' or 'fp32x'")
            self._qat_scales()
        self._qat = mode
        return self

    def qat_layers(self):
        """(names of the convs that fine-tune on int8-grid weights and inputs, the graph values that
        are fake-quantised for them): precision "int8"'s W8A8 launches and what they read.  A
        property of the architecture; needs neither a device nor scales."""
        from .engine import channel_strides, int8_layout
        elig, _, need = int8_layout(self._graph, channel_strides(self._graph))
        return [self._graph.nodes[i].name for i in sorted(elig)], sorted(need, key=lambda v: (len(v), v))

    def _qat_scales(self) -> dict:
        """{value: calibrated scale} of the fake-quantised values (the engine's error without them)."""
        _, need = self.qat_layers()
        scales = self._act_scales or {}
        missing = sorted(v for v in need if v not in scales)
        if missing:
            raise RuntimeError(f"int8: no calibrated activation scale for {missing} (DRNSeg.calibrate_int8)")
        return {v: float(scales[v]) for v in need}

    def set_block_sparse(self, enabled: bool) -> "DRNSeg":
        """bf16: let pruned (all-zero) 16 x 32 weight units skip their MFMAs (opt-in; results are
        bit-identical either way; layers with < SPARSE_MIN_ZERO_UNITS zero units stay dense).
        Takes effect at the next pack."""
        self.block_sparse = bool(enabled)
        for pk in self._packed.values():
            pk.block_sparse = self.block_sparse
        self._pack_key = None
        return self

    def set_sparse24(self, enabled: bool) -> "DRNSeg":
        """bf16 inference: run every conv whose weights are 2:4 sparse along the input channels (at most
        two non-zeros in every four consecutive channels of a tap: NMPruner) and that has the sparse
        kernel's shape (cin >= 64, ks 1 / 3, no folded downsample) on the structured-sparse MFMA
        (include/drnmi.h DRNMI_BF16_SP24).  Layers with a violating group stay dense.
        int8 inference: the int8 launches with cin >= 128 whose int8 weights are 2:4 (a masked fp32 zero
        quantises to 0) run on the sparse int8 MFMA (DRNMI_I8_SP24) where that measured faster than the
        dense int8 tile (engine.SP24_I8_SHAPES; engine.SP24_I8_EVERY routes every eligible layer).
        int32 sums are exact, so every sparse int8 launch is bit-identical to the dense one it
        replaces: the switch changes no output of an int8 model, only launch names, weight bytes
        (0.625 x) and time.  fp8, fp32 and fp32x are untouched.
        Opt-in, off by default; takes effect at the next pack."""
        self.sparse24 = bool(enabled)
        for pk in self._packed.values():
            pk.sparse24 = self.sparse24
        self._pack_key = None
        return self

    def sparse24_layers(self, device=None) -> list:
        """Names of the conv nodes the current precision's pack launches on the 2:4 sparse kernel
        (packs first if needed; [] with the switch off or outside bf16 / int8)."""
        if not self.sparse24 or self.precision not in ("bf16", "int8"):
            return []
        device = torch.device(device or next(self.parameters()).device)
        return self._packed_net(device).sparse24_layers()

    def plan(self, n, h, w, device=None, keep_all=False) -> Plan:
        device = device or next(self.parameters()).device
        plan, _ = self._prepare(n, h, w, torch.device(device), keep_all=keep_all)
        return plan

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self._key_tensors = None
        fixed = {}
        for k, v in state_dict.items():
            if k.startswith("module."):
                k = k[len("module."):]
            if k.startswith("base."):
                k = "layer." + k[len("base."):]
            fixed[k] = v
        return super().load_state_dict(fixed, strict=strict, assign=assign)

    # ----------------------------------------------------------------- internals
    def _up_plane(self, device):
        return self.up.weight[0, 0].detach().to(device, torch.float32).contiguous()

    def _apply(self, fn, *args, **kwargs):
        self._key_tensors = None          # .to() / .cuda() / .float() may swap tensors
        return super()._apply(fn, *args, **kwargs)

    def _state_key(self):
        """Repack key: every parameter/buffer's storage and version counter (an in-place update
        -- optimizer step, apply_masks, load_state_dict -- bumps the version).  The tensor list
        is cached (building it cost ~0.6 ms per call); _apply / load_state_dict reset it, and a
        Parameter or buffer swapped in anywhere in the tree (conv.weight = nn.Parameter(...))
        changes the object ids checked here, which rebuilds it."""
        ts = self._key_tensors
        ids = tuple(id(v) for d in self._key_dicts for v in d.values()) if ts is not None else None
        if ts is None or ids != self._key_ids:
            ts = self._key_tensors = list(self.parameters()) + list(self.buffers())
            self._key_dicts = [d for mod in self.modules() for d in (mod._parameters, mod._buffers, mod._modules)]
            self._key_ids = tuple(id(v) for d in self._key_dicts for v in d.values())
        return (self.precision, tuple((t.data_ptr(), t._version) for t in ts))

    def _prepare(self, n, h, w, device, keep_all=False):
        pk = self._packed_net(device)
        pkey = (self.precision, n, h, w, keep_all)
        plan = self._plans.get(pkey)
        if plan is None:
            plan = Plan(pk, n, h, w, keep_all=keep_all)
            self._plans[pkey] = plan
        return plan, _lib.stream_ptr(device)

    def _packed_net(self, device) -> PackedNet:
        """The current precision's PackedNet, (re)packed if the weights or a packing switch changed."""
        if device.type != "cuda":
            raise RuntimeError("drnmi.DRNSeg runs on the HIP engine only: move the model and input "
                               "to a ROCm device (no CPU fallback by design)")
        if self.training:
            raise RuntimeError("predict()/segment() are inference paths: call .eval() first "
                               "(train-mode forward is DRNSeg.forward)")
        _lib.load()
        key = self._state_key()
        if key != self._pack_key:
            if self.precision in self._packed:
                self._packed[self.precision].pack()
                for pkey, plan in list(self._plans.items()):
                    if pkey[0] == self.precision:
                        try:
                            plan.refresh_weight_ptrs()
                        except RuntimeError:      # the repack changed the plan's launch structure
                            del self._plans[pkey]
            self._pack_key = key
        if self.precision in ("int8", "fp8") and self._act_scales is None:
            raise RuntimeError(f"precision '{self.precision}' needs activation scales: call calibrate_int8(frames) or "
                               "load_int8_state(saved) first")
        pk = self._packed.get(self.precision)
        if pk is None:
            pk = PackedNet(self._graph, self.precision, device, block_sparse=self.block_sparse,
                           act_scales=self._act_scales, sparse24=getattr(self, "sparse24", False))
            self._packed[self.precision] = pk
        return pk


def load_info(path: str):
    with open(path) as f:
        info = json.load(f)
    return tuple(info["mean"]), tuple(info["std"])


def build(model_name: str = "drn_d_22", classes: int = 19, seed: int | None = 0, device="cuda",
          precision: str = "fp32") -> DRNSeg:
    """DRNSeg with hash-initialised weights (drnmi.weights), in eval mode, on `device`."""
    from .weights import synth_state_dict
    m = DRNSeg(model_name, classes, pretrained=False)
    if seed is not None:
        m.load_state_dict(synth_state_dict(m, seed))
    return m.to(device).eval().set_precision(precision)


__all__ = ["DRNSeg", "fill_up_weights", "build", "INFO_MEAN", "INFO_STD", "load_info",
           "os"]
