"""Evaluation drivers on the GPU: the callers of the hot path in semantic_seg.py (SURVEY.md §8a
rows a18/a19, §8f row 4), same names and arguments.

  test(eval_data_loader, model, num_classes, has_gt=True,
       output_dir='pred', save_vis=False)                          semantic_seg.py:429-468
  val_miou(val_loader, model, num_classes, args=None, has_gt=True) semantic_seg.py:638-671
  test_ms(eval_data_loader, model, num_classes, scales, has_gt=True,
          output_dir='pred', save_vis=False)                       semantic_seg.py:507-557
  resize_4d_tensor(tensor, width, height)                         semantic_seg.py:471-504
  validate(val_loader, model, criterion, epoch, writer, args,
           eval_score=None, print_freq=10)                         semantic_seg.py:234-283

Everything per image stays on the device: the forward (DRNSeg, HIP engine), the Pillow-exact
bilinear resize of every log-prob plane and the fp32 scale sum (drnmi_resize_bilinear_f32,
accumulate), the argmax (drnmi_argmax_nchw_f32) and the confusion matrix (drnmi_confusion_matrix).
Without save_vis only the 19 x 19 histogram ever comes back to the host.  With save_vis=True every
image's label map goes to output_dir/<name[:-4]>.png (mode L) and its palette image to
output_dir + '_color'/<name[:-4]>.png (save_output_images / save_colorful_images,
semantic_seg.py:400-426): the colouring runs on the GPU (drnmi_render_labels) and only the finished
uint8 images come to the host, where Pillow writes them.
Deviations: output_dir and save_vis are keyword arguments (the reference has output_dir before
has_gt positionally); the palette image is RGB for every palette -- the reference's TRIPLET_PALETTE
(num_classes == 3) is RGBA with alpha 255 everywhere, and its 4th column is dropped
(drnmi.palette); test_ms picks the palette by num_classes as test does (the reference's test_ms
always takes CITYSCAPE_PALETTE); and the loader's tensors are moved to the model's device.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import metrics, ops
from .palette import palette_for


def resize_4d_tensor(tensor: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """[N, C, h, w] fp32 -> [N, C, height, width] with Pillow's Image.resize(BILINEAR) 'F'-mode
    arithmetic per plane (the reference runs it per channel in threads on the CPU).  Returns the
    tensor itself when the size already matches, as the reference does."""
    if tensor.size(2) == height and tensor.size(3) == width:
        return tensor
    return ops.resize_bilinear_f32(tensor.float().contiguous(), (height, width))


def _device_of(model):
    return next(model.parameters()).device


def _miou_of(hist: torch.Tensor) -> float:
    ious = metrics.per_class_iu(hist) * 100
    return round(float(np.nanmean(ious)), 2)


def _unwrap(model):
    """The DRNSeg inside a DataParallel / DDP wrapper (semantic_seg.py:812 and :1074 hand the
    wrapped model to val_miou; the multigpu script hands a DDP one)."""
    while hasattr(model, "module") and not hasattr(model, "predict"):
        model = model.module
    return model


def _save_png(array: np.ndarray, output_dir: str, filename: str) -> None:
    from PIL import Image
    fn = os.path.join(output_dir, filename[:-4] + '.png')
    out_dir = os.path.split(fn)[0]
    if not os.path.exists(out_dir):
        os.makedirs(out_dir)
    Image.fromarray(array).save(fn)


def _save_vis(pred: torch.Tensor, names, output_dir: str, num_classes: int) -> None:
    """pred [B, H, W] labels on the GPU -> the label PNG and the palette PNG of every image."""
    if isinstance(names, str):
        names = [names]
    lab8 = pred.to(torch.uint8)                  # what the label PNG holds (the reference's astype(np.uint8))
    color = ops.render_labels(lab8 if num_classes <= 256 else pred, palette_for(num_classes)).cpu().numpy()
    lab = lab8.cpu().numpy()
    for ind in range(len(names)):
        _save_png(lab[ind], output_dir, names[ind])
        _save_png(color[ind], output_dir + '_color', names[ind])


def test(eval_data_loader, model, num_classes, has_gt=True, *, output_dir='pred', save_vis=False):
    """Single-scale eval loop: model(image)[0] -> torch.max(final, 1) -> fast_hist (on the GPU)."""
    model.eval()
    model = _unwrap(model)
    dev = _device_of(model)
    hist = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=dev)
    for it, batch in enumerate(eval_data_loader):
        image = batch[0].to(dev)
        pred = model.predict(image)                  # fused forward + argmax (int64 labels)
        if save_vis:
            _save_vis(pred, batch[2], output_dir, num_classes)
        if has_gt:
            metrics.fast_hist(pred, batch[1].to(dev).long().reshape(pred.shape), num_classes, hist)
    if has_gt:
        return _miou_of(hist)
    return None


def val_miou(val_loader, model, num_classes, args=None, has_gt=True):
    """semantic_seg.py:638-671 -- the same loop over (image, label) batches."""
    return test(val_loader, model, num_classes, has_gt=has_gt)


def test_ms(eval_data_loader, model, num_classes, scales, has_gt=True, *, output_dir='pred', save_vis=False):
    """Multi-scale eval: the log-probs of the image and of its len(scales) rescaled copies (the
    loader's SegListMS items: image, label, name, *scaled images) are each resized to the input
    size and summed in fp32 in the reference's order, then argmax(axis=1) and fast_hist."""
    model.eval()
    model = _unwrap(model)
    dev = _device_of(model)
    hist = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=dev)
    num_scales = len(scales)
    preds = []
    for it, input_data in enumerate(eval_data_loader):
        label = input_data[1] if has_gt else None
        h, w = input_data[0].size()[2:4]
        images = [input_data[0]]
        images.extend(input_data[-num_scales:])
        final = None
        for image in images:
            out = model(image.to(dev))[0]
            if final is None:
                final = resize_4d_tensor(out, w, h).clone()   # 0 + out_0: the sum's first term is exact
            elif out.size(2) == h and out.size(3) == w:
                final += out
            else:                                             # final += resize(out), fp32, in order
                ops.resize_bilinear_f32(out, (h, w), out=final, accumulate=True)
        pred = ops.argmax_nchw(final)
        preds.append(pred)
        if save_vis:
            _save_vis(pred, input_data[2] if has_gt else input_data[1], output_dir, num_classes)
        if has_gt:
            metrics.fast_hist(pred, label.to(dev).long().reshape(pred.shape), num_classes, hist)
    if has_gt:
        return _miou_of(hist)
    return preds


def validate(val_loader, model, criterion, epoch=0, writer=None, args=None, eval_score=None, print_freq=10):
    """semantic_seg.py:234-283 -- the per-epoch validation of the fine-tune loop: eval-mode
    model(input)[0], criterion(output, target.long().squeeze(1)), eval_score(output, target), each
    averaged with the weight input.size(0) as the reference's AverageMeter does (sum += val * n,
    avg = sum / count).  Returns score.avg (0 when eval_score is None) and sends the loss mean to
    writer.add_scalar('Loss/Eval', ., epoch) when a writer is given.

    The sums stay on the device: the loss in fp64 (the reference's meter adds the Python floats
    of loss.item()), the score in fp32 (its meter adds the fp32 score tensors).  The host reads
    them only to print, every print_freq batches, and at the end; the reference's loss.item()
    synchronises every batch.  Deviations: epoch / writer / args are optional; the bare
    print(loss_val) after every batch is dropped; the returned score is a Python float (the
    reference returns the 0-dim tensor)."""
    import time
    model.eval()
    dev = _device_of(_unwrap(model))
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    score_sum = torch.zeros((), dtype=torch.float32, device=dev)
    count = 0
    loss_val = 0.0
    n_batches = len(val_loader) if hasattr(val_loader, "__len__") else -1
    end = time.time()
    with torch.no_grad():
        for i, (input, target) in enumerate(val_loader):
            if type(criterion) in (torch.nn.L1Loss, torch.nn.MSELoss):
                target = target.float()
            input = input.to(dev)
            target = target.to(dev, non_blocking=True)
            target_var = target.long()
            if target_var.dim() == 4:                       # the reference's squeeze(1) of [n, 1, h, w]
                target_var = target_var.squeeze(1)
            output = model(input)[0]
            loss = criterion(output, target_var)
            bs = input.size(0)
            loss_sum += loss.detach().double() * bs
            count += bs
            s = None
            if eval_score is not None:
                s = eval_score(output, target_var)
                score_sum += torch.as_tensor(s, dtype=torch.float32, device=dev) * bs
            if i % print_freq == 0:
                now = time.time()
                print('Test: [{0}/{1}]\tTime {2:.3f}\tLoss {3:.4f} ({4:.4f})\tScore {5:.3f} ({6:.3f})'.format(
                    i, n_batches, now - end, float(loss), float(loss_sum) / count,
                    float(s) if s is not None else 0.0, float(score_sum) / count))
                end = now
    if count:
        loss_val = float(loss_sum) / count
    score_avg = float(score_sum / count) if (eval_score is not None and count) else 0
    print(' * Loss {} : {}'.format(loss_val, epoch))
    if writer is not None:
        writer.add_scalar('Loss/Eval', loss_val, epoch)
    print(' * Score {:.3f}'.format(score_avg))
    return score_avg


__all__ = ["resize_4d_tensor", "test", "val_miou", "test_ms", "validate"]
