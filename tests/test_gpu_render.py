"""Rendering of label maps on the GPU (csrc/render.hip): the kernel, DRNSeg.segment(render=...),
torch.cuda.graph capture of torch.ops.drnmi.segment_render, and the save_vis images of the eval
drivers.  The arithmetic is exact integer arithmetic, so every comparison is == on every byte
against tests/render_ref.py."""
import functools

import numpy as np
import pytest
import torch

import render_ref as R
from drnmi import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.drnmi.*)
from drnmi.palette import CITYSCAPE_PALETTE, TRIPLET_PALETTE

pytestmark = pytest.mark.gpu
DEV = "cuda"
PALETTES = {20: CITYSCAPE_PALETTE, 3: TRIPLET_PALETTE}
# labels [n, lh, lw] -> out oh x ow: crop + odd width + 63-byte rows; no crop; several blocks, row
# tails, lw != ow (3 * 37 * 261 pixels = 7 full tiles of 256 threads x 16 pixels and a partial one)
SHAPES = [((2, 16, 24), (13, 21)), ((1, 8, 8), (8, 8)), ((3, 40, 264), (37, 261))]
PAD = 80            # bytes behind the output that must stay as they were


@functools.lru_cache(maxsize=None)
def _case(shape, out_hw):
    """Labels random in 0..18 plus planted 19, 200 and 255, and frames, for one shape (shared)."""
    rng = np.random.default_rng(hash((shape, out_hw)) % (1 << 32))
    lab = rng.integers(0, 19, size=shape, dtype=np.uint8)
    flat = lab.reshape(-1)
    where = rng.choice(flat.size, size=min(24, flat.size // 2), replace=False)
    flat[where] = np.resize(np.array([19, 200, 255], dtype=np.uint8), where.size)
    lab[:, out_hw[0] - 1, out_hw[1] - 1] = 255          # the last pixel of the crop, and what lies past it
    lab[:, :, out_hw[1]:] = 7
    lab[:, out_hw[0]:, :] = 9
    assert set(np.unique(lab[:, :out_hw[0], :out_hw[1]])) >= {19, 200, 255}
    frames = rng.integers(0, 256, size=(shape[0], *out_hw, 3), dtype=np.uint8)
    lab.setflags(write=False)
    frames.setflags(write=False)
    return lab, frames


def _padded_out(n, oh, ow, offset=0):
    size = n * oh * ow * 3
    buf = torch.full((offset + size + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[offset:offset + size].view(n, oh, ow, 3)


def _check(buf, out, want, offset=0):
    got = buf.cpu().numpy()
    size = want.size
    assert np.array_equal(got[offset:offset + size].reshape(want.shape), want)
    assert (got[:offset] == 0xA5).all() and (got[offset + size:] == 0xA5).all()     # nothing outside is written
    assert out.data_ptr() == buf.data_ptr() + offset


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("P", [20, 3])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("shape,out_hw", SHAPES)
def test_kernel_matches_reference(shape, out_hw, dtype, P, swap):
    lab_np, frames_np = _case(shape, out_hw)
    pal = PALETTES[P]
    lab = torch.from_numpy(lab_np.copy()).to(DEV).to(dtype)
    frames = torch.from_numpy(frames_np.copy()).to(DEV)
    n, (oh, ow) = shape[0], out_hw
    buf, out = _padded_out(n, oh, ow)
    ret = ops.render_labels(lab, pal, bgr=bool(swap), out_hw=out_hw, out=out)
    assert ret is out
    _check(buf, out, R.render_ref(lab_np, pal, bgr=bool(swap), out_hw=out_hw))
    for alpha in (0.0, 0.6, 1.0):
        buf, out = _padded_out(n, oh, ow)
        ops.render_labels(lab, pal, frames, alpha=alpha, bgr=bool(swap), out=out)
        want = R.render_ref(lab_np, pal, frames_np, alpha=alpha, bgr=bool(swap))
        _check(buf, out, want)
        if alpha == 0.0:
            assert np.array_equal(want, frames_np)
    assert torch.equal(frames.cpu(), torch.from_numpy(frames_np.copy()))          # inputs untouched


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_kernel_unaligned_buffers_take_the_byte_path(dtype):
    """Output / frame addresses that are not 16-B aligned (slices of a larger buffer)."""
    shape, out_hw = SHAPES[2]
    lab_np, frames_np = _case(shape, out_hw)
    lab = torch.from_numpy(lab_np.copy()).to(DEV).to(dtype)
    n, (oh, ow) = shape[0], out_hw
    fbuf = torch.zeros(frames_np.size + 3, dtype=torch.uint8, device=DEV)
    frames = fbuf[3:].view(frames_np.shape)
    frames.copy_(torch.from_numpy(frames_np.copy()))
    for offset in (1, 4):
        buf, out = _padded_out(n, oh, ow, offset)
        ops.render_labels(lab, None, frames, alpha=0.6, out=out)
        _check(buf, out, R.render_ref(lab_np, CITYSCAPE_PALETTE, frames_np, alpha=0.6), offset)
    lab_off = torch.zeros(lab_np.size + 1, dtype=torch.uint8, device=DEV)[1:].view(lab_np.shape)   # labels at +1 B
    lab_off.copy_(torch.from_numpy(lab_np.copy()))
    got = ops.render_labels(lab_off, None, out_hw=out_hw)
    assert np.array_equal(got.cpu().numpy(), R.render_ref(lab_np, CITYSCAPE_PALETTE, out_hw=out_hw))


def test_render_op_and_defaults():
    shape, out_hw = SHAPES[0]
    lab_np, frames_np = _case(shape, out_hw)
    lab = torch.from_numpy(lab_np.copy()).to(DEV)
    frames = torch.from_numpy(frames_np.copy()).to(DEV)
    from drnmi.palette import as_device_palette
    pal = as_device_palette(CITYSCAPE_PALETTE, DEV)
    full = torch.ops.drnmi.render_labels(lab, pal, None, 0, False, shape[1], shape[2])
    assert np.array_equal(full.cpu().numpy(), R.render_ref(lab_np, CITYSCAPE_PALETTE))
    assert torch.equal(ops.render_labels(lab), full)                              # defaults: label size, Cityscapes
    ov = torch.ops.drnmi.render_labels(lab, pal, frames, 154, True, *out_hw)
    assert np.array_equal(ov.cpu().numpy(), R.render_ref(lab_np, CITYSCAPE_PALETTE, frames_np, 0.6, bgr=True))
    assert torch.equal(ops.render_labels(lab, frames=frames, bgr=True), ov)       # defaults: frame size, alpha 0.6
    with pytest.raises(ValueError):
        ops.render_labels(lab, out_hw=(17, 24))
    with pytest.raises(ValueError):
        ops.render_labels(lab, frames=frames, alpha=1.5)
    with pytest.raises(ValueError):
        ops.render_labels(lab.float())


def test_kernel_offsets_past_2_to_31():
    """One picture whose output is larger than 2^31 bytes (64-bit offsets): the first rows, the
    rows around byte 2^31 and the last rows against the reference."""
    lh, lw, oh, ow = 26800, 26816, 26800, 26800
    assert oh * ow * 3 > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(11)
    lab = torch.randint(0, 22, (1, lh, lw), dtype=torch.uint8, device=DEV, generator=g)
    out = ops.render_labels(lab, out_hw=(oh, ow))
    mid = 2 ** 31 // (ow * 3)
    for r0, r1 in ((0, 3), (mid - 2, mid + 3), (oh - 3, oh)):
        want = R.render_ref(lab[:, r0:r1].cpu().numpy(), CITYSCAPE_PALETTE, out_hw=(r1 - r0, ow))
        assert np.array_equal(out[:, r0:r1].cpu().numpy(), want), (r0, r1)


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _model(precision):
    from drnmi.drnseg import build
    return build("drn_d_22", 19, seed=0, device=DEV, precision=precision)


@functools.lru_cache(maxsize=None)
def _frames(n, h, w):
    from drnmi.weights import synth_frames
    f = synth_frames(21, n, h, w)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("render", ["color", "overlay"])
def test_segment_render(render, precision):
    m = _model(precision)
    for n, h, w in ((2, 64, 96), (1, 60, 100)):
        f_np = _frames(n, h, w)
        frames = torch.from_numpy(f_np.copy()).to(DEV)
        plain = m.segment(frames)
        labels, image = m.segment(frames, render=render)
        assert torch.equal(labels, plain) and labels.dtype == torch.uint8
        assert image.shape == (n, h, w, 3) and image.dtype == torch.uint8
        want = R.render_ref(plain.cpu().numpy(), CITYSCAPE_PALETTE, f_np if render == "overlay" else None,
                            out_hw=(h, w))
        assert np.array_equal(image.cpu().numpy(), want)


def test_segment_render_resized_frames():
    """size=: the picture has the size of the frames the network saw, drawn over the resized frames."""
    m = _model("bf16")
    f_np = _frames(2, 90, 150)
    frames = torch.from_numpy(f_np.copy()).to(DEV)
    base = ops.resize_bilinear_u8(frames, (60, 100)).cpu().numpy()
    plain = m.segment(frames, size=(60, 100))
    labels, image = m.segment(frames, size=(60, 100), render="overlay")
    assert torch.equal(labels, plain) and tuple(labels.shape) == (2, 64, 104)
    assert tuple(image.shape) == (2, 60, 100, 3)
    assert np.array_equal(image.cpu().numpy(), R.render_ref(plain.cpu().numpy(), CITYSCAPE_PALETTE, base))
    _, frame_only = m.segment(frames, size=(60, 100), render="overlay", alpha=0.0)
    assert np.array_equal(frame_only.cpu().numpy(), base)          # the overlay base is resize_bilinear_u8's output


def test_segment_render_bgr_palette_and_labels_buffer():
    m = _model("bf16")
    f_np = _frames(2, 64, 96)
    frames = torch.from_numpy(f_np.copy()).to(DEV)
    plain = m.segment(frames, bgr=True)
    labels, image = m.segment(frames, bgr=True, render="overlay")
    assert torch.equal(labels, plain)
    assert np.array_equal(image.cpu().numpy(),
                          R.render_ref(plain.cpu().numpy(), CITYSCAPE_PALETTE, f_np, bgr=True))
    buf = torch.empty(2, 64, 96, dtype=torch.int64, device=DEV)
    labels, image = m.segment(frames, labels=buf, render="color", palette=TRIPLET_PALETTE)
    assert labels is buf and torch.equal(buf, m.segment(frames).long())
    assert np.array_equal(image.cpu().numpy(), R.render_ref(buf.cpu().numpy(), TRIPLET_PALETTE))


def test_segment_render_graph_capture():
    from drnmi.palette import as_device_palette
    from drnmi.weights import synth_frames
    m = _model("bf16")
    frames = torch.from_numpy(synth_frames(9, 2, 64, 96)).to(DEV)
    pal = as_device_palette(CITYSCAPE_PALETTE, DEV)
    mean, std = [0.29, 0.33, 0.29], [0.18, 0.19, 0.18]

    def step():
        return torch.ops.drnmi.segment_render(frames, m._handle, mean, std, False, pal, 154, True)

    # warm-up on a side stream first: packing, plan buffers and kernel attributes are set up
    # outside the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_labels, cap_image = step()
    for seed in (9, 10):                                            # the second replay sees new frame contents
        frames.copy_(torch.from_numpy(synth_frames(seed, 2, 64, 96)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        labels, image = step()
        assert torch.equal(cap_labels, labels) and torch.equal(cap_image, image)
        assert np.array_equal(image.cpu().numpy(),
                              R.render_ref(labels.cpu().numpy(), CITYSCAPE_PALETTE, frames.cpu().numpy()))


# ------------------------------------------------------------------ eval drivers
def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, np.array(im)


def test_eval_save_vis(tmp_path):
    from drnmi import evaluate
    m = _model("fp32")
    g = torch.Generator().manual_seed(6)
    names = ["a/x_leftImg8bit.png", "b.png"]
    images = [torch.randn(1, 3, 32, 64, generator=g) for _ in names]
    gts = [torch.randint(0, 19, (1, 32, 64), generator=g) for _ in names]
    loader = [(images[0], gts[0], [names[0]]), (images[1], gts[1], names[1])]   # collated list / plain string
    preds = [m.predict(im.to(DEV)).cpu().numpy()[0] for im in images]

    out = tmp_path / "pred"
    miou = evaluate.test(loader, m, 19, save_vis=True, output_dir=str(out))
    assert miou == evaluate.test(loader, m, 19)
    assert sorted(p.relative_to(tmp_path).as_posix() for p in tmp_path.rglob("*.png")) == sorted(
        ["pred/a/x_leftImg8bit.png", "pred/b.png", "pred_color/a/x_leftImg8bit.png", "pred_color/b.png"])
    for name, pred in zip(names, preds):
        mode, lab = _png(out / name)
        assert mode == "L" and np.array_equal(lab, pred)
        mode, col = _png(tmp_path / "pred_color" / name)
        assert mode == "RGB" and np.array_equal(col, CITYSCAPE_PALETTE[pred])

    scales = [0.5]
    ms_loader = [(im, gt, nm, torch.nn.functional.interpolate(im, size=(16, 32), mode="bilinear",
                                                              align_corners=False))
                 for im, gt, nm in loader]
    out = tmp_path / "ms"
    miou = evaluate.test_ms(ms_loader, m, 19, scales, save_vis=True, output_dir=str(out))
    assert miou == evaluate.test_ms(ms_loader, m, 19, scales)
    ms_preds = [p.cpu().numpy()[0] for p in evaluate.test_ms(ms_loader, m, 19, scales, has_gt=False)]
    for name, pred in zip(names, ms_preds):
        mode, lab = _png(out / name)
        assert mode == "L" and np.array_equal(lab, pred)
        mode, col = _png(tmp_path / "ms_color" / name)
        assert mode == "RGB" and np.array_equal(col, CITYSCAPE_PALETTE[pred])
    # without ground truth the name is the item's second entry
    nogt = [(im, nm, sc) for im, _, nm, sc in ms_loader]
    evaluate.test_ms(nogt, m, 19, scales, has_gt=False, save_vis=True, output_dir=str(tmp_path / "nogt"))
    for name, pred in zip(names, ms_preds):
        assert np.array_equal(_png(tmp_path / "nogt" / name)[1], pred)
