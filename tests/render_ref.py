"""numpy reference of the renderer's contract (include/drnmi.h drnmi_render_labels): the palette
lookup with the clamp, the top-left crop, the channel swap and the integer blend."""
import numpy as np


def alpha_q8(alpha: float) -> int:
    return int(round(float(alpha) * 256))


def blend(frame, colour, a_q8: int):
    """Per channel (f * (256 - a) + c * a + 128) >> 8 on uint8 arrays, a in 0..256."""
    f = np.asarray(frame).astype(np.int64)
    c = np.asarray(colour).astype(np.int64)
    return ((f * (256 - a_q8) + c * a_q8 + 128) >> 8).astype(np.uint8)


def colour(labels, palette, out_hw=None, bgr=False):
    """palette[min(label, P - 1)] of the top-left out_hw of the label maps [n, lh, lw] -> [n, oh, ow, 3]."""
    pal = np.asarray(palette)[:, :3].astype(np.uint8)
    lab = np.asarray(labels)
    oh, ow = lab.shape[1:] if out_hw is None else out_hw
    img = pal[np.minimum(lab[:, :oh, :ow].astype(np.int64), len(pal) - 1)]
    return img[..., ::-1].copy() if bgr else img


def render_ref(labels, palette, frames=None, alpha=0.6, bgr=False, out_hw=None):
    """What drnmi.ops.render_labels returns, on numpy arrays."""
    if frames is not None:
        out_hw = np.asarray(frames).shape[1:3]
    img = colour(labels, palette, out_hw, bgr)
    return img if frames is None else blend(frames, img, alpha_q8(alpha))
