"""The labels-only NHWC head for 1 .. 256 classes (csrc/head_wide.hip up8_labels_wide_tile_kernel,
drnmi_up8_labels_nhwc_wide) against the route it replaces: drnmi_up8_logsoftmax_argmax without
log-probs on the NCHW form of the same values.  n = 2, logits 128 x 256 (two 1024 x 2048 frames), at
c = 150 and c = 32, on two inputs:
  * network: the bf16 seg logits of build("drn_d_22", c, seed=0) for the bench's synthetic frames
    (synth_frames(7, ..)) -- the workload;
  * random: randn * 3 -- the worst case, margins are tiny and almost every window is slow.
Per input: the share of fast windows / candidate pixels / fallback pixels (the counting entry), the
two kernels' times and whether the labels are equal.  Then DRNSeg.segment() end to end at 150
classes, 8 x 1024 x 2048, bf16, with engine.LABELS_NHWC off, on, and off again (the difference
between the two "off" columns is the run-to-run spread the gain has to exceed).
Each figure is the median of REPS single launches timed with device events after WARM warm-up
launches, the compared launches alternating one by one; the device clocks as rocm-smi reports them
are printed before and after.
python scripts/wide_labels_micro.py"""
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-seg-model-compress_amd"))
import torch  # noqa: E402

from drnmi import _lib, drnseg, engine  # noqa: E402
from drnmi.weights import bilinear_up_kernel, synth_frames  # noqa: E402

WARM, REPS = 5, 31
N, H, W = 2, 128, 256
DEV = torch.device("cuda")
lib = _lib.load()
st = ctypes.c_void_p(_lib.stream_ptr())
up = torch.from_numpy(bilinear_up_kernel(16)).float().to(DEV)


def clocks(tag):
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        keep = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        print(f"clocks {tag}: " + ("; ".join(keep) if keep else "not reported"), flush=True)
    except Exception as e:  # noqa: BLE001
        print(f"clocks {tag}: not available ({type(e).__name__})", flush=True)


def timed(fns):
    """Median us per launch of each callable, launches alternating between them."""
    for _ in range(WARM):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return f"{t[0]:9.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def network_rows(c):
    """[N][H][W][cs] fp32 rows as the bf16 seg conv of a c-class D-22 writes them."""
    m = drnseg.build("drn_d_22", c, seed=0, device=DEV, precision="bf16")
    frames = torch.from_numpy(synth_frames(7, N, 8 * H, 8 * W)).to(DEV)
    m.segment(frames)
    plan = m.plan(N, 8 * H, 8 * W)
    assert plan.labels_path() == "nhwc", plan.labels_path()
    return plan.bufs["logits_nhwc"].view(N, H, W, plan.seg_cs).clone()


def random_rows(c):
    g = torch.Generator(device="cuda").manual_seed(c)
    rows = torch.randn(N, H, W, (c + 3) // 4 * 4, device=DEV, generator=g) * 3
    return rows


def compare(tag, c, rows):
    cs = rows.shape[-1]
    nchw = rows[..., :c].permute(0, 3, 1, 2).contiguous()
    lab = torch.empty(N, 8 * H, 8 * W, dtype=torch.uint8, device=DEV)
    lab2 = torch.empty_like(lab)
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    _lib.check(lib.drnmi_up8_labels_nhwc_wide_stats(rows.data_ptr(), cs, up.data_ptr(), lab.data_ptr(), _lib.DRNMI_U8,
                                                    N, c, H, W, st, counts.data_ptr()), "stats")
    fast, cand, full = (int(v) for v in counts.cpu())
    px = lab.numel()
    t_new, t_old = timed([
        lambda: _lib.check(lib.drnmi_up8_labels_nhwc_wide(rows.data_ptr(), cs, up.data_ptr(), lab.data_ptr(),
                                                          _lib.DRNMI_U8, N, c, H, W, st), "wide nhwc"),
        lambda: _lib.check(lib.drnmi_up8_logsoftmax_argmax(nchw.data_ptr(), up.data_ptr(), None, lab2.data_ptr(),
                                                           _lib.DRNMI_U8, N, c, H, W, st), "nchw")])
    print(f"{tag} c={c}: fast windows {fast} ({64 * fast / px:.3f} of the pixels), candidate pixels {cand} "
          f"({cand / px:.3f}), fallback pixels {full} ({full / px:.3f})", flush=True)
    print(f"{tag} c={c}: nhwc wide {fmt(t_new)} | nchw labels-only {fmt(t_old)} | ratio {t_old[0] / t_new[0]:.2f}x | "
          f"labels equal {torch.equal(lab, lab2)}, {len(lab.unique())} classes", flush=True)


clocks("before")
for c in (150, 32):
    compare("network", c, network_rows(c))
    compare("random ", c, random_rows(c))

m = drnseg.build("drn_d_22", 150, seed=0, device=DEV, precision="bf16")
frames = torch.from_numpy(synth_frames(7, 8, 1024, 2048)).to(DEV)
out = torch.empty(8, 1024, 2048, dtype=torch.uint8, device=DEV)


def segment(nhwc):
    def run():
        engine.LABELS_NHWC = nhwc
        m.segment(frames, labels=out)
    return run


segment(False)()
ref = out.clone()
segment(True)()
same = torch.equal(out, ref)
t_off, t_on, t_off2 = timed([segment(False), segment(True), segment(False)])
engine.LABELS_NHWC = True
print(f"segment() 150 classes 8 x 1024 x 2048 bf16: LABELS_NHWC off {fmt(t_off)} | on {fmt(t_on)} | off again "
      f"{fmt(t_off2)} | labels equal {same}", flush=True)
print(f"gain {t_off[0] - t_on[0]:.1f} us ({(t_off[0] - t_on[0]) / t_off[0] * 100:.2f} %), spread between the two off "
      f"columns {abs(t_off[0] - t_off2[0]):.1f} us", flush=True)
clocks("after")
