"""The distillation criterion's kernels (csrc/train.hip, drnmi_distill_loss_f32 / _bwd_f32) at the
fine-tune bench's shape, 2 x 19 x 1024 x 768, and at an ADE20K-like 2 x 150 x 512 x 512 (the generic
walk), forward and backward, against
  * drnmi_ce_loss_f32 / _bwd_f32 alone: the criterion the step has without a teacher;
  * the ATen formulation a user would write on top of it: drnmi's CrossEntropyLoss plus
    F.kl_div(log_softmax(s / T), softmax(t / T), "sum") / D, forward and autograd backward.
One process, the arms interleaved: each repetition times every arm once, between a pair of HIP
events, on the next of SETS operand sets (student, teacher, gradient; together above the 256 MiB
Infinity Cache, so the reads come from HBM).  Kernel arms: ITERS launches per window.  Medians of
REPS windows after WARM warm-up repetitions; GB/s from the bytes the kernel has to move
(forward 8c + 8 per pixel, backward 12c + 8; CE alone 4c + 8 and 8c + 8).
python scripts/distill_micro.py"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-seg-model-compress_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from drnmi import _lib  # noqa: E402
from drnmi.train import CrossEntropyLoss  # noqa: E402

WARM, REPS, ITERS, SETS = 3, 20, 8, 3
T, SW, DW, IGNORE = 2.0, 0.5, 0.5, 255
DEV = torch.device("cuda")
lib = _lib.load()
st = ctypes.c_void_p(_lib.stream_ptr())


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def window(f, iters, k0):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        f(k0 + k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def fmt(ts, nbytes=None):
    m = statistics.median(ts)
    s = f"{m:9.1f} us (min {min(ts):.1f}, max {max(ts):.1f})"
    return s + (f" | {nbytes / m / 1e3:6.0f} GB/s" if nbytes else "")


def run_shape(n, c, h, w):
    hw, pix = h * w, n * h * w
    g = torch.Generator(device="cuda").manual_seed(1)
    S = [F.log_softmax(3 * torch.randn(n, c, h, w, device=DEV, generator=g), 1) for _ in range(SETS)]
    Tt = [F.log_softmax(3 * torch.randn(n, c, h, w, device=DEV, generator=g), 1) for _ in range(SETS)]
    G = [torch.empty(n, c, h, w, device=DEV) for _ in range(SETS)]
    tg = torch.randint(0, c, (n, h, w), device=DEV, generator=g)
    tg[torch.rand(n, h, w, device=DEV, generator=g) < 0.1] = IGNORE
    out3, count, one = torch.empty(3, device=DEV), torch.empty((), device=DEV), torch.ones((), device=DEV)
    ws = torch.empty(lib.drnmi_distill_workspace_bytes(), dtype=torch.uint8, device=DEV)

    def kd_fwd(k):
        _lib.check(lib.drnmi_distill_loss_f32(vp(S[k % SETS]), vp(Tt[k % SETS]), vp(tg), n, c, hw, IGNORE, SW, DW, T, 0,
                                              vp(out3), vp(count), vp(ws), st), "distill")

    def kd_bwd(k):
        _lib.check(lib.drnmi_distill_loss_bwd_f32(vp(S[k % SETS]), vp(Tt[k % SETS]), vp(tg), n, c, hw, IGNORE, SW, DW, T,
                                                  0, vp(one), vp(count), vp(G[k % SETS]), st), "distill bwd")

    def ce_fwd(k):
        _lib.check(lib.drnmi_ce_loss_f32(vp(S[k % SETS]), vp(tg), n, c, hw, IGNORE, vp(out3), vp(count), vp(ws), st), "ce")

    def ce_bwd(k):
        _lib.check(lib.drnmi_ce_loss_bwd_f32(vp(S[k % SETS]), vp(tg), n, c, hw, IGNORE, vp(one), vp(count),
                                             vp(G[k % SETS]), st), "ce bwd")

    crit = CrossEntropyLoss(ignore_index=IGNORE)
    leaves = [s.clone().requires_grad_(True) for s in S]
    state = {}

    def aten_fwd(k):
        s = leaves[k % SETS]
        s.grad = None
        kd = F.kl_div(F.log_softmax(s / T, 1), F.softmax(Tt[k % SETS] / T, 1), reduction="sum") / pix
        state["loss"] = SW * crit(s, tg) + DW * kd

    def aten_bwd(k):
        state["loss"].backward()

    arms = [("distill fwd", kd_fwd, ITERS, pix * (8 * c + 8)), ("distill bwd", kd_bwd, ITERS, pix * (12 * c + 8)),
            ("ce fwd", ce_fwd, ITERS, pix * (4 * c + 8)), ("ce bwd", ce_bwd, ITERS, pix * (8 * c + 8)),
            ("aten ce+kl_div fwd", aten_fwd, 1, None), ("aten ce+kl_div bwd", aten_bwd, 1, None)]
    times = {name: [] for name, *_ in arms}
    for rep in range(WARM + REPS):
        for name, f, iters, _ in arms:
            t = window(f, iters, rep * ITERS)
            if rep >= WARM:
                times[name].append(t)
    print(f"shape {n} x {c} x {h} x {w} fp32, T = {T}, weights ({SW}, {DW}), 10 % ignore_index", flush=True)
    for name, _, _, nbytes in arms:
        print(f"  {name:20s} {fmt(times[name], nbytes)}", flush=True)
    kd_fwd(0)
    aten_fwd(0)
    torch.cuda.synchronize()
    print(f"  loss: kernel {float(out3[0]):.6f}, aten {float(state['loss'].detach()):.6f}", flush=True)
    m = {k: statistics.median(v) for k, v in times.items()}
    print(f"  distill fwd + bwd {m['distill fwd'] + m['distill bwd']:.1f} us; ce fwd + bwd "
          f"{m['ce fwd'] + m['ce bwd']:.1f} us; aten fwd + bwd {m['aten ce+kl_div fwd'] + m['aten ce+kl_div bwd']:.1f} us "
          f"({(m['aten ce+kl_div fwd'] + m['aten ce+kl_div bwd']) / (m['distill fwd'] + m['distill bwd']):.1f}x)", flush=True)


for shape in ((2, 19, 1024, 768), (2, 150, 512, 512)):
    run_shape(*shape)
    torch.cuda.empty_cache()
