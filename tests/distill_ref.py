"""fp64 restatement of the distillation loss (drnmi.train.DistillationLoss, csrc/train.hip): the
yardstick of tests/test_distill.py (which ties it to torch's fp64 autograd) and
tests/test_gpu_distill.py (which holds the kernels to it).

Per pixel, with a = s / T and b = t / T on student / teacher log-probs s, t [n, c, ...]:
    logp = a - lse(a), logq = b - lse(b), q = exp(logq)
    kd_i = sum_k q[k] * (logq[k] - logp[k])                 every pixel
    ce_i = lse(s) - s[target]                               target != ignore_index
    CE = sum ce_i / count;  KD = sum kd_i / D, D = n * hw ("mean") or n ("batchmean")
    loss = student_wt * CE + distill_wt * KD                (no T^2 factor)
    g_s = student_wt / count * (softmax(s) - onehot) [labelled] + distill_wt / (D * T) * (p - q)"""
import torch


def _lse(x):
    mx = x.max(1, keepdim=True)[0]
    return mx + (x - mx).exp().sum(1, keepdim=True).log()


def distill_ref(s, t, target, student_wt=0.5, distill_wt=0.5, temperature=1.0, ignore_index=-100,
                kd_reduction="mean"):
    """(loss, ce, kd, count, g_s) as fp64 CPU tensors; g_s is d loss / d s.  An out-of-range target
    other than ignore_index gives a NaN ce / loss and counts as ignored in g_s."""
    s, t = s.detach().double().cpu(), t.detach().double().cpu()
    target = target.detach().cpu()
    n, c = s.shape[0], s.shape[1]
    s3, t3, tg = s.reshape(n, c, -1), t.reshape(n, c, -1), target.reshape(n, -1)
    hw = s3.shape[2]
    d = float(n if kd_reduction == "batchmean" else n * hw)
    a, b = s3 / temperature, t3 / temperature
    logp, logq = a - _lse(a), b - _lse(b)
    q = logq.exp()
    kd = (q * (logq - logp)).sum() / d
    bad = (tg != ignore_index) & ((tg < 0) | (tg >= c))
    live = (tg != ignore_index) & ~bad
    idx = torch.where(live, tg, torch.zeros_like(tg))
    ce_i = _lse(s3)[:, 0] - s3.gather(1, idx[:, None])[:, 0]
    count = live.sum().double()
    ce = torch.where(live, ce_i, torch.zeros_like(ce_i)).sum() / count
    if bool(bad.any()):
        ce = torch.full_like(ce, float("nan"))
    loss = student_wt * ce + distill_wt * kd
    onehot = torch.zeros_like(s3).scatter_(1, idx[:, None], 1.0)
    g = student_wt / count * ((s3 - _lse(s3)).exp() - onehot) * live[:, None]
    g = g + distill_wt / (d * temperature) * (logp.exp() - q)
    return loss, ce, kd, count, g.reshape(s.shape)


def make_case(n, c, h, w, seed, ignore_index=255, all_ignored_image=None):
    """The inputs of the tests: log_softmax(3 * randn) for student and teacher, targets with 30 %
    set to ignore_index and row 0 all ignored (and, optionally, one whole image)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.log_softmax(3 * torch.randn(n, c, h, w, generator=g), 1)
    t = torch.log_softmax(3 * torch.randn(n, c, h, w, generator=g), 1)
    tg = torch.randint(0, c, (n, h, w), generator=g)
    tg[torch.rand(n, h, w, generator=g) < 0.3] = ignore_index
    tg[:, 0, :] = ignore_index
    if all_ignored_image is not None:
        tg[all_ignored_image] = ignore_index
    return s, t, tg


# (n, c, h, w): the 16-byte four-pixel form with image 1 entirely ignored; odd hw (per-pixel form);
# the generic walk at 150 and 256 classes; two classes
SHAPES = [(2, 19, 24, 40), (1, 19, 23, 41), (1, 150, 8, 24), (1, 256, 3, 5), (2, 2, 5, 7)]
TEMPERATURES = [1.0, 2.0, 4.0]
REDUCTIONS = ["mean", "batchmean"]
WEIGHTS = [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0)]


def case_for(shape, seed=0):
    return make_case(*shape, seed=seed + sum(shape), all_ignored_image=1 if shape == (2, 19, 24, 40) else None)
