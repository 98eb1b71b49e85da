"""Quantisation-aware fine-tuning on the GPU (csrc/qat.hip, drnmi.train with DRNSeg.set_qat).

The three kernels are compared bit for bit with tests/qat_ref.py: their arithmetic has one defined
fp32 rounding per step.  The wiring is checked on the recorded launches of one D-22 fp32x step with
hand-set scales (which conv reads fq(v), which reads v; the packs of the shadow weights), and the
step's loss and parameter gradients against the float64 restatement of the specified network
(qat_ref.net_step), under the bounds tests/test_gpu_train.py applies to D-22: gradients 1e-3
relative L2 (train_case.rel_l2), loss 1e-4 relative."""
import ctypes

import numpy as np
import pytest
import torch

import qat_ref as R
import train_case as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
# the activation kernels stream with at most 2048 workgroups of 256 lanes, 8 elements per lane
WRAP = 2048 * 256 * 8


def _lib():
    from drnmi import _lib as L
    return L, L.load()


def _sp():
    L, _ = _lib()
    return ctypes.c_void_p(L.stream_ptr(torch.device(DEV)))


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _inputs(n, s, seed):
    """n values: +-0, exact half-way points (k + 0.5) s for even and odd k, the clip's neighbourhood,
    far outliers, denormals, then random values; cycled when n is smaller than the list."""
    rng = np.random.default_rng(seed)
    s32 = F32(s)
    k = np.arange(-130, 131, dtype=F32)
    head = np.concatenate([
        np.array([0.0, -0.0], dtype=F32), (k + F32(0.5)) * s32,
        np.array([127, -127, 127.5, -127.5, 128, -128, 1e6, -1e6], dtype=F32) * s32,
        np.array([1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38], dtype=F32)]).astype(F32)
    x = (rng.standard_normal(n) * 50).astype(F32) * s32
    if n >= head.size:
        x[:head.size] = head
    else:
        x[:] = head[rng.permutation(head.size)[:n]]
        x[:min(n, 8)] = np.array([0.0, -0.0, 0.5, 1.5, 2.5, 127.5, -128, 1e6], dtype=F32)[:min(n, 8)] * s32
    return x


@pytest.mark.parametrize("s", [0.25, 0.0371])
@pytest.mark.parametrize("n", [8, 24, 4104, WRAP + 4104])
def test_fake_quant_forward_and_backward_bitwise(n, s):
    L, lib = _lib()
    x = _inputs(n, s, seed=n % 1000)
    s32, inv = R.scale_pair(s)
    xd = torch.from_numpy(x).to(DEV)
    yd = torch.full_like(xd, float("nan"))
    L.check(lib.drnmi_fake_quant_f32(_vp(xd), n, float(s32), float(inv), _vp(yd), _sp()), "fake_quant")
    want = R.fq(x, s)
    assert np.array_equal(_bits(yd.cpu().numpy()), _bits(want))
    rng = np.random.default_rng(n % 1000 + 1)
    dq = rng.standard_normal(n).astype(F32)
    dx0 = rng.standard_normal(n).astype(F32)
    m = R.mask(x, s)
    assert n < 64 or (not m.all() and m.any())
    dqd = torch.from_numpy(dq).to(DEV)
    for acc in (0, 1):
        dxd = torch.from_numpy(dx0).to(DEV) if acc else torch.full_like(xd, float("nan"))
        L.check(lib.drnmi_fake_quant_bwd_f32(_vp(dqd), _vp(xd), n, float(inv), _vp(dxd), acc, _sp()), "fake_quant_bwd")
        ref = R.fq_bwd(dq, x, s, dx0 if acc else None)
        assert np.array_equal(_bits(dxd.cpu().numpy()), _bits(ref)), acc
    assert torch.equal(xd.cpu(), torch.from_numpy(x)) and torch.equal(dqd.cpu(), torch.from_numpy(dq))


ROW_SHAPES = [(16, 27), (19, 512), (128, 1152), (5, 4608), (3, 1)]


def _rows(rows, cols, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((rows, cols)) * rng.uniform(0.01, 3.0, (rows, 1))).astype(F32)
    w[0] = 0                                   # an all-zero row
    w[1] = 0
    w[1, cols // 2] = 0.7                      # one non-zero
    j = int(np.abs(w[2]).argmax())
    w[2, j] = -abs(w[2, j]) * 1.5 - 0.1        # the absmax is a negative weight
    return w


def test_fake_quant_rows_bitwise_and_batched():
    L, lib = _lib()
    ws = [_rows(r, c, 10 + i) for i, (r, c) in enumerate(ROW_SHAPES)]
    wd = [torch.from_numpy(w).to(DEV) for w in ws]
    single = []
    for w, d in zip(ws, wd):
        q = torch.full_like(d, float("nan"))
        sc = torch.full((w.shape[0],), float("nan"), device=DEV)
        L.check(lib.drnmi_fake_quant_rows_f32(_vp(d), w.shape[0], w.shape[1], _vp(q), _vp(sc), _sp()), "fq rows")
        wq, s = R.fq_rows(w)
        assert np.array_equal(_bits(q.cpu().numpy()), _bits(wq)), w.shape
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(s)), w.shape
        assert s[0] == 1 and not wq[0].any() and np.count_nonzero(wq[1]) == 1 and wq[2].min() == -127 * s[2]
        single.append((q, sc))
    qs = [torch.full_like(d, float("nan")) for d in wd]
    scs = [torch.full((w.shape[0],), float("nan"), device=DEV) for w in ws]
    rows, total = [], 0
    for w, d, q, sc in zip(ws, wd, qs, scs):
        rows.append([d.data_ptr(), q.data_ptr(), sc.data_ptr(), w.shape[0], w.shape[1], total])
        total += w.shape[0]
    tab = torch.tensor(rows, dtype=torch.int64)
    tot = ctypes.c_int64(0)
    L.check(lib.drnmi_fake_quant_rows_table_check(_vp(tab), len(rows), ctypes.byref(tot)), "table")
    assert tot.value == total
    tabd = tab.to(DEV)
    L.check(lib.drnmi_fake_quant_rows_batched_f32(_vp(tabd), len(rows), total, _sp()), "fq rows batched")
    for (q1, s1), q, sc in zip(single, qs, scs):
        assert torch.equal(q1.view(torch.int32), q.view(torch.int32))
        assert torch.equal(s1.view(torch.int32), sc.view(torch.int32))


# ------------------------------------------------------------------------------ one recorded step
ARCH, SHAPE, SEED = "drn_d_22", (2, 3, 64, 64), 5
# hand-set activation scales (clip = 127 s): the values reach 5.2 .. 6.9 on this input, so 0.055 clips
# nothing, 0.0625 is a power of two, and the last four clip the tail of their value
SCALES = {"v12": 0.0625, "v13": 0.02, "v15": 0.03125, "v20": 0.025, "v24": 0.02}
DEFAULT_SCALE = 0.055
CLIPPED = ("v13", "v15", "v20", "v24")


def _case():
    from drnmi.drnseg import DRNSeg
    from drnmi.weights import synth_state_dict
    torch.manual_seed(SEED)
    m = DRNSeg(ARCH, 19, pretrained=False)
    m.load_state_dict(synth_state_dict(m, SEED))
    x = torch.randn(*SHAPE)
    t = torch.randint(0, 19, (SHAPE[0], SHAPE[2], SHAPE[3]))
    t[torch.rand(t.shape) < 0.2] = 255
    return m, x, t


def _state(m, scales=None):
    sc = {v: (scales or SCALES).get(v, DEFAULT_SCALE) for v in m._int8_values()}
    return {"version": 1, "method": None, "percentile": None, "scales": sc}


def _step(m, x, t, record=None):
    """One forward / backward of m (on the GPU, train mode) from zeroed gradients; returns the loss."""
    from drnmi.train import CrossEntropyLoss, TrainRunner
    if getattr(m, "_train_runner", None) is None:
        m._train_runner = TrainRunner(m)
    m._train_runner.record = record
    for p in m.parameters():
        p.grad = None
    loss = CrossEntropyLoss(ignore_index=255)(m(x.to(DEV))[0], t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    m._train_runner.record = None
    return float(loss.detach())


def _grads(m):
    return {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None}


class _Step:
    pass


_CACHE = {}


def _recorded():
    """The QAT-off step and then the QAT-on step of one model on the same input, each recorded once."""
    if "s" in _CACHE:
        return _CACHE["s"]
    m, x, t = _case()
    m = m.to(DEV).train().set_precision("fp32x")
    out = _Step()
    out.m, out.x, out.t = m, x, t
    recs = []
    keep = lambda kind, name, d: recs.append((kind, name, {k: (v.detach().cpu() if torch.is_tensor(v) else v)
                                                           for k, v in d.items()}))
    out.loss_off = _step(m, x, t, keep)
    out.recs_off, out.grads_off = list(recs), _grads(m)
    recs.clear()
    m.load_int8_state(_state(m)).set_qat("int8")
    out.loss = _step(m, x, t, keep)
    out.recs, out.grads = list(recs), _grads(m)
    out.packed = [(st.wf.detach().cpu(), None if st.wd is None else st.wd.detach().cpu())
                  for st in m._train_runner.state]
    _CACHE["s"] = out
    return out


def _nhwc(t2d, n, c):
    hw = t2d.shape[0] // n
    h = int(round(hw ** 0.5))
    return t2d.reshape(n, h, hw // h, c)


def test_qat_off_records_none_of_the_new_kinds():
    s = _recorded()
    kinds = {k for k, _, _ in s.recs_off}
    assert not kinds & {"fq", "fq_bwd", "fq_rows"} and "conv" in kinds
    assert {"fq", "fq_bwd", "fq_rows"} <= {k for k, _, _ in s.recs}


def test_wiring_of_the_recorded_step():
    L, lib = _lib()
    s = _recorded()
    m = s.m
    e_names, q_vals = m.qat_layers()
    nodes = {nd.name: (i, nd) for i, nd in enumerate(m._graph.nodes)}
    fq = {name: d for k, name, d in s.recs if k == "fq"}
    fq_rows = {name: d for k, name, d in s.recs if k == "fq_rows"}
    fq_bwd = {name: d for k, name, d in s.recs if k == "fq_bwd"}
    convs = {name: d for k, name, d in s.recs if k == "conv"}
    bn_act = {name: d for k, name, d in s.recs if k == "bn_act"}
    wgrad = {name: d for k, name, d in s.recs if k == "wgrad"}
    assert sorted(fq) == sorted(q_vals) == sorted(fq_bwd) and sorted(fq_rows) == sorted(e_names)
    assert len([1 for k, _, _ in s.recs if k == "fq"]) == len(q_vals)          # once per value per step
    z_of = {nodes[name][1].dst: d["z"] for name, d in bn_act.items()}
    scales = _state(m)["scales"]
    for v, d in fq.items():
        s32, inv = R.scale_pair(scales[v])
        assert F32(d["scale"]) == s32 and F32(d["inv_scale"]) == inv
        assert torch.equal(d["x"], z_of[v])
        y = d["y"].numpy()
        assert np.array_equal(_bits(y), _bits(R.fq(d["x"].numpy(), scales[v])))
        # on the grid: an integer level in [-127, 127] whose fp32 product with s is the value (the
        # quotient y / s itself is the level only up to that product's rounding, hence the rint)
        lvl = np.rint(y.astype(np.float64) / np.float64(s32))
        assert np.abs(lvl).max() <= 127 and np.array_equal((lvl.astype(F32) * s32).astype(F32), y)
    for name, (i, nd) in nodes.items():
        x_rec = convs[name]["x"]
        if name in e_names:
            assert torch.equal(x_rec, fq[nd.src]["y"]), name
            assert torch.equal(wgrad[name]["x"], fq[nd.src]["y"]), name
            if nd.res:
                assert torch.equal(bn_act[name]["res"], fq[nd.res]["y"]), name
        else:
            src = z_of[nd.src] if nd.src != "input" else None
            assert src is None or torch.equal(x_rec, src), name
            assert nd.src not in fq or not torch.equal(x_rec, fq[nd.src]["y"]), name
            if nd.res:
                assert torch.equal(bn_act[name]["res"], z_of[nd.res]), name
    # the shadow weights are the row quantiser's, and the packs the step used are packs of them
    runner = m._train_runner
    for name in e_names:
        i, nd = nodes[name]
        d, st = fq_rows[name], runner.state[i]
        w = d["w"].numpy()
        wq, sc = R.fq_rows(w.reshape(w.shape[0], -1))
        assert np.array_equal(_bits(d["wq"].numpy().reshape(w.shape[0], -1)), _bits(wq)), name
        assert np.array_equal(_bits(d["scale"].numpy()), _bits(sc)), name
        assert torch.equal(d["w"], nd.conv.weight.detach().cpu())
        cout, cin, ks, _ = w.shape
        shadow = d["wq"].to(DEV).contiguous()
        wf = torch.empty_like(st.wf)
        L.check(lib.drnmi_pack_conv_weight(_vp(shadow), cout, cin, ks, runner.cstride[nd.src], st.cout_pad, st.k_pad, 0,
                                           None, L.DRNMI_F32, _vp(wf), _sp()), "pack")
        assert torch.equal(wf.cpu(), s.packed[i][0]), name
        assert not torch.equal(wf.cpu(), torch.zeros_like(s.packed[i][0]))
        wd = torch.empty_like(st.wd)
        L.check(lib.drnmi_pack_conv_weight(_vp(shadow), cout, cin, ks, st.dys, st.rows_d, st.kd_pad, 1, None,
                                           L.DRNMI_F32, _vp(wd), _sp()), "pack dgrad")
        assert torch.equal(wd.cpu(), s.packed[i][1]), name
    # the straight-through fold: checked bit for bit on its own recorded inputs, and some scales clip
    for v, d in fq_bwd.items():
        before = None if d["before"] is None else d["before"].numpy()
        ref = R.fq_bwd(d["dq"].numpy(), d["x"].numpy(), scales[v], before)
        assert np.array_equal(_bits(d["after"].numpy()), _bits(ref)), v
        assert torch.equal(d["x"], z_of[v])
    for v in CLIPPED:
        mk = R.mask(fq[v]["x"].numpy(), scales[v])
        assert not mk.all() and mk.mean() > 0.5, (v, mk.mean())
    assert R.mask(fq["v11"]["x"].numpy(), scales["v11"]).all()


def test_gradients_match_the_float64_restatement():
    s = _recorded()
    m = s.m
    e_names, q_vals = m.qat_layers()
    elig = {i for i, nd in enumerate(m._graph.nodes) if nd.name in e_names}
    scales = {v: sc for v, sc in _state(m)["scales"].items() if v in q_vals}
    n = SHAPE[0]
    levels = {}
    for k, v, d in s.recs:
        if k == "fq":
            y = d["y"].double()
            lv = torch.round(y / float(F32(scales[v])))
            levels[v] = _nhwc(lv, n, y.shape[1]).permute(0, 3, 1, 2).contiguous()
    cpu = m.__class__(ARCH, 19, pretrained=False)
    cpu.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    loss, grads, _, diffs = R.net_step(cpu, s.x, s.t, elig, scales, levels)
    total = sum(lv.numel() for lv in levels.values())
    print(f"levels the restatement's own rounding would have chosen differently: {sum(diffs.values())} of {total} "
          f"({ {v: c for v, c in diffs.items() if c} })")
    print(f"loss GPU {s.loss:.8f} float64 {loss:.8f} (QAT off: {s.loss_off:.8f})")
    assert abs(s.loss - loss) <= 1e-4 * abs(loss)
    worst = ("", 0.0)
    assert set(grads) == {k for k in s.grads if not k.startswith("up.")}
    for k, g in grads.items():
        e = TC.rel_l2(s.grads[k].numpy(), g.numpy())
        worst = max(worst, (k, e), key=lambda a: a[1])
    print(f"worst parameter gradient vs float64: {worst[1]:.2e} at {worst[0]}")
    for k, g in grads.items():
        e = TC.rel_l2(s.grads[k].numpy(), g.numpy())
        assert e <= 1e-3, (k, e)


def test_qat_changes_the_gradients_and_follows_new_scales():
    s = _recorded()
    m = s.m
    e_names, _ = m.qat_layers()
    changed = [n for n in e_names if not torch.equal(s.grads[n + ".weight"], s.grads_off[n + ".weight"])]
    assert changed, "QAT left every weight gradient of the int8 convs as it was"
    assert s.loss != s.loss_off
    # new scales take effect at the next forward
    fq0 = {name: d["y"] for k, name, d in s.recs if k == "fq"}
    from drnmi.weights import synth_frames
    frames = torch.from_numpy(synth_frames(7, 2, 128, 256)).to(DEV)
    old = dict(m._act_scales)
    m.eval()
    m.calibrate_int8(frames)
    m.train()
    assert m._act_scales != old and m._qat == "int8"
    recs = []
    _step(m, s.x, s.t, lambda kind, name, d: recs.append((name, d["y"].cpu(), d["scale"])) if kind == "fq" else None)
    assert len(recs) == len(fq0)
    for name, y, sc in recs:
        assert sc == m._act_scales[name]
        assert sc == old[name] or not torch.equal(y, fq0[name]), name
    assert any(not torch.equal(y, fq0[name]) for name, y, _ in recs)
    _CACHE.clear()                     # the cached model now carries other scales
