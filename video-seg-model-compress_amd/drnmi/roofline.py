"""Algorithmic work and the per-layer roofline of a DRN-D plan.

Per conv node l:  F_l = 2 * M * Cout * (Cin * k * k)       (M = output pixels)
                  B_l = in + weights + out (+ residual)    (activations/weights at the
                        plan's element size; the stem reads the uint8 frame; the seg
                        logits are fp32 and the head writes uint8 labels)
t_l = max(F_l / P_mfma, B_l / BW_hbm),  T* = sum_l t_l,  network fraction = T* / T_measured.
Peaks from /opt/skills/guides/MI355X_MICROARCH.md: HBM 8.0 TB/s, dense bf16 MFMA 2.5 PFLOP/s,
f32-input MFMA 157.3 TFLOP/s.
"""
from __future__ import annotations

HBM_PEAK_BPS = 8.0e12
# int8: dense i8 MFMA = 2x bf16 (fp8 launches, nd.i8 too, run e4m3 on the K-128 f8f6f4 MFMA at the same
# peak and one byte per element); fp32x: fp32-accurate split-bf16 arithmetic, 6 bf16 MFMAs per fp32
# product (csrc/conv_x6.hip) = 2.5 PF / 6
MFMA_PEAK = {"bf16": 2.5e15, "fp32": 157.3e12, "int8": 5.0e15, "fp32x": 2.5e15 / 6}


def kernel_peak(kernel_name: str, base: str) -> float:
    """MFMA peak of the arithmetic a kernel (named as rocprofv3 names it) runs."""
    if kernel_name.startswith("conv_sp24_i8"):    # 2:4 sparse int8: dense-equivalent OPs against the 2x sparse peak
        return 2 * MFMA_PEAK["int8"]
    # conv_i8_*, conv_w1_i8_*, conv_w1h_i8_*; conv_f8_*: e4m3 on the K-128 f8f6f4 MFMA runs at the same 8-bit peak
    if kernel_name.startswith(("conv_i8", "conv_f8")) or "_i8_" in kernel_name:
        return MFMA_PEAK["int8"]
    if kernel_name.startswith("conv_x6"):
        return MFMA_PEAK["fp32x"]
    if kernel_name.startswith("conv_sp24"):       # 2:4 sparse bf16: dense-equivalent FLOPs against AMD's 2x sparse peak
        return 2 * MFMA_PEAK["bf16"]
    return MFMA_PEAK["fp32" if base == "fp32x" else base]


def node_work(plan):
    """[(name, flops, bytes)] for every conv node, plus the head (up+argmax)."""
    pk = plan.packed
    base = 2 if pk.base == "bf16" else 4        # fp32 / fp32x: fp32 activations
    out = []
    for nd in pk.graph.nodes:
        esz = 1 if nd.i8 else base          # int8 launches: int8 activations and weights
        c = nd.conv
        ih, iw = plan.shapes[nd.src]
        oh, ow = plan.shapes[nd.dst]
        m = plan.n * oh * ow
        cin, cout, k = c.in_channels, c.out_channels, c.kernel_size[0]
        flops = 2.0 * m * cout * cin * k * k
        if nd.src == "input":
            in_b = plan.n * ih * iw * 3 * 1          # uint8 frame
        else:
            in_b = plan.n * ih * iw * cin * esz
        w_b = cout * cin * k * k * esz
        out_b = m * cout * (4 if nd.out_fp32_nchw else esz)
        res_b = m * cout * esz if nd.res else 0
        out.append((nd.name, flops, float(in_b + w_b + out_b + res_b)))
    lh, lw = plan.shapes["logits"]
    c = pk.graph.channels["logits"]
    H, W = plan.out_hw
    head_b = plan.n * c * lh * lw * 4 + plan.n * H * W * 1
    head_f = plan.n * H * W * c * 8.0             # 4 MAC per class per output pixel
    out.append(("head", head_f, float(head_b)))
    return out


def node_peaks(plan):
    """MFMA peak per row of node_work (int8 launches at the i8 rate)."""
    pk = plan.packed
    base = MFMA_PEAK["fp32" if pk.base == "fp32x" else pk.base]
    return [MFMA_PEAK["int8"] if nd.i8 else MFMA_PEAK["fp32x"] if nd.x6 else base
            for nd in pk.graph.nodes] + [base]


def launch_work(plan, video: bool = True):
    """node_work re-cut along the launches the plan really issues (Plan.launches; rows stay
    index-aligned with plan.args, a launch fills its `row`, an absorbed node's row becomes
    (name, 0, 0)).  video=True: the uint8-frame segment() path with its fused front or stem + layer1
    and the labels-only seg forms; False: frames ingested as NCHW, full logits.
    A launch's FLOPs are the sum over its nodes, its bytes that sum minus the passes the fusion
    removes: a value written and read only inside the launch (the front's and the stem's 16-channel
    intermediates, a block's, the residual a folded 1x1 downsample would have written,
    lmodels/drn.py:181-186) costs neither its write nor its reads, and a value several nodes of the
    launch read (a fused block's input: conv1 and the residual) is read once."""
    per_node = node_work(plan)
    nodes, channels = plan.packed.graph.nodes, plan.packed.graph.channels
    # (the plan's element size: every fused launch runs bf16, or fp32 nodes, never int8 ones)
    esz = 2 if plan.packed.base == "bf16" else 4
    rows = [(name, 0.0, 0.0) for name, _, _ in per_node]
    rows[-1] = per_node[-1]
    labels_only = video and plan.labels_path() != "nchw"
    for l in plan.launches("u8" if video and plan.stem_u8 is not None else "nchw", labels_only):
        flops = sum(per_node[k][1] for k in l.nodes)
        nbytes = sum(per_node[k][2] for k in l.nodes)
        if l.kind == "conv_seg":
            # not the rule above: the classifier in the last conv's epilogue (drnmi_conv_stag_seg) trades
            # the fp32 logits for two partial-logit planes, which it writes and the head reads instead
            # (so the head's row moves too), and the conv's output it keeps back is int8 in int8 nets
            j, i = l.nodes
            oh, ow = plan.shapes[nodes[j].dst]
            act = plan.n * oh * ow * nodes[j].conv.out_channels * (1 if nodes[j].i8 else esz)
            lh, lw = plan.shapes[nodes[i].dst]
            logits = plan.n * lh * lw * nodes[i].conv.out_channels * 4
            part = 2 * plan.n * lh * lw * plan.SEG_NHWC_CS * 4
            nbytes += part - 2 * act - logits
            rows[-1] = (rows[-1][0], rows[-1][1], rows[-1][2] - logits + part)
        else:
            reads = [v for k in l.nodes for v in (nodes[k].src, nodes[k].res) if v]
            inside = {nodes[k].dst for k in l.nodes} - set(l.writes)
            for v in set(reads):
                h, w = plan.shapes[v]
                passes = reads.count(v) + 1 if v in inside else reads.count(v) - 1
                nbytes -= passes * plan.n * h * w * channels[v] * esz
        rows[l.row] = (rows[l.row][0], flops, nbytes)
    return rows


def _t_star(rows, peaks):
    return sum(max(f / pk_, b / HBM_PEAK_BPS) for (_, f, b), pk_ in zip(rows, peaks))


def network_roofline(plan, video: bool = True):
    """T* two ways: per layer (every conv charged its unfused bytes) and the fused floor (the
    launches the plan issues, charged the bytes they move: launch_work).  The fused floor is the
    smaller, honest bound; bench.py reports frac against it."""
    rows = node_work(plan)
    peaks = node_peaks(plan)
    fused = launch_work(plan, video)
    return {
        "flops": sum(f for _, f, _ in rows),
        "bytes": sum(b for _, _, b in rows),
        "fused_bytes": sum(b for _, _, b in fused),
        "t_star_s": _t_star(rows, peaks),
        "t_star_fused_s": _t_star(fused, peaks),
        "t_mfma_s": sum(f / pk_ for (_, f, _), pk_ in zip(rows, peaks)),
        "t_hbm_s": sum(b for _, _, b in rows) / HBM_PEAK_BPS,
    }
