"""The comparison rule of the per-launch device-against-simulator tests (a plain module, not a conftest): a pure function over host tensors, so the
rule itself is tested without a GPU (test_opcheck_cpu.py plants faults and asserts the verdicts).  plan_check.ops_device_vs_sim and
test_gpu_convlayers._ops_against_simulator do the transport and call compare_op for the arithmetic.

A workspace / IO buffer is one region, measured as max|device - simulator| / max|simulator| over the buffer.  The gradient and the state arena are one
region each for change detection only: inside them every tensor of plan.params / plan.state is measured ON ITS OWN, relative to its own largest
element - the largest gradient of a model (a first- or last-layer conv weight) is 1e3 .. 1e5 times the recurrent block's, and a bar relative to it
would pass a weight_hh gradient of all zeros.

  * a tensor the simulator changed in this op: max|d - s| / max|s_tensor| against the arena's bar (1e-3; 4e-3 for a bf16 recurrence op);
  * a tensor the simulator left alone, and the bytes between tensors: every byte the device changed is a stray byte;
  * the arithmetic of a weight gradient happens one step earlier: every WGRAD launch writes the partial sums of its GEMM into a slice of ONE
    workspace buffer, `gradpart`, which SPLITSUM folds and UNPACK gathers into the arena (a copy, or a short sum for a bias).  Relative to the largest
    element of that buffer the launch of a weight_hh gradient is as invisible as its tensor was in the arena, so `gradpart` is split by launch: the
    elements the simulator's op changed are measured against their own largest element, at the same bar, and a byte the device changes elsewhere
    in the buffer is stray (rows `gradpart+<first element of the slice>`);
  * per_element (saturating gate biases): a buffer or tensor whose OWN largest element exceeds 1 is measured per element, floor 1.

A tensor's denominator is widened in two named cases, to a tensor of the same layer (never to the arena's largest element):
  * a conv bias in front of a norm (analytically zero gradient: rounding noise of the sums that make the same conv's weight gradient, the rule of
    plan_check.check_dccrn_plan_vs_oracle and test_gpu_plan_configs.noise_bias): the larger of its own and that weight gradient's largest element;
  * a PReLU slope, `.2.weight` (ONE scalar summed over a whole layer, free to cancel to near zero; simutil.check_syncbn_result): the larger of its own
    value and the same layer's norm-weight gradient's largest element.
`num_batches_tracked` (a count) compares exactly."""
from collections import namedtuple

import numpy as np
import torch

GRAD, STATE = 2, 3                              # sefd_amd.plan ARENA_GRAD, ARENA_STATE
BF16 = 1                                        # buffer dtype code of Plan.buffer
OP_RUNGEMM, OP_LSTM_FWD, OP_LSTM_BWD = 1, 9, 10  # sefd_desc.h OpKind
PARTIALS = "gradpart"                           # plan_builder.h finish_unpack: the partial sums of EVERY weight-gradient GEMM of the plan, one slice per launch

# regions: [(arena, byte offset, bytes, dtype code, name)]; tensors: {arena: [(name, float offset, numel)]} for the arenas split per tensor
Table = namedtuple("Table", "regions tensors")
# worst: largest err / tol of the op; where: "<name> err .. tol .."; elems: elements compared; stray: stray bytes;
# rows: [(name, max|simulator|, err, tol)] of everything compared (arena tensors as "A_GRAD:<name>")
Verdict = namedtuple("Verdict", "worst where elems stray rows")


def arena_regions(grad_bytes, state_bytes):
    """The gradient and the state arena as single fp32 regions (change detection and transport; compare_op splits them per tensor)."""
    return [(GRAD, 0, grad_bytes, 0, "A_GRAD"), (STATE, 0, state_bytes, 0, "A_STATE")]


def region_table(plan):
    """The plan's named buffers, then the gradient and the state arena as single regions with their tensor tables."""
    regions = [plan.buffer(n) + (n,) for n in plan.buffer_names()] + arena_regions(plan.arena_bytes[GRAD], plan.arena_bytes[STATE])
    numel = lambda shape: int(np.prod(shape)) if len(shape) else 1
    tensors = {GRAD: [(n, off, numel(s)) for n, (off, s) in plan.params.items()], STATE: [(n, off, numel(s)) for n, (off, s) in plan.state.items()]}
    return Table(regions, tensors)


def tolerance(dt, name, kind, dtype):
    """fp32 1e-3, bf16 buffers 1.6e-2 = two bf16 ulps of the largest element (simulator and kernel round slightly different fp32 accumulations of
    the SAME bf16 operands)."""
    tol = 1.6e-2 if dt == BF16 else 1e-3
    if dt != BF16 and dtype == "bf16" and kind == OP_RUNGEMM and name.endswith(".bnpart"):
        tol = 4e-3     # fp32 partial sums of the bf16 gradient tile this launch ALSO stores: where kernel and simulator round an
                       # element of that tile to different bf16 neighbours (allowed above: 2 ulps), a 128-row sum with cancellation
                       # moves by up to that ulp (seen 1.06e-3 of the region's largest sum)
    if dt != BF16 and dtype == "bf16" and kind in (OP_LSTM_FWD, OP_LSTM_BWD):
        tol = 4e-3     # fp32 state of a bf16 recurrence (cell state, dh): h_t is rounded to bf16 every frame, and a
                       # rounding flip (one bf16 ulp = 4e-3 of h) between kernel and simulator feeds back into c
    return tol


def _typed(u8, dt):
    return u8.view(torch.bfloat16 if dt == BF16 else torch.float32)


def measure(hv, gv, per_element, widen=0.0):
    """(err, max|hv|) of device values gv against simulator values hv (float64): max|hv - gv| / max(max|hv|, widen), or per element with floor 1
    where per_element and max|hv| > 1.  A NaN or Inf on either side that the other does not share is an infinite error."""
    own = float(hv.abs().max())
    diff = (hv - gv).abs()
    if per_element and own > 1.0:
        err = float((diff / hv.abs().clamp(min=1.0)).max())
    else:
        den = max(own, widen)
        err = float(diff.max()) / (den if den > 0 else 1.0)
    return (err if np.isfinite(err) else float("inf")), own


def arena_max_error(hv, gv):
    """The rule before the per-tensor split, kept for the record: the whole arena relative to its largest element."""
    return measure(hv.double(), gv.double(), False)[0]


def _widen(name, hv_all, index):
    """The two named exceptions: largest simulator element of the sibling tensor(s) that may stand in the denominator of `name` (0: none)."""
    sib = []
    if name.endswith("conv.bias") and ".0." in name:
        layer = name.rsplit(".0.", 1)[0] + "."
        if any(k.startswith(layer + "1.") for k in index):                       # a norm follows the conv
            sib = [name[:-len("bias")] + "weight"]
    elif name.endswith(".2.weight"):
        layer = name[:-len("2.weight")]
        sib = [layer + "1." + k for k in ("weight", "Wrr", "Wri", "Wii")]        # BatchNorm / ComplexBatchNorm weights
    out = 0.0
    for k in sib:
        if k in index:
            off, n = index[k]
            out = max(out, float(hv_all[off:off + n].abs().max()))
    return out


def _split_arena(label, p8, h8, g8, tensors, tol, per_element):
    """One changed fp32 arena, tensor by tensor.  Returns (rows, stray bytes)."""
    n32 = p8.numel() // 4
    pi, hi, gi = (t[:n32 * 4].view(torch.int32) for t in (p8, h8, g8))
    hf, gf = h8[:n32 * 4].view(torch.float32), g8[:n32 * 4].view(torch.float32)
    sim_ne = hi != pi
    untouched = torch.ones(n32, dtype=torch.bool)
    index = {name: (off, n) for name, off, n in tensors}
    rows = []
    for name, off, n in tensors:
        if not bool(sim_ne[off:off + n].any()):
            continue
        untouched[off:off + n] = False
        hv, gv = hf[off:off + n].double(), gf[off:off + n].double()
        if name.endswith("num_batches_tracked"):
            err, own = (0.0 if torch.equal(hi[off:off + n], gi[off:off + n]) else float("inf")), float(hv.abs().max())
        else:
            err, own = measure(hv, gv, per_element, _widen(name, hf, index))
        rows.append((f"{label}:{name}", own, err, tol, n))
    dev_ne = (gi != pi) & untouched                                              # untouched tensors and the bytes between tensors
    stray = int((g8[:n32 * 4].view(-1, 4)[dev_ne] != p8[:n32 * 4].view(-1, 4)[dev_ne]).sum()) if bool(dev_ne.any()) else 0
    stray += int((g8[n32 * 4:] != p8[n32 * 4:]).sum())
    return rows, stray


def _split_partials(label, p8, h8, g8, tol, per_element):
    """The weight-gradient partial sums, launch by launch: the elements the simulator's op changed against THEIR largest element; a byte the device
    changes anywhere else in the buffer is stray.  Returns (rows, stray bytes)."""
    n32 = p8.numel() // 4
    pi, hi, gi = (t[:n32 * 4].view(torch.int32) for t in (p8, h8, g8))
    ne = hi != pi
    hv = h8[:n32 * 4].view(torch.float32)[ne].double()
    gv = g8[:n32 * 4].view(torch.float32)[ne].double()
    err, own = measure(hv, gv, per_element)
    dev_ne = (gi != pi) & ~ne
    stray = int((g8[:n32 * 4].view(-1, 4)[dev_ne] != p8[:n32 * 4].view(-1, 4)[dev_ne]).sum()) if bool(dev_ne.any()) else 0
    return [(f"{label}+{int(torch.argmax(ne.to(torch.uint8)))}", own, err, tol, hv.numel())], stray


def compare_op(before, sim, dev, table, kind, dtype, per_element=False, candidates=None):
    """The verdict on ONE op.  before / sim / dev: {arena: host tensor} (or lists indexed by arena) - the arenas in front of the op, after the op on
    the simulator and after the op on the device; table: region_table(plan); kind: the op's OpKind; dtype: the plan's activation dtype, "fp32" or
    "bf16"; candidates: indices into table.regions that may have changed (a driver that has detected changes on its own; None: every region)."""
    worst, where, elems, stray, rows = 0.0, "", 0, 0, []
    for idx in (range(len(table.regions)) if candidates is None else candidates):
        a, off, nb, dt, name = table.regions[idx]
        if nb <= 0:
            continue
        p8, h8, g8 = (x[a].view(torch.uint8)[off:off + nb] for x in (before, sim, dev))
        if torch.equal(h8, p8):
            # stray write: the device changed bytes of a region the simulator did not touch
            stray += int((g8 != p8).sum())
            continue
        tol = tolerance(dt, name, kind, dtype)
        if a in table.tensors and dt != BF16:
            new, s = _split_arena(name, p8, h8, g8, table.tensors[a], tol, per_element)
            stray += s
        elif name == PARTIALS and dt != BF16:
            new, s = _split_partials(name, p8, h8, g8, tol, per_element)
            stray += s
        else:
            hv, gv = _typed(h8, dt).double(), _typed(g8, dt).double()
            err, own = measure(hv, gv, per_element)
            new = [(name, own, err, tol, hv.numel())]
        for rname, own, err, rtol, n in new:
            elems += n
            rows.append((rname, own, err, rtol))
            if err / rtol > worst:
                worst, where = err / rtol, f"{rname} err {err:.2e} tol {rtol:.0e}"
    return Verdict(worst, where, elems, stray, rows)


class TensorLog:
    """Per-tensor figures over a run: the table that ends every report file."""

    def __init__(self):
        self.rows = {}

    def add(self, verdict):
        for name, own, err, tol in verdict.rows:
            m, e, t = self.rows.get(name, (0.0, 0.0, tol))
            self.rows[name] = (max(m, own), max(e, err), max(t, tol))

    def worst(self):
        """(err / tol, name) of the worst tensor or buffer of the run."""
        return max(((e / t, n) for n, (m, e, t) in self.rows.items()), default=(0.0, ""))

    def lines(self):
        out = ["", f"{'tensor':64s} {'max|s|':>10s} {'worst err':>10s} {'tol':>8s}"]
        out += [f"{n:64s} {m:10.3e} {e:10.3e} {t:8.0e}" for n, (m, e, t) in self.rows.items()]
        w, n = self.worst()
        return out + [f"worst err/tol {w:.3e} {n}"]
