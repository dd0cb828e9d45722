"""The persistent form of the 128-row LDS-DMA GEMM (csrc/rungemm_persist.hip; knobs RG_PERSIST / RG_PERSIST_GRID, read per launch).

* every launch of two small DCCRN plans against the host simulator with every launch of the kernel's form on the persistent kernel, at grid 1 (ONE
  workgroup walks every tile of a launch: the ring positions carry over tile after tile), grid 3 (uneven split) and the resident grid;
* forward + backward of the same plans with the kernel off and on: every byte the phases write must be equal - the accumulation order, the
  rounding and the order of the statistics sums are those of rungemm_kernel, so "close" is not the bar;
* which launches took the kernel is asserted through Plan.op_info()["family"]: at least one N = 128 and one N = 64 launch per case, and among the
  launches taken one with at most two K tiles (the first ring stage of the next tile is then the whole or half of its K loop).

The cases are rows of test_gpu_ops.py: B = 3, L = 4000, kernel_num (16, 32, 32, 64, 64, 64): M is no multiple of 128 anywhere (tail tiles, tiles
across batch items), N = 32 / 64 / 128 and N = 256 as two 128-wide column tiles, a 2-K-tile launch at N = 32; B = 1, L = 2400, kernel_num
(32, 64, 128, 256, 256, 256): N = 64 with two K tiles (K = 80), phase-interleaved decoder outputs and the two-destination input gradients (n2)."""
import ctypes as C
import struct

import pytest
import torch

from util import knobs

CASES = [("DCCRN", 3, 4000, "R", (16, 32, 32, 64, 64, 64), 128, "bf16"),
         ("DCCRN", 1, 2400, "C", (32, 64, 128, 256, 256, 256), 256, "bf16")]
GRIDS = [1, 3, 0]
KIND_RUNGEMM = 1
_RUNGEMM_OFF, _NSEG_OFF, _SEG_OFF, _SEG_SIZE = 16, 108, 112, 20      # csrc/sefd_desc.h: Op header, RunGemm::nseg, RunGemm::seg, sizeof(Seg)


def _make_plan(case):
    from simutil import Plan
    model, B, L, mode, kn, ru, dtype = case
    return Plan(B, L, masking_mode=mode, kernel_num=kn, rnn_units=ru, act_dtype=dtype, model=model)


def _k_tiles(plan, phase, i, K):
    """64-deep K tiles of RUNGEMM op i: every run starts a tile of its own."""
    raw = C.string_at(plan.ops_ptr(phase) + i * plan.lib.sefd_op_size(), plan.lib.sefd_op_size())[_RUNGEMM_OFF:]
    nseg = struct.unpack_from("<i", raw, _NSEG_OFF)[0]
    lens = [struct.unpack_from("<5i", raw, _SEG_OFF + _SEG_SIZE * s)[3] for s in range(nseg)]
    assert 0 < nseg <= 8 and sum(lens) == K, "RunGemm layout moved: fix the offsets above"
    return sum((n + 63) // 64 for n in lens)


def _persistent_ops(plan):
    """[(phase, op, N, K tiles)] of the RUNGEMM ops that a launch would put on the persistent kernel under the knobs of the moment."""
    from sefd_amd.plan import RUN_FAMILY_PERSIST
    out = []
    for phase in (0, 1):
        for i in range(plan.num_ops(phase)):
            o = plan.op_info(phase, i)
            if o["kind"] == KIND_RUNGEMM and o["family"] == RUN_FAMILY_PERSIST:
                out.append((phase, i, o["N"], _k_tiles(plan, phase, i, o["K"])))
    return out


def _assert_coverage(plan):
    ops = _persistent_ops(plan)
    assert any(n == 128 for _, _, n, _ in ops), ops
    assert any(n == 64 for _, _, n, _ in ops), ops
    assert any(kt <= 2 for _, _, _, kt in ops), ops
    return ops


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_chosen_cases_cover_the_kernel(case):
    """No GPU: the planner and the selection rule alone.  Off: no launch is taken; default rule: these small launches do not fill the grid twice."""
    plan = _make_plan(case)
    knobs.set("RG_PERSIST", "0")
    assert _persistent_ops(plan) == []
    knobs.unset("RG_PERSIST")
    assert _persistent_ops(plan) == []
    knobs.set("RG_PERSIST", "2")
    for grid in GRIDS:
        knobs.set("RG_PERSIST_GRID", str(grid))
        taken = {(p, k) for p, k, _, _ in _assert_coverage(plan)}
        for phase in (0, 1):                           # fp32, accumulating, register-staged and unaligned-output launches stay where they were
            for i in range(plan.num_ops(phase)):
                o = plan.op_info(phase, i)
                if o["kind"] == KIND_RUNGEMM and (o["dtype"] != 1 or (o["flags"] & 2) or not (o["flags"] & 8) or not (o["flags"] & 1)):
                    assert (phase, i) not in taken, (phase, i, o)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_every_op_against_host_simulator_persistent(case, grid):
    from test_gpu_ops import every_op_against_host_simulator
    knobs.set("RG_PERSIST", "2")
    knobs.set("RG_PERSIST_GRID", str(grid))
    _assert_coverage(_make_plan(case))
    every_op_against_host_simulator(*case, report_prefix=f"ops_report_persist_g{grid}")


_reference = {}


def _run_both_phases(case, plan):
    """Arenas after forward + backward of `plan` from the formula weights and the test signals, under the knobs of the moment."""
    from oracle.dccrn import DCCRNConfig, dccrn_state_shapes
    from oracle.weights import formula_state_dict, test_signals as make_signals
    from simutil import PHASE_BWD, PHASE_FWD, fill_params
    model, B, L, mode, kn, ru, dtype = case
    dev = plan.alloc_arenas("cuda")
    fill_params(plan, dev, formula_state_dict(dccrn_state_shapes(DCCRNConfig(masking_mode=mode, kernel_num=kn, rnn_units=ru))))
    x, _ = make_signals(B, L)
    g = torch.Generator().manual_seed(1)
    plan.io(dev, "wav", (B, L)).copy_(x)
    plan.io(dev, "grad_wav", (B, L)).copy_(torch.randn(B, L, generator=g) * 1e-3)
    plan.io(dev, "grad_real", (B, plan.NF, plan.T)).copy_(torch.randn(B, plan.NF, plan.T, generator=g) * 1e-4)
    plan.io(dev, "grad_imag", (B, plan.NF, plan.T)).copy_(torch.randn(B, plan.NF, plan.T, generator=g) * 1e-4)
    for phase in (PHASE_FWD, PHASE_BWD):
        plan.run(phase, dev, 0)
    torch.cuda.synchronize()
    assert plan.lib.sefd_plan_status(plan.h, 0) == 0
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_bit_identical_to_the_tiled_kernel(case, grid):
    plan = _make_plan(case)
    if case not in _reference:                         # the tiled kernel's result: computed once per case, never changed
        knobs.set("RG_PERSIST", "0")
        assert _persistent_ops(plan) == []
        _reference[case] = _run_both_phases(case, plan)
    ref = _reference[case]
    knobs.set("RG_PERSIST", "2")
    knobs.set("RG_PERSIST_GRID", str(grid))
    _assert_coverage(plan)
    got = _run_both_phases(case, plan)
    # every buffer of the plan by name (activations, statistics partial rows, input gradients, weight-gradient partials, packed weights), then
    # the flat gradient and state arenas and the I/O block as wholes
    diff = []
    for name in plan.buffer_names():
        a, off, nb, _ = plan.buffer(name)
        if nb > 0 and not torch.equal(ref[a].view(torch.uint8)[off:off + nb], got[a].view(torch.uint8)[off:off + nb]):
            diff.append(name)
    for a, name in ((2, "A_GRAD"), (3, "A_STATE"), (5, "A_IO"), (0, "A_WS")):
        if not torch.equal(ref[a].view(torch.uint8), got[a].view(torch.uint8)):
            diff.append(name)
    assert not diff, "buffers that differ: " + " ".join(diff)
