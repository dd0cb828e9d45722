"""Which weight-gradient launches take the frame-staged kernel (csrc/thin_wgrad.hip; knob THIN_WGRAD, read per launch), asserted through
Plan.op_info()["family"] without a GPU - the planner and the selection rule alone (the pattern of test_gpu_thin_stage.py::test_selection_rule).

The kernel is built as <channels per position of the run operand, N>: <32, 64> and <8, 32> (the benchmark's channel counts: the second-to-last decoder
layer and the second encoder layer; the mask layer) and <16, 32> (the same two layers at kernel_num[0] = 16).  At kernel_num[0] = 16 the mask layer's
two launches would need <8, 16> (N = 16 in a 32-row packed matrix): not built, so the form check refuses them and they stay on the 32-wide LDS-DMA tile -
the test names them."""
import pytest

from test_gpu_rungemm_persist import _make_plan
from util import knobs

CASES = [("DCCRN", 3, 4000, "R", (16, 32, 32, 64, 64, 64), 128, "bf16"),
         ("DCCRN", 1, 2400, "C", (32, 64, 128, 256, 256, 256), 256, "bf16")]
KIND_WGRAD = 2


def wgrad_ops(plan):
    return [(i, plan.op_info(1, i)) for i in range(plan.num_ops(1)) if plan.op_info(1, i)["kind"] == KIND_WGRAD]


def taken(plan):
    """[(tag, N, K)] of the WGRAD launches that would run the frame-staged kernel under the knobs of the moment, in launch order."""
    from sefd_amd.plan import WG_FAMILY_THIN
    return [(o["tag"], o["N"], o["K"]) for _, o in wgrad_ops(plan) if o["family"] == WG_FAMILY_THIN]


def expected(case):
    """((tag, N, K) of the launches built, (tag, N, K) of the launches of the form that are refused because their (channels, N) is not instantiated).
    The decoder gradients are one launch per source: N = the source's channels, K = 2 frames x 5 positions x the layer's output channels (8 in the mask
    layer's buffer); the encoder layer's: N = its output channels, K = 2 x 5 x its input channels."""
    kn = case[4]
    c0, c1 = kn[0], kn[1]                                  # channels (real and imaginary together) of the first two encoder layers
    mask = [(405, c0, 2 * 5 * 8)] * 2
    rest = [(404, c1, 2 * 5 * c0)] * 2 + [(101, c1, 2 * 5 * c0)]
    return (mask + rest, []) if kn[0] == 32 else (rest, mask)


@pytest.fixture(autouse=True)
def _knobs_off():
    names = ("THIN_WGRAD", "THIN_MASK", "THIN_STAGE", "WG_SWAP")
    knobs.unset(*names)
    yield
    knobs.unset(*names)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[1]}_{c[3]}")
def test_selection_rule(case):
    from sefd_amd.plan import WG_FAMILY_DMA32, WG_FAMILY_F32, WG_FAMILY_NAMES, WG_FAMILY_THIN, wg_family_name
    # appended behind the families there were; named beside WG_FAMILY_NAMES, which keeps the families a plan reaches by its shape alone
    assert WG_FAMILY_THIN == WG_FAMILY_F32 + 1 == len(WG_FAMILY_NAMES)
    assert wg_family_name(WG_FAMILY_THIN) == "frame-staged thin" and wg_family_name(WG_FAMILY_DMA32) == WG_FAMILY_NAMES[WG_FAMILY_DMA32]
    plan = _make_plan(case)
    knobs.set("THIN_WGRAD", "0")
    assert taken(plan) == []
    before = [o["family"] for _, o in wgrad_ops(plan)]
    knobs.unset("THIN_WGRAD")
    assert taken(plan) == []                               # default rule: these plans are below its row threshold
    assert [o["family"] for _, o in wgrad_ops(plan)] == before
    knobs.set("THIN_WGRAD", "1")
    assert taken(plan) == []
    knobs.unset("THIN_WGRAD")
    knobs.set("THIN_MASK", "2")
    knobs.set("THIN_STAGE", "2")
    assert taken(plan) == []                               # the knobs of the forward / input-gradient kernels do not switch this one
    knobs.unset("THIN_MASK", "THIN_STAGE")
    knobs.set("THIN_WGRAD", "2")
    built, refused = expected(case)
    assert sorted(taken(plan)) == sorted(built) and len(built) >= 3, (taken(plan), built)
    # the refused launches keep the kernel they had, and every other launch its family
    after = [o["family"] for _, o in wgrad_ops(plan)]
    for (i, o), fb, fa in zip(wgrad_ops(plan), before, after):
        key = (o["tag"], o["N"], o["K"])
        if key in refused:
            assert fa == fb == WG_FAMILY_DMA32, (key, "refused: <8, 16> is not instantiated", fa, fb)
        elif key not in built:
            assert fa == fb, (key, fa, fb)
    assert sum((o["tag"], o["N"], o["K"]) in refused for _, o in wgrad_ops(plan)) == len(refused)
    # nothing in the fp32 twin, with DCCRN-large channels, or with the decoder gradients in their forward form (the encoder layer's stays)
    assert taken(_make_plan(case[:6] + ("fp32",))) == []
    assert taken(_make_plan(("DCCRN", 1, 2400, "C", (64, 128, 256, 512, 512, 512), 512, "bf16"))) == []
    knobs.set("WG_SWAP", "0")
    try:
        unswapped = _make_plan(case)
    finally:
        knobs.unset("WG_SWAP")
    assert [t for t in taken(unswapped) if t[0] != 101] == [] and taken(unswapped) == [b for b in built if b[0] == 101]


def _form(plan, i):
    """The fields of WGRAD op i that the kernel's form check reads (sizes and batch count apart)."""
    import exact_data as ed
    g = ed.gemm(plan, i)
    return (g.N, g.Npad, g.ldw, g.Fo, g.nseg, g.fstride[0], g.rowlen[0], g.xdt, g.ydt, g.flags & 0xffffffff, g.x[1].arena,
            tuple((g.seg[s].src, g.seg[s].dt, g.seg[s].off, g.seg[s].len, g.seg[s].koff) for s in range(g.nseg)))


def test_crn_takes_only_descriptors_that_are_dccrns():
    """CRN's conv layers keep their biases (no BatchNorm zeroes them out of the plan), so its weight gradients carry a ones run and its decoder gradients are
    in the forward form: whatever a CRN plan puts on the kernel must be, field for field, a descriptor DCCRN puts there."""
    from sefd_amd.plan import WG_FAMILY_THIN
    knobs.set("THIN_WGRAD", "2")
    dccrn = set()
    for case in CASES:
        plan = _make_plan(case)
        dccrn |= {_form(plan, i) for i, o in wgrad_ops(plan) if o["family"] == WG_FAMILY_THIN}
    assert len(dccrn) >= 4
    for case in CASES:
        crn = _make_plan(("CRN",) + case[1:])
        for i, o in wgrad_ops(crn):
            if o["family"] == WG_FAMILY_THIN:
                assert _form(crn, i) in dccrn, (o["tag"], o["N"], o["K"])
