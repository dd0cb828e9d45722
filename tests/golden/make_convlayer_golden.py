"""Golden vectors for the conv layers and ComplexBatchNorm on their own (tools_for_model.py:199-607) and for one stack of them.

RUN ONLY WHERE THE REFERENCE IS AVAILABLE (same import shim as make_golden.py, which is imported, never edited).  Per case of
tests/convlayer_common (CASES, CBN_CASES, CORR_CASES, STACK; B = 2) the real reference modules run on the CPU in float64 (`module.double()`) and in float32:
y = f(x), loss = sum(y * cot), backward.  Inputs, cotangents and parameter values are closed form (splitmix streams of oracle/weights.py at the
stored seed: convlayer_common.fill_ / *_inputs), so a fixture holds the seed and the results only: every float64 output, input gradient,
parameter gradient and buffer after the forward, rounded to float32, and per tensor ref32_err = max|ref32 - ref64| / max|ref64|.

The integer variant (convlayer_common.INT_CASES, convlayer_<name>_int.npz; `int` on the command line makes these alone): x and the cotangent integers
in -3 .. 3, every weight and bias an integer in -1 .. 1 (convlayer_common.int_inputs / fill_int_).  Asserted here: every y, dx and parameter gradient
is an integer far below 2^24, and the reference's float32 run equals its float64 run exactly - so the fixture is the one right answer of any kernel
whose accumulators are at least fp32, whatever its order of additions.

    python tests/golden/make_convlayer_golden.py [case ...]
"""
import os
import sys

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import convlayer_common as lc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 200 * 1000


def write(name, r64, r32):
    rec = dict(seed=lc.SEED)
    e32 = {}
    for k, v in r64.items():
        rec["ref/" + k] = v.float().numpy()
        e32[k] = lc.err_of(k, r32, r64, name)
        rec["ref32_err/" + k] = e32[k]
    path = os.path.join(HERE, f"convlayer_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"convlayer_{name}: {os.path.getsize(path)} bytes, {sum(v.numel() for v in r64.values())} values, E32 {max(e32.values()):.2e}")
    return max(e32.values())


def write_corr(name, r64, r32):
    """A correlated ComplexBatchNorm case: the float64 results and, per complex channel and family of tensors, the float32 run's error."""
    rec = dict(seed=lc.SEED)
    for k, v in r64.items():
        rec["ref/" + k] = v.float().numpy()
    e32 = lc.channel_errors(r32, r64)
    for fam, e in e32.items():
        rec["ref32_err_ch/" + fam] = e.numpy()
    path = os.path.join(HERE, f"convlayer_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"convlayer_{name}: {os.path.getsize(path)} bytes; float32 error per channel: " + ", ".join(f"{fam} {float(e.max()):.2e}" for fam, e in e32.items()))


def both(build, inp, training=True, forward_of=None):
    res = []
    for dtype in (torch.float64, torch.float32):
        m = build()
        lc.fill_(m, lc.SEED)
        m = m.to(dtype).train(training)
        res.append(lc.run_module(m, inp, dtype, forward=forward_of(m) if forward_of else None))
    return res


def write_int(tfm, name):
    res = []
    for dtype in (torch.float64, torch.float32):
        m = lc.make_conv(tfm, name)
        lc.fill_int_(m, lc.SEED)
        res.append(lc.run_module(m.to(dtype).train(True), lc.int_inputs(name), dtype))
    r64, r32 = res
    rec = dict(seed=lc.SEED)
    for k, v in r64.items():
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 16, (name, k, float(v.abs().max()))      # integers far below 2^24
        assert torch.equal(r32[k], v), (name, k)                                                            # float32 == float64, exactly
        assert float(v.abs().max()) > 0, (name, k)
        rec["ref/" + k] = v.float().numpy()
    path = os.path.join(HERE, f"convlayer_{name}_int.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
    print(f"convlayer_{name}_int: {os.path.getsize(path)} bytes, largest |value| {max(float(v.abs().max()) for v in r64.values()):.0f}")


def main():
    _, _, tfm, _ = mg.import_reference()
    torch.set_num_threads(4)
    want = sys.argv[1:]
    if not want or "int" in want:
        for name in lc.INT_CASES:
            write_int(tfm, name)
        if want:
            return
    e = []
    for name in lc.CASES:
        if not want or name in want:
            e.append(write(name, *both(lambda: lc.make_conv(tfm, name), lc.conv_inputs(name))))
    for name, (C, rest, training, momentum) in lc.CBN_CASES.items():
        if not want or name in want:
            e.append(write(name, *both(lambda: tfm.ComplexBatchNorm(C, momentum=momentum), lc.cbn_inputs(name), training)))
    for name in lc.CORR_CASES:
        if not want or name in want:
            write_corr(name, *both(lambda: tfm.ComplexBatchNorm(lc.CORR_C, momentum=lc.CORR_MOMENTUM), lc.corr_inputs(name), True))
    if not want or lc.STACK in want:
        e.append(write(lc.STACK, *both(lambda: lc.make_stack(tfm), lc.stack_inputs(), True, lc.stack_forward)))
    if e:
        print(f"E32 over {len(e)} cases: {min(e):.2e} .. {max(e):.2e}")


if __name__ == "__main__":
    main()
