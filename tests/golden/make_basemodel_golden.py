"""Golden vectors for BaseModel on its own (tools_for_model.py:801-1185): `unfold`, the seven norms and `_reduce_complexity_separately`.

RUN ONLY WHERE THE REFERENCE IS AVAILABLE (same import shim as make_golden.py, which is imported, never edited).  Per case of
tests/basemodel_common.py: the real reference `tools_for_model.BaseModel` statics on the CPU, in float64 and in float32, on the closed-form inputs of
the case: y = f(x), loss = sum(y * cot), backward.  Stored per case in basemodel_<case>.npz: the seed, ref/y and ref/grad_x (ref/grad_x2 for the
two-input reduce case) in float64, and per tensor ref32_err = max|ref32 - ref64| / max|ref64| - the reference's own float32 error, which the GPU
test's bar is a multiple of.

The generator refuses to write a fixture whose bar would be loose: ref32_err < 2e-6 for every tensor, and every file stays under 200 kB.

    python tests/golden/make_basemodel_golden.py [case ...]
"""
import os
import sys

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import basemodel_common as bc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_REF32_ERR = 2e-6
MAX_BYTES = 200_000


def basemodel_case(BaseModel, name):
    inp = bc.inputs(name, bc.SEED)
    r64 = bc.run_case(BaseModel, name, torch.float64, inp=inp)
    r32 = bc.run_case(BaseModel, name, torch.float32, inp=inp)
    rec = {"seed": np.int64(bc.SEED)}
    worst = 0.0
    for k, v in r64.items():
        assert tuple(v.shape) == (bc.out_shape(name) if k == "y" else tuple(inp["x2" if k == "grad_x2" else "x"].shape)), (name, k, v.shape)
        assert bool(torch.isfinite(v).all()), (name, k)
        e = bc.rel_err(r32[k], v)
        if not e < MAX_REF32_ERR:
            raise SystemExit(f"basemodel_{name}: the reference's own float32 error of {k} is {e:.3e} >= {MAX_REF32_ERR}: the bar would be loose")
        worst = max(worst, e)
        rec["ref/" + k] = v.numpy()
        rec["ref32_err/" + k] = np.float64(e)
    path = os.path.join(HERE, f"basemodel_{name}.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (path, size)
    print(f"basemodel_{name}: ref32_err {worst:.2e}, {size} bytes")
    return size


def main():
    _, _, tfm, _ = mg.import_reference()
    torch.set_num_threads(4)
    total = sum(basemodel_case(tfm.BaseModel, name) for name in (sys.argv[1:] or bc.CASES))
    print(f"{total} bytes in all")


if __name__ == "__main__":
    main()
