"""Digests of the DEFAULT FullSubNet plans, to pin them across a change of the planner (tests/test_fsn_knobs_cpu.py).

Run on the commit whose plans are to be preserved - never on the code under test - and commit the output:

    python tests/golden/make_fsn_plan_digests.py > tests/golden/fsn_plan_digests.json

For the default `fsn` dict with each sequence model, norm_type, activation dtype and training / eval (B = 2, T = 21): sha256 over the op-kind
sequences of both phases, over the raw op arrays, over the constant image, and the arena sizes.  Needs no GPU: plans are built on the host.
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, T = 2, 21
NORMS = ("offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm")


def cases():
    for seq, norm, dt, training in itertools.product(("LSTM", "GRU"), NORMS, ("fp32", "bf16"), (True, False)):
        yield f"{seq}/{norm}/{dt}/{'train' if training else 'eval'}", dict(sequence_model=seq, norm_type=norm), dt, training


def plan_digest(plan):
    sz = plan.lib.sefd_op_size()
    rec = dict(arena_bytes=[int(v) for v in plan.arena_bytes], op_size=int(sz))
    for ph, nm in ((0, "fwd"), (1, "bwd")):
        n = plan.num_ops(ph)
        kinds = plan.op_kinds(ph)[0].astype("<i4").tobytes() if n else b""
        raw = bytes((C.c_uint8 * (n * sz)).from_address(plan.ops_ptr(ph))) if n else b""
        rec[nm] = dict(n=int(n), kinds=hashlib.sha256(kinds).hexdigest(), ops=hashlib.sha256(raw).hexdigest())
    rec["const"] = hashlib.sha256(np.ascontiguousarray(plan.const_image()).tobytes()).hexdigest()
    return rec


def all_digests():
    import sefd_amd  # noqa: F401
    from sefd_amd.plan import Plan
    return {name: plan_digest(Plan(B, T, model="FullSubNet", fsn=fsn, act_dtype=dt, training=training)) for name, fsn, dt, training in cases()}


if __name__ == "__main__":
    json.dump(all_digests(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
