#!/usr/bin/env python3
"""Fingerprints of the planner's output (CPU only): for a fixed matrix of model configurations and tuning knobs, one line per plan,
`name  sha256[:16]` over everything the C ABI exposes - error, frames, arena sizes, both parameter tables, the buffer table, the
constant image, the raw op arrays of both phases, sync points and the gradient bucket.  Two builds whose outputs match on every line
launch the same kernels with the same descriptors.

    python tools/plan_fingerprint.py [--dump DIR]        # DIR/<name>.{fwd,bwd,const}.bin: raw op arrays and constant image
    python tools/plan_fingerprint.py --diff DIR_A DIR_B  # first differing op per phase (index, kind, tag, byte offset inside Op)"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL = dict(kernel_num=(16, 32, 32, 64, 64, 64), rnn_units=128)
ARM = dict(B=2, L=16000, act_dtype="bf16", masking_mode="C")          # the knob arms' DCCRN bf16 base (B = 2, 1 s)
CRN = dict(model="CRN", **SMALL)

# (name, Plan keyword arguments (B, L included), tuning knobs)
MATRIX = [(f"dccrn_{dt}_{m}", dict(B=2, L=8000, act_dtype=dt, masking_mode=mm), {})
          for dt in ("fp32", "bf16") for m, mm in (("E", "E"), ("C", "C"), ("R", "R"), ("direct", "Direct(None make)"))]
for dt in ("fp32", "bf16"):
    MATRIX += [
        (f"dccrn_{dt}_small", dict(B=2, L=4000, act_dtype=dt, **SMALL), {}),
        (f"dccrn_{dt}_cbn", dict(B=2, L=4000, act_dtype=dt, use_cbn=True, **SMALL), {}),
        (f"dccrn_{dt}_noskip", dict(B=2, L=4000, act_dtype=dt, skip_type=False, **SMALL), {}),
        (f"dccrn_{dt}_lstm_real", dict(B=2, L=4000, act_dtype=dt, lstm="real", **SMALL), {}),
        (f"dccrn_{dt}_win_none", dict(B=2, L=4000, act_dtype=dt, win_type=None, **SMALL), {}),
        (f"dccrn_{dt}_win_hamming", dict(B=2, L=4000, act_dtype=dt, win_type="hamming", **SMALL), {}),
        (f"dccrn_{dt}_rnn512", dict(B=2, L=4000, act_dtype=dt, kernel_num=(16, 32, 32, 64, 64, 64), rnn_units=512), {}),
        (f"dccrn_{dt}_eval", dict(B=2, L=4000, act_dtype=dt, training=False, **SMALL), {}),
        (f"dccrn_{dt}_world2", dict(B=2, L=4000, act_dtype=dt, masking_mode="C", bn_world=2, **SMALL), {}),
        (f"dccrn_{dt}_world4", dict(B=2, L=4000, act_dtype=dt, masking_mode="C", bn_world=4, **SMALL), {}),
        (f"dccrn_{dt}_buckets2", dict(B=2, L=4000, act_dtype=dt, grad_buckets=2, **SMALL), {}),
        (f"dccrn_{dt}_refused", dict(B=2, L=4000, act_dtype=dt, kernel_num=(16, 32, 32, 64, 64, 64), rnn_units=2050), {}),
        (f"crn_{dt}_mask", dict(B=2, L=4000, act_dtype=dt, masking_mode="E", **CRN), {}),
        (f"crn_{dt}_direct", dict(B=2, L=4000, act_dtype=dt, masking_mode="Direct(None make)", **CRN), {}),
        (f"crn_{dt}_world2", dict(B=2, L=4000, act_dtype=dt, masking_mode="E", bn_world=2, **CRN), {}),
        (f"crn_{dt}_stft_gemm", dict(B=2, L=4000, act_dtype=dt, masking_mode="E", **CRN), {"STFT_GEMM": 1}),
        (f"crn_{dt}_noskip", dict(B=2, L=4000, act_dtype=dt, masking_mode="E", skip_type=False, **CRN), {}),
        (f"crn_{dt}_eval", dict(B=2, L=4000, act_dtype=dt, masking_mode="E", training=False, **CRN), {}),
        # the recurrent block of lstm="real": per-frame cells (by knob, by size), the early gradient bucket, spectral mapping
        (f"dccrn_{dt}_lstm_real_stepped", dict(B=2, L=4000, act_dtype=dt, lstm="real", **SMALL), {"LSTM_STEPPED": 1}),
        (f"dccrn_{dt}_lstm_real_rnn512", dict(B=2, L=4000, act_dtype=dt, lstm="real", kernel_num=(16, 32, 32, 64, 64, 64), rnn_units=512), {}),
        (f"dccrn_{dt}_lstm_real_buckets2", dict(B=2, L=4000, act_dtype=dt, lstm="real", grad_buckets=2, **SMALL), {}),
        (f"dccrn_{dt}_lstm_real_direct", dict(B=2, L=4000, act_dtype=dt, lstm="real", masking_mode="Direct(None make)", **SMALL), {}),
    ]
MATRIX += [
    ("frontend", dict(B=2, L=8000, model="STFT"), {}),
    ("frontend_stft_gemm", dict(B=2, L=8000, model="STFT"), {"STFT_GEMM": 1}),
    ("frontend_hamming", dict(B=2, L=8000, model="STFT", win_type="hamming"), {}),
    ("fsn_fp32", dict(B=2, L=9, model="FullSubNet", fsn=dict(fb_hidden=64, sb_hidden=32, keep=0.2)), {}),
    ("fsn_bf16", dict(B=2, L=9, act_dtype="bf16", model="FullSubNet", fsn=dict(fb_hidden=256, sb_hidden=192, keep=0.2)), {}),
    ("torchstft", dict(B=2, L=6000, win_len=400, win_inc=300, fft_len=512, model="TorchSTFT"), {}),
    ("torchistft", dict(B=2, L=6000, win_len=400, win_inc=300, fft_len=512, model="TorchISTFT"), {}),
    ("bench_dccrn_bf16_C_b32_3s", dict(B=32, L=48000, act_dtype="bf16", masking_mode="C"), {}),
    ("bench_BN_FUSE=0", dict(B=32, L=48000, act_dtype="bf16", masking_mode="C"), {"BN_FUSE": 0}),
    ("arm_base", dict(ARM), {}),
    ("dccrn_fp32_arm_base", dict(ARM, act_dtype="fp32"), {}),
    ("dccrn_fp32_ENC_BIAS_ZERO=0", dict(ARM, act_dtype="fp32"), {"ENC_BIAS_ZERO": 0}),
    ("arm_ENC0_DIRECT=0+SPECPAD_FUSE=0", dict(ARM), {"ENC0_DIRECT": 0, "SPECPAD_FUSE": 0}),
]
for knob, val in (("STFT_GEMM", 1), ("ENC0_DIRECT", 0), ("ENC0_BNFUSE", 0), ("BN_FUSE", 2), ("PHASE_MERGE_MAXN", 0), ("WG_SWAP", 0),
                  ("MASK_COLSUM", 0), ("LANE_ALL", 0), ("LSTM_STEPPED", 1), ("ENC_BIAS_ZERO", 0), ("GX_MERGE", 0), ("DX_MERGE", 0),
                  ("LSTM_CHUNKS", 1)):
    MATRIX.append((f"arm_{knob}={val}", dict(ARM), {knob: val}))
MATRIX.append(("arm_LSTM_STEPPED=1+GX_MERGE=0", dict(ARM), {"LSTM_STEPPED": 1, "GX_MERGE": 0}))
BASES = {"bench_BN_FUSE=0": "bench_dccrn_bf16_C_b32_3s", "dccrn_fp32_ENC_BIAS_ZERO=0": "dccrn_fp32_arm_base",
         "arm_ENC0_DIRECT=0+SPECPAD_FUSE=0": "arm_ENC0_DIRECT=0", "arm_LSTM_STEPPED=1+GX_MERGE=0": "arm_LSTM_STEPPED=1",
         "frontend_stft_gemm": "frontend"}
for dt in ("fp32", "bf16"):
    BASES.update({f"crn_{dt}_{arm}": f"crn_{dt}_mask" for arm in ("stft_gemm", "noskip", "eval")})
    BASES.update({f"dccrn_{dt}_lstm_real_{arm}": f"dccrn_{dt}_lstm_real" for arm in ("stepped", "rnn512", "buckets2", "direct")})


def plan_bytes(kw, knobs):
    """{'meta': bytes, 'fwd': bytes, 'bwd': bytes, 'const': bytes} of one configuration (a refused plan: its message as 'meta')."""
    from sefd_amd import tuning
    from sefd_amd.plan import ARENA_COUNT, Plan
    kw = dict(kw)
    B, L = kw.pop("B"), kw.pop("L")
    with tuning.scope(**knobs):
        try:
            p = Plan(B, L, **kw)
        except ValueError as e:
            return {"meta": ("refused: " + str(e)).encode()}
    lib, h = p.lib, p.h
    meta = [f"error={lib.sefd_plan_error(h).decode()!r} T={p.T}", "arenas=" + ",".join(str(lib.sefd_plan_arena_bytes(h, a)) for a in range(ARENA_COUNT))]
    shp = (C.c_int64 * 4)()
    for kind in (0, 1):
        for i in range(lib.sefd_plan_num_params(h, kind)):
            nd = lib.sefd_plan_param_shape(h, kind, i, shp)
            meta.append(f"param{kind} {lib.sefd_plan_param_name(h, kind, i).decode()} {lib.sefd_plan_param_offset(h, kind, i)} "
                        f"{lib.sefd_plan_param_numel(h, kind, i)} {tuple(int(shp[k]) for k in range(nd))}")
    for name in sorted(p.buffer_names()):
        meta.append(f"buf {name} {p.buffer(name)}")
    meta.append(f"syncs={p.sync_points()}")
    meta.append(f"bucket={p.grad_bucket_range()}")
    out = {"meta": "\n".join(meta).encode(), "const": p.const_image().tobytes()}
    sz = lib.sefd_op_size()
    for ph, key in ((0, "fwd"), (1, "bwd")):
        n = p.num_ops(ph)
        out[key] = C.string_at(p.ops_ptr(ph), n * sz) if n else b""
    return out


def digest(parts):
    h = hashlib.sha256()
    for key in ("meta", "const", "fwd", "bwd"):
        v = parts.get(key, b"")
        h.update(key.encode() + len(v).to_bytes(8, "little") + v)
    return h.hexdigest()[:16]


def diff(da, db):
    from sefd_amd import _lib
    sz = _lib.lib().sefd_op_size()
    for name, _, _ in MATRIX:
        for key in ("fwd", "bwd", "const"):
            fa, fb = (os.path.join(d, f"{name}.{key}.bin") for d in (da, db))
            if not (os.path.exists(fa) and os.path.exists(fb)):
                continue
            a, b = open(fa, "rb").read(), open(fb, "rb").read()
            if a == b:
                continue
            if key == "const":
                m = min(len(a), len(b))
                offs = np.flatnonzero(np.frombuffer(a, np.uint8, m) != np.frombuffer(b, np.uint8, m))
                first = int(offs[0]) if len(offs) else m
                print(f"{name} const: {len(a)} vs {len(b)} bytes, first difference at byte {first}")
                continue
            na, nb = len(a) // sz, len(b) // sz
            for i in range(min(na, nb)):
                oa, ob = np.frombuffer(a[i * sz:(i + 1) * sz], np.uint8), np.frombuffer(b[i * sz:(i + 1) * sz], np.uint8)
                offs = np.nonzero(oa != ob)[0]
                if len(offs):
                    kind, tag = (int(x) for x in np.frombuffer(a[i * sz:i * sz + 8], np.int32))
                    print(f"{name} {key}: {na} vs {nb} ops, first difference at op {i} (kind {kind}, tag {tag}), byte offsets {offs[:16].tolist()}")
                    break
            else:
                print(f"{name} {key}: {na} vs {nb} ops, common prefix identical")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--diff", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args()
    if args.diff:
        diff(*args.diff)
        return
    import sefd_amd  # noqa: F401
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    hashes = {}
    for name, kw, knobs in MATRIX:
        parts = plan_bytes(kw, knobs)
        hashes[name] = digest(parts)
        print(f"{name}  {hashes[name]}", flush=True)
        if args.dump:
            for key, v in parts.items():
                with open(os.path.join(args.dump, f"{name}.{key}.bin"), "wb") as f:
                    f.write(v)
    # a knob arm that hashes like its own default tests nothing
    for name in hashes:
        base = BASES.get(name, "arm_base" if name.startswith("arm_") and name != "arm_base" else None)
        if base and hashes[name] == hashes[base]:
            print(f"warning: {name} plans the same as {base}", file=sys.stderr)


if __name__ == "__main__":
    main()
