"""Golden vectors for ConvSTFT and ConviSTFT on their own (tools_for_model.py:36-112): both feature types, both modules, both ConviSTFT input forms.

RUN ONLY WHERE THE REFERENCE IS AVAILABLE (same import shim as make_golden.py, which is imported, never edited).  Per case of
tests/convstft_common.CASES (B = 2) the real reference modules run on the CPU in float64 (`module.double()`) and in float32:
y = f(x), loss = sum(y * cot) with fixed cotangents, backward.  Inputs and cotangents are closed form (convstft_common.case_inputs: splitmix
streams of oracle/weights.py at the stored seed), so the fixtures hold the seed and the results only: every float64 output and input gradient,
rounded to float32 (a case's spectra in float64 alone would pass the 200 KB a fixture may have; the rounding, 6e-8, is 3 % of the smallest
bar), in two files per case (`_stft`, `_istft`), and per tensor ref32_err = max|ref32 - ref64| / max|ref64| (phase: circular difference).

The seed is the first of 16 at which every bin of the waveform's float64 spectrum has m >= 1e-3 max m: below that atan2 and the gradient
through it (~ 1 / m) are noise in float32, in the reference as much as anywhere.  The generator refuses to write a fixture if no seed does.
(The magnitudes FED to ConviSTFT are |u| as they come: the polar form and its gradients have no 1 / m.)

    python tests/golden/make_convstft_golden.py
"""
import os
import sys

import numpy as np
import torch

import make_golden as mg

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import convstft_common as cc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 200 * 1000


def reference_run(tfm, shape, inp, dtype):
    W, hop, NFFT, _, win_type = shape
    mods = [tfm.ConvSTFT(W, hop, NFFT, win_type, "complex"), tfm.ConvSTFT(W, hop, NFFT, win_type, "real"), tfm.ConviSTFT(W, hop, NFFT, win_type, "real")]
    sc, sr, inv = (m.to(dtype) for m in mods)
    return cc.run_all(sc, sr, lambda a, ph: inv(a, ph), inp, dtype)


def case(tfm, name):
    shape = cc.CASES[name]
    for seed in range(16):
        inp = cc.case_inputs(name, seed)
        r64 = reference_run(tfm, shape, inp, torch.float64)
        m1 = r64["mags"]
        if float(m1.min()) >= 1e-3 * float(m1.max()):
            break
        print(f"  {name}: seed {seed} has a bin at {float(m1.min() / m1.max()):.2e} of the largest magnitude (< 1e-3)")
    else:
        raise SystemExit(f"convstft_{name}: none of 16 seeds keeps every magnitude above 1e-3 of the largest")
    r32 = reference_run(tfm, shape, inp, torch.float32)
    e32 = cc.measure(r64, r32)
    T, NF, Lout = cc.geometry(*shape[:4])
    for part, keys in (("stft", cc.STFT_KEYS), ("istft", cc.ISTFT_KEYS)):
        rec = dict(seed=seed, T=T, NF=NF, Lout=Lout)
        for k in keys:
            rec[f"ref/{k}"] = r64[k].float().numpy()
            rec[f"ref32_err/{k}"] = e32[k]
        path = os.path.join(HERE, f"convstft_{name}_{part}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
        print(f"convstft_{name}_{part}: seed {seed}, {os.path.getsize(path)} bytes, ref32_err " + ", ".join(f"{k} {e32[k]:.2e}" for k in keys))


def main():
    _, _, tfm, _ = mg.import_reference()
    torch.set_num_threads(4)
    for name in (sys.argv[1:] or cc.CASES):
        case(tfm, name)


if __name__ == "__main__":
    main()
