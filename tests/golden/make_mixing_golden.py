#!/usr/bin/env python3
"""Captures goldens of the reference's offline SNR mixing (generate_noisy_data.py `generate_noisy_wav`) for tests/test_oracle_mixing.py.

    python tests/golden/make_mixing_golden.py <reference checkout>

The reference module imports librosa / soundfile at import time, so only the function body is executed, from its source text, with
np.random.randint patched to return each case's segment start.  Inputs and outputs go to tests/golden/mixing_golden.npz."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from test_oracle_mixing import CASES, mixing_inputs  # noqa: E402


def main():
    src = os.path.join(sys.argv[1], "generate_noisy_data.py")
    tree = ast.parse(open(src).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "generate_noisy_wav")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), src, "exec"), ns)
    speech, noise = mixing_inputs()
    outs = []
    for snr, start in CASES:
        orig = np.random.randint
        np.random.randint = lambda lo, hi: start
        try:
            outs.append(ns["generate_noisy_wav"](speech, noise, snr))
        finally:
            np.random.randint = orig
    np.savez_compressed(os.path.join(HERE, "mixing_golden.npz"), speech=speech, noise=noise, cases=np.array(CASES, dtype=np.int64),
                        noisy=np.stack(outs))
    print("cases", CASES, "dtype", outs[0].dtype)


if __name__ == "__main__":
    main()
