"""CPU: the mixing oracle against the reference's own generate_noisy_wav, through outputs of that function captured with
tests/golden/make_mixing_golden.py (tests/golden/mixing_golden.npz: the inputs, the (SNR, segment start) cases and the int16 mixtures)."""
import numpy as np

from oracle.mixing import generate_noisy_wav

CASES = ((0, 17), (5, 9000), (-5, 15999))          # (SNR in dB, noise segment start)


def mixing_inputs():
    rng = np.random.default_rng(0)
    speech = (rng.standard_normal(4000) * 0.1 + 0.01)
    noise = rng.standard_normal(20000) * 0.3 - 0.02
    return speech, noise


def test_mixing_oracle_equals_reference_function():
    from util import load_golden
    g = load_golden("mixing_golden")
    assert [tuple(c) for c in g["cases"].tolist()] == list(CASES)
    assert g["noisy"].dtype == np.int16
    speech, noise = g["speech"], g["noise"]
    for (snr, start), ref in zip(CASES, g["noisy"]):
        assert np.array_equal(ref, generate_noisy_wav(speech, noise, snr, start))
