"""Golden vectors for SequenceModel on its own (tools_for_model.py:726-795): any depth, both directions, LSTM and GRU, all four head activations.

RUN ONLY WHERE THE REFERENCE IS AVAILABLE (same import shim as make_golden.py, which is imported, never edited).  Per case: the real reference
`tools_for_model.SequenceModel` with the formula weights of oracle/weights.py, train mode with the inter-layer dropout patched to 0,
y = m(x), loss = mean((y - tgt)^2), backward.  Stored: x, tgt, y, loss, dx in full; grad_norm of every parameter; the gradients of the small tensors
(biases, the head) in full and of the others sampled (make_golden.sample, stride 211); meta.

The generator refuses to write a fixture unless, with the reference alone,
  1. the head's activation is exercised on every side of its kinks (make_fsn_knobs_golden.head_stats); where the formula weights do not reach a
     kink the head's weight and bias are scaled by g/meta/head_scale (the tests apply the same factor after fill_state_dict_).  The factor is
     the SMALLEST power of two for which the rule holds: it exists to reach the kinks, and every further doubling only multiplies the error of
     the last layer's h in the output (|d pre| = scale * |W_fc . dh|) without exercising anything more;
  2. zeroing any single weight_hh_* moves y by at least 0.05 (max-abs relative to max|y|): a recurrence that is ignored or run in the wrong
     direction cannot pass a 1e-3 bar.  The measured minimum, and the effect of flipping the time axis of x, are stored under g/meta/.

    python tests/golden/make_seqmodel_golden.py
"""
import os

import numpy as np
import torch

import make_golden as mg
from make_golden import fill_state_dict_, flat, sample
from make_fsn_knobs_golden import head_stats
from oracle.weights import splitmix_uniform

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (sequence_model, I, O, H, num_layers, bidirectional, activation, B, T)
CASES = {
    "lstm_l3_bi": ("LSTM", 21, 5, 64, 3, True, "Tanh", 3, 9),
    "gru_l3_bi": ("GRU", 21, 5, 64, 3, True, "ReLU6", 3, 9),
    "lstm_l1_uni": ("LSTM", 21, 5, 64, 1, False, None, 3, 9),
    "gru_l4_uni": ("GRU", 21, 5, 64, 4, False, "ReLU", 3, 9),
    "lstm_h192_l3_bi": ("LSTM", 21, 5, 192, 3, True, "Tanh", 18, 10),
    "lstm_h256_l2_bi": ("LSTM", 21, 5, 256, 2, True, None, 18, 11),
}
MIN_HH_EFFECT = 0.05


def inputs(B, I, O, T):
    """Closed-form input and target: x = 6 |u| (non-negative, like a magnitude feature), tgt = u', both from the splitmix stream of oracle/weights.py."""
    x = torch.from_numpy((6.0 * np.abs(splitmix_uniform(1001, B * I * T))).astype(np.float32).reshape(B, I, T))
    tgt = torch.from_numpy(splitmix_uniform(1002, B * O * T).astype(np.float32).reshape(B, O, T))
    return x, tgt


def build(tfm, name, scale):
    seq, I, O, H, NL, bi, act, B, T = CASES[name]
    m = tfm.SequenceModel(I, O, H, NL, bi, seq, act)
    fill_state_dict_(m)
    with torch.no_grad():
        m.fc_output_layer.weight.mul_(scale)
        m.fc_output_layer.bias.mul_(scale)
    m.train()
    m.sequence_model.dropout = 0.0
    return m


def head_scale(tfm, name):
    """Smallest power of two (from 1) at which head_stats accepts the head's pre-activations; None: no factor up to 2^16 does."""
    seq, I, O, H, NL, bi, act, B, T = CASES[name]
    x, _ = inputs(B, I, O, T)
    for e in range(17):
        m = build(tfm, name, float(2 ** e))
        with torch.no_grad():
            pre = m.fc_output_layer(m.sequence_model(x.permute(0, 2, 1))[0])
        if head_stats(act, pre)[1]:
            return float(2 ** e)
    return None


def seq_case(tfm, name):
    seq, I, O, H, NL, bi, act, B, T = CASES[name]
    scale = head_scale(tfm, name)
    if scale is None:
        raise SystemExit(f"seqmodel_{name}: no head scale up to 2^16 exercises the {act} on every side of its kinks")
    m = build(tfm, name, scale)
    x, tgt = inputs(B, I, O, T)
    x.requires_grad_(True)
    pre = {}
    hook = m.fc_output_layer.register_forward_hook(lambda mod, i, o: pre.__setitem__("y", o.detach().clone()))
    y = m(x)
    hook.remove()
    lossv = ((y - tgt) ** 2).mean()
    lossv.backward()
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    st, ok = head_stats(act, pre["y"])
    print(f"  {name} head ({act}, scale {scale:g}): " + ", ".join(f"{a} {b:.4g}" for a, b in st.items()))
    if not ok:
        raise SystemExit(f"seqmodel_{name}: the head's {act} is not exercised on every side of its kinks: {st}")
    # condition 2, with the reference alone
    y0 = y.detach()
    den = float(y0.abs().max())
    effects = {}
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "weight_hh" not in k:
                continue
            keep = p.detach().clone()
            p.zero_()
            effects[k] = float((m(x) - y0).abs().max()) / den
            p.copy_(keep)
        flip = float((m(x.flip(2)).flip(2) - y0).abs().max()) / den
    worst = min(effects.values())
    print(f"  {name}: smallest weight_hh effect {worst:.4f} ({min(effects, key=effects.get)}), time flip {flip:.4f}")
    if worst < MIN_HH_EFFECT:
        raise SystemExit(f"seqmodel_{name}: zeroing {min(effects, key=effects.get)} moves y by {worst:.4f} < {MIN_HH_EFFECT}")
    meta = dict(sequence_model=np.array(seq), I=I, O=O, H=H, num_layers=NL, bidirectional=int(bi), act=np.array(str(act)), B=B, T=T, head_scale=scale,
                head_pre=st, min_hh_effect=worst, flip_effect=flip)
    small = lambda k: "bias" in k or k.startswith("fc_output_layer")
    rec = dict(meta=meta, x=x.detach().numpy(), tgt=tgt.numpy(), y=y0.numpy(), loss=float(lossv), dx=x.grad.detach().numpy(),
               grad_norm={k: float(v.double().norm()) for k, v in g.items()},
               grad={k: v.numpy() for k, v in g.items() if small(k)},
               grad_samp={k: sample(v, 211)["samp"] for k, v in g.items() if not small(k)})
    path = os.path.join(HERE, f"seqmodel_{name}.npz")
    np.savez_compressed(path, **flat(rec, "g"))
    assert os.path.getsize(path) <= 326568, (path, os.path.getsize(path))      # the largest fixture so far, fsn_knobs_default_fb4.npz
    print(f"seqmodel_{name}: loss {float(lossv):.6f}, {os.path.getsize(path)} bytes")


def main():
    import sys
    _, _, tfm, _ = mg.import_reference()
    torch.set_num_threads(4)
    for name in (sys.argv[1:] or CASES):
        seq_case(tfm, name)


if __name__ == "__main__":
    main()
