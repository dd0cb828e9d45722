"""Golden vectors for NavieComplexLSTM on its own (tools_for_model.py:141-181): one and two directions, with and without the projection.

RUN ONLY WHERE THE REFERENCE IS AVAILABLE (same import shim as make_golden.py, which is imported, never edited).  Per case of tests/clstm_common.py: the
real reference `tools_for_model.NavieComplexLSTM` with the formula weights of oracle/weights.py, [out_r, out_i] = m([x_real, x_imag]),
loss = mean(out_r * g_real) + mean(out_i * g_imag), backward.  Stored: the four inputs, both outputs, the loss, both input gradients in full; grad_norm of
every parameter; the gradients of the tensors of at most 4096 elements in full and of the others sampled (make_golden.sample, stride 211); meta
(sizes, the state_dict's keys and shapes in order, loss_scale = mean |out . g| over both outputs).

The generator refuses to write a fixture unless, with the reference alone,
  1. zeroing any single weight_hh_* moves the outputs by at least 0.05 (max-abs relative to max |y|): a recurrence that is ignored or run in the wrong
     direction cannot pass a 1e-3 bar;
  2. flipping the time axis of the inputs moves them (by at least the same 0.05).
The measured values are stored under g/meta/.

    python tests/golden/make_clstm_golden.py
"""
import os
import sys

import numpy as np
import torch

import make_golden as mg
from make_golden import fill_state_dict_, flat, sample

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clstm_common as cc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_HH_EFFECT = 0.05


def clstm_case(tfm, name):
    case = cc.CASES[name]
    isz, hsz, pdim, bi, B, T = case
    m = tfm.NavieComplexLSTM(isz, hsz, projection_dim=pdim, bidirectional=bi)
    fill_state_dict_(m)
    m.train()
    xr, xi, gr, gi = cc.inputs(case)
    xr.requires_grad_(True)
    xi.requires_grad_(True)
    out_r, out_i = m([xr, xi])
    lossv = cc.loss_of(out_r, out_i, gr, gi)
    lossv.backward()
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    y0 = torch.cat([out_r, out_i], 2).detach()
    den = float(y0.abs().max())
    effects = {}
    with torch.no_grad():
        run = lambda a, b: torch.cat(m([a, b]), 2)
        for k, p in m.named_parameters():
            if "weight_hh" not in k:
                continue
            keep = p.detach().clone()
            p.zero_()
            effects[k] = float((run(xr, xi) - y0).abs().max()) / den
            p.copy_(keep)
        flip = float((run(xr.flip(0), xi.flip(0)).flip(0) - y0).abs().max()) / den
    worst = min(effects.values())
    print(f"  {name}: smallest weight_hh effect {worst:.4f} ({min(effects, key=effects.get)}), time flip {flip:.4f}")
    if worst < MIN_HH_EFFECT:
        raise SystemExit(f"clstm_{name}: zeroing {min(effects, key=effects.get)} moves the outputs by {worst:.4f} < {MIN_HH_EFFECT}")
    if flip < MIN_HH_EFFECT:
        raise SystemExit(f"clstm_{name}: flipping the time axis of the inputs moves the outputs by {flip:.4f} < {MIN_HH_EFFECT}")
    sd = m.state_dict()
    assert list(sd) == list(cc.torch_shapes(case)) and [tuple(v.shape) for v in sd.values()] == list(cc.torch_shapes(case).values())
    meta = dict(input_size=isz, hidden_size=hsz, projection_dim=-1 if pdim is None else pdim, bidirectional=int(bi), B=B, T=T,
                keys=np.array(list(sd)), shapes=np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64),
                min_hh_effect=worst, flip_effect=flip, loss_scale=cc.loss_scale(out_r.detach(), out_i.detach(), gr, gi))
    small = lambda k: g[k].numel() <= 4096                             # every bias; the projection matrices of the small cases
    rec = dict(meta=meta, xr=xr.detach().numpy(), xi=xi.detach().numpy(), gr=gr.numpy(), gi=gi.numpy(), out_r=out_r.detach().numpy(),
               out_i=out_i.detach().numpy(), loss=float(lossv), dxr=xr.grad.detach().numpy(), dxi=xi.grad.detach().numpy(),
               grad_norm={k: float(v.double().norm()) for k, v in g.items()},
               grad={k: v.numpy() for k, v in g.items() if small(k)},
               grad_samp={k: sample(v, cc.STRIDE)["samp"] for k, v in g.items() if not small(k)})
    path = os.path.join(HERE, f"clstm_{name}.npz")
    np.savez_compressed(path, **flat(rec, "g"))
    assert os.path.getsize(path) <= 326568, (path, os.path.getsize(path))      # the largest fixture so far, fsn_knobs_default_fb4.npz
    print(f"clstm_{name}: loss {float(lossv):.6e}, {os.path.getsize(path)} bytes")


def main():
    _, _, tfm, _ = mg.import_reference()
    torch.set_num_threads(4)
    for name in (sys.argv[1:] or cc.CASES):
        clstm_case(tfm, name)


if __name__ == "__main__":
    main()
