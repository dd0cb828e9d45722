"""Golden vectors for the FullSubNet knobs beyond the default: fb_num_neighbors > 0, any sb_num_neighbors, all four output activations.

RUN ONLY WHERE THE REFERENCE IS AVAILABLE (same import shim as make_golden.py, which is imported, never edited).  One train step of the
real reference FullSubNet per case (dropout patched to 0, formula weights of oracle/weights.py, B = 2, L = 6000), recorded the way
make_golden.fsn_case records it.  A clip that never clips tests nothing, so the generator checks on the CPU, with the reference alone, that
every activation is exercised on both sides of its kinks and stores the fractions under g/meta/: where the formula weights do not reach a
kink, that head's fc_output_layer weight and bias are scaled by the factor stored in g/meta/{fb,sb}_head_scale (the tests apply the same
factor after fill_state_dict_).

    python tests/golden/make_fsn_knobs_golden.py
"""
import os

import numpy as np
import torch

import make_golden as mg
from make_golden import fill_state_dict_, flat, sample, test_signals

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (sb_num_neighbors, fb_num_neighbors, sequence_model, norm_type, fb act, sb act, hidden, fb head scale, sb head scale)
CASES = {
    "fb4": (15, 4, "LSTM", "offline_laplace_norm", "ReLU", None, (128, 64), 1.0, 1.0),
    "fb1_tanh": (15, 1, "LSTM", "offline_laplace_norm", "Tanh", "Tanh", (128, 64), 32.0, 32.0),
    "fb2_relu6_gru": (15, 2, "GRU", "cumulative_layer_norm", "ReLU6", "ReLU", (128, 64), 64.0, 1.0),
    "fb3_cumlaplace": (15, 3, "LSTM", "cumulative_laplace_norm", None, "ReLU6", (128, 64), 1.0, 256.0),
    "sb10_gauss": (10, 0, "LSTM", "offline_gaussian_norm", "ReLU", None, (128, 64), 1.0, 1.0),
    "default_fb4": (15, 4, "LSTM", "offline_laplace_norm", "ReLU", None, (512, 384), 1.0, 1.0),
}


def head_stats(act, pre):
    """Fractions of the head's pre-activations on each side of the activation's kinks, and how many sit within 1e-4 of one."""
    v = pre.detach().double().reshape(-1)
    st = dict(n=v.numel(), lt0=float((v < 0).double().mean()), gt6=float((v > 6).double().mean()),
              mid=float(((v > 0) & (v < 6)).double().mean()), abs_gt1=float((v.abs() > 1).double().mean()),
              near_kink=int(((v.abs() < 1e-4) | ((v - 6).abs() < 1e-4)).sum()) if act in ("ReLU", "ReLU6") else 0)
    if act == "ReLU6":
        ok = st["gt6"] >= 0.01 and st["lt0"] >= 0.01 and st["mid"] >= 0.01
    elif act == "ReLU":
        ok = st["lt0"] >= 0.05 and 1.0 - st["lt0"] >= 0.05
    elif act == "Tanh":
        ok = st["abs_gt1"] >= 0.01
    else:
        ok = True
    return st, ok


def knobs_case(cfg, models, tfm, name, B=2, L=6000):
    ns, nf, seq, norm, fb_act, sb_act, hidden, fb_scale, sb_scale = CASES[name]
    cfg.loss = "MSE"
    torch.manual_seed(0)
    m = models.FullSubNet(sb_num_neighbors=ns, fb_num_neighbors=nf, sequence_model=seq, fb_output_activate_function=fb_act,
                          sb_output_activate_function=sb_act, fb_model_hidden_size=hidden[0], sb_model_hidden_size=hidden[1], norm_type=norm)
    fill_state_dict_(m)
    with torch.no_grad():
        for net, s in ((m.fb_model, fb_scale), (m.sb_model, sb_scale)):
            net.fc_output_layer.weight.mul_(s)
            net.fc_output_layer.bias.mul_(s)
    m.train()
    m.fb_model.sequence_model.dropout = 0.0
    m.sb_model.sequence_model.dropout = 0.0
    pre = {}
    hooks = [net.fc_output_layer.register_forward_hook(lambda mod, i, o, k=k: pre.__setitem__(k, o.detach().clone()))
             for k, net in (("fb", m.fb_model), ("sb", m.sb_model))]
    x, y = test_signals(B, L)
    nc, cc = tfm.stft(x), tfm.stft(y)
    noisy_mag, _ = tfm.mag_phase(nc)
    cirm = tfm.build_complex_ideal_ratio_mask(nc, cc)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    crm = m(noisy_mag)
    lossv = m.loss(cirm, crm)
    opt.zero_grad()
    lossv.backward()
    for h in hooks:
        h.remove()
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    opt.step()
    sd = m.state_dict()
    meta = dict(B=B, L=L, fb_hidden=hidden[0], sb_hidden=hidden[1], sequence_model=seq, norm_type=norm, loss=np.array("MSE"),
                sb_num_neighbors=ns, fb_num_neighbors=nf, fb_act=np.array(str(fb_act)), sb_act=np.array(str(sb_act)),
                fb_head_scale=fb_scale, sb_head_scale=sb_scale)
    for k, act in (("fb", fb_act), ("sb", sb_act)):
        st, ok = head_stats(act, pre[k])
        print(f"  {k} head ({act}): " + ", ".join(f"{a} {b:.4g}" for a, b in st.items()))
        if not ok:
            raise SystemExit(f"fsn_knobs_{name}: the {k} head's {act} is not exercised on every side of its kinks: {st}")
        meta[k + "_pre"] = st
    small = lambda k: "bias" in k or k.startswith("sb_model.fc_output_layer")
    rec = dict(meta=meta, noisy_mag=noisy_mag.numpy()[:, ::4, ::3], cirm=cirm.numpy()[:, ::4, ::3], crm=crm.detach().numpy(), loss=float(lossv),
               grad_norm={k: float(v.double().norm()) for k, v in g.items()},
               grad={k: v.numpy() for k, v in g.items() if small(k)},
               grad_samp={k: sample(v, 211)["samp"] for k, v in g.items() if not small(k)},
               after_adam={k: sd[k].numpy().copy() for k in g if small(k)})
    np.savez_compressed(os.path.join(HERE, f"fsn_knobs_{name}.npz"), **flat(rec, "g"))
    print(f"fsn_knobs_{name}: loss {float(lossv):.6f}")


def main():
    import sys
    cfg, models, tfm, _ = mg.import_reference()
    torch.set_num_threads(4)
    for name in (sys.argv[1:] or CASES):
        knobs_case(cfg, models, tfm, name)


if __name__ == "__main__":
    main()
