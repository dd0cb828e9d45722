"""Shared by tests/test_seqmodel_cpu.py and tests/test_gpu_seqmodel.py: the SequenceModel cases of tests/golden/make_seqmodel_golden.py, the formula
weights keyed like torch's state_dict, and the comparison against a golden at the project's bars."""
import numpy as np
import torch

from oracle.weights import formula_state_dict
from util import rel_err, rel_l2, sub

# name: (sequence_model, I, O, H, num_layers, bidirectional, activation, B, T)
CASES = {
    "lstm_l3_bi": ("LSTM", 21, 5, 64, 3, True, "Tanh", 3, 9),
    "gru_l3_bi": ("GRU", 21, 5, 64, 3, True, "ReLU6", 3, 9),
    "lstm_l1_uni": ("LSTM", 21, 5, 64, 1, False, None, 3, 9),
    "gru_l4_uni": ("GRU", 21, 5, 64, 4, False, "ReLU", 3, 9),
    "lstm_h192_l3_bi": ("LSTM", 21, 5, 192, 3, True, "Tanh", 18, 10),
    "lstm_h256_l2_bi": ("LSTM", 21, 5, 256, 2, True, None, 18, 11),
}
ACTS = {None: lambda v: v, "None": lambda v: v, "Tanh": torch.tanh, "ReLU": torch.relu, "ReLU6": torch.nn.functional.relu6}
STRIDE = 211          # make_seqmodel_golden.py: sample(v, 211)


def torch_shapes(seq, I, O, H, NL, bi):
    """{state_dict name: shape} of the reference's SequenceModel: torch's own nn.LSTM / nn.GRU state_dict, then fc_output_layer."""
    rnn = (torch.nn.LSTM if seq == "LSTM" else torch.nn.GRU)(I, H, NL, batch_first=True, bidirectional=bi)
    shapes = {"sequence_model." + k: tuple(v.shape) for k, v in rnn.state_dict().items()}
    shapes["fc_output_layer.weight"] = (O, H * (2 if bi else 1))
    shapes["fc_output_layer.bias"] = (O,)
    return shapes


def seq_dict(seq, I, O, H, NL, bi, keep=1.0):
    return dict(input_size=I, output_size=O, hidden_size=H, num_layers=NL, bidirectional=bi, sequence_model=seq, keep=keep)


def formula_params(shapes, head_scale=1.0):
    P = formula_state_dict(shapes)
    for leaf in ("weight", "bias"):
        P["fc_output_layer." + leaf] = P["fc_output_layer." + leaf] * head_scale
    return P


def time_major(x):
    """[B, I, T] -> the plan's io.x [T, B, roundup(I, 8)] with zero pad columns."""
    xt = x.permute(2, 0, 1)
    pad = -xt.shape[2] % 8
    return torch.nn.functional.pad(xt, (0, pad)).contiguous() if pad else xt.contiguous()


def golden_errors(g, y, loss, dx, grads):
    """Every figure the bars apply to: dict(y, y_l2, dx, loss, norm={k: rel}, grad={k: rel_l2 of the stored or sampled gradient})."""
    e = dict(y=rel_err(y, g["g/y"]), y_l2=rel_l2(y, g["g/y"]), dx=rel_err(dx, g["g/dx"]),
             loss=abs(float(loss) - float(g["g/loss"])) / abs(float(g["g/loss"])), norm={}, grad={})
    for k, v in sub(g, "g/grad_norm").items():
        e["norm"][k] = abs(float(grads[k].double().norm()) - float(v)) / float(v)
    for k, v in sub(g, "g/grad").items():
        e["grad"][k] = rel_l2(grads[k], v)
    for k, v in sub(g, "g/grad_samp").items():
        e["grad"][k] = rel_l2(grads[k].reshape(-1)[::STRIDE], v)
    return e


def assert_fp32(e, tol):
    assert e["y"] < tol and e["dx"] < tol and e["loss"] < tol, e
    for k, v in e["norm"].items():
        assert v < tol, ("grad_norm", k, v)
    for k, v in e["grad"].items():
        assert v < tol, ("grad", k, v)


def torch_reference(seq, I, O, H, NL, bi, act, P, x, tgt):
    """The restatement for shapes without a golden: torch's own nn.LSTM / nn.GRU + Linear in fp64 on the CPU with the same weights.
    Returns (y, loss, dx, {name: grad}) for loss = mean((y - tgt)^2)."""
    rnn = (torch.nn.LSTM if seq == "LSTM" else torch.nn.GRU)(I, H, NL, batch_first=True, bidirectional=bi).double()
    fc = torch.nn.Linear(H * (2 if bi else 1), O).double()
    rnn.load_state_dict({k[len("sequence_model."):]: v.double() for k, v in P.items() if k.startswith("sequence_model.")})
    fc.load_state_dict({"weight": P["fc_output_layer.weight"].double(), "bias": P["fc_output_layer.bias"].double()})
    xd = x.detach().cpu().double().requires_grad_(True)
    y = ACTS[act](fc(rnn(xd.permute(0, 2, 1))[0])).permute(0, 2, 1)
    loss = ((y - tgt.cpu().double()) ** 2).mean()
    loss.backward()
    grads = {"sequence_model." + k: p.grad for k, p in rnn.named_parameters()}
    grads.update({"fc_output_layer." + k: p.grad for k, p in fc.named_parameters()})
    return y.detach(), float(loss.detach()), xd.grad, grads
