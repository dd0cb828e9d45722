"""CPU: the optimizer's reference formulas against torch's own optimizers, the torch-format state dict of a grouped optimizer, and the refusals."""
import pytest
import torch

from optim_ref import clip_coef, grad_norm, optim_update


def _small_model():
    import sefd_amd  # noqa: F401
    from sefd_amd import config as cfg, models
    cfg.dccrn_kernel_num = [16, 32, 32, 64, 64, 64]
    return models.DCCRN(rnn_units=128)


@pytest.mark.parametrize("cls,decoupled", [(torch.optim.Adam, False), (torch.optim.AdamW, True)])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_reference_update_is_torchs(cls, decoupled, amsgrad):
    """Three fp64 steps with weight_decay 1e-2: optim_ref.optim_update against torch.optim.Adam / AdamW (agreement 1.5e-17 to 7e-17 measured)."""
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(300, generator=gen, dtype=torch.float64)
    grads = [torch.randn(300, generator=gen, dtype=torch.float64) * s for s in (1e-2, 5e-3, 2e-2)]
    q = torch.nn.Parameter(p0.clone())
    opt = cls([q], lr=1e-3, weight_decay=1e-2, amsgrad=amsgrad)
    p, m, v, vmax = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0)
    for k, g in enumerate(grads):
        q.grad = g.clone()
        opt.step()
        p, m, v, vmax = optim_update(p, g, m, v, vmax, k + 1, weight_decay=1e-2, decoupled=decoupled, amsgrad=amsgrad)
    st = opt.state[q]
    pairs = [(p, q.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])] + ([(vmax, st["max_exp_avg_sq"])] if amsgrad else [])
    for mine, theirs in pairs:
        assert float((mine - theirs).abs().max()) < 1e-12


def test_reference_clip_coefficient_is_clip_grad_norm():
    gen = torch.Generator().manual_seed(6)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64)) for n in (7, 130)]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    gs = [p.grad.clone() for p in ps]
    norm = grad_norm(gs)
    for max_norm in (0.5 * float(norm), 2.0 * float(norm)):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(float(total) - float(norm)) < 1e-12
        c = clip_coef(float(norm), max_norm)
        assert (max_norm > float(norm)) == (c == 1.0)
        for p, g in zip(ps, gs):
            assert float((p.grad - g * c).abs().max()) < 1e-12


def test_grouped_state_dict_is_torchs_format():
    """get_params' two groups: `params` indices run in group order (weights, then biases), each group carries its own weight_decay and amsgrad, and the
    dict loads into torch.optim.Adam over the same groups."""
    from sefd_amd.optim import Adam
    m = _small_model()
    groups = m.get_params(1e-5)
    n_w, n_all = len(groups[0]["params"]), len(list(m.parameters()))
    assert 0 < n_w < n_all
    sd = Adam(m.get_params(1e-5), amsgrad=True).state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 2
    assert sd["param_groups"][0]["params"] == list(range(n_w)) and sd["param_groups"][1]["params"] == list(range(n_w, n_all))
    assert sd["param_groups"][0]["weight_decay"] == 1e-5 and sd["param_groups"][1]["weight_decay"] == 0.0
    assert sd["param_groups"][0]["amsgrad"] is True and sd["param_groups"][1]["amsgrad"] is True
    ref = torch.optim.Adam(m.get_params(1e-5), amsgrad=True)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["weight_decay"] == 1e-5 and ref.param_groups[1]["weight_decay"] == 0.0 and ref.param_groups[1]["amsgrad"] is True
    # and back: torch's state after a step, kept until the model is on the GPU, keeps both groups and the amsgrad moment
    for p in m.parameters():
        p.grad = torch.full_like(p, 0.01)
    ref.step()
    opt = Adam(m.get_params(1e-5), amsgrad=True)
    opt.load_state_dict(ref.state_dict())
    back = opt.state_dict()
    assert opt._pending is not None and len(back["param_groups"]) == 2 and "max_exp_avg_sq" in back["state"][n_all - 1]


def test_default_state_dict_is_unchanged():
    from sefd_amd.optim import Adam, AdamW
    m = _small_model()
    sd = Adam(m.parameters(), lr=1e-3).state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1
    g = sd["param_groups"][0]
    assert g["params"] == list(range(len(list(m.parameters())))) and g["lr"] == 1e-3 and g["weight_decay"] == 0 and g["amsgrad"] is False
    want = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3).state_dict()["param_groups"][0], params=g["params"])
    assert g == want
    gw = AdamW(m.parameters()).state_dict()["param_groups"][0]
    assert gw["weight_decay"] == 1e-2
    assert gw == dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0], params=g["params"])


def test_refusals():
    from sefd_amd.optim import Adam, AdamW
    m = _small_model()
    ps = list(m.parameters())
    for kw in (dict(weight_decay=-1e-3), dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1))):
        for cls in (Adam, AdamW):
            with pytest.raises(ValueError):
                cls(ps, **kw)
    with pytest.raises(ValueError):
        Adam([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": -0.5}])
    assert len(Adam([{"params": [p]} for p in ps[:8]]).param_groups) == 8
    with pytest.raises(ValueError):
        Adam([{"params": [p]} for p in ps[:9]])
    with pytest.raises(ValueError):
        Adam([{"params": ps[:3]}, {"params": ps[2:]}])                 # a parameter in two groups: torch's own error
    other = _small_model()
    with pytest.raises(ValueError):
        Adam(ps + [next(other.parameters())]).bind()                   # a parameter of another model, refused wherever the model is
    with pytest.raises(ValueError):
        Adam(ps + [torch.nn.Parameter(torch.zeros(3))]).bind()         # ... or of none
    with pytest.raises(RuntimeError):
        Adam(ps).bind()                                                # its own parameters: only the missing GPU is in the way


def test_chunk_table_layout():
    """No chunk crosses a segment, none is longer than the chunk size, frozen ranges are absent, sorted by begin."""
    from sefd_amd.optim import CHUNK, chunk_table
    segs = [(5000, 1, 1), (0, 3, 0), (3, 2 * CHUNK + 5, 2), (9000, CHUNK, 0)]
    tab = chunk_table(segs)
    assert tab.dtype.itemsize == 16 and list(tab["begin"]) == sorted(tab["begin"])
    covered = {}
    for b, c, g in zip(tab["begin"], tab["count"], tab["group"]):
        assert 1 <= c <= CHUNK
        seg = [s for s in segs if s[0] <= b and b + c <= s[0] + s[1]]
        assert len(seg) == 1 and seg[0][2] == g
        for i in range(b, b + c):
            assert i not in covered
            covered[i] = g
    assert len(covered) == sum(s[1] for s in segs) and 4000 not in covered
