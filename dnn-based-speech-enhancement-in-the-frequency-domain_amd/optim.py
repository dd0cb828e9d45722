"""Fused Adam / AdamW over the model's flat parameter buffer (torch.optim.Adam defaults: train_interface.py:59).

`Adam(model.parameters(), lr)` keeps the reference's construction line working; `step()` updates every parameter
with ONE kernel launch on the flat fp32 arena (`sefd_adam_step`), and exposes `state_dict()/load_state_dict()` in
torch.optim.Adam's format so reference checkpoints ({'model','optimizer','epoch'}) interchange.

Anything beyond that one configuration - weight decay (L2, or decoupled in `AdamW`), amsgrad, several parameter groups with their own
hyper-parameters (`model.get_params(weight_decay)`, models.py:289), an optimizer over a subset of the parameters (the others are frozen) and
global-norm clipping (`max_grad_norm`) - goes through `sefd_grad_norm` + `sefd_optim_step` (csrc/optim.hip): still one update launch for all
groups, over a chunk table built once at bind time, with the hyper-parameters read from `param_groups` at every step (schedulers work).

Life cycle (the reference's resume order works unchanged, train_interface.py:52-59, 101-116): the optimizer finds the model
that owns its parameters by itself (the sefd models tag their parameters), flattens it if that has not happened yet, and a
`load_state_dict` that arrives before the model is on the GPU is kept and applied at bind time."""
import ctypes as C

import numpy as np
import torch

from . import _lib

CHUNK = 1024             # SEFD_OPTIM_CHUNK
MAX_GROUPS = 8           # SEFD_OPTIM_MAX_GROUPS
_CHUNK_DTYPE = np.dtype([("begin", "<i8"), ("count", "<i4"), ("group", "<i4")])          # sefd_optim_chunk


class _Group(C.Structure):
    """Mirror of `sefd_optim_group` (include/sefd.h)."""
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("flags", C.c_uint32)]


def chunk_table(segments):
    """The chunk table of include/sefd.h for `segments` = [(begin, count, group), ...] (one per parameter tensor): every segment cut into chunks
    of at most CHUNK elements, sorted by begin.  A numpy array of `sefd_optim_chunk`."""
    parts = []
    for begin, count, group in segments:
        b = begin + np.arange(0, count, CHUNK, dtype=np.int64)
        t = np.empty(len(b), dtype=_CHUNK_DTYPE)
        t["begin"], t["count"], t["group"] = b, np.minimum(CHUNK, begin + count - b), group
        parts.append(t)
    tab = np.concatenate(parts) if parts else np.empty(0, dtype=_CHUNK_DTYPE)
    return np.ascontiguousarray(tab[np.argsort(tab["begin"], kind="stable")])


def table_to_device(tab, device="cuda"):
    return torch.from_numpy(tab.view(np.int64).reshape(-1, 2).copy()).to(device)


class Adam(torch.optim.Optimizer):
    _decoupled = False               # AdamW: weight decay acts on the parameter, not on the gradient
    _torch_class = torch.optim.Adam

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None):
        self._check_hyper(dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"sefd_amd.optim: at most {MAX_GROUPS} parameter groups (got {len(self.param_groups)})")
        for g in self.param_groups:
            self._check_hyper(g)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None   # with max_grad_norm: 0-d device tensor, the norm of the last step's gradient before clipping (rewritten by every step)
        self._model = None
        self._index = None           # per group, its parameters' positions in the model's flat order (bind)
        self._m = self._v = self._vmax = None
        self._step = 0
        self._pending = None         # a state_dict loaded before the model could be bound
        self.grad_scale = 1.0        # DDP: 1/world_size applied inside the kernel

    @staticmethod
    def _check_hyper(g):
        """torch.optim.Adam's argument checks."""
        if not 0.0 <= g["lr"]:
            raise ValueError(f"Invalid learning rate: {g['lr']}")
        if not 0.0 <= g["eps"]:
            raise ValueError(f"Invalid epsilon value: {g['eps']}")
        if not 0.0 <= g["betas"][0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {g['betas'][0]}")
        if not 0.0 <= g["betas"][1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {g['betas'][1]}")
        if not 0.0 <= g["weight_decay"]:
            raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")

    # ---- binding
    def _owner(self):
        for grp in self.param_groups:
            for p in grp["params"]:
                ref = getattr(p, "_sefd_owner", None)
                if ref is not None and ref() is not None:
                    return ref()
        return None

    def _map(self, model):
        """Per group, the indices of its parameters in the model's flat order.  A parameter of another model (or of none) is refused."""
        index = {id(p): i for i, (_, p) in enumerate(model._trainable())}
        out = []
        for grp in self.param_groups:
            for p in grp["params"]:
                if id(p) not in index:
                    raise ValueError("sefd_amd.optim: a parameter of this optimizer does not belong to the model it is bound to")
            out.append([index[id(p)] for p in grp["params"]])
        return out

    def bind(self, model=None):
        """Attach to the sefd model whose parameters are views of one flat buffer.  Called lazily by `train_step`, `step` and
        `load_state_dict`; flattens the model first if no forward has done so yet."""
        model = model if model is not None else (self._model if self._model is not None else self._owner())
        if model is None:
            raise RuntimeError("sefd_amd.optim.Adam: the parameters do not belong to a sefd_amd model")
        if self._model is not model or self._index is None:
            self._index = self._map(model)       # refuses a foreign parameter, wherever the model is
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("sefd_amd.optim.Adam: move the model to the GPU first (model.to(DEVICE)); there is no CPU path")
        if not model._flat_ok(dev):
            model._flatten(dev)
        if self._model is model and self._m is not None and self._m.device == model._flat_param.device \
                and self._m.numel() == model._flat_param.numel():
            return
        self._model = model
        index = self._index
        self._m = torch.zeros_like(model._flat_param)
        self._v = torch.zeros_like(model._flat_param)
        self._vmax = None
        # one group that holds every parameter in the model's order: what sefd_adam_step_guarded_dp updates (with no decay, amsgrad or clipping)
        self._covers_all = len(index) == 1 and index[0] == list(range(len(model._param_slices)))
        segs = [(model._param_slices[i][0], model._param_slices[i][1], gi) for gi, idx in enumerate(index) for i in idx]
        self._table_host = chunk_table([s for s in segs if s[1] > 0])
        self._table_dev = table_to_device(self._table_host, dev)
        self._norm_ws = torch.zeros(_lib.lib().sefd_grad_norm_ws_floats(model._flat_param.numel()) // 2, dtype=torch.float64, device=dev)
        self._norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
        if self._pending is not None:
            sd, self._pending = self._pending, None
            self._apply_state(sd)

    def _need_vmax(self):
        if self._vmax is None:
            self._vmax = torch.zeros_like(self._m)
        return self._vmax

    def _legacy(self):
        g = self.param_groups[0]
        return self._covers_all and g["weight_decay"] == 0 and not g["amsgrad"] and self.max_grad_norm is None

    def step_flat(self, grad=None):
        m = self._model
        g = m._flat_grad if grad is None else grad
        self._step += 1
        # guarded by the status word of the plan that produced the gradient: a kernel of that plan that gave up (cluster LSTM hand-over
        # timeout) set it earlier on this stream, and the update is then skipped on the device - no garbage step, no host sync here
        plan = getattr(m, "_status_plan", None)
        guard = plan.status_word() if plan is not None else None
        # data parallel (train_step sets nan_guard to the poisoned element of the last all-reduced bucket): EVERY rank skips a step that any
        # rank's plan gave up on - the replicas stay identical (Plan.status_poison)
        nan_guard, self.nan_guard = getattr(self, "nan_guard", None), None
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if self._legacy():
            grp = self.param_groups[0]
            rc = L.sefd_adam_step_guarded_dp(C.c_void_p(m._flat_param.data_ptr()), C.c_void_p(g.data_ptr()),
                                             C.c_void_p(self._m.data_ptr()), C.c_void_p(self._v.data_ptr()),
                                             m._flat_param.numel(), self._step, grp["lr"], grp["betas"][0], grp["betas"][1],
                                             grp["eps"], self.grad_scale, C.c_void_p(guard) if guard else None,
                                             C.c_void_p(nan_guard.data_ptr()) if nan_guard is not None else None, stream)
            if rc != 0:
                raise RuntimeError(f"sefd_adam_step_guarded_dp failed ({rc})")
            return
        # every other configuration: [norm of the owned gradient -> clip coefficient, both left on the device] -> one update launch over the chunk table
        hyper = (_Group * MAX_GROUPS)()
        for i, grp in enumerate(self.param_groups):
            self._check_hyper(grp)
            flags = (1 if self._decoupled else 0) | (2 if grp["amsgrad"] else 0)
            hyper[i] = _Group(grp["lr"], grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], flags)
            if grp["amsgrad"]:
                self._need_vmax()
        n, nchunks = m._flat_param.numel(), len(self._table_host)
        table_host, table_dev = C.c_void_p(self._table_host.ctypes.data), vp(self._table_dev)
        coef = None
        if self.max_grad_norm is not None:
            # after the DDP all-reduce, of grad * grad_scale: every rank computes the same norm and clips alike
            rc = L.sefd_grad_norm(vp(g), n, self.grad_scale, self.max_grad_norm, table_host, table_dev, nchunks, vp(self._norm_ws),
                                  vp(self._norm_out), stream)
            if rc != 0:
                raise RuntimeError(f"sefd_grad_norm failed ({rc})")
            self.last_grad_norm = self._norm_out[0]
            coef = C.c_void_p(self._norm_out.data_ptr() + 4)
        rc = L.sefd_optim_step(vp(m._flat_param), vp(g), vp(self._m), vp(self._v), vp(self._vmax), n, self._step, hyper, len(self.param_groups),
                               table_host, table_dev, nchunks, self.grad_scale, coef, C.c_void_p(guard) if guard else None, vp(nan_guard), stream)
        if rc != 0:
            raise RuntimeError(f"sefd_optim_step failed ({rc})")

    def _owned(self):
        """(parameter, (offset, numel, shape)) of every parameter of every group, in group order (torch's state index order)."""
        sl = self._model._param_slices
        return [(p, sl[i]) for grp, idx in zip(self.param_groups, self._index) for p, i in zip(grp["params"], idx)]

    @torch.no_grad()
    def step(self, closure=None):
        """Generic path (after `loss.backward()`): gathers p.grad into the flat gradient buffer, then the fused kernel.
        A parameter whose `.grad` is None is left untouched (value and moments), as torch.optim.Adam does."""
        self.bind()
        m = self._model
        state = [self._m, self._v] + ([self._vmax] if self._vmax is not None else [])
        skipped = []
        for p, (off, n, _) in self._owned():
            if p.grad is not None:
                m._flat_grad[off:off + n].copy_(p.grad.reshape(-1))
            else:
                m._flat_grad[off:off + n].zero_()
                skipped.append((off, n, [t[off:off + n].clone() for t in [m._flat_param] + state]))
        self.step_flat()
        for off, n, saved in skipped:
            for t, s in zip([m._flat_param] + state, saved):
                t[off:off + n].copy_(s)

    # ---- torch.optim.Adam compatible checkpoint format
    def state_dict(self):
        # every param_group carries every key of the installed torch.optim.Adam's (AdamW's) defaults (maximize, foreach, ...) so
        # that the checkpoint also loads into the reference's optimizer class (train_interface.py:59, 110); `params` indices run in group
        # order, as torch's do, and state[i] belongs to that index
        tmpl = dict(self._torch_class([torch.nn.Parameter(torch.zeros(1))]).defaults)
        sd = {"state": {}, "param_groups": []}
        start = 0
        for grp in self.param_groups:
            k = len(grp["params"])
            sd["param_groups"].append({**tmpl, **{key: v for key, v in grp.items() if key != "params"}, "params": list(range(start, start + k))})
            start += k
        if self._pending is not None and self._m is None:
            return self._pending
        if self._m is not None and self._step > 0:
            ams = [bool(grp["amsgrad"]) for grp in self.param_groups for _ in grp["params"]]
            for i, (_, (off, n, shape)) in enumerate(self._owned()):
                sd["state"][i] = {"step": torch.tensor(float(self._step)), "exp_avg": self._m[off:off + n].view(shape).clone(),
                                  "exp_avg_sq": self._v[off:off + n].view(shape).clone()}
                if ams[i]:
                    sd["state"][i]["max_exp_avg_sq"] = self._need_vmax()[off:off + n].view(shape).clone()
        return sd

    def _apply_state(self, sd):
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(a["params"]) != len(b["params"]) for a, b in zip(sd["param_groups"], self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        if not sd["state"]:              # a checkpoint taken before the first step: back to a fresh optimizer
            self._m.zero_(); self._v.zero_(); self._step = 0
            if self._vmax is not None:
                self._vmax.zero_()
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        for i, (_, (off, n, shape)) in zip(ids, self._owned()):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None:
                continue
            self._m[off:off + n].copy_(st["exp_avg"].reshape(-1))
            self._v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            if "max_exp_avg_sq" in st:
                self._need_vmax()[off:off + n].copy_(st["max_exp_avg_sq"].reshape(-1))
            self._step = int(float(st["step"]))
        for g, mine in zip(sd["param_groups"], self.param_groups):
            for k in ("lr", "betas", "eps", "weight_decay", "amsgrad"):
                if k in g:
                    mine[k] = tuple(g[k]) if k == "betas" else g[k]

    def load_state_dict(self, sd):
        """train_interface.py:110: `optimizer.load_state_dict(checkpoint['optimizer'])` right after construction."""
        model = self._model if self._model is not None else self._owner()
        if model is not None and next(model.parameters()).device.type != "cuda":
            self._pending = sd           # model not on the GPU yet (the one deferrable case): applied by the first bind
            return
        self.bind()                      # anything else that fails here (foreign parameters, allocation, ...) is a failed resume: raise
        self._apply_state(sd)


class AdamW(Adam):
    """Adam with decoupled weight decay (torch.optim.AdamW): p *= 1 - lr * weight_decay in front of the update, default weight_decay 1e-2."""
    _decoupled = True
    _torch_class = torch.optim.AdamW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, max_grad_norm=max_grad_norm)
