"""A plan together with its device arenas: what every HIP-backed module caches per shape and runs on the current stream."""
import weakref

import torch


class Runtime:
    """`rt.plan`, `rt.arenas`, or `plan, arenas = rt`.  `stamp` counts the forwards whose activations went into the workspace arena (models._PlanFunction)."""

    def __init__(self, plan, arenas):
        self.plan, self.arenas, self.stamp = plan, arenas, 0

    @classmethod
    def owned(cls, plan, device):
        """A parameter-free plan: every arena is the runtime's own."""
        return cls(plan, plan.alloc_arenas(device))

    @classmethod
    def bound(cls, plan, owner, device):
        """PARAM / GRAD / STATE are the flat tensors of `owner` (a models._SefdModule, flattened on `device`); the plan's parameter table must agree
        with the module tree (names, order, offsets)."""
        plan.owner = weakref.ref(owner)            # running it makes it this model's `_status_plan` (guarded Adam, checkpoint check)
        assert [n for n, _ in owner._trainable()] == list(plan.params.keys()), "parameter order differs from the plan"
        assert [s[0] for s in owner._param_slices] == [v[0] for v in plan.params.values()], "parameter offsets differ from the plan"
        return cls(plan, plan.alloc_arenas(device, flat=(owner._flat_param, owner._flat_grad, owner._flat_state)))

    def __getitem__(self, i):                      # indexing and unpacking, as the (plan, arenas) pair
        return (self.plan, self.arenas)[i]

    def io(self, name, shape):
        return self.plan.io(self.arenas, name, shape)

    def view(self, name):
        return self.plan.view(self.arenas, name)

    def run(self, phase):
        self.plan.run(phase, self.arenas, torch.cuda.current_stream().cuda_stream)


def cached(cache, key, make):
    """cache[key], made by `make()` on first use."""
    rt = cache.get(key)
    if rt is None:
        rt = cache[key] = make()
    return rt
