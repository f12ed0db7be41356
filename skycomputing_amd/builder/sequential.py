"""Tuple-splatting sequential container.

Capability parity with the reference's SequentialWrapper
(reference: scaelum/builder/sequential_wrapper.py:8-20): a tuple/list output
of layer i is splatted into layer i+1's ``forward(*args)`` — required because
the BERT pipeline layers pass (hidden, mask, ...) tuples.

Pairing protocol: a module may offer to run itself AND its successor as one
call. It does so with a method ``fuse_with_next(next_module)`` that returns
either None or a callable taking the module's own inputs and returning what
``next_module(*module(*inputs))`` returns. The wrapper asks only when the
successor is the next module of this same wrapper and neither module has
hooks registered (a fused call enters neither module's ``__call__``, so
their hooks would not fire); otherwise, and when the offer is None, the two
modules run one after the other as before. Both stay ordinary submodules:
parameters, state-dict keys and their order do not depend on the pairing.
"""

from __future__ import annotations

import torch.nn as nn
import torch.nn.modules.module as _nnm

_HOOK_DICTS = ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks",
               "_backward_pre_hooks")
_GLOBAL_HOOK_DICTS = ("_global_forward_hooks", "_global_forward_pre_hooks",
                      "_global_backward_hooks", "_global_backward_pre_hooks")


def _has_hooks(module: nn.Module) -> bool:
    return (any(getattr(module, d, None) for d in _HOOK_DICTS)
            or any(getattr(_nnm, d, None) for d in _GLOBAL_HOOK_DICTS))


def _call(fn, out):
    if isinstance(out, (tuple, list)):
        return fn(*out)
    return fn(out)


class SequentialWrapper(nn.Sequential):
    def forward(self, *inputs):
        out = inputs
        modules = list(self)
        i = 0
        while i < len(modules):
            module = modules[i]
            fused = None
            offer = getattr(module, "fuse_with_next", None)
            if offer is not None and i + 1 < len(modules):
                nxt = modules[i + 1]
                if not (_has_hooks(module) or _has_hooks(nxt)):
                    fused = offer(nxt)
            if fused is not None:
                out = _call(fused, out)
                i += 2
            else:
                out = _call(module, out)
                i += 1
        return out
