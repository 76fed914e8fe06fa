"""The ``backend="torch" | "hip"`` switch of the predictor classes."""
import importlib

import torch

_HIP = {}        # the *_hip modules imported so far: importlib.import_module on every forward costs more than the statement it replaces


def check(model_name, backend):
    if backend not in ("torch", "hip"):
        raise ValueError("%s backend must be 'torch' or 'hip', got %r" % (model_name, backend))
    return backend


def hip_forward(model, hip_module, x, **extra):
    """-> the output of ``<hip_module>.forward`` where ``model.backend`` is "hip" and that module (imported here, on first use) serves the
    call; None where the caller's torch path has to.  Records which in ``model.backend_used``.  Outside train mode, or with gradients
    disabled, the HIP path runs under ``no_grad`` and keeps nothing for a backward.  ``extra`` is handed to that forward as it is (ST-WA: the noise)."""
    if model.backend == "hip":
        hip = _HIP.get(hip_module)
        if hip is None:
            hip = _HIP[hip_module] = importlib.import_module("." + hip_module, __package__)
        if hip.supported(model, x):
            model.backend_used = "hip"
            if model.training and torch.is_grad_enabled():
                return hip.forward(model, x, keep=True, **extra)
            with torch.no_grad():
                return hip.forward(model, x, keep=False, **extra)
    model.backend_used = "torch"
    return None
