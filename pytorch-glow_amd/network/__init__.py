"""Flow layers and models (host-side mirror of the reference's ``network`` package for the flow hot path), plus the two
callers either side of it: `Builder` (model / optimiser / schedule / snapshot glue), `Trainer` (the reference's training loop
around `training.TrainLoop`) and `Inferer` (the inverse-path application) -- the names ``network/__init__.py:1-16`` exports."""
from . import model as _model
from . import module as _module
from .builder import Builder
from .evaluate import EvalResult, Evaluator
from .inferer import Inferer
from .latents import Latents
from .posterior import LatentMALA, PosteriorInfo
from .restore import (COILS_MAX, LatentFit, PsfFit, RestoreInfo, check_coil_maps, check_fourier_shape, coil_maps, coils2d, coils2d_adjoint,
                      coils_scratch, fourier2d, fourier2d_adjoint, fourier_mask, fourier_scratch, gaussian_operator, psf_from_logits,
                      psf_gradient, restore_objective)
from .trainer import Trainer

_LAYERS = ("ActNorm", "LinearZeros", "Conv2d", "Conv2dZeros", "CouplingNet", "f", "Invertible1x1Conv", "Invertible1x1ConvLU",
           "Permutation2d", "GaussianDiag", "Split2d", "Squeeze2d")
_MODELS = ("FlowStep", "FlowModel", "Glow")

for _n in _LAYERS:
    globals()[_n] = getattr(_module, _n)
for _n in _MODELS:
    globals()[_n] = getattr(_model, _n)

__all__ = _MODELS + _LAYERS + ("Builder", "Trainer", "Inferer", "Evaluator", "EvalResult", "Latents", "LatentMALA", "PosteriorInfo", "LatentFit", "RestoreInfo", "restore_objective", "gaussian_operator",
                               "PsfFit", "psf_from_logits", "psf_gradient", "fourier2d", "fourier2d_adjoint", "fourier_mask", "fourier_scratch",
                               "check_fourier_shape", "COILS_MAX", "check_coil_maps", "coil_maps", "coils2d", "coils2d_adjoint", "coils_scratch")
