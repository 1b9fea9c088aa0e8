"""Env wrappers (reference ``fluidgym/wrappers``): observation extraction and flattening in plain torch, sensor and action noise from
a per-row counter-based generator on the GPU (``noise.py``), running normalisation of observations and rewards
on the GPU (``normalize.py``).  They wrap a ``FluidEnv`` (un-batched or batched),
a ``ParallelFluidEnv`` or each other."""
from .flatten_obs import FlattenObservation
from .fluid_wrapper import FluidWrapper
from .noise import ActionNoise, SensorNoise
from .normalize import NormalizeObservation, NormalizeReward
from .obs_extraction import ObsExtraction

__all__ = ["FluidWrapper", "ObsExtraction", "FlattenObservation", "ActionNoise", "SensorNoise", "NormalizeObservation", "NormalizeReward"]
