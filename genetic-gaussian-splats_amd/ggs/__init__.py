"""ggs — MI355X-native 2D Gaussian-splat render + fitness (host side).

Plain Python + numpy over libggs.so (hand-written HIP for gfx950, C ABI in
include/ggs.h).  The drop-in modules with the reference's names live in
``modules/`` next to this package.
"""
from ._lib import (GGS_FIT_BOOST, GGS_FIT_NONE, GGS_FIT_WEIGHTED, GGS_LAYOUT_AXES,  # noqa: F401
                   GGS_LAYOUT_RENDERER, GGSDeviceError, GGSError, GGSInputError, LIB_PATH, ensure_init, lib,
                   runtime_info, select_devices)
from .parallel import RcclGather  # noqa: F401
from .api import (LossParams, TargetPlan, TargetPlanSet, as_f32, density_relocate, encode, fitness,  # noqa: F401
                  fitness_device,
                  fitness_grad, fitness_grad_device, fitness_population, image_loss, image_loss_device,
                  loss_grad, loss_grad_device, preprocess, profile_enable, profile_read, profile_reset, render,
                  render_device, render_layout_device, render_vjp, render_vjp_device, seed_sites)
from .de import differential_evolution  # noqa: F401
from .refine import DensityParams  # noqa: F401
from .seed import SeedParams, SeedRound, seed_genomes, seed_schedule, seeded_population  # noqa: F401

__version__ = "0.1.0"
