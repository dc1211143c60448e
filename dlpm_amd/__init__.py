"""dlpm_amd -- MI355X-native (gfx950) implementation of DLPM's reverse-time sampling loop.

Host-side mirror of the reference's entry points over libdlpm_amd.so (include/dlpm_amd.h):

    GenerationManager(method, dataloader, is_image, **eval_kwargs).generate(models, nsamples)
    GenerativeLevyProcess(alpha, device, reverse_steps, ...).sample(models, shape, reverse_steps, ...)
    UNetModel(...) / MLPModel(p)   with   model(x, t) -> eps

See DESIGN.md for the scope and INTEGRATION.md for the binding.
"""
from .method import GenerativeLevyProcess, ReferenceStreams, init_method_by_parameter  # noqa: F401
from .process import DLPM  # noqa: F401
from .unet import UNetModel, unet_from_config  # noqa: F401
from .mlp import MLPModel  # noqa: F401
from .generation import GenerationManager, ShapeProbe  # noqa: F401
from .evaluation import EvaluationManager, ImageDump  # noqa: F401
from .metrics import mmd, MMD_loss, kmeans, prd  # noqa: F401
from .metrics import compute_prd_from_embedding, compute_precision_recall_curve, prd_to_max_f_beta_pair, compute_f_beta  # noqa: F401
from .metrics import wass, wass_device, compute_wasserstein_distance  # noqa: F401
from .metrics import w1, w1_device, compute_w1_distance  # noqa: F401
from .metrics import tail, tail_device, msle, hill_index  # noqa: F401
from .metrics import prdc, prdc_device, compute_prdc  # noqa: F401
from .metrics import fd, fd_device, feature_statistics, calculate_frechet_distance  # noqa: F401
from .weights import rerandomize_  # noqa: F401
from .config import load_config, is_image_dataset, init_model_by_parameter  # noqa: F401
from . import checkpoint  # noqa: F401
from . import datasets  # noqa: F401
from .datasets import Generator, get_dataset, ToyLoader  # noqa: F401
from . import training  # noqa: F401
from .training import MLPTrainer, TrainingManager  # noqa: F401
