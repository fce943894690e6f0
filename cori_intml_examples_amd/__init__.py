"""cori_intml_examples_amd — MI355X-native interactive distributed deep learning + HPO.

Capabilities of mlhenderson/cori-intml-examples re-designed for gfx950: Keras-shaped
CNN models whose layer stack runs on hand-written CDNA4 HIP kernels, Horovod-shaped
synchronous data parallelism over RCCL, an IPyParallel-shaped one-node task farm, and
random / genetic / grid hyper-parameter search with live monitoring widgets.
"""
__version__ = "0.1.0"

from . import activations, models, optim, regularizers, train, utils  # noqa: F401
from .models import (ELU, Activation, AveragePooling2D, BatchNormalization, Conv2D, Dense, Dropout,  # noqa: F401
                     Flatten, GlobalAveragePooling2D, GlobalMaxPooling2D, Input, LeakyReLU, MaxPooling2D, Model,
                     Sequential, load_model)
