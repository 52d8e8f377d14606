"""Drop-in for reference lib/utils/utils.py: the ELBO wrapper and training helpers."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from vae2.model import FullModel_D, FullModel_encdec  # noqa: E402,F401
from vae2.trainer import (AverageMeter, adjust_learning_rate, create_logger,  # noqa: E402,F401
                          dynamic_coeff, get_rank, get_world_size)
