from .optimizer import OptimConfig, Optimizer
from .params import StageParams
from .stage import Stage
from .trainer import Trainer, default_distribution

__all__ = ["OptimConfig", "Optimizer", "Stage", "StageParams", "Trainer", "default_distribution"]
