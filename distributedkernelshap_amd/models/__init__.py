from .predictors import (  # noqa: F401
    KernelMachinePredictor,
    LinearPredictor,
    MLPPredictor,
    MulticlassSVCPredictor,
    RoutedTreeEnsemblePredictor,
    TorchPredictor,
    TreeEnsemblePredictor,
    make_predictor,
)
from .synthetic import SyntheticData, make_adult_like, make_tabular  # noqa: F401
