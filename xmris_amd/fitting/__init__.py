"""Quantification: AMARES time-domain fitting on the GPU (reference ``src/xmris/fitting``)."""
from .amares import fit_amares
from .dataset import LabeledDataset
from .prior_knowledge import PriorKnowledge, read_prior_knowledge
from .simulation import simulate_fid

__all__ = ["LabeledDataset", "PriorKnowledge", "fit_amares", "read_prior_knowledge", "simulate_fid"]
