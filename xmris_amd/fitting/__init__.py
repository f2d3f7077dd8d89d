"""Quantification: AMARES and basis-set time-domain fitting on the GPU (reference ``src/xmris/fitting``)."""
from .amares import fit_amares
from .basis import basis_model, fit_basis
from .dataset import LabeledDataset
from .kinetics import fit_kinetics, simulate_kinetics
from .prior_knowledge import PriorKnowledge, read_prior_knowledge
from .simulation import simulate_fid

__all__ = ["LabeledDataset", "PriorKnowledge", "basis_model", "fit_amares", "fit_basis", "fit_kinetics", "read_prior_knowledge",
           "simulate_fid", "simulate_kinetics"]
