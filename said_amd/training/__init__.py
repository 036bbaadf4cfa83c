"""Training on the MI355X: the BCVAE (script/train_vae.py of the reference)."""
from .vae import (BCVAETrainer, LossEpochOutput, LossStepOutput, VAEWindowDataset, bcvae_init_state_dict, get_data_paths, make_dataloaders,
                  mirror_permutation)

__all__ = ["BCVAETrainer", "LossEpochOutput", "LossStepOutput", "VAEWindowDataset", "bcvae_init_state_dict", "get_data_paths",
           "make_dataloaders", "mirror_permutation"]
