"""Training on the MI355X: the BCVAE (script/train_vae.py of the reference) and the UNet denoiser (script/train.py)."""
from .unet import (TrainWindowDataset, UNetLossEpochOutput, UNetLossStepOutput, UNetTrainer, ValWindowDataset, make_unet_dataloaders, normalize_deltas,
                   trainable_shapes, unet_init_state_dict)
from .vae import (BCVAETrainer, LossEpochOutput, LossStepOutput, VAEWindowDataset, bcvae_init_state_dict, get_data_paths, make_dataloaders,
                  mirror_permutation)

__all__ = ["TrainWindowDataset", "ValWindowDataset", "make_unet_dataloaders", "unet_init_state_dict", "BCVAETrainer", "LossEpochOutput", "LossStepOutput", "UNetLossEpochOutput", "UNetLossStepOutput", "UNetTrainer", "VAEWindowDataset",
           "bcvae_init_state_dict", "get_data_paths", "make_dataloaders", "mirror_permutation", "normalize_deltas", "trainable_shapes"]
