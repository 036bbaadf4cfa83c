"""Evaluation metrics of generated animation (said/metric): Frechet distance, multimodality and WInD over BCVAE latents.

The passes over the latents run on the MI355X (include/said_metrics.h); beat consistency is not provided (the reference's evaluation does
not call it, and it needs librosa)."""
from . import frechet_distance, multimodality, wind

__all__ = ["frechet_distance", "multimodality", "wind"]
