"""Evaluation metrics of generated animation (said/metric): Frechet distance, multimodality and WInD over BCVAE latents, beat consistency
of the coefficients with the audio, and the vertex error against the real animation.

Every pass over the data runs on the MI355X: the latent metrics through include/said_metrics.h, beat consistency (a float64 restatement of
librosa's onset detection; librosa is not needed) and the vertex error through include/said_beat.h."""
from . import beat_consistency, frechet_distance, multimodality, vertex_error, wind

__all__ = ["beat_consistency", "frechet_distance", "multimodality", "vertex_error", "wind"]
