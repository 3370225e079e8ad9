"""Perception Encoder (reference: libs/perception_encoder/) on the HIP kernels: the vision tower only."""
