"""Datasets of the training loops under the reference's module names."""
