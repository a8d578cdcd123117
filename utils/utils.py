"""`from utils.utils import compute_loss, compute_metrics` -- the reference's import path (train.py:16, test.py:11)."""
from pytorch_segmentation_amd.utils.loss import (boundary_width, compute_boundary_metrics, compute_loss,  # noqa: F401
                                                  compute_metrics, predict_mask, update_boundary_counts, update_class_counts)
