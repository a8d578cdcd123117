"""`from utils.inference import inference` -- the reference's import path (inference.py:14)."""
from pytorch_segmentation_amd.utils.inference import inference  # noqa: F401
