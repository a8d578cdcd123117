"""`from utils.datasets import CocoDataset, CocoInstance, VOC_COLORMAP` -- the reference's import path (train.py:15, test.py:10,
inference.py:13)."""
from pytorch_segmentation_amd.utils.datasets import VOC_COLORMAP, CocoDataset, CocoInstance, voc_colormap  # noqa: F401
