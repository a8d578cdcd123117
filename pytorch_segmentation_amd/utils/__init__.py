from .datasets import VOC_COLORMAP, voc_colormap
from .dist import GradReducer, all_reduce_counters, broadcast_buffers
from .loss import (boundary_weight_table, boundary_weighted_cross_entropy_loss, boundary_width, compute_boundary_metrics,
                   compute_loss, compute_metrics, compute_surface_metrics, lovasz_softmax_loss, make_loss,
                   predict_mask, predict_mask_ensemble, predict_mask_windows, signed_distance, surface_loss, tversky_loss,
                   update_boundary_counts, update_class_counts, update_surface_stats, weighted_cross_entropy_loss)
from .inference import inference
from .trainer import Fetcher, FlatOptimizer, Trainer

__all__ = ['compute_loss', 'lovasz_softmax_loss', 'weighted_cross_entropy_loss', 'tversky_loss', 'boundary_weighted_cross_entropy_loss',
           'boundary_weight_table', 'surface_loss', 'signed_distance', 'make_loss', 'compute_metrics', 'predict_mask', 'predict_mask_ensemble', 'predict_mask_windows', 'update_class_counts', 'boundary_width',
           'update_boundary_counts', 'compute_boundary_metrics', 'update_surface_stats', 'compute_surface_metrics', 'GradReducer',
           'all_reduce_counters', 'broadcast_buffers', 'Fetcher', 'FlatOptimizer', 'Trainer', 'inference', 'voc_colormap',
           'VOC_COLORMAP']
