from .functional import (conv2d, batchnorm_act, batchnorm_add_relu, add_relu,
                         add_relu_tap, downsample_a,
                         global_avg_pool, linear, cross_entropy, kd_loss, wa_loss,
                         accuracy, max_pool, crop_resize,
                         crop_resize_ragged, crop_resize_ragged_reference)
from .nme import nme_prototypes, nme_topk
from .pod import pod_pool, pod_spatial, pod_dist, pod_loss
from .cosine import cosine_linear, flat_loss, flat_dist
from .margin import margin_rank_loss, margin_rank_select
from .lsc import lsc_reduce, nca_loss, nca_rows
from .kmeans import kmeans_proxies
from ._backend import have_ext

__all__ = ["conv2d", "batchnorm_act", "batchnorm_add_relu", "add_relu",
           "add_relu_tap", "downsample_a",
           "global_avg_pool", "linear", "cross_entropy", "kd_loss", "wa_loss", "accuracy",
           "max_pool", "crop_resize", "crop_resize_ragged",
           "crop_resize_ragged_reference", "nme_prototypes", "nme_topk",
           "pod_pool", "pod_spatial", "pod_dist", "pod_loss",
           "cosine_linear", "flat_loss", "flat_dist",
           "margin_rank_loss", "margin_rank_select",
           "lsc_reduce", "nca_loss", "nca_rows", "kmeans_proxies",
           "have_ext"]
