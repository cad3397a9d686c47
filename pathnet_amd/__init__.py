"""pathnet_amd -- MI355X-native implementation of PathNet's path-aggregation hot path.

  pathnet_amd.sampler   MERW random-walk path sampler (GPU walker + the gen_merw CLI)
  pathnet_amd.pathfile  the reference's text path-file format
  pathnet_amd.modules   PathNet / PathNet_homo / PAGG nn.Modules on hand-written HIP kernels
  pathnet_amd.dist      node sharding across the GPUs of one box (RCCL)
  pathnet_amd.optim     CrossEntropyLoss / Adam of the reference's training step as single launches; AdamW, amsgrad,
                        gradient-norm clipping and a device-side learning-rate schedule (LRSchedule)
  pathnet_amd.trainer   train_fixed_indices with everything resident on the GPU
  pathnet_amd.walkstats statistics of sampled paths, counted on the GPU (the walkstats CLI)
  pathnet_amd.pathprob  transition probabilities and path likelihoods under the sampler's tables; importance weights
  pathnet_amd.ensemble  predictions averaged over resampled paths on the GPU: Ensemble, Prediction, model.predict()
  pathnet_amd.calibration  fit_temperature / model.calibrate(), Ensemble(temperature=), Prediction.calibration(): a temperature
                        fitted and applied on the GPU, reliability bins, ECE, NLL, Brier score and risk-coverage
  pathnet_amd.contrast  contrastive_loss: NT-Xent between two path draws, tiled forward and backward with exact fp32
                        products and no [2S, 2S] array; model.pretrain() / trainer.pretrain() for unlabelled nodes
  pathnet_amd.neighbours  knn: exact k nearest neighbours of embeddings (cosine / dot) with a total order and no [Sq, N] array;
                        knn_classify: the weighted k-NN vote; model.embed() / model.knn_probe(), the label-free monitor
  pathnet_amd.cluster   kmeans: k-means++ / Lloyd clustering of embeddings (cosine / euclidean) with defined ties, fp64 means in
                        a fixed order and no [N, K] array; cluster_scores: contingency table, NMI, ARI, purity;
                        model.cluster_probe(), the judgement that needs no labels at all
  pathnet_amd.explain   which paths, nodes or edges a prediction rests on: exact occlusion of path groups (disjoint or
                        overlapping) on the GPU, model.explain(), NodeTotals
  pathnet_amd.synth     path-pattern census: the labels of the synthetic experiment (the gen_*_syn CLI)

Everything computes through csrc/libpathnet_hip.so (C ABI: include/pathnet_hip.h).
"""
from . import _lib  # noqa: F401
from .modules import PAGG, PathNet, PathNet_homo  # noqa: F401
from .optim import (Adam, AdamW, CrossEntropyLoss, LRSchedule, StepState, backward, balanced_class_weight,  # noqa: F401
                    clip_grad_norm_, cross_entropy)
from .sampler import (DRAW_GLIBC_REPLAY, DRAW_PHILOX, BiasedSampler, MerwSampler, PathAnnotator,  # noqa: F401
                      PathReport, UniformSampler)
from .ensemble import Ensemble, Prediction  # noqa: F401
from .calibration import Calibration, Temperature, fit_temperature  # noqa: F401
from .contrast import Contrast, contrastive_loss  # noqa: F401
from .neighbours import KnnVote, Neighbours, knn, knn_classify  # noqa: F401
from .cluster import Clusters, ClusterScores, cluster_scores, kmeans  # noqa: F401
from .explain import (Explanation, NodeTotals, explain, explain_groups, explain_overlap, explain_units,  # noqa: F401
                      member_nodes)
from .pathprob import PathProb, importance_weights  # noqa: F401
from .synth import PatternCensus  # noqa: F401
from .walkstats import WalkStats, path_multiplicity, walk_stats  # noqa: F401

__version__ = "0.1.0"
