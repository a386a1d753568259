"""ured_hip — the MI355X (gfx950) hot path of U-RED on libured_hip.so.

  _lib     ctypes loader of the C-ABI (include/ured_hip.h); raises if missing
  nn       nearest-neighbour / chamfer autograd ops (dense + ragged segments) and knn(): the K
           nearest neighbours, 1 <= K <= 1024, sorted by (distance, index), with valid lengths
           (the stand-in for pytorch3d.ops.knn_points: parity-unpinned, semantics from its docs)
  kernels  typed wrappers of the fused per-point MLP entry points
  mlp      PointEncoderFn / ResidualNetFn / PointChainFn autograd chains
  attn     graph-node multi-head attention (DeformNet's GraphAttentionNet core)
  optim    FlatAdam: per-module gradient clipping + Adam over flat buffers
  node     DeformNet graph-node GEMM / BatchNorm launches
  ops      device-side part building (segment sums, AABBs)
  occ      partial (occluded) target clouds: ball / random / slice / part occlusion, centring, rotation
  group    PointNet++ set abstraction primitives: farthest-point sampling, ball query, grouping (GroupFn)
  interp   PointNet++ feature propagation: three_nn and the inverse-distance interpolation (InterpFn)
  gcn      3D-GCN graph convolution: neighbor_dirs, GcnConvFn, GcnPoolFn, GcnLinearFn
  vn       Vector-Neuron DGCNN layers: knn_rows, VnEdgeFn, VnPointFn, VnMaxPoolFn, VnFrameFn, VnLinearFn
  dcd      density-aware chamfer as a training loss: DcdLossFn / dcd_loss (one launch each way after the NN)
  pcn      the PCN completion network: PcnEncoderFn, PcnDecoderFn and the fold / pool / ReLU kernels
  vrc      VRCNet's self-attention encoder and decoder: SaFn, SkMeanFn, SkMixFn, EdgePoolFn, UnpoolFn,
           LinearRowsFn, the expansion units' EfEdgeFn, EfMaxFn, FoldFn, CenterFn, and Model's LatentFn (latent
           heads, KL terms) and GaussKernelFn (the MMD kernel matrix), both also exported here
  losshead the step's loss head (chamfer families, contrastive, residual, reconstruction, weighted sum)
"""
from . import _lib, attn, dcd, gcn, group, interp, kernels, losshead, nn, node, occ, ops, optim, pcn, syncbn, vn, vrc  # noqa: F401
from .vrc import GaussKernelFn, LatentFn  # noqa: E402,F401
