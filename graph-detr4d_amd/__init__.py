"""graph-detr4d_amd: MI355X-native decoder hot path of Graph-DETR4D.

Importing the package registers the attention / transformer modules under the reference's type
names (`Deform3DCrossAttn`, `Detr3DCrossAtten`, `Detr3DTransformer`, ...) in the registry shim and,
when mmcv/mmdet are importable, in their real registries.
"""
__version__ = '0.1.0'

from .registry import (ATTENTION, BACKBONES, BBOX_ASSIGNERS, BBOX_CODERS, CONV_LAYERS, HEADS, LOSSES, NECKS, TRANSFORMER, TRANSFORMER_LAYER, TRANSFORMER_LAYER_SEQUENCE,  # noqa: F401
                       build_assigner, build_attention, build_backbone, build_bbox_coder, build_conv_layer, build_head, build_loss, build_neck, build_transformer, build_transformer_layer,
                       build_transformer_layer_sequence)
from .transformer_layers import (FFN, BaseTransformerLayer, DetrTransformerDecoderLayer,  # noqa: F401
                                 MultiheadAttention, TransformerLayerSequence)
from .deform3d_cross_attn import Deform3DCrossAttn  # noqa: F401
from .deform3d_cross_attn_mp import Deform3DCrossAttnMP  # noqa: F401
from .bbox_coder import NMSFreeCoder  # noqa: F401
from .criterion import Detr3DCriterion, HDetr3DCriterion, HungarianAssigner3D  # noqa: F401
from .distill import DistillHungarianAssigner3D, FeatureDistillLoss, get_feat_distill_loss, get_instance_distill_loss  # noqa: F401
from .dgcnn_attn import DGCNNAttn  # noqa: F401
from .head_pe import FeaturePositionEmbedding  # noqa: F401
from .depth_net import DepthNet  # noqa: F401
from .recipe import TrainRecipe  # noqa: F401
from .grid_mask import GridMask  # noqa: F401
from .fpn import CPFPN, FPN  # noqa: F401
from .dcn import ModulatedDeformConv2d, ModulatedDeformConv2dPack  # noqa: F401
from .backbones import BasicBlock, Bottleneck, ResNet, VoVNet, VoVNetCP  # noqa: F401
from . import functional, plumbing  # noqa: F401
from .detr3d_transformer import (Detr3DCrossAtten, Detr3DCrossAttenV2, Detr3DTransformer, Detr3DTransformerDecoder,  # noqa: F401
                                 HDetr3DTransformer, feature_sampling, inverse_sigmoid)
from .petr_transformer import (PETRMultiheadAttention, PETRTransformer, PETRTransformerDecoder,  # noqa: F401
                               PETRTransformerDecoderLayer, PETRTransformerEncoder)
from .petr_head import PETRHead, PETRHeadseg, PETRv2Head, Sigmoid_ce_loss  # noqa: F401

__all__ = ['Deform3DCrossAttn', 'Deform3DCrossAttnMP', 'DGCNNAttn', 'Detr3DCrossAtten', 'Detr3DCrossAttenV2', 'feature_sampling', 'Detr3DTransformer',
           'Detr3DTransformerDecoder', 'HDetr3DTransformer', 'MultiheadAttention', 'FFN', 'BaseTransformerLayer',
           'DetrTransformerDecoderLayer', 'TransformerLayerSequence', 'inverse_sigmoid',
           'NMSFreeCoder', 'HungarianAssigner3D', 'Detr3DCriterion', 'HDetr3DCriterion', 'DistillHungarianAssigner3D', 'get_instance_distill_loss', 'FeatureDistillLoss', 'get_feat_distill_loss', 'FeaturePositionEmbedding', 'DepthNet', 'TrainRecipe', 'GridMask', 'FPN', 'CPFPN', 'NECKS', 'build_neck', 'ModulatedDeformConv2d', 'ModulatedDeformConv2dPack', 'CONV_LAYERS', 'build_conv_layer',
           'BasicBlock', 'Bottleneck', 'ResNet', 'VoVNet', 'VoVNetCP', 'BACKBONES', 'build_backbone', 'BBOX_CODERS', 'BBOX_ASSIGNERS', 'ATTENTION', 'TRANSFORMER', 'TRANSFORMER_LAYER', 'TRANSFORMER_LAYER_SEQUENCE',
           'PETRMultiheadAttention', 'PETRTransformer', 'PETRTransformerDecoder', 'PETRTransformerDecoderLayer', 'PETRTransformerEncoder',
           'PETRHead', 'PETRv2Head', 'HEADS', 'build_head', 'PETRHeadseg', 'Sigmoid_ce_loss', 'LOSSES', 'build_loss']
