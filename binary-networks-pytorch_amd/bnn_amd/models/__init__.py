from .bats import AuxiliaryHead, BATSNetworkCIFAR, BATSNetworkImageNet, Cell
from .bats_ops import (ALL_OPS, EXTENDED_OPS, OPS, PRIMITIVES, DilConv, FactorizedConv, FactorizedReduce, Genotype,
                       ReLUConvBN, SepConv, Zero, channel_shuffle, drop_path)
from .blocks import BasicBlock, Bottleneck, HBlock, PreBasicBlock, PreBottleneck, conv1x1, conv3x3
from .resnet import DaBNNStem, ResNet, resnet18, resnet34, resnet50

__all__ = ["BasicBlock", "Bottleneck", "HBlock", "PreBasicBlock", "PreBottleneck", "conv1x1",
           "conv3x3", "DaBNNStem", "ResNet", "resnet18", "resnet34", "resnet50",
           "channel_shuffle", "SepConv", "DilConv", "ReLUConvBN", "FactorizedConv",
           "Genotype", "PRIMITIVES", "OPS", "EXTENDED_OPS", "ALL_OPS", "Zero", "FactorizedReduce", "drop_path", "Cell",
           "AuxiliaryHead",
           "BATSNetworkCIFAR", "BATSNetworkImageNet"]
