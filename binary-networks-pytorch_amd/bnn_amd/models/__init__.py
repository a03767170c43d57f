from .bats_ops import DilConv, ReLUConvBN, SepConv, channel_shuffle
from .blocks import BasicBlock, Bottleneck, HBlock, PreBasicBlock, PreBottleneck, conv1x1, conv3x3
from .resnet import DaBNNStem, ResNet, resnet18, resnet34, resnet50

__all__ = ["BasicBlock", "Bottleneck", "HBlock", "PreBasicBlock", "PreBottleneck", "conv1x1",
           "conv3x3", "DaBNNStem", "ResNet", "resnet18", "resnet34", "resnet50",
           "channel_shuffle", "SepConv", "DilConv", "ReLUConvBN"]
