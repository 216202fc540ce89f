from .flat import FlatParams
from .layers import (BasicBlock, Conv2d, ConvBN, ConvBNPool, Flatten, GlobalAvgPool, Linear,
                     MaxPool, Softmax)
from .loss import CrossEntropyLoss, EvalMetrics, MixTarget, count_correct, cross_entropy
from .program import Ctx, Layer, Program
from .syncbn import convert_sync_batchnorm

__all__ = ["convert_sync_batchnorm", "FlatParams","Program", "Layer", "Ctx", "Conv2d", "Linear", "Flatten", "Softmax",
           "ConvBN", "ConvBNPool", "BasicBlock", "MaxPool", "GlobalAvgPool", "CrossEntropyLoss", "MixTarget",
           "cross_entropy", "count_correct", "EvalMetrics"]
