from .augment import DeviceAugment, philox4x32
from .datasets import (MNIST, SyntheticImageNet, SyntheticMNIST, TensorDataset, input_affine,
                       load_mnist, normalize_input, synthetic_classification)
from .loader import DeviceCursor, DeviceLoader, Gathered
from .mix import DeviceMix
from .samplers import (MySampler, PartitionSampler, RandomSampleSampler, ShardSampler,
                       make_sampler)

__all__ = ["MNIST", "SyntheticMNIST", "SyntheticImageNet", "TensorDataset", "load_mnist",
           "synthetic_classification", "input_affine", "normalize_input", "DeviceLoader", "DeviceCursor", "DeviceAugment", "DeviceMix", "philox4x32", "Gathered", "MySampler", "PartitionSampler",
           "RandomSampleSampler", "ShardSampler", "make_sampler"]
