from . import comm, env
from .comm import (GradAggregator, allgather_average_gradients, allreduce_average_gradients,
                   average_gradients, dist_init, init_parameters)
from .compress import Q8Compressor, TopKCompressor, payload_bytes, topk_payload_bytes
from .ddp import DDP, DistributedDataParallel
from .straggler import Straggler

__all__ = ["env", "comm", "GradAggregator", "dist_init", "init_parameters",
           "allreduce_average_gradients", "allgather_average_gradients", "average_gradients",
           "DistributedDataParallel", "DDP", "Straggler", "Q8Compressor", "payload_bytes",
           "TopKCompressor", "topk_payload_bytes"]
