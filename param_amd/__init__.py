"""param_amd -- MI355X-native (gfx950) embedding-lookup + DLRM all-to-all hot path of PARAM.

Layout (only what the hot path needs):
  csrc/              hand-written HIP kernels + the C ABI (include/param_amd.h) -> libparam_amd.so
  _lib.py            ctypes binding (no fallback: raises if the library is missing)
  embedding_bag.py   EmbeddingBagMI355 / BatchedEmbeddingBagMI355 (nn.EmbeddingBag / TBE surface), EmbeddingMI355 (nn.Embedding),
                     MaxEmbeddingBagMI355 / MaxBatchedEmbeddingBagMI355 (max pooling)
  quantized_bag.py   QuantizedBatchedEmbeddingBagMI355 / QuantizedEmbeddingBagMI355 / QuantizedEmbeddingMI355: pooled and un-pooled
                     lookups over 8- / 4-bit row-quantised tables
  float8_bag.py      Float8BatchedEmbeddingBagMI355 / Float8EmbeddingBagMI355 / Float8EmbeddingMI355: pooled and un-pooled lookups
                     over OCP FP8 (e4m3fn / e5m2) tables
  mixed_bag.py       MixedBatchedEmbeddingBagMI355: pooled and un-pooled lookups over tables that are EACH in their own format
                     (fp32 / bf16 / fp16 / FP8 / 8- / 4-bit rows), one launch
  indices.py         uniform / Zipf index generation (reference init_indices + a scalable form)
  compute/pt/        mirror of the reference train/compute/pt emb driver CLI
  comms/pt/          mirror of the reference train/comms/pt backend plug-in, metrics and drivers
"""
from ._lib import LIB_PATH, ParamAmdError, load as load_library, set_backward_tuning, set_forward_tuning, set_hybrid_min_tiles, set_hybrid_rest, set_hybrid_tuning, set_sort_tuning, set_tuning  # noqa: F401
from .embedding_bag import (  # noqa: F401
    BatchedEmbeddingBagMI355,
    EmbeddingBagMI355,
    EmbeddingMI355,
    MaxBatchedEmbeddingBagMI355,
    MaxEmbeddingBagMI355,
    check_request,
    fill_random_,
)
from .quantized_bag import QuantizedBatchedEmbeddingBagMI355, QuantizedEmbeddingBagMI355, QuantizedEmbeddingMI355  # noqa: F401
from .float8_bag import Float8BatchedEmbeddingBagMI355, Float8EmbeddingBagMI355, Float8EmbeddingMI355  # noqa: F401
from .mixed_bag import MixedBatchedEmbeddingBagMI355  # noqa: F401

__version__ = "0.1.0"
