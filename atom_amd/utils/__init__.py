from .cat_tensor import BatchLenInfo  # noqa: F401
from .kvcache import (BatchedKvCacheInt4, KvCacheInt4, KvPoolInt4, RollingKvCacheInt4, StaticBatchedKvCacheInt4,  # noqa: F401
                      StaticBeamKvCacheInt4)
from .lora import LlamaLoraManager, LlamaLoraWeight, LoraManager, LoraWeight, permute_intermediate  # noqa: F401
