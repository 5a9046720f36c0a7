"""Native-kernel Llama building blocks with the call graph of the reference's e2e tree
(e2e/punica-atom/punica/models/llama.py): the 4-tuple (outlier, norms, outlier_scales, norm_scales) flows between ops."""
from .llama import (LinearInt4, LlamaAttention, LlamaDecoderLayer, LlamaForCausalLM, LlamaMLP, LlamaModel,  # noqa: F401
                    LlamaRMSNorm, LlamaRMSNormInt4)
from .generate import BeamDecodeGraph, BeamHypothesis, DecodeGraph, LogitPenalties, Sampler, SamplingParams, TokenLogprobs, backtrack_beams, beam_search, generate, perplexity, score  # noqa: F401
from .generate import NgramDrafter, SpecDecodeGraph, SpecStats, SpeculativeParams  # noqa: F401
from .guide import LogitGuide, TokenAutomaton  # noqa: F401
from .mixtral import MixtralDecoderLayer, MixtralForCausalLM, MixtralModel, MixtralSparseMoeInt4  # noqa: F401
from .llama_lora import LlamaDecoderLayerWithLora, LlamaForCausalLMWithLora, LlamaModelWithLora  # noqa: F401
