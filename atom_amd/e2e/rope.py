"""RoPE scaling of a model config -> what the INT4 paged-KV attention ops take (ops.batch_decode_i4 / ops.batch_prefill_i4).

``rope_init(config)`` returns ``(theta, rope_scale, inv_freq, attention_factor)``:

    theta             the RoPE base (``rope_theta``)
    rope_scale        the ops' position divisor: ``factor`` for type ``linear``, else 1.0
    inv_freq          float64 [64], radians per position of pair i (dims i, i + 64) -- or None where the ops' own
                      ``theta ** (-2 i / 128) / rope_scale`` is the definition (no scaling, ``default``, ``linear``)
    attention_factor  what HF multiplies cos / sin by (YaRN); the logits take its square (``attn_scale``).  1.0 elsewhere.

Both config spellings are read: ``config.rope_parameters`` (transformers 5: a dict with ``rope_theta`` and ``rope_type``; ``rope_theta``
itself may then be None or absent) and ``config.rope_theta`` + ``config.rope_scaling`` (transformers 4; the type key is ``rope_type`` or
the legacy ``type``).  The definitions are those of ``transformers.modeling_rope_utils`` (``_compute_llama3_parameters``,
``_compute_yarn_parameters``, ``_compute_linear_scaling_rope_parameters``), computed in float64 -- transformers computes in fp32 --
for head_dim 128, full rotary.  Types whose frequencies depend on the running length (``dynamic``, ``longrope``) or that this tree has
no kernel argument for (``proportional``, YaRN's ``mscale`` / ``mscale_all_dim``, a partial rotary factor) raise NotImplementedError
naming the type: a config is never silently run with other frequencies than its own."""
import math

import numpy as np

HEAD_DIM = 128


def _get(obj, key, default=None):
    if isinstance(obj, dict):
        return obj.get(key, default)
    return getattr(obj, key, default)


def rope_parameters(config) -> dict:
    """the config's RoPE settings as one dict with ``rope_theta`` and ``rope_type`` always set, from either spelling"""
    rp = _get(config, "rope_parameters")
    if rp is not None:
        rp = dict(rp)
    else:
        rp = dict(_get(config, "rope_scaling") or {})
    theta = rp.get("rope_theta")
    if theta is None:
        theta = _get(config, "rope_theta")
    rp["rope_theta"] = 1e4 if theta is None else float(theta)
    kind = rp.get("rope_type", rp.get("type"))
    rp["rope_type"] = "default" if kind is None else str(kind)
    return rp


def _llama3(rp, base):
    for key in ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings"):
        if rp.get(key) is None:
            raise ValueError(f"rope type llama3 needs {key!r}")
    factor, low, high = float(rp["factor"]), float(rp["low_freq_factor"]), float(rp["high_freq_factor"])
    old_len = float(rp["original_max_position_embeddings"])
    inv = 1.0 / base ** (np.arange(0, HEAD_DIM, 2, dtype=np.float64) / HEAD_DIM)
    wavelen = 2.0 * math.pi / inv
    out = np.where(wavelen > old_len / low, inv / factor, inv)
    smooth = (old_len / wavelen - low) / (high - low)
    smoothed = (1.0 - smooth) * out / factor + smooth * out
    medium = ~(wavelen < old_len / high) & ~(wavelen > old_len / low)
    return np.where(medium, smoothed, out), 1.0


def _yarn(rp, base, config):
    if rp.get("mscale") or rp.get("mscale_all_dim"):
        raise NotImplementedError("rope type 'yarn' with mscale / mscale_all_dim is not implemented")
    if rp.get("original_max_position_embeddings") is None:
        raise ValueError("rope type yarn needs 'original_max_position_embeddings'")
    orig = float(rp["original_max_position_embeddings"])
    factor = rp.get("factor")
    if factor is None:
        factor = float(_get(config, "max_position_embeddings")) / orig
    factor = float(factor)
    attention_factor = rp.get("attention_factor")
    if attention_factor is None:
        attention_factor = 1.0 if factor <= 1 else 0.1 * math.log(factor) + 1.0
    beta_fast, beta_slow = rp.get("beta_fast") or 32, rp.get("beta_slow") or 1
    truncate = rp.get("truncate", True)

    def correction_dim(rotations):
        return (HEAD_DIM * math.log(orig / (rotations * 2 * math.pi))) / (2 * math.log(base))

    low, high = correction_dim(beta_fast), correction_dim(beta_slow)
    if truncate:
        low, high = math.floor(low), math.ceil(high)
    low, high = max(low, 0), min(high, HEAD_DIM - 1)
    if low == high:
        high += 0.001
    pos_freqs = base ** (np.arange(0, HEAD_DIM, 2, dtype=np.float64) / HEAD_DIM)
    ramp = np.clip((np.arange(HEAD_DIM // 2, dtype=np.float64) - low) / (high - low), 0.0, 1.0)
    extrapolation = 1.0 - ramp
    inv = (1.0 / (factor * pos_freqs)) * (1.0 - extrapolation) + (1.0 / pos_freqs) * extrapolation
    return inv, float(attention_factor)


def rope_init(config):
    """(theta, rope_scale, inv_freq float64 [64] or None, attention_factor) of a config -- see the module's text"""
    rp = rope_parameters(config)
    theta, kind = rp["rope_theta"], rp["rope_type"]
    if not theta > 0:
        raise ValueError(f"rope_theta must be positive, got {theta}")
    if float(rp.get("partial_rotary_factor") or 1.0) != 1.0:
        raise NotImplementedError(f"partial rotary embeddings (partial_rotary_factor {rp['partial_rotary_factor']}) are not implemented")
    if kind == "default":
        return theta, 1.0, None, 1.0
    if kind == "linear":
        if rp.get("factor") is None or not float(rp["factor"]) > 0:
            raise ValueError("rope type linear needs a positive 'factor'")
        return theta, float(rp["factor"]), None, 1.0
    if kind == "llama3":
        inv, af = _llama3(rp, theta)
        return theta, 1.0, inv, af
    if kind == "yarn":
        inv, af = _yarn(rp, theta, config)
        return theta, 1.0, inv, af
    raise NotImplementedError(f"rope type {kind!r} is not implemented (supported: default, linear, llama3, yarn)")
