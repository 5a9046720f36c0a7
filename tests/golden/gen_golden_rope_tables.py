"""Writes tests/golden/rope_tables.json: inv_freq (fp32, radians per position, 64 pairs of head_dim 128) and attention_factor of the
RoPE-scaling configs below, as transformers.modeling_rope_utils computes them (recorded with transformers 5.15.0).

    python tests/golden/gen_golden_rope_tables.py

tests/test_rope_table_cpu.py compares atom_amd.e2e.rope.rope_init with the file, so the check does not need transformers."""
import json
import os

CONFIGS = {
    "llama-3.1-8b": dict(rope_type="llama3", rope_theta=5e5, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                         original_max_position_embeddings=8192),
    "llama-3.2": dict(rope_type="llama3", rope_theta=5e5, factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                      original_max_position_embeddings=8192),
    "linear-2": dict(rope_type="linear", rope_theta=1e4, factor=2.0),
    "yarn-4": dict(rope_type="yarn", rope_theta=1e4, factor=4.0, original_max_position_embeddings=4096),
    "yarn-4-options": dict(rope_type="yarn", rope_theta=1e4, factor=4.0, original_max_position_embeddings=4096, beta_fast=16, beta_slow=2,
                           attention_factor=1.25, truncate=False),
}
MAX_POSITIONS = 131072


def hf_config(rope_parameters):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=4096, num_attention_heads=32, max_position_embeddings=MAX_POSITIONS, rope_parameters=dict(rope_parameters))


def hf_values(rope_parameters):
    """(inv_freq as a list of 64 floats, each an fp32 value; attention_factor) from transformers"""
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    inv_freq, attention_factor = ROPE_INIT_FUNCTIONS[rope_parameters["rope_type"]](hf_config(rope_parameters), "cpu")
    return [float(x) for x in inv_freq.float().tolist()], float(attention_factor)


if __name__ == "__main__":
    import transformers
    out = {"transformers": transformers.__version__, "configs": {}}
    for name, rp in CONFIGS.items():
        inv_freq, attention_factor = hf_values(rp)
        assert len(inv_freq) == 64
        out["configs"][name] = dict(rope_parameters=rp, inv_freq=inv_freq, attention_factor=attention_factor)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rope_tables.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)
