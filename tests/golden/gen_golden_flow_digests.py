"""Writes tests/golden/flow_ref_cpu_digests.json: the sha256 digest of every array the UNMODIFIED reference flow
(tests/flow_run.py --impl reference) produces for each CPU configuration of tests/test_flow_reference_cpu.py, so that the
test holds this repository's flow mirrors to the reference's output where the reference tree is absent.  Needs the reference."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_flow_reference_cpu import DIGESTS, digest  # noqa: E402

CONFIGS = [("rtn_w4a16", "rtn_w4a4"), ("gptq_w4a16", "gptq_w4a4"), ("rtn_w4a16_gqa", "rtn_w4a4_gqa")]


def main():
    z = np.load(os.path.join(ROOT, "tests", "golden", "flow_tokens.npz"))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for config, stream in CONFIGS:
            tok = os.path.join(d, f"tokens_{stream}.npz")
            np.savez(tok, **{k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(stream + ".")})
            res = os.path.join(d, f"ref_{config}.npz")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "flow_run.py"), "--impl", "reference", "--config", config,
                                "--tokens", tok, "--out", res], capture_output=True, text=True, cwd=ROOT)
            assert r.returncode == 0 and "FLOW_OK" in r.stdout, r.stderr[-3000:]
            a = np.load(res)
            out[config] = {k: digest(a[k]) for k in sorted(a.files)}
    with open(DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", DIGESTS, {c: len(v) for c, v in out.items()})


if __name__ == "__main__":
    main()
